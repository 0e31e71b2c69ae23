// From a finished device batch to the host arrays a caller sees (sp_match_batch_t, sp_lex_batch_t): which documents count, what
// is copied from where to where, the `exclusive` elimination and the packing in document order.  Host only: no HIP header and no
// HIP call in here -- the copies are a functor of the caller (copySync for a context, memcpy for the test entry and the
// stand-alone program tests/micro/batch_fetch_san.cpp), so the same code runs with and without a device.
#ifndef SPA_BATCH_FETCH_HPP
#define SPA_BATCH_FETCH_HPP
#include "../../include/strus_pattern_amd.h"
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <utility>
#include <vector>

namespace spa {

// malloc'ed array of n elements for the caller (sp_free, sp_*_batch_free)
template <class T>
T* hostArray( uint64_t n)
{
	T* p = (T*)std::malloc( (size_t)n * sizeof(T));
	if (!p) throw std::bad_alloc();
	return p;
}

// the host arrays of a batch of `ndocs` documents with room for `nresults` results and `nitems` items (sp_match_batch_free)
void allocMatchBatch( sp_match_batch_t* out, size_t ndocs, uint64_t nresults, uint64_t nitems, bool withFormats);
// the host arrays of a batch of `ndocs` documents with `nlexems` lexems (sp_lex_batch_free)
void allocLexBatch( sp_lex_batch_t* out, size_t ndocs, uint64_t nlexems);

// "document range outside the last batch" unless [firstDoc, firstDoc+ndocs) lies inside a batch of `batchDocs` documents
void checkDocRange( size_t firstDoc, size_t ndocs, size_t batchDocs);

// `count` records from `src` of a device array to `dst` of the packed host array
struct CopySegment { uint64_t src, count, dst; };

// ---- document blocks (records: lexems or results).  The device appends whole documents in completion order and says where in
// a (first, count) range per document.
struct DocBlocks
{
	std::vector<uint64_t> range;		// per document (first, count) in the packed array; count 0: the document comes out empty
	std::vector<CopySegment> segments;
	uint64_t packed = 0;			// records of the packed array
	size_t ndocs() const { return range.size()/2; }
	uint64_t first( size_t di) const { return range[ 2*di]; }
	uint64_t count( size_t di) const { return range[ 2*di+1]; }
};
// `range`, `status`: of the wanted documents; `inBuffer`: the records that lie inside the device buffer.  A failed document and
// one whose range ends outside the buffer come out empty.  whole: the whole batch is wanted -- one bulk segment, the packed
// array is the device array; else one segment per non-empty document, packed one after the other.
DocBlocks planDocBlocks( std::vector<uint64_t> range, const int32_t* status, uint64_t inBuffer, bool whole);

// ---- item blocks (rule matcher): the items of one document are one block in result order, [first item_begin, + sum of item_count)
struct ItemBlocks
{
	std::vector<CopySegment> segments;
	uint64_t packed = 0;			// items of the packed array
	uint64_t kept = 0;			// items of the documents that count
};
// `raw`: the packed results of `docs`; their item_begin is re-based to the packed item array.  Throws when a block lies outside
// the `inBuffer` items of the device buffer.
ItemBlocks planItemBlocks( const DocBlocks& docs, sp_result_t* raw, uint64_t inBuffer, bool whole);

// `exclusive` option over the n results of one document: covered[ i] != 0 for every result that another one covers
// (src/patternMatcher.cpp:192-246, :278-289)
void eliminateCovered( const sp_result_t* r, uint64_t n, uint32_t maxResultSize, std::vector<char>& covered);

// ---- the caller's batch in document order from the packed arrays: offsets, item_begin without gaps, format handles (rawrf,
// rawif: NULL without format strings), nresults / nitems as kept after the elimination.  doc_stats is allocated, not filled.
void regroupMatchBatch( const DocBlocks& docs, const int32_t* status, const sp_result_t* raw, const sp_result_item_t* rawitems,
			const uint32_t* rawrf, const uint32_t* rawif, uint64_t nitems, bool exclusive, uint32_t maxResultSize, sp_match_batch_t* out);
// (raw NULL: the packed array is the caller's own, `docs` planned without `whole`; its lexems are left to be copied in)
void regroupLexBatch( const DocBlocks& docs, const int32_t* status, const sp_lexem_t* raw, sp_lex_batch_t* out);

// ---- a batch in the device layout; `copy( dst, src, bytes)` reads it
struct MatchBatchSource
{
	const sp_result_t* results; uint64_t nresults;		// (counts: what lies inside the buffers)
	const sp_result_item_t* items; uint64_t nitems;
	const uint32_t* resultFormat; const uint32_t* itemFormat;	// NULL for a matcher without format strings
	const uint64_t* docRange; const int32_t* docStatus;
	const uint64_t* docStats;				// NULL: doc_stats is left to the caller
	size_t ndocs;
};
struct LexBatchSource
{
	const sp_lexem_t* lexems; uint64_t nlexems;
	const uint64_t* docRange; const int32_t* docStatus;
	size_t ndocs;
};

// Host copy of the documents [firstDoc, firstDoc+ndocs) of `src`, regrouped by document, with the `exclusive` elimination
// applied on the way.  The whole batch is copied in bulk; a sub-range copies only the result and item blocks of its own documents.
template <class COPY>
void fetchMatchBatch( const MatchBatchSource& src, size_t firstDoc, size_t ndocs, bool exclusive, uint32_t maxResultSize, COPY copy, sp_match_batch_t* out)
{
	checkDocRange( firstDoc, ndocs, src.ndocs);
	const bool whole = (firstDoc == 0 && ndocs == src.ndocs);
	const bool withFormats = src.resultFormat != 0;
	std::vector<uint64_t> range( ndocs*2);
	std::vector<int32_t> status( ndocs);
	if (ndocs)
	{
		copy( range.data(), src.docRange + 2*firstDoc, ndocs*2*sizeof(uint64_t));
		copy( status.data(), src.docStatus + firstDoc, ndocs*sizeof(int32_t));
	}
	const DocBlocks docs = planDocBlocks( std::move( range), status.data(), src.nresults, whole);
	std::vector<sp_result_t> raw( docs.packed+1);
	std::vector<uint32_t> rawrf( withFormats ? docs.packed+1 : 0);
	for (const CopySegment& s : docs.segments)
	{
		copy( raw.data() + s.dst, src.results + s.src, s.count*sizeof(sp_result_t));
		if (withFormats) copy( rawrf.data() + s.dst, src.resultFormat + s.src, s.count*sizeof(uint32_t));
	}
	const ItemBlocks items = planItemBlocks( docs, raw.data(), src.nitems, whole);
	std::vector<sp_result_item_t> rawitems( items.packed+1);
	std::vector<uint32_t> rawif( withFormats ? 2*items.packed+2 : 0);
	for (const CopySegment& s : items.segments)
	{
		copy( rawitems.data() + s.dst, src.items + s.src, s.count*sizeof(sp_result_item_t));
		if (withFormats) copy( rawif.data() + 2*s.dst, src.itemFormat + 2*s.src, 2*s.count*sizeof(uint32_t));
	}
	regroupMatchBatch( docs, status.data(), raw.data(), rawitems.data(), withFormats ? rawrf.data() : 0, withFormats ? rawif.data() : 0,
				items.kept, exclusive, maxResultSize, out);
	if (ndocs && src.docStats) copy( out->doc_stats, src.docStats + 4*firstDoc, ndocs*4*sizeof(uint64_t));
}

// The same for the lexems of the documents [firstDoc, firstDoc+ndocs).  Lexems need no work but their place, and the packed array
// of per-document segments already is the caller's: without `bulk` every document is copied straight to its place.  bulk (the
// host entry point, whose batches may be many small documents): one copy of the whole batch, put in document order on the host.
template <class COPY>
void fetchLexBatch( const LexBatchSource& src, size_t firstDoc, size_t ndocs, bool bulk, COPY copy, sp_lex_batch_t* out)
{
	checkDocRange( firstDoc, ndocs, src.ndocs);
	bulk = bulk && firstDoc == 0 && ndocs == src.ndocs;
	std::vector<uint64_t> range( ndocs*2);
	std::vector<int32_t> status( ndocs);
	if (ndocs)
	{
		copy( range.data(), src.docRange + 2*firstDoc, ndocs*2*sizeof(uint64_t));
		copy( status.data(), src.docStatus + firstDoc, ndocs*sizeof(int32_t));
	}
	const DocBlocks docs = planDocBlocks( std::move( range), status.data(), src.nlexems, bulk);
	if (bulk)
	{
		std::vector<sp_lexem_t> raw( docs.packed+1);
		for (const CopySegment& s : docs.segments) copy( raw.data() + s.dst, src.lexems + s.src, s.count*sizeof(sp_lexem_t));
		regroupLexBatch( docs, status.data(), raw.data(), out);
	}
	else
	{
		regroupLexBatch( docs, status.data(), 0, out);
		for (const CopySegment& s : docs.segments) copy( out->lexems + s.dst, src.lexems + s.src, s.count*sizeof(sp_lexem_t));
	}
}

} // namespace
#endif
