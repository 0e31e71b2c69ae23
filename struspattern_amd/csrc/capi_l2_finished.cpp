// C-ABI of level 2, second half: the last device batch finished on the device and what is made of the finished batch there --
// matched text, result values, pattern frequencies, index terms, the batch dictionary, its order, the term blocks, the batch postings, the posting positions, the posting blocks -- with their fetch and timing calls.  Every product is one
// ProductCall (capi_l2_ctx.hpp) behind the finish; sp_matcher_ctx::Products::drop() is what a new batch or finish does to them.
#include "capi_l2_ctx.hpp"
#include "l2_finish.h"
#include "l2_text.h"
#include "l2_freq.h"
#include "l2_values.h"
#include "l2_terms.h"
#include "l2_dict.h"
#include "l2_dictorder.h"
#include "l2_termblocks.h"
#include "l2_postings.h"
#include "l2_positions.h"
#include "l2_postingblocks.h"
#include "match_terms.hpp"
#include "match_dict.hpp"
#include "match_dictorder.hpp"
#include "match_termblocks.hpp"
#include "match_postings.hpp"
#include "match_positions.hpp"
#include "match_postingblocks.hpp"
#include "span_text.hpp"
#include "pattern_freq.hpp"
#include "finished_host.hpp"

typedef sp_matcher_ctx::ByteFamilies ByteFamilies;

namespace {

// a fetch call: the host waits for the product `run` (without one: `missing`), `copy` fills `out`, which is empty after a failure
template <int N, class OUT, class FN>
int fetchProduct( sp_matcher_ctx* c, const PassRun<N>& run, const char* missing, OUT* out, void (*release)( OUT*), FN copy)
{
	std::memset( out, 0, sizeof(*out));
	const int rc = guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		if (!run.done) throw std::runtime_error( missing);
		HIP_CHECK( hipSetDevice( c->device));
		HIP_CHECK( hipStreamSynchronize( run.stream));
		copy();
	});
	if (rc != SP_OK) release( out);
	return rc;
}

// ---- the two products of bytes per record (text, values)

// the text source of both calls, checked against the finished batch
void checkTextSource( const sp_matcher_ctx* c, const sp_text_source_t* src)
{
	if (!src || !src->d_seg_offsets || (!src->d_text && src->nbytes)) throw std::runtime_error( "no text source");
	requireFinished( c);
	if (!src->d_doc_seg_offsets && src->nseg != c->lastNdocs) throw std::runtime_error( "without document segment offsets every document is one segment: nseg must be ndocs");
}

// The working arrays of the families in `flags`, sized from the totals of the finish; the run begins; P gets what TextParams and
// ValuesParams name alike: the text source, and per family the records of the finish and the buffers.  `named` sets what
// the family structs name differently.
template <class PARAMS, class NAMED>
void beginByteFamilies( ProductCall& call, ByteFamilies& b, uint32_t flags, const sp_text_source_t* src, PARAMS& P, NAMED named)
{
	const sp_matcher_ctx::Finished& fin = call.c->prod.fin;
	for (int f=0; f<2; ++f) if (flags & (1u << f))
	{
		reserveOrNoMem( b.dWork[ f], (call.finished[ f]+1)*sizeof(uint32_t));
		reserveOrNoMem( b.dOffsets[ f], (call.finished[ f]+1)*sizeof(uint64_t));
		reserveOrNoMem( b.dDocBytes[ f], (call.ndocs+1)*sizeof(uint64_t));
		reserveOrNoMem( b.dDocOffsets[ f], (call.ndocs+1)*sizeof(uint64_t));
	}
	call.begin( b.dStatus, b.dTotals, 2, b.dCursor, 4);
	std::memset( &P, 0, sizeof(P));
	P.text = (const uint8_t*)src->d_text; P.nbytes = src->nbytes;
	P.segOffsets = (const uint64_t*)src->d_seg_offsets; P.nseg = src->nseg;
	P.docSegOffsets = (const uint64_t*)src->d_doc_seg_offsets;
	P.ndocs = (uint32_t)call.ndocs; P.docStatus = (int32_t*)b.dStatus.ptr; P.families = flags;
	for (int f=0; f<2; ++f) if (flags & (1u << f))
	{
		auto& F = P.family[ f];
		F.records = (const uint32_t*)(f ? fin.dItems.ptr : fin.dResults.ptr);
		F.docOffsets = (const uint64_t*)(f ? fin.dDocItemOffsets.ptr : fin.dDocResultOffsets.ptr);
		F.nrecords = call.finished[ f];
		F.docBytes = (uint64_t*)b.dDocBytes[ f].ptr; F.total = (uint64_t*)b.dTotals.ptr + f; F.cursor = (uint32_t*)b.dCursor.ptr + 2*f;
		named( F, (uint32_t*)b.dWork[ f].ptr, (uint64_t*)b.dDocOffsets[ f].ptr, (uint64_t*)b.dOffsets[ f].ptr, f);
	}
}

// the passes of both calls: the byte buffers are sized from what the counting passes counted
template <class PARAMS, class FAMILY>
void byteFamilyPasses( ProductCall& call, ByteFamilies& b, uint32_t flags, PARAMS& P, uint8_t* FAMILY::*outBytes,
		       hipError_t (*count)( const PARAMS&, unsigned, hipStream_t), hipError_t (*place)( const PARAMS&, unsigned, hipStream_t))
{
	uint64_t totals[ 2];
	call.passes( P, count, place, b.dTotals, totals, 2, [&]{
		for (int f=0; f<2; ++f) if (flags & (1u << f))
		{
			reserveOrNoMem( b.dBytes[ f], totals[ f] + 16);
			P.family[ f].*outBytes = (uint8_t*)b.dBytes[ f].ptr; P.family[ f].outCapacity = totals[ f];
		}
	});
	b.flags = flags; b.ndocs = call.ndocs;
	for (int f=0; f<2; ++f) { b.nrecords[ f] = call.finished[ f]; b.totals[ f] = (flags & (1u << f)) ? totals[ f] : 0; }
}

// plain copy of the buffers into the arrays of a host struct allocated for b.nrecords and b.totals
void fetchByteFamilies( const sp_matcher_ctx* c, const ByteFamilies& b, int32_t* status, char* const bytes[ 2], uint64_t* const offsets[ 2])
{
	if (b.ndocs) copySync( c->own, status, b.dStatus.ptr, b.ndocs*sizeof(int32_t), hipMemcpyDeviceToHost);
	for (int f=0; f<2; ++f) if (b.flags & (1u << f))
	{
		copySync( c->own, offsets[ f], b.dOffsets[ f].ptr, (b.nrecords[ f]+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (b.totals[ f]) copySync( c->own, bytes[ f], b.dBytes[ f].ptr, b.totals[ f], hipMemcpyDeviceToHost);
	}
}

// test hook: the bits of a term's hash that the device keeps (32 and more = all)
std::atomic<unsigned>& termHashBits() { static std::atomic<unsigned> bits( 32); return bits; }
// test hook: the bits of a radix digit of the partitions of the postings and of the positions
std::atomic<unsigned>& postingsDigitBits() { static std::atomic<unsigned> bits( POSTINGS_MAX_DIGIT_BITS); return bits; }

// diagnostics: whether a positions call records an event behind every launch
std::atomic<unsigned>& positionsLaunchEvents() { static std::atomic<unsigned> on( 0); return on; }

// ---- the sources of the terms and of the dictionary call: the results families of the values call (0) and of the text call (1)
// that `flags` selects, which must have run since the finish
struct TermSources
{
	const ByteFamilies* family[ 2]; uint32_t flags;
	bool selected( int s) const { return (flags & (1u << s)) != 0; }
	TermSources( const sp_matcher_ctx* c, uint32_t flags_) :family{ &c->prod.val, &c->prod.txt }, flags(flags_)
	{
		if (selected( 0) && !(family[ 0]->run.done && (family[ 0]->flags & SP_VALUE_RESULTS)))
			throw std::runtime_error( "no values of the results of the last finished batch (sp_matcher_ctx_finished_values_device with SP_VALUE_RESULTS)");
		if (selected( 1) && !(family[ 1]->run.done && (family[ 1]->flags & SP_TEXT_RESULTS)))
			throw std::runtime_error( "no text of the results of the last finished batch (sp_matcher_ctx_finished_text_device with SP_TEXT_RESULTS)");
	}
	// they are those of the `nresults` results of the finish
	void requireResults( uint64_t nresults) const
	{
		if (selected( 0) && family[ 0]->nrecords[ 0] != nresults) throw std::runtime_error( "the values are not those of the finished batch");
		if (selected( 1) && family[ 1]->nrecords[ 0] != nresults) throw std::runtime_error( "the text is not that of the finished batch");
	}
	// `stream` runs behind their placements, which nobody has waited for yet
	void waitFor( hipStream_t stream) const
	{
		for (int s=0; s<2; ++s) if (selected( s) && stream != family[ s]->run.stream) HIP_CHECK( hipStreamWaitEvent( stream, family[ s]->run.ev[ 1], 0));
	}
	// what TermsParams and DictParams name alike: the flags, the hash mask and the sources
	template <class PARAMS>
	void describe( PARAMS& P) const
	{
		const unsigned bits = termHashBits().load( std::memory_order_relaxed);
		P.hashMask = bits >= 32 ? 0xFFFFFFFFu : ((1u << bits) - 1u);
		describeSources( P);
	}
	// ... and what DictOrderParams names as they do: the flags and the sources
	template <class PARAMS>
	void describeSources( PARAMS& P) const
	{
		P.flags = flags;
		for (int s=0; s<2; ++s) if (selected( s))
		{
			const ByteFamilies& b = *family[ s];
			const TermSourceDevice S = { (const uint8_t*)b.dBytes[ 0].ptr, (const uint64_t*)b.dOffsets[ 0].ptr, b.totals[ 0], (const int32_t*)b.dStatus.ptr };
			P.source[ s] = S;
		}
	}
};

} // namespace

extern "C" {

// ---- the last device batch finished on the device: document order, `exclusive` applied, items without gaps (l2_finish.h)
int sp_matcher_ctx_batch_finish_device( sp_matcher_ctx_t* c, void* stream, sp_match_finished_batch_t* out)
{ return sp_matcher_ctx_batch_finish_device_ex( c, stream, 0, out); }

// flags: SP_FINISH_CANONICAL orders the results of every document by the tuple T of the header
int sp_matcher_ctx_batch_finish_device_ex( sp_matcher_ctx_t* c, void* stream_, uint32_t flags, sp_match_finished_batch_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		if (flags & ~(uint32_t)SP_FINISH_CANONICAL) throw std::runtime_error( "unknown finish flags");
		const bool canonical = (flags & SP_FINISH_CANONICAL) != 0;
		if (!c->haveBatch) throw std::runtime_error( "no batch to finish: no batch has run on this context");
		hipStream_t stream = (hipStream_t)stream_;
		HIP_CHECK( hipSetDevice( c->device));
		c->prod.drop();
		sp_matcher_ctx::Finished& fin = c->prod.fin;
		// the buffers are sized from what the batch counted: this read waits for the batch, the passes below do not
		HIP_CHECK( hipStreamSynchronize( c->lastStream));
		const BatchCounts counts = readCounts( c);
		const uint64_t devResults = counts.results, devItems = counts.items;
		const size_t ndocs = c->lastNdocs;
		const bool exclusive = c->inst->compiler.exclusive();
		fin.dResults.reserve( (devResults+1)*sizeof(sp_result_t));
		fin.dItems.reserve( (devItems+1)*sizeof(sp_result_item_t));
		if (c->io.withFormats)
		{
			fin.dResultFormat.reserve( (devResults+1)*sizeof(uint32_t));
			fin.dItemFormat.reserve( (devItems+1)*2*sizeof(uint32_t));
		}
		fin.dDocResultOffsets.reserve( (ndocs+1)*sizeof(uint64_t));
		fin.dDocItemOffsets.reserve( (ndocs+1)*sizeof(uint64_t));
		fin.dKept.reserve( (ndocs+1)*2*sizeof(uint32_t));
		if (!fin.dTotals.ptr) fin.dTotals.alloc( 2*sizeof(uint64_t));
		if (!fin.dCursor.ptr) fin.dCursor.alloc( 2*sizeof(uint32_t));
		if (exclusive) fin.dCovered.reserve( devResults+1);
		if (canonical)
		{
			for (int i=0; i<2; ++i)
			{
				fin.dSortKeys[ i].reserve( (devResults+1)*sizeof(uint64_t));
				fin.dSortIdx[ i].reserve( (devResults+1)*sizeof(uint32_t));
			}
			if (!fin.dSortCursor.ptr) fin.dSortCursor.alloc( sizeof(uint32_t));
		}
		// another stream than the batch's runs behind the batch (evStop closes every launch sequence, reruns included)
		fin.run.begin( stream, c->lastStream, c->evStop);
		hipEvent_t ev[ 5];
		fin.run.events( ev);
		HIP_CHECK( hipMemsetAsync( fin.dCursor.ptr, 0, 2*sizeof(uint32_t), stream));
		if (exclusive) HIP_CHECK( hipMemsetAsync( fin.dCovered.ptr, 0, devResults+1, stream));
		if (canonical) HIP_CHECK( hipMemsetAsync( fin.dSortCursor.ptr, 0, sizeof(uint32_t), stream));
		FinishParams F;
		std::memset( &F, 0, sizeof(F));
		F.results = (const uint32_t*)c->io.results.ptr(); F.items = (const uint32_t*)c->io.items.ptr();
		F.docRange = (const uint64_t*)c->io.dDocRange.ptr; F.docStatus = (const int32_t*)c->io.dDocStatus.ptr;
		F.resultFormat = (const uint32_t*)c->io.dResultFormat.ptr; F.itemFormat = (const uint32_t*)c->io.dItemFormat.ptr;
		F.nofResults = devResults; F.nofItems = devItems;
		F.ndocs = (uint32_t)ndocs; F.withFormats = c->io.withFormats ? 1u : 0u;
		F.exclusive = exclusive ? 1u : 0u; F.maxResultSize = c->inst->compiler.maxResultSize();
		F.covered = (uint8_t*)fin.dCovered.ptr; F.kept = (uint32_t*)fin.dKept.ptr; F.cursor = (uint32_t*)fin.dCursor.ptr;
		F.outResults = (uint32_t*)fin.dResults.ptr; F.outItems = (uint32_t*)fin.dItems.ptr;
		F.docResultOffsets = (uint64_t*)fin.dDocResultOffsets.ptr; F.docItemOffsets = (uint64_t*)fin.dDocItemOffsets.ptr;
		F.outResultFormat = (uint32_t*)fin.dResultFormat.ptr; F.outItemFormat = (uint32_t*)fin.dItemFormat.ptr;
		F.totals = (uint64_t*)fin.dTotals.ptr;
		if (canonical)
		{
			F.canonical = 1;
			for (int i=0; i<2; ++i) { F.sortKeys[ i] = (uint64_t*)fin.dSortKeys[ i].ptr; F.sortIdx[ i] = (uint32_t*)fin.dSortIdx[ i].ptr; }
			F.sortCursor = (uint32_t*)fin.dSortCursor.ptr;
		}
		HIP_CHECK( launchL2Finish( F, c->numCUs, stream, ev));
		fin.run.completed( stream); fin.canonical = canonical;
		if (out)
		{
			out->ndocs = ndocs;
			out->d_results = fin.dResults.ptr; out->d_items = fin.dItems.ptr;
			out->d_doc_result_offsets = fin.dDocResultOffsets.ptr; out->d_doc_item_offsets = fin.dDocItemOffsets.ptr;
			out->d_result_format = c->io.withFormats ? fin.dResultFormat.ptr : 0;
			out->d_item_format = c->io.withFormats ? fin.dItemFormat.ptr : 0;
			out->d_totals = fin.dTotals.ptr;
		}
	});
}

// plain copy of the finished buffers: nothing is regrouped or eliminated on the host
int sp_matcher_ctx_finished_fetch( sp_matcher_ctx_t* c, sp_match_batch_t* out)
{
	std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		const sp_matcher_ctx::Finished& fin = c->prod.fin;
		requireFinished( c);
		HIP_CHECK( hipSetDevice( c->device));
		HIP_CHECK( hipStreamSynchronize( fin.run.stream));
		const size_t ndocs = c->lastNdocs;
		uint64_t totals[ 2];
		copySync( c->own, totals, fin.dTotals.ptr, sizeof(totals), hipMemcpyDeviceToHost);
		allocMatchBatch( out, ndocs, totals[ 0], totals[ 1], c->io.withFormats);
		if (totals[ 0]) copySync( c->own, out->results, fin.dResults.ptr, totals[ 0]*sizeof(sp_result_t), hipMemcpyDeviceToHost);
		if (totals[ 1]) copySync( c->own, out->items, fin.dItems.ptr, totals[ 1]*sizeof(sp_result_item_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->doc_result_offsets, fin.dDocResultOffsets.ptr, (ndocs+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (ndocs)
		{
			copySync( c->own, out->doc_stats, c->io.dDocStats.ptr, ndocs*4*sizeof(uint64_t), hipMemcpyDeviceToHost);
			copySync( c->own, out->doc_status, c->io.dDocStatus.ptr, ndocs*sizeof(int32_t), hipMemcpyDeviceToHost);
		}
		if (c->io.withFormats)
		{
			if (totals[ 0]) copySync( c->own, out->result_format, fin.dResultFormat.ptr, totals[ 0]*sizeof(uint32_t), hipMemcpyDeviceToHost);
			if (totals[ 1]) copySync( c->own, out->item_format, fin.dItemFormat.ptr, totals[ 1]*2*sizeof(uint32_t), hipMemcpyDeviceToHost);
		}
	});
}

// durations of the three passes of the last finish in milliseconds (HIP events on its stream)
int sp_matcher_ctx_last_finish_ms( sp_matcher_ctx_t* c, double* count_ms, double* offsets_ms, double* place_ms)
{
	const sp_matcher_ctx::Finished& fin = c->prod.fin;
	*offsets_ms = *place_ms = -1.0;
	// (a canonical finish sorts between the offsets and the placement: the placement starts at ev[4] then)
	int rc = fin.run.ms( 0, 1, count_ms);
	if (rc == SP_OK) rc = fin.run.ms( 1, 2, offsets_ms);
	if (rc == SP_OK) rc = fin.run.ms( fin.canonical ? 4 : 2, 3, place_ms);
	return rc;
}

// duration of the sorting pass of the last finish (0.0 after a finish without SP_FINISH_CANONICAL)
int sp_matcher_ctx_last_finish_sort_ms( sp_matcher_ctx_t* c, double* sort_ms)
{
	const sp_matcher_ctx::Finished& fin = c->prod.fin;
	if (fin.run.evValid && !fin.canonical) { *sort_ms = 0.0; return SP_OK; }
	return fin.run.ms( 2, 4, sort_ms);
}

uint32_t sp_matcher_finish_sort_tile(void) { return FINISH_SORT_TILE; }

// ---- the text that the results and items of the finished batch cover, gathered on the device (l2_text.h)
int sp_matcher_ctx_finished_text_device( sp_matcher_ctx_t* c, const sp_text_source_t* src, uint32_t flags, void* stream, sp_match_text_batch_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		if (!flags || (flags & ~(uint32_t)(SP_TEXT_RESULTS | SP_TEXT_ITEMS))) throw std::runtime_error( "unknown or no text flags");
		checkTextSource( c, src);
		ByteFamilies& t = c->prod.txt;
		ProductCall call( c, t.run, stream);
		TextParams P;
		beginByteFamilies( call, t, flags, src, P, []( TextFamily& F, uint32_t* work, uint64_t* docOffsets, uint64_t* offsets, int){
			F.spanWork = work; F.docTextOffsets = docOffsets; F.spanOffsets = offsets;
		});
		byteFamilyPasses( call, t, flags, P, &TextFamily::outText, launchL2TextCount, launchL2TextPlace);
		if (out)
		{
			out->ndocs = call.ndocs;
			if (flags & SP_TEXT_RESULTS) { out->d_result_text = t.dBytes[ 0].ptr; out->d_result_text_offsets = t.dOffsets[ 0].ptr; }
			if (flags & SP_TEXT_ITEMS) { out->d_item_text = t.dBytes[ 1].ptr; out->d_item_text_offsets = t.dOffsets[ 1].ptr; }
			out->d_doc_text_status = t.dStatus.ptr; out->d_totals = t.dTotals.ptr;
		}
	});
}

// plain copy of the text buffers
int sp_matcher_ctx_finished_text_fetch( sp_matcher_ctx_t* c, sp_match_text_t* out)
{
	const ByteFamilies& t = c->prod.txt;
	return fetchProduct( c, t.run, "no text of the last batch of this context (sp_matcher_ctx_finished_text_device)", out, sp_match_text_free, [&]{
		allocMatchText( out, t.ndocs, t.nrecords[ 0], t.nrecords[ 1], t.flags);
		out->totals[ 0] = t.totals[ 0]; out->totals[ 1] = t.totals[ 1];
		allocMatchTextBytes( out, t.flags);
		char* const text[ 2] = {out->result_text, out->item_text};
		uint64_t* const offsets[ 2] = {out->result_text_offsets, out->item_text_offsets};
		fetchByteFamilies( c, t, out->doc_text_status, text, offsets);
	});
}

// duration of the passes of the last text call in milliseconds (HIP events on its stream)
int sp_matcher_ctx_last_text_ms( sp_matcher_ctx_t* c, double* ms) { return c->prod.txt.run.ms( 0, 1, ms); }

uint32_t sp_matcher_text_long_span(void) { return TEXT_LONG_SPAN; }

// ---- the values of the format strings of the finished batch, built on the device (l2_values.h)
int sp_matcher_ctx_finished_values_device( sp_matcher_ctx_t* c, const sp_text_source_t* src, uint32_t flags, void* stream, sp_match_values_batch_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		if (!flags || (flags & ~(uint32_t)(SP_VALUE_RESULTS | SP_VALUE_ITEMS))) throw std::runtime_error( "unknown or no value flags");
		checkTextSource( c, src);
		const FormatTable& table = c->inst->formats();
		if (!table.error.empty()) throw std::runtime_error( table.error);
		const sp_matcher_ctx::Finished& fin = c->prod.fin;
		sp_matcher_ctx::Values& v = c->prod.val;
		ProductCall call( c, v.run, stream);
		if (!v.uploaded)
		{
			// the format table: once per context
			reserveOrNoMem( v.dFmtParts, (table.fmtParts.size()+1)*sizeof(uint32_t));
			reserveOrNoMem( v.dParts, (table.parts.size()+1)*sizeof(uint32_t));
			reserveOrNoMem( v.dPool, table.pool.size()+16);
			copySync( c->own, v.dFmtParts.ptr, table.fmtParts.data(), table.fmtParts.size()*sizeof(uint32_t), hipMemcpyHostToDevice);
			if (!table.parts.empty()) copySync( c->own, v.dParts.ptr, table.parts.data(), table.parts.size()*sizeof(uint32_t), hipMemcpyHostToDevice);
			if (!table.pool.empty()) copySync( c->own, v.dPool.ptr, table.pool.data(), table.pool.size(), hipMemcpyHostToDevice);
			v.poolBytes = (uint32_t)table.pool.size();
			v.uploaded = true;
		}
		ValuesParams P;
		beginByteFamilies( call, v, flags, src, P, [&]( ValuesFamily& F, uint32_t* work, uint64_t* docOffsets, uint64_t* offsets, int f){
			F.valueWork = work; F.docValueOffsets = docOffsets; F.valueOffsets = offsets;
			F.format = (const uint32_t*)(f ? fin.dItemFormat.ptr : fin.dResultFormat.ptr);
		});
		// a matcher without format strings has no format arrays: every value is empty, the passes only lay out the offsets
		const bool withFormats = c->io.withFormats && table.count;
		for (int f=0; f<2; ++f) if ((flags & (1u << f)) && !withFormats)
		{
			HIP_CHECK( hipMemsetAsync( v.dOffsets[ f].ptr, 0, (call.finished[ f]+1)*sizeof(uint64_t), call.stream));
		}
		P.families = withFormats ? flags : 0;
		P.fmtParts = (const uint32_t*)v.dFmtParts.ptr; P.parts = (const uint32_t*)v.dParts.ptr; P.pool = (const uint8_t*)v.dPool.ptr;
		P.formatCount = table.count; P.poolBytes = v.poolBytes;
		P.items = (const uint32_t*)fin.dItems.ptr; P.itemFormat = (const uint32_t*)fin.dItemFormat.ptr;
		P.docItemOffsets = (const uint64_t*)fin.dDocItemOffsets.ptr; P.nitems = call.finished[ 1];
		byteFamilyPasses( call, v, flags, P, &ValuesFamily::outValues, launchL2ValuesCount, launchL2ValuesPlace);
		if (out)
		{
			out->ndocs = call.ndocs;
			if (flags & SP_VALUE_RESULTS) { out->d_result_values = v.dBytes[ 0].ptr; out->d_result_value_offsets = v.dOffsets[ 0].ptr; }
			if (flags & SP_VALUE_ITEMS) { out->d_item_values = v.dBytes[ 1].ptr; out->d_item_value_offsets = v.dOffsets[ 1].ptr; }
			out->d_doc_value_status = v.dStatus.ptr; out->d_totals = v.dTotals.ptr;
		}
	});
}

// plain copy of the value buffers
int sp_matcher_ctx_finished_values_fetch( sp_matcher_ctx_t* c, sp_match_values_t* out)
{
	const ByteFamilies& v = c->prod.val;
	return fetchProduct( c, v.run, "no values of the last batch of this context (sp_matcher_ctx_finished_values_device)", out, sp_match_values_free, [&]{
		allocMatchValues( out, v.ndocs, v.nrecords[ 0], v.nrecords[ 1], v.flags);
		out->totals[ 0] = v.totals[ 0]; out->totals[ 1] = v.totals[ 1];
		allocMatchValuesBytes( out, v.flags);
		char* const bytes[ 2] = {out->result_values, out->item_values};
		uint64_t* const offsets[ 2] = {out->result_value_offsets, out->item_value_offsets};
		fetchByteFamilies( c, v, out->doc_value_status, bytes, offsets);
	});
}

// duration of the passes of the last values call in milliseconds (HIP events on its stream)
int sp_matcher_ctx_last_values_ms( sp_matcher_ctx_t* c, double* ms) { return c->prod.val.run.ms( 0, 1, ms); }

uint32_t sp_matcher_value_max_depth(void) { return VALUE_MAX_DEPTH; }

// the same rule over host arrays (result_values.hpp)
int sp_match_batch_values( const sp_matcher_t* m, const sp_match_batch_t* mb, const char* text, uint64_t nbytes, const uint64_t* seg_offsets,
			   size_t nseg, const uint64_t* doc_seg_offsets, uint32_t flags, sp_match_values_t* out, char* err, size_t errsize)
{
	return hostProduct( out, sp_match_values_free, err, errsize, [&]{
		if (!m) throw std::runtime_error( "no matcher");
		if (!mb) throw std::runtime_error( "no batch");
		const TextSource S = { text, nbytes, seg_offsets, nseg, doc_seg_offsets };
		matchBatchValues( m->formats(), *mb, S, flags, out);
	});
}

// ---- the pattern frequencies of the finished batch, summed on the device (l2_freq.h)
int sp_matcher_ctx_finished_pattern_freq_device( sp_matcher_ctx_t* c, void* stream, sp_pattern_freq_device_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		const sp_matcher_ctx::Finished& fin = c->prod.fin;
		sp_matcher_ctx::Freq& q = c->prod.frq;
		// (every result index is checked against the total of the finish)
		ProductCall call( c, q.run, stream);
		const size_t ndocs = call.ndocs;
		const uint32_t bound = sp_matcher_handle_bound( c->inst);
		reserveOrNoMem( q.dDocCount, (ndocs+1)*sizeof(uint32_t));
		reserveOrNoMem( q.dDocMeta, (ndocs+1)*4*sizeof(uint32_t));
		reserveOrNoMem( q.dDocOffsets, (ndocs+1)*sizeof(uint64_t));
		reserveOrNoMem( q.dHandleResults, (size_t)bound*sizeof(uint64_t));
		reserveOrNoMem( q.dHandleDocs, (size_t)bound*sizeof(uint32_t));
		call.begin( q.dStatus, q.dTotals, 1, q.dCursor, 2);
		HIP_CHECK( hipMemsetAsync( q.dHandleResults.ptr, 0, (size_t)bound*sizeof(uint64_t), call.stream));
		HIP_CHECK( hipMemsetAsync( q.dHandleDocs.ptr, 0, (size_t)bound*sizeof(uint32_t), call.stream));
		FreqParams P;
		std::memset( &P, 0, sizeof(P));
		P.results = (const uint32_t*)fin.dResults.ptr; P.docOffsets = (const uint64_t*)fin.dDocResultOffsets.ptr;
		P.nresults = call.finished[ 0]; P.ndocs = (uint32_t)ndocs; P.handleBound = bound;
		P.docCount = (uint32_t*)q.dDocCount.ptr; P.docMeta = (uint32_t*)q.dDocMeta.ptr; P.cursor = (uint32_t*)q.dCursor.ptr;
		P.docStatus = (int32_t*)q.dStatus.ptr; P.docFreqOffsets = (uint64_t*)q.dDocOffsets.ptr; P.total = (uint64_t*)q.dTotals.ptr;
		P.handleResults = (uint64_t*)q.dHandleResults.ptr; P.handleDocs = (uint32_t*)q.dHandleDocs.ptr;
		uint64_t total = 0;
		call.passes( P, launchL2FreqCount, launchL2FreqPlace, q.dTotals, &total, 1, [&]{
			reserveOrNoMem( q.dRecords, (total+1)*sizeof(sp_pattern_freq_t));
			P.records = (uint32_t*)q.dRecords.ptr; P.capacity = total;
			if (total) HIP_CHECK( hipMemsetAsync( q.dRecords.ptr, 0, total*sizeof(sp_pattern_freq_t), call.stream));
		});
		q.ndocs = ndocs; q.handleBound = bound; q.total = total;
		if (out)
		{
			out->ndocs = ndocs; out->handle_bound = bound;
			out->d_records = q.dRecords.ptr; out->d_doc_offsets = q.dDocOffsets.ptr; out->d_doc_freq_status = q.dStatus.ptr;
			out->d_handle_results = q.dHandleResults.ptr; out->d_handle_docs = q.dHandleDocs.ptr; out->d_totals = q.dTotals.ptr;
		}
	});
}

// plain copy of the frequency buffers
int sp_matcher_ctx_finished_pattern_freq_fetch( sp_matcher_ctx_t* c, sp_pattern_freq_batch_t* out)
{
	const sp_matcher_ctx::Freq& q = c->prod.frq;
	return fetchProduct( c, q.run, "no pattern frequencies of the last batch of this context (sp_matcher_ctx_finished_pattern_freq_device)", out, sp_pattern_freq_batch_free, [&]{
		allocPatternFreq( out, q.ndocs, q.handleBound);
		allocPatternFreqRecords( out, q.total);
		if (q.total) copySync( c->own, out->records, q.dRecords.ptr, q.total*sizeof(sp_pattern_freq_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->doc_offsets, q.dDocOffsets.ptr, (q.ndocs+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (q.ndocs) copySync( c->own, out->doc_freq_status, q.dStatus.ptr, q.ndocs*sizeof(int32_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->handle_results, q.dHandleResults.ptr, (size_t)q.handleBound*sizeof(uint64_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->handle_docs, q.dHandleDocs.ptr, (size_t)q.handleBound*sizeof(uint32_t), hipMemcpyDeviceToHost);
	});
}

// duration of the passes of the last frequency call in milliseconds (HIP events on its stream)
int sp_matcher_ctx_last_pattern_freq_ms( sp_matcher_ctx_t* c, double* ms) { return c->prod.frq.run.ms( 0, 1, ms); }

uint32_t sp_matcher_pattern_freq_window(void) { return FREQ_WINDOW; }

// ---- the index terms of the finished batch, grouped on the device (l2_terms.h)
void sp_test_term_hash_bits( unsigned bits) { termHashBits().store( bits, std::memory_order_relaxed); }

int sp_matcher_ctx_finished_terms_device( sp_matcher_ctx_t* c, uint32_t flags, void* stream, sp_match_terms_device_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		if (!flags || (flags & ~(uint32_t)(SP_TERM_VALUES | SP_TERM_TEXT))) throw std::runtime_error( "unknown or no term flags");
		requireFinished( c);
		const sp_matcher_ctx::Finished& fin = c->prod.fin;
		const TermSources sources( c, flags);
		sp_matcher_ctx::Terms& t = c->prod.trm;
		c->prod.dropDictionary();		// (a dictionary is that of the terms it was built from)
		// (every result index is checked against the total of the finish)
		ProductCall call( c, t.run, stream);
		const size_t ndocs = call.ndocs;
		const uint32_t bound = sp_matcher_handle_bound( c->inst);
		const uint64_t nresults = call.finished[ 0];
		sources.requireResults( nresults);
		const unsigned waves = l2TermsWaves( ndocs, c->numCUs);
		reserveOrNoMem( t.dLeader, (nresults+1)*sizeof(uint32_t));
		reserveOrNoMem( t.dTable, (nresults+1)*2*sizeof(uint32_t));
		reserveOrNoMem( t.dResultTerm, (nresults+1)*sizeof(uint32_t));
		reserveOrNoMem( t.dHistogram, (size_t)waves*bound*sizeof(uint32_t));
		reserveOrNoMem( t.dDocCount, (ndocs+1)*sizeof(uint32_t));
		reserveOrNoMem( t.dDocOffsets, (ndocs+1)*sizeof(uint64_t));
		// behind the finish, and behind the values and the text call, whose placements nobody has waited for yet
		call.begin( t.dStatus, t.dTotals, 1, t.dCursor, 2);
		sources.waitFor( call.stream);
		TermsParams P;
		std::memset( &P, 0, sizeof(P));
		P.results = (const uint32_t*)fin.dResults.ptr; P.docOffsets = (const uint64_t*)fin.dDocResultOffsets.ptr;
		P.resultFormat = c->io.withFormats ? (const uint32_t*)fin.dResultFormat.ptr : 0;
		P.nresults = nresults; P.ndocs = (uint32_t)ndocs; P.handleBound = bound;
		sources.describe( P);
		P.leader = (uint32_t*)t.dLeader.ptr; P.table = (uint32_t*)t.dTable.ptr; P.histogram = (uint32_t*)t.dHistogram.ptr;
		P.docCount = (uint32_t*)t.dDocCount.ptr; P.cursor = (uint32_t*)t.dCursor.ptr;
		P.docStatus = (int32_t*)t.dStatus.ptr; P.docTermOffsets = (uint64_t*)t.dDocOffsets.ptr; P.total = (uint64_t*)t.dTotals.ptr;
		P.resultTerm = (uint32_t*)t.dResultTerm.ptr;
		uint64_t total = 0;
		call.passes( P, launchL2TermsCount, launchL2TermsPlace, t.dTotals, &total, 1, [&]{
			reserveOrNoMem( t.dRecords, (total+1)*sizeof(sp_match_term_t));
			P.records = (uint32_t*)t.dRecords.ptr; P.capacity = total;
		});
		t.ndocs = ndocs; t.handleBound = bound; t.flags = flags; t.nresults = nresults; t.total = total;
		if (out)
		{
			out->ndocs = ndocs; out->handle_bound = bound; out->flags = flags;
			out->d_records = t.dRecords.ptr; out->d_doc_term_offsets = t.dDocOffsets.ptr; out->d_result_term = t.dResultTerm.ptr;
			out->d_doc_term_status = t.dStatus.ptr; out->d_totals = t.dTotals.ptr;
		}
	});
}

// plain copy of the term buffers
int sp_matcher_ctx_finished_terms_fetch( sp_matcher_ctx_t* c, sp_match_terms_t* out)
{
	const sp_matcher_ctx::Terms& t = c->prod.trm;
	return fetchProduct( c, t.run, "no terms of the last batch of this context (sp_matcher_ctx_finished_terms_device)", out, sp_match_terms_free, [&]{
		allocMatchTerms( out, t.ndocs, t.nresults, t.handleBound, t.flags);
		allocMatchTermRecords( out, t.total);
		if (t.total) copySync( c->own, out->records, t.dRecords.ptr, t.total*sizeof(sp_match_term_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->doc_term_offsets, t.dDocOffsets.ptr, (t.ndocs+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (t.nresults) copySync( c->own, out->result_term, t.dResultTerm.ptr, t.nresults*sizeof(uint32_t), hipMemcpyDeviceToHost);
		if (t.ndocs) copySync( c->own, out->doc_term_status, t.dStatus.ptr, t.ndocs*sizeof(int32_t), hipMemcpyDeviceToHost);
	});
}

// duration of the passes of the last terms call in milliseconds (HIP events on its stream)
int sp_matcher_ctx_last_terms_ms( sp_matcher_ctx_t* c, double* ms) { return c->prod.trm.run.ms( 0, 1, ms); }

uint32_t sp_matcher_term_tile(void) { return TERM_TILE; }

// ---- the dictionary of the terms of the finished batch, built on the device (l2_dict.h)
int sp_matcher_ctx_finished_dictionary_device( sp_matcher_ctx_t* c, void* stream, sp_match_dictionary_device_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		requireFinished( c);
		const sp_matcher_ctx::Finished& fin = c->prod.fin;
		const sp_matcher_ctx::Terms& t = c->prod.trm;
		if (!t.run.done) throw std::runtime_error( "no terms of the last finished batch (sp_matcher_ctx_finished_terms_device)");
		const uint32_t flags = t.flags;
		const TermSources sources( c, flags);
		sp_matcher_ctx::Dict& q = c->prod.dct;
		c->prod.dropPostings();			// (postings are those of the dictionary they were built from)
		ProductCall call( c, q.run, stream);
		const size_t ndocs = call.ndocs;
		const uint64_t nresults = call.finished[ 0], nterms = t.total;
		if (t.ndocs != ndocs || t.nresults != nresults) throw std::runtime_error( "the terms are not those of the finished batch");
		sources.requireResults( nresults);
		if (nterms >= 0xFFFFFFFFull) throw std::runtime_error( "2^32 - 1 term records or more: the indices of a dictionary are 32 bits");
		const uint32_t bound = t.handleBound, slots = l2DictTableSlots( nterms);
		reserveOrNoMem( q.dTable, (size_t)slots*sizeof(uint32_t));
		reserveOrNoMem( q.dSlot, (nterms+1)*sizeof(uint32_t));
		reserveOrNoMem( q.dLeader, (nterms+1)*sizeof(uint32_t));
		reserveOrNoMem( q.dTermDict, (nterms+1)*sizeof(uint32_t));
		reserveOrNoMem( q.dDocOffsets, (ndocs+1)*sizeof(uint64_t));
		reserveOrNoMem( q.dHandleTerms, ((size_t)bound+1)*sizeof(uint32_t));
		// behind the finish, and behind the terms call and the calls whose buffers the terms point into, whose placements nobody
		// has waited for yet.  (The entries first seen per document are counted where every other product keeps a status.)
		call.begin( q.dDocCount, q.dTotals, 1, q.dCursor, 4);
		if (call.stream != t.run.stream) HIP_CHECK( hipStreamWaitEvent( call.stream, t.run.ev[ 1], 0));
		sources.waitFor( call.stream);
		HIP_CHECK( hipMemsetAsync( q.dTable.ptr, 0xFF, (size_t)slots*sizeof(uint32_t), call.stream));
		HIP_CHECK( hipMemsetAsync( q.dHandleTerms.ptr, 0, ((size_t)bound+1)*sizeof(uint32_t), call.stream));
		DictParams P;
		std::memset( &P, 0, sizeof(P));
		P.terms = (const uint32_t*)t.dRecords.ptr; P.docTermOffsets = (const uint64_t*)t.dDocOffsets.ptr; P.nterms = nterms;
		P.docOffsets = (const uint64_t*)fin.dDocResultOffsets.ptr;
		P.resultFormat = c->io.withFormats ? (const uint32_t*)fin.dResultFormat.ptr : 0;
		P.nresults = nresults; P.ndocs = (uint32_t)ndocs; P.handleBound = bound;
		sources.describe( P);
		P.table = (uint32_t*)q.dTable.ptr; P.tableSlots = slots; P.slot = (uint32_t*)q.dSlot.ptr; P.leader = (uint32_t*)q.dLeader.ptr;
		P.docCount = (uint32_t*)q.dDocCount.ptr; P.cursor = (uint32_t*)q.dCursor.ptr;
		P.docDictOffsets = (uint64_t*)q.dDocOffsets.ptr; P.total = (uint64_t*)q.dTotals.ptr;
		P.termDict = (uint32_t*)q.dTermDict.ptr; P.handleTerms = (uint32_t*)q.dHandleTerms.ptr;
		uint64_t total = 0;
		call.passes( P, launchL2DictCount, launchL2DictPlace, q.dTotals, &total, 1, [&]{
			reserveOrNoMem( q.dRecords, (total+1)*sizeof(sp_dict_term_t));
			P.records = (uint32_t*)q.dRecords.ptr; P.capacity = total;
		});
		q.ndocs = ndocs; q.handleBound = bound; q.flags = flags; q.nterms = nterms; q.total = total;
		if (out)
		{
			out->ndocs = ndocs; out->handle_bound = bound; out->flags = flags;
			out->d_records = q.dRecords.ptr; out->d_term_dict = q.dTermDict.ptr; out->d_doc_dict_offsets = q.dDocOffsets.ptr;
			out->d_handle_terms = q.dHandleTerms.ptr; out->d_totals = q.dTotals.ptr;
		}
	});
}

// plain copy of the dictionary buffers
int sp_matcher_ctx_finished_dictionary_fetch( sp_matcher_ctx_t* c, sp_match_dictionary_t* out)
{
	const sp_matcher_ctx::Dict& q = c->prod.dct;
	return fetchProduct( c, q.run, "no dictionary of the last terms of this context (sp_matcher_ctx_finished_dictionary_device)", out, sp_match_dictionary_free, [&]{
		allocMatchDictionary( out, q.ndocs, q.nterms, q.handleBound, q.flags);
		allocMatchDictionaryRecords( out, q.total);
		if (q.total) copySync( c->own, out->records, q.dRecords.ptr, q.total*sizeof(sp_dict_term_t), hipMemcpyDeviceToHost);
		if (q.nterms) copySync( c->own, out->term_dict, q.dTermDict.ptr, q.nterms*sizeof(uint32_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->doc_dict_offsets, q.dDocOffsets.ptr, (q.ndocs+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (q.handleBound) copySync( c->own, out->handle_terms, q.dHandleTerms.ptr, (size_t)q.handleBound*sizeof(uint32_t), hipMemcpyDeviceToHost);
	});
}

// duration of the five launches of the last dictionary call in milliseconds (HIP events on its stream; the memsets that clear the
// table and handle_terms are enqueued before the first event)
int sp_matcher_ctx_last_dictionary_ms( sp_matcher_ctx_t* c, double* ms) { return c->prod.dct.run.ms( 0, 1, ms); }

// ---- the order of the dictionary of the finished batch, sorted on the device (l2_dictorder.h)
int sp_matcher_ctx_finished_dictionary_order_device( sp_matcher_ctx_t* c, void* stream, sp_match_dictionary_order_device_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		requireFinished( c);
		const sp_matcher_ctx::Finished& fin = c->prod.fin;
		const sp_matcher_ctx::Terms& t = c->prod.trm;
		const sp_matcher_ctx::Dict& d = c->prod.dct;
		if (!t.run.done || !d.run.done) throw std::runtime_error( "no dictionary of the last terms of the last finished batch (sp_matcher_ctx_finished_dictionary_device)");
		const TermSources sources( c, d.flags);
		sp_matcher_ctx::DictOrder& q = c->prod.ord;
		c->prod.dropOrder();			// (term blocks are those of the order they were built from)
		// (the dictionary call waited for ndict and knows N: nothing is waited for here)
		ProductCall call( c, q.run, stream, ProductCall::Sized());
		const size_t ndocs = call.ndocs;
		const uint64_t nterms = d.nterms, ndict = d.total, nresults = t.nresults;
		if (d.ndocs != ndocs || t.ndocs != ndocs || t.total != nterms) throw std::runtime_error( "the dictionary is not that of the terms of the finished batch");
		if (nterms >= 0xFFFFFFFFull || ndict > nterms) throw std::runtime_error( "a dictionary of more entries than term records, or of 2^32 - 1 records or more");
		sources.requireResults( nresults);
		const uint32_t bound = d.handleBound;
		reserveOrNoMem( q.dOrder, (ndict+1)*sizeof(uint32_t));
		reserveOrNoMem( q.dRank, (ndict+1)*sizeof(uint32_t));
		reserveOrNoMem( q.dPrefixBytes, (ndict+1)*sizeof(uint32_t));
		reserveOrNoMem( q.dHandleOffsets, ((size_t)bound+1)*sizeof(uint64_t));
		for (int i=0; i<2; ++i)
		{
			reserveOrNoMem( q.dKeys[ i], (ndict+1)*sizeof(uint64_t));
			reserveOrNoMem( q.dIndex[ i], (ndict+1)*sizeof(uint32_t));
		}
		reserveOrNoMem( q.dValueAt, (ndict+1)*sizeof(uint64_t));
		reserveOrNoMem( q.dValueLen, (ndict+1)*sizeof(uint32_t));
		// behind the dictionary, whose placement nobody has waited for yet; that runs behind the terms, their sources and the finish
		call.beginBehind( d.run.stream, d.run.ev[ 1], q.dTotals, 1, q.dCursor, DICTORDER_CURSORS);
		sources.waitFor( call.stream);
		HIP_CHECK( hipMemsetAsync( q.dRank.ptr, 0xFF, (ndict+1)*sizeof(uint32_t), call.stream));
		DictOrderParams P;
		std::memset( &P, 0, sizeof(P));
		P.dictRecords = (const uint32_t*)d.dRecords.ptr; P.handleTerms = (const uint32_t*)d.dHandleTerms.ptr;
		P.terms = (const uint32_t*)t.dRecords.ptr; P.docTermOffsets = (const uint64_t*)t.dDocOffsets.ptr;
		P.docOffsets = (const uint64_t*)fin.dDocResultOffsets.ptr;
		P.resultFormat = c->io.withFormats ? (const uint32_t*)fin.dResultFormat.ptr : 0;
		P.nterms = nterms; P.nresults = nresults; P.ndict = (uint32_t)ndict; P.ndocs = (uint32_t)ndocs; P.handleBound = bound;
		sources.describeSources( P);
		P.tiles = l2DictOrderTiles( ndict); P.levels = l2DictOrderLevels( ndict);
		for (int i=0; i<2; ++i) { P.keys[ i] = (uint64_t*)q.dKeys[ i].ptr; P.index[ i] = (uint32_t*)q.dIndex[ i].ptr; }
		P.valueAt = (uint64_t*)q.dValueAt.ptr; P.valueLen = (uint32_t*)q.dValueLen.ptr; P.cursor = (uint32_t*)q.dCursor.ptr;
		P.order = (uint32_t*)q.dOrder.ptr; P.rank = (uint32_t*)q.dRank.ptr; P.prefixBytes = (uint32_t*)q.dPrefixBytes.ptr;
		P.handleOffsets = (uint64_t*)q.dHandleOffsets.ptr; P.total = (uint64_t*)q.dTotals.ptr;
		HIP_CHECK( hipEventRecord( q.run.ev[ 0], call.stream));
		HIP_CHECK( launchL2DictOrder( P, c->numCUs, call.stream));
		HIP_CHECK( hipEventRecord( q.run.ev[ 1], call.stream));
		q.run.completed( call.stream);
		q.ndict = ndict; q.handleBound = bound;
		if (out)
		{
			out->ndict = (size_t)ndict; out->handle_bound = bound;
			out->d_order = q.dOrder.ptr; out->d_rank = q.dRank.ptr; out->d_prefix_bytes = q.dPrefixBytes.ptr;
			out->d_handle_offsets = q.dHandleOffsets.ptr; out->d_totals = q.dTotals.ptr;
		}
	});
}

// plain copy of the order's buffers
int sp_matcher_ctx_finished_dictionary_order_fetch( sp_matcher_ctx_t* c, sp_match_dictionary_order_t* out)
{
	const sp_matcher_ctx::DictOrder& q = c->prod.ord;
	return fetchProduct( c, q.run, "no order of the last dictionary of this context (sp_matcher_ctx_finished_dictionary_order_device)", out, sp_match_dictionary_order_free, [&]{
		allocMatchDictionaryOrder( out, q.ndict, q.handleBound);
		if (q.ndict)
		{
			copySync( c->own, out->order, q.dOrder.ptr, q.ndict*sizeof(uint32_t), hipMemcpyDeviceToHost);
			copySync( c->own, out->rank, q.dRank.ptr, q.ndict*sizeof(uint32_t), hipMemcpyDeviceToHost);
			copySync( c->own, out->prefix_bytes, q.dPrefixBytes.ptr, q.ndict*sizeof(uint32_t), hipMemcpyDeviceToHost);
		}
		copySync( c->own, out->handle_offsets, q.dHandleOffsets.ptr, ((size_t)q.handleBound+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->totals, q.dTotals.ptr, sizeof(uint64_t), hipMemcpyDeviceToHost);
	});
}

// duration of the launches of the last order call in milliseconds (HIP events on its stream; the memsets that clear the cursor
// and the total and fill the rank are enqueued before the first event)
int sp_matcher_ctx_last_dictionary_order_ms( sp_matcher_ctx_t* c, double* ms) { return c->prod.ord.run.ms( 0, 1, ms); }

uint32_t sp_matcher_dictionary_order_tile(void) { return DICTORDER_TILE; }

// ---- the term blocks of the order of the finished batch, coded on the device (l2_termblocks.h)
int sp_matcher_ctx_finished_term_blocks_device( sp_matcher_ctx_t* c, void* stream, sp_match_term_blocks_device_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		requireFinished( c);
		const sp_matcher_ctx::Dict& d = c->prod.dct;
		const sp_matcher_ctx::DictOrder& o = c->prod.ord;
		if (!c->prod.trm.run.done || !d.run.done || !o.run.done)
			throw std::runtime_error( "no order of the last dictionary of the last finished batch (sp_matcher_ctx_finished_dictionary_order_device)");
		const TermSources sources( c, d.flags);
		sp_matcher_ctx::TermBlocks& q = c->prod.blk;
		// (the dictionary call waited for ndict: the one wait of this call is for nbytes)
		ProductCall call( c, q.run, stream, ProductCall::Sized());
		const uint64_t ndict = d.total;
		if (o.ndict != ndict || ndict >= 0xFFFFFFFFull) throw std::runtime_error( "the order is not that of the dictionary of the finished batch");
		const uint32_t B = termBlockEntries();
		const uint64_t nblocks = l2TermBlocksCount( ndict, B);
		reserveOrNoMem( q.dBlockOffsets, (nblocks+1)*sizeof(uint64_t));
		reserveOrNoMem( q.dBlockHandles, (nblocks+1)*sizeof(uint32_t));
		reserveOrNoMem( q.dBlockSize, (nblocks+1)*sizeof(uint64_t));
		// behind the order, which nobody has waited for yet; that runs behind the dictionary, the terms, their sources and the finish
		call.beginBehind( o.run.stream, o.run.ev[ 1], q.dTotals, 4, q.dCursor, 1);
		sources.waitFor( call.stream);
		TermBlocksParams P;
		std::memset( &P, 0, sizeof(P));
		P.dictRecords = (const uint32_t*)d.dRecords.ptr; P.order = (const uint32_t*)o.dOrder.ptr; P.prefixBytes = (const uint32_t*)o.dPrefixBytes.ptr;
		P.valueAt = (const uint64_t*)o.dValueAt.ptr; P.valueLen = (const uint32_t*)o.dValueLen.ptr;
		sources.describeSources( P);
		P.ndict = (uint32_t)ndict; P.blockEntries = B; P.nblocks = (uint32_t)nblocks;
		P.blockSize = (uint64_t*)q.dBlockSize.ptr; P.blockOffsets = (uint64_t*)q.dBlockOffsets.ptr; P.blockHandles = (uint32_t*)q.dBlockHandles.ptr;
		P.totals = (uint64_t*)q.dTotals.ptr;
		uint64_t totals[ 4] = { 0, 0, B, 0};
		if (ndict)
		{
			call.passes( P, launchL2TermBlocksCount, launchL2TermBlocksPlace, q.dTotals, totals, 4, [&]{
				reserveOrNoMem( q.dBytes, totals[ 1] + 16);
				P.bytes = (uint8_t*)q.dBytes.ptr; P.capacity = totals[ 1];
			});
		}
		else
		{
			// nothing to code, nothing to launch: block_offsets = [0], the totals {0, 0, B, 0}
			HIP_CHECK( hipEventRecord( q.run.ev[ 0], call.stream));
			HIP_CHECK( hipMemsetAsync( q.dBlockOffsets.ptr, 0, sizeof(uint64_t), call.stream));
			HIP_CHECK( hipMemsetD32Async( (hipDeviceptr_t)((uint64_t*)q.dTotals.ptr + 2), (int)B, 1, call.stream));
			HIP_CHECK( hipEventRecord( q.run.ev[ 1], call.stream));
			q.run.completed( call.stream);
		}
		q.ndict = ndict; q.nblocks = nblocks; q.nbytes = totals[ 1]; q.blockEntries = B;
		if (out)
		{
			out->ndict = (size_t)ndict; out->nblocks = (size_t)nblocks; out->nbytes = (size_t)totals[ 1]; out->block_entries = B;
			out->d_bytes = q.dBytes.ptr; out->d_block_offsets = q.dBlockOffsets.ptr; out->d_block_handles = q.dBlockHandles.ptr;
			out->d_totals = q.dTotals.ptr;
		}
	});
}

// plain copy of the blocks' buffers
int sp_matcher_ctx_finished_term_blocks_fetch( sp_matcher_ctx_t* c, sp_match_term_blocks_t* out)
{
	const sp_matcher_ctx::TermBlocks& q = c->prod.blk;
	return fetchProduct( c, q.run, "no term blocks of the last order of this context (sp_matcher_ctx_finished_term_blocks_device)", out, sp_match_term_blocks_free, [&]{
		allocMatchTermBlocks( out, q.ndict, q.nblocks, q.blockEntries);
		allocMatchTermBlockBytes( out, q.nbytes);
		if (q.nbytes) copySync( c->own, out->bytes, q.dBytes.ptr, q.nbytes, hipMemcpyDeviceToHost);
		copySync( c->own, out->block_offsets, q.dBlockOffsets.ptr, (q.nblocks+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (q.nblocks) copySync( c->own, out->block_handles, q.dBlockHandles.ptr, q.nblocks*sizeof(uint32_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->totals, q.dTotals.ptr, 4*sizeof(uint64_t), hipMemcpyDeviceToHost);
	});
}

// duration of the launches of the last term-blocks call in milliseconds (HIP events on its stream; the memsets that clear the
// totals are enqueued before the first event; the host's one wait lies inside)
int sp_matcher_ctx_last_term_blocks_ms( sp_matcher_ctx_t* c, double* ms) { return c->prod.blk.run.ms( 0, 1, ms); }

// ---- the postings of the dictionary of the finished batch, partitioned on the device (l2_postings.h)
void sp_test_postings_digit_bits( unsigned bits)
{
	postingsDigitBits().store( bits >= 1 && bits <= POSTINGS_MAX_DIGIT_BITS ? bits : POSTINGS_MAX_DIGIT_BITS, std::memory_order_relaxed);
}

int sp_matcher_ctx_finished_postings_device( sp_matcher_ctx_t* c, void* stream, sp_match_postings_device_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		requireFinished( c);
		const sp_matcher_ctx::Terms& t = c->prod.trm;
		const sp_matcher_ctx::Dict& d = c->prod.dct;
		if (!t.run.done || !d.run.done) throw std::runtime_error( "no dictionary of the last terms of the last finished batch (sp_matcher_ctx_finished_dictionary_device)");
		sp_matcher_ctx::Postings& q = c->prod.pst;
		c->prod.dropPositions();		// (positions are those of the postings they were built from)
		// (the dictionary call waited for ndict and knows N: nothing is waited for here)
		ProductCall call( c, q.run, stream, ProductCall::Sized());
		const size_t ndocs = call.ndocs;
		const uint64_t nterms = d.nterms, ndict = d.total;
		if (d.ndocs != ndocs || t.total != nterms) throw std::runtime_error( "the dictionary is not that of the terms of the finished batch");
		if (nterms >= 0xFFFFFFFFull || ndict > nterms) throw std::runtime_error( "a dictionary of more entries than term records, or of 2^32 - 1 records or more");
		const uint32_t bits = postingsDigitBits().load( std::memory_order_relaxed);
		const uint32_t tiles = l2PostingsTiles( nterms), passes = l2PostingsPasses( ndict, bits);
		reserveOrNoMem( q.dPostings, (nterms+1)*sizeof(sp_posting_t));
		reserveOrNoMem( q.dEntryOffsets, (ndict+1)*sizeof(uint64_t));
		reserveOrNoMem( q.dRecordPosting, (nterms+1)*sizeof(uint32_t));
		reserveOrNoMem( q.dDocOf, (nterms+1)*sizeof(uint32_t));
		for (int i=0; i<2; ++i) reserveOrNoMem( q.dPairs[ i], (nterms+1)*sizeof(uint64_t));
		reserveOrNoMem( q.dHist, ((size_t)tiles+1)*sizeof(uint32_t) << POSTINGS_MAX_DIGIT_BITS);
		// behind the dictionary, whose placement nobody has waited for yet; that runs behind the terms and the finish
		call.beginBehind( d.run.stream, d.run.ev[ 1], q.dTotals, 1, q.dCursor, POSTINGS_CURSORS);
		PostingsParams P;
		std::memset( &P, 0, sizeof(P));
		P.terms = (const uint32_t*)t.dRecords.ptr; P.docTermOffsets = (const uint64_t*)t.dDocOffsets.ptr;
		P.termDict = (const uint32_t*)d.dTermDict.ptr; P.dictRecords = (const uint32_t*)d.dRecords.ptr;
		P.nterms = nterms; P.ndict = (uint32_t)ndict; P.ndocs = (uint32_t)ndocs;
		P.digitBits = bits; P.passes = passes; P.tiles = tiles;
		P.docOf = (uint32_t*)q.dDocOf.ptr; P.hist = (uint32_t*)q.dHist.ptr; P.cursor = (uint32_t*)q.dCursor.ptr;
		for (int i=0; i<2; ++i) P.pairs[ i] = (uint64_t*)q.dPairs[ i].ptr;
		P.postings = (uint32_t*)q.dPostings.ptr; P.entryOffsets = (uint64_t*)q.dEntryOffsets.ptr;
		P.recordPosting = (uint32_t*)q.dRecordPosting.ptr; P.total = (uint64_t*)q.dTotals.ptr;
		HIP_CHECK( hipEventRecord( q.run.ev[ 0], call.stream));
		HIP_CHECK( launchL2Postings( P, c->numCUs, call.stream));
		HIP_CHECK( hipEventRecord( q.run.ev[ 1], call.stream));
		q.run.completed( call.stream);
		q.ndocs = ndocs; q.nterms = nterms; q.ndict = ndict;
		if (out)
		{
			out->ndocs = ndocs; out->nterms = (size_t)nterms; out->ndict = (size_t)ndict;
			out->d_postings = q.dPostings.ptr; out->d_entry_offsets = q.dEntryOffsets.ptr;
			out->d_record_posting = q.dRecordPosting.ptr; out->d_totals = q.dTotals.ptr;
		}
	});
}

// plain copy of the postings' buffers
int sp_matcher_ctx_finished_postings_fetch( sp_matcher_ctx_t* c, sp_match_postings_t* out)
{
	const sp_matcher_ctx::Postings& q = c->prod.pst;
	return fetchProduct( c, q.run, "no postings of the last dictionary of this context (sp_matcher_ctx_finished_postings_device)", out, sp_match_postings_free, [&]{
		allocMatchPostings( out, q.ndocs, q.nterms, q.ndict);
		if (q.nterms) copySync( c->own, out->postings, q.dPostings.ptr, q.nterms*sizeof(sp_posting_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->entry_offsets, q.dEntryOffsets.ptr, (q.ndict+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (q.nterms) copySync( c->own, out->record_posting, q.dRecordPosting.ptr, q.nterms*sizeof(uint32_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->totals, q.dTotals.ptr, sizeof(uint64_t), hipMemcpyDeviceToHost);
	});
}

// duration of the launches of the last postings call in milliseconds (HIP events on its stream; the memsets that clear the
// cursors and the total are enqueued before the first event)
int sp_matcher_ctx_last_postings_ms( sp_matcher_ctx_t* c, double* ms) { return c->prod.pst.run.ms( 0, 1, ms); }

uint32_t sp_matcher_postings_tile(void) { return POSTINGS_TILE; }

// ---- the positions of the postings of the finished batch, partitioned on the device (l2_positions.h)
void sp_test_positions_launch_events( unsigned on) { positionsLaunchEvents().store( on, std::memory_order_relaxed); }

int sp_matcher_ctx_finished_positions_device( sp_matcher_ctx_t* c, void* stream, sp_match_positions_device_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		requireFinished( c);
		const sp_matcher_ctx::Finished& fin = c->prod.fin;
		const sp_matcher_ctx::Terms& t = c->prod.trm;
		const sp_matcher_ctx::Postings& s = c->prod.pst;
		if (!t.run.done || !c->prod.dct.run.done || !s.run.done)
			throw std::runtime_error( "no postings of the last dictionary of the last finished batch (sp_matcher_ctx_finished_postings_device)");
		sp_matcher_ctx::Positions& q = c->prod.pos;
		c->prod.pbk.run.done = false;		// (posting blocks are those of the positions they were built from)
		q.launches = 0;
		// (the terms call read the finished total and the postings call knows N: the one wait of this call is for nocc and the largest ordpos)
		ProductCall call( c, q.run, stream, ProductCall::Sized());
		const size_t ndocs = call.ndocs;
		const uint64_t nresults = t.nresults, nterms = s.nterms;
		if (t.ndocs != ndocs || s.ndocs != ndocs || t.total != nterms) throw std::runtime_error( "the postings are not those of the terms of the finished batch");
		if (nresults >= 0xFFFFFFFFull) throw std::runtime_error( "2^32 - 1 results or more: the indices of the positions are 32 bits");
		const uint32_t bits = postingsDigitBits().load( std::memory_order_relaxed);
		reserveOrNoMem( q.dOccurrences, (nresults+1)*sizeof(sp_occurrence_t));		// (sized by the finished total before the wait: nocc is at most that)
		reserveOrNoMem( q.dPostingOffsets, (nterms+1)*sizeof(uint64_t));
		reserveOrNoMem( q.dPostingPositions, (nterms+1)*sizeof(uint32_t));
		reserveOrNoMem( q.dDocOf, (nresults+1)*sizeof(uint32_t));
		for (int i=0; i<2; ++i) reserveOrNoMem( q.dPairs[ i], (nresults+1)*sizeof(uint64_t));
		reserveOrNoMem( q.dHist, radixHistWords( nresults)*sizeof(uint32_t));
		PositionsLaunchEvents events = { 0, 0, 0, 0};
		if (positionsLaunchEvents().load( std::memory_order_relaxed))
		{
			const size_t capacity = 8 + 3*64;		// (two marks in front, keys, offsets, rekey, place, three a pass)
			if (q.launchEv.size() < capacity) q.launchEv = std::vector<Event>( capacity);
			q.launchEvHandles.resize( capacity); q.launchKind.assign( capacity, POS_NONE);
			for (size_t i=0; i<capacity; ++i) { q.launchEv[ i].create(); q.launchEvHandles[ i] = q.launchEv[ i]; }
			events.ev = q.launchEvHandles.data(); events.kind = q.launchKind.data(); events.capacity = capacity;
		}
		// behind the postings, whose placement nobody has waited for yet; that runs behind the dictionary, the terms and the finish
		call.beginBehind( s.run.stream, s.run.ev[ 1], q.dTotals, 3, q.dCursor, POSITIONS_CURSORS);
		HIP_CHECK( hipMemsetAsync( q.dPostingPositions.ptr, 0, (nterms+1)*sizeof(uint32_t), call.stream));
		PositionsParams P;
		std::memset( &P, 0, sizeof(P));
		P.results = (const uint32_t*)fin.dResults.ptr; P.docOffsets = (const uint64_t*)fin.dDocResultOffsets.ptr;
		P.resultTerm = (const uint32_t*)t.dResultTerm.ptr; P.docTermOffsets = (const uint64_t*)t.dDocOffsets.ptr;
		P.postings = (const uint32_t*)s.dPostings.ptr; P.recordPosting = (const uint32_t*)s.dRecordPosting.ptr;
		P.nresults = nresults; P.nterms = nterms; P.ndocs = (uint32_t)ndocs;
		P.digitBits = bits; P.tiles = radixTiles( nresults);
		P.docOf = (uint32_t*)q.dDocOf.ptr; P.hist = (uint32_t*)q.dHist.ptr; P.cursor = (uint32_t*)q.dCursor.ptr;
		for (int i=0; i<2; ++i) P.pairs[ i] = (uint64_t*)q.dPairs[ i].ptr;
		P.occurrences = (uint32_t*)q.dOccurrences.ptr; P.postingOffsets = (uint64_t*)q.dPostingOffsets.ptr;
		P.postingPositions = (uint32_t*)q.dPostingPositions.ptr; P.totals = (uint64_t*)q.dTotals.ptr;
		P.events = events.ev ? &events : 0;
		uint64_t counted[ 3] = { 0, 0, 0};		// nocc, (the sum of posting_positions: the placement's), the largest participating ordpos
		call.passes( P, launchL2PositionsCount, launchL2PositionsPlace, q.dTotals, counted, 3, [&]{
			P.nocc = counted[ 0] < nresults ? counted[ 0] : nresults;
			P.passes[ 0] = radixPasses( counted[ 2] & 0xFFFFFFFFull, bits);
			// (a result that does not participate sorts behind the last posting with the key N)
			P.passes[ 1] = radixPasses( P.nocc < nresults ? nterms : (nterms ? nterms - 1 : 0), bits);
		});
		q.ndocs = ndocs; q.nterms = nterms; q.nocc = P.nocc; q.launches = events.n;
		if (out)
		{
			out->ndocs = ndocs; out->nterms = (size_t)nterms; out->nocc = (size_t)P.nocc;
			out->d_occurrences = q.dOccurrences.ptr; out->d_posting_offsets = q.dPostingOffsets.ptr;
			out->d_posting_positions = q.dPostingPositions.ptr; out->d_totals = q.dTotals.ptr;
		}
	});
}

// plain copy of the positions' buffers
int sp_matcher_ctx_finished_positions_fetch( sp_matcher_ctx_t* c, sp_match_positions_t* out)
{
	const sp_matcher_ctx::Positions& q = c->prod.pos;
	return fetchProduct( c, q.run, "no positions of the last postings of this context (sp_matcher_ctx_finished_positions_device)", out, sp_match_positions_free, [&]{
		allocMatchPositions( out, q.ndocs, q.nterms, q.nocc);
		if (q.nocc) copySync( c->own, out->occurrences, q.dOccurrences.ptr, q.nocc*sizeof(sp_occurrence_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->posting_offsets, q.dPostingOffsets.ptr, (q.nterms+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (q.nterms) copySync( c->own, out->posting_positions, q.dPostingPositions.ptr, q.nterms*sizeof(uint32_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->totals, q.dTotals.ptr, 2*sizeof(uint64_t), hipMemcpyDeviceToHost);
	});
}

// duration of the launches of the last positions call in milliseconds (HIP events on its stream; the memsets that clear the
// cursors, the totals and posting_positions are enqueued before the first event; the host's one wait lies inside)
int sp_matcher_ctx_last_positions_ms( sp_matcher_ctx_t* c, double* ms) { return c->prod.pos.run.ms( 0, 1, ms); }

// the launches of the last positions call summed by kind (sp_test_positions_launch_events)
int sp_matcher_ctx_last_positions_launch_ms( sp_matcher_ctx_t* c, double ms[ 6])
{
	const sp_matcher_ctx::Positions& q = c->prod.pos;
	for (int k=0; k<6; ++k) ms[ k] = 0.0;
	if (!q.run.evValid || !q.launches) return SP_ERR_INVALID;
	if (hipEventSynchronize( q.run.ev[ 1]) != hipSuccess) return SP_ERR_DEVICE;
	for (size_t i=1; i<q.launches; ++i)
	{
		const int kind = q.launchKind[ i];
		double one = 0.0;
		if (kind < 0 || kind >= 6) continue;		// (a mark in front of a half, or the scan of the posting offsets)
		if (!elapsedMs( q.launchEvHandles[ i-1], q.launchEvHandles[ i], one)) return SP_ERR_DEVICE;
		ms[ kind] += one;
	}
	return SP_OK;
}

uint32_t sp_matcher_positions_tile(void) { return POSITIONS_TILE; }

// ---- the posting blocks of the order, the postings and the positions of the finished batch, coded on the device (l2_postingblocks.h)
int sp_matcher_ctx_finished_posting_blocks_device( sp_matcher_ctx_t* c, void* stream, sp_match_posting_blocks_device_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		requireFinished( c);
		const sp_matcher_ctx::Dict& d = c->prod.dct;
		const sp_matcher_ctx::DictOrder& o = c->prod.ord;
		const sp_matcher_ctx::Postings& s = c->prod.pst;
		const sp_matcher_ctx::Positions& x = c->prod.pos;
		if (!c->prod.trm.run.done || !d.run.done || !o.run.done || !s.run.done || !x.run.done)
			throw std::runtime_error( "no order, postings and positions of the last dictionary of the last finished batch (sp_matcher_ctx_finished_dictionary_order_device, sp_matcher_ctx_finished_postings_device, sp_matcher_ctx_finished_positions_device)");
		sp_matcher_ctx::PostingBlocks& q = c->prod.pbk;
		// (the dictionary call waited for ndict, the positions call for nocc: the one wait of this call is for nbytes)
		ProductCall call( c, q.run, stream, ProductCall::Sized());
		const uint64_t ndict = d.total, nterms = s.nterms, nocc = x.nocc;
		if (o.ndict != ndict || s.ndict != ndict || x.nterms != nterms || s.ndocs != call.ndocs || ndict >= 0xFFFFFFFFull || nterms >= 0xFFFFFFFFull || (ndict && !nterms))
			throw std::runtime_error( "the order, the postings or the positions are not those of the dictionary of the finished batch");
		const uint32_t B = termBlockEntries();
		const uint64_t nblocks = (ndict + B - 1) / B;
		reserveOrNoMem( q.dBlockOffsets, (nblocks+1)*sizeof(uint64_t));
		reserveOrNoMem( q.dBlockSize, (nblocks+1)*sizeof(uint64_t));
		reserveOrNoMem( q.dListOffsets, (ndict+1)*sizeof(uint64_t));
		reserveOrNoMem( q.dListStart, (ndict+1)*sizeof(uint64_t));
		reserveOrNoMem( q.dPostingBytes, (nterms+1)*sizeof(uint64_t));
		// behind the order, the postings and the positions, which nobody has waited for yet
		call.beginBehind( o.run.stream, o.run.ev[ 1], q.dTotals, 4, q.dCursor, 1);
		if (call.stream != s.run.stream) HIP_CHECK( hipStreamWaitEvent( call.stream, s.run.ev[ 1], 0));
		if (call.stream != x.run.stream) HIP_CHECK( hipStreamWaitEvent( call.stream, x.run.ev[ 1], 0));
		PostingBlocksParams P;
		std::memset( &P, 0, sizeof(P));
		P.order = (const uint32_t*)o.dOrder.ptr; P.entryOffsets = (const uint64_t*)s.dEntryOffsets.ptr; P.postings = (const uint32_t*)s.dPostings.ptr;
		P.postingOffsets = (const uint64_t*)x.dPostingOffsets.ptr; P.postingPositions = (const uint32_t*)x.dPostingPositions.ptr;
		P.occurrences = (const uint32_t*)x.dOccurrences.ptr;
		P.ndict = (uint32_t)ndict; P.ndocs = (uint32_t)call.ndocs; P.nterms = nterms; P.nocc = nocc; P.blockEntries = B; P.nblocks = (uint32_t)nblocks;
		P.listOffsets = (uint64_t*)q.dListOffsets.ptr; P.listStart = (uint64_t*)q.dListStart.ptr; P.postingBytes = (uint64_t*)q.dPostingBytes.ptr;
		P.blockSize = (uint64_t*)q.dBlockSize.ptr; P.blockOffsets = (uint64_t*)q.dBlockOffsets.ptr; P.totals = (uint64_t*)q.dTotals.ptr;
		uint64_t totals[ 4] = { 0, 0, B, 0};
		if (ndict)
		{
			call.passes( P, launchL2PostingBlocksCount, launchL2PostingBlocksPlace, q.dTotals, totals, 4, [&]{
				reserveOrNoMem( q.dBytes, totals[ 1] + 16);
				P.bytes = (uint8_t*)q.dBytes.ptr; P.capacity = totals[ 1];
			});
		}
		else
		{
			// nothing to code, nothing to launch: block_offsets = [0], the totals {0, 0, B, 0}
			HIP_CHECK( hipEventRecord( q.run.ev[ 0], call.stream));
			HIP_CHECK( hipMemsetAsync( q.dBlockOffsets.ptr, 0, sizeof(uint64_t), call.stream));
			HIP_CHECK( hipMemsetD32Async( (hipDeviceptr_t)((uint64_t*)q.dTotals.ptr + 2), (int)B, 1, call.stream));
			HIP_CHECK( hipEventRecord( q.run.ev[ 1], call.stream));
			q.run.completed( call.stream);
		}
		q.ndict = ndict; q.nblocks = nblocks; q.nbytes = totals[ 1]; q.blockEntries = B;
		if (out)
		{
			out->ndict = (size_t)ndict; out->nblocks = (size_t)nblocks; out->nbytes = (size_t)totals[ 1]; out->block_entries = B;
			out->d_bytes = q.dBytes.ptr; out->d_block_offsets = q.dBlockOffsets.ptr; out->d_totals = q.dTotals.ptr;
		}
	});
}

// plain copy of the blocks' buffers
int sp_matcher_ctx_finished_posting_blocks_fetch( sp_matcher_ctx_t* c, sp_match_posting_blocks_t* out)
{
	const sp_matcher_ctx::PostingBlocks& q = c->prod.pbk;
	return fetchProduct( c, q.run, "no posting blocks of the last order, postings and positions of this context (sp_matcher_ctx_finished_posting_blocks_device)", out, sp_match_posting_blocks_free, [&]{
		allocMatchPostingBlocks( out, q.ndict, q.nblocks, q.blockEntries);
		allocMatchPostingBlockBytes( out, q.nbytes);
		if (q.nbytes) copySync( c->own, out->bytes, q.dBytes.ptr, q.nbytes, hipMemcpyDeviceToHost);
		copySync( c->own, out->block_offsets, q.dBlockOffsets.ptr, (q.nblocks+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->totals, q.dTotals.ptr, 4*sizeof(uint64_t), hipMemcpyDeviceToHost);
	});
}

// duration of the launches of the last posting-blocks call in milliseconds (HIP events on its stream; the memsets that clear the
// totals are enqueued before the first event; the host's one wait lies inside)
int sp_matcher_ctx_last_posting_blocks_ms( sp_matcher_ctx_t* c, double* ms) { return c->prod.pbk.run.ms( 0, 1, ms); }

} // extern "C"
