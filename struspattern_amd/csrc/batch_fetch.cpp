// Regroup of a finished device batch for the host (batch_fetch.hpp): host only, no device needed.
#include "batch_fetch.hpp"

namespace spa {

void allocMatchBatch( sp_match_batch_t* out, size_t ndocs, uint64_t nresults, uint64_t nitems, bool withFormats)
{
	out->ndocs = ndocs; out->nresults = (size_t)nresults; out->nitems = (size_t)nitems;
	out->doc_stats = hostArray<uint64_t>( ndocs*4+1);
	out->doc_status = hostArray<int32_t>( ndocs+1);
	out->doc_result_offsets = hostArray<uint64_t>( ndocs+1);
	out->results = hostArray<sp_result_t>( nresults+1);
	out->items = hostArray<sp_result_item_t>( nitems+1);
	if (withFormats)
	{
		out->result_format = hostArray<uint32_t>( nresults+1);
		out->item_format = hostArray<uint32_t>( (nitems+1)*2);
	}
}

void allocLexBatch( sp_lex_batch_t* out, size_t ndocs, uint64_t nlexems)
{
	out->ndocs = ndocs;
	out->doc_lexem_offsets = hostArray<uint64_t>( ndocs+1);
	out->doc_status = hostArray<int32_t>( ndocs+1);
	out->lexems = hostArray<sp_lexem_t>( nlexems+1);
}

void checkDocRange( size_t firstDoc, size_t ndocs, size_t batchDocs)
{
	if (firstDoc > batchDocs || ndocs > batchDocs - firstDoc) throw std::runtime_error( "document range outside the last batch");
}

DocBlocks planDocBlocks( std::vector<uint64_t> range, const int32_t* status, uint64_t inBuffer, bool whole)
{
	DocBlocks rt;
	rt.range = std::move( range);
	if (whole)
	{
		if (inBuffer) rt.segments.push_back( CopySegment{ 0, inBuffer, 0});
		rt.packed = inBuffer;
	}
	for (size_t di=0; di<rt.ndocs(); ++di)
	{
		const uint64_t b = rt.range[ 2*di], n = rt.range[ 2*di+1];
		if (status[ di] != 0 || n > inBuffer || b > inBuffer - n) { rt.range[ 2*di+1] = 0; continue; }
		if (whole) continue;
		// the blocks of the wanted documents only, packed one after the other
		if (n) rt.segments.push_back( CopySegment{ b, n, rt.packed});
		rt.range[ 2*di] = rt.packed; rt.packed += n;
	}
	return rt;
}

ItemBlocks planItemBlocks( const DocBlocks& docs, sp_result_t* raw, uint64_t inBuffer, bool whole)
{
	ItemBlocks rt;
	if (whole)
	{
		if (inBuffer) rt.segments.push_back( CopySegment{ 0, inBuffer, 0});
		rt.packed = inBuffer;
	}
	for (size_t di=0; di<docs.ndocs(); ++di)
	{
		const uint64_t b = docs.first( di), n = docs.count( di);
		uint64_t first = 0, cnt = 0;
		for (uint64_t ri=0; ri<n; ++ri) if (raw[ b+ri].item_count) { if (!cnt) first = raw[ b+ri].item_begin; cnt += raw[ b+ri].item_count; }
		if (!cnt) continue;
		if (cnt > inBuffer || first > inBuffer - cnt) throw std::runtime_error( "item block of a document lies outside the device buffer");
		rt.kept += cnt;
		if (whole) continue;
		rt.segments.push_back( CopySegment{ first, cnt, rt.packed});
		for (uint64_t ri=0; ri<n; ++ri) if (raw[ b+ri].item_count) raw[ b+ri].item_begin = (uint32_t)(raw[ b+ri].item_begin - first + rt.packed);
		rt.packed += cnt;
	}
	return rt;
}

void eliminateCovered( const sp_result_t* raw, uint64_t n, uint32_t maxResultSize, std::vector<char>& covered)
{
	covered.assign( n, 0);
	for (uint64_t ai=0; ai<n; ++ai)
	{
		const sp_result_t& r = raw[ ai];
		for (uint64_t ni=ai; ni<n; ++ni)
		{
			const sp_result_t& f = raw[ ni];
			if (f.origseg > r.origendseg || f.origpos >= r.origend + maxResultSize) break;
			bool differ = (f.origendseg != r.origendseg || f.origend != r.origend || f.origseg != r.origseg || f.origpos != r.origpos);
			if (f.origseg <= r.origseg && f.origpos <= r.origpos && f.origendseg >= r.origendseg && f.origend >= r.origend && differ) covered[ ai] = 1;
			if (f.origseg >= r.origseg && f.origpos >= r.origpos && f.origendseg <= r.origendseg && f.origend <= r.origend && differ) covered[ ni] = 1;
		}
	}
}

void regroupMatchBatch( const DocBlocks& docs, const int32_t* status, const sp_result_t* raw, const sp_result_item_t* rawitems,
			const uint32_t* rawrf, const uint32_t* rawif, uint64_t nitems, bool exclusive, uint32_t maxResultSize, sp_match_batch_t* out)
{
	const size_t ndocs = docs.ndocs();
	uint64_t total = 0;
	for (size_t di=0; di<ndocs; ++di) total += docs.count( di);
	allocMatchBatch( out, ndocs, total, nitems, rawrf != 0);	// (`exclusive` may keep fewer: nresults, nitems below)
	if (ndocs) std::memcpy( out->doc_status, status, ndocs*sizeof(int32_t));
	uint64_t rp = 0, ip = 0;
	std::vector<char> covered;
	for (size_t di=0; di<ndocs; ++di)
	{
		out->doc_result_offsets[ di] = rp;
		const uint64_t b = docs.first( di), n = docs.count( di);
		if (exclusive) eliminateCovered( raw + b, n, maxResultSize, covered);
		for (uint64_t ri=0; ri<n; ++ri)
		{
			if (exclusive && covered[ ri]) continue;
			sp_result_t r = raw[ b+ri];
			uint32_t ib = r.item_begin, ic = r.item_count;
			r.item_begin = (uint32_t)ip;
			if (rawrf)
			{
				out->result_format[ rp] = rawrf[ b+ri];
				for (uint32_t k=0; k<ic; ++k) { out->item_format[ 2*(ip+k)] = rawif[ 2*(ib+k)]; out->item_format[ 2*(ip+k)+1] = rawif[ 2*(ib+k)+1]; }
			}
			for (uint32_t k=0; k<ic; ++k) out->items[ ip++] = rawitems[ ib+k];
			out->results[ rp++] = r;
		}
	}
	out->doc_result_offsets[ ndocs] = rp;
	out->nresults = rp; out->nitems = ip;
}

void regroupLexBatch( const DocBlocks& docs, const int32_t* status, const sp_lexem_t* raw, sp_lex_batch_t* out)
{
	const size_t ndocs = docs.ndocs();
	uint64_t total = 0;
	for (size_t di=0; di<ndocs; ++di) total += docs.count( di);
	allocLexBatch( out, ndocs, total);
	if (ndocs) std::memcpy( out->doc_status, status, ndocs*sizeof(int32_t));
	uint64_t lp = 0;
	for (size_t di=0; di<ndocs; ++di)
	{
		out->doc_lexem_offsets[ di] = lp;
		if (raw && docs.count( di)) std::memcpy( out->lexems + lp, raw + docs.first( di), docs.count( di)*sizeof(sp_lexem_t));
		lp += docs.count( di);
	}
	out->doc_lexem_offsets[ ndocs] = lp;
	out->nlexems = lp;
}

} // namespace

// test hook: the fetch of a context over host arrays in the device layout, memcpy for every copy
extern "C" int sp_match_batch_regroup( const sp_result_t* results, uint64_t nresults, const sp_result_item_t* items, uint64_t nitems,
					const uint32_t* result_format, const uint32_t* item_format, const uint64_t* doc_ranges, const int32_t* doc_status,
					size_t batch_ndocs, size_t first_doc, size_t ndocs, int exclusive, uint32_t max_result_size,
					sp_match_batch_t* out, char* err, size_t errsize)
{
	std::memset( out, 0, sizeof(*out));
	if (err && errsize) err[ 0] = 0;
	try
	{
		spa::MatchBatchSource src;
		src.results = results; src.nresults = nresults; src.items = items; src.nitems = nitems;
		src.resultFormat = result_format; src.itemFormat = result_format ? item_format : 0;
		src.docRange = doc_ranges; src.docStatus = doc_status; src.docStats = 0; src.ndocs = batch_ndocs;
		spa::fetchMatchBatch( src, first_doc, ndocs, exclusive != 0, max_result_size, []( void* dst, const void* s, size_t n){ std::memcpy( dst, s, n); }, out);
		std::memset( out->doc_stats, 0, ndocs*4*sizeof(uint64_t));
		return SP_OK;
	}
	catch (const std::bad_alloc&) { return SP_ERR_NOMEM; }
	catch (const std::exception& e)
	{
		if (err && errsize) { std::strncpy( err, e.what(), errsize-1); err[ errsize-1] = 0; }
		return SP_ERR_INVALID;
	}
}
