// Pattern frequencies of a finished batch over host arrays (pattern_freq.hpp): host only, no device needed.
#include "pattern_freq.hpp"
#include "finished_host.hpp"
#include <algorithm>

namespace spa {

namespace {
enum {FREQ_ERR_RANGE = SP_DOC_ERR_RANGE};

// the results of one document as (handle, ordpos, ordend), ascending by handle: equal handles are neighbours
struct Occurrence
{
	uint32_t handle, ordpos, ordend;
	bool operator<( const Occurrence& o) const { return handle < o.handle; }
};

} // namespace

void allocPatternFreq( sp_pattern_freq_batch_t* out, size_t ndocs, uint32_t handleBound)
{
	out->ndocs = ndocs; out->nrecords = 0; out->handle_bound = handleBound; out->totals[ 0] = 0;
	out->doc_offsets = filledArray<uint64_t>( ndocs + 1);
	out->doc_freq_status = filledArray<int32_t>( ndocs + 1);
	out->handle_results = filledArray<uint64_t>( handleBound);
	out->handle_docs = filledArray<uint32_t>( handleBound);
}

void allocPatternFreqRecords( sp_pattern_freq_batch_t* out, uint64_t nrecords)
{
	out->records = filledArray<sp_pattern_freq_t>( nrecords);
	out->nrecords = (size_t)nrecords; out->totals[ 0] = nrecords;
}

void patternFreq( const sp_result_t* results, uint64_t nresults, const uint64_t* docOffsets, const int32_t* docStatus,
		  size_t ndocs, uint32_t handleBound, sp_pattern_freq_batch_t* out)
{
	if (!handleBound) throw std::runtime_error( "a handle bound of 0 leaves no valid handle");
	if (!docOffsets) throw std::runtime_error( "batch without document offsets");
	if (nresults && !results) throw std::runtime_error( "batch without results");
	checkDocOffsets( docOffsets, ndocs, nresults);

	allocPatternFreq( out, ndocs, handleBound);
	std::vector<sp_pattern_freq_t> records;
	std::vector<Occurrence> occ;
	for (size_t d=0; d<ndocs; ++d)
	{
		out->doc_offsets[ d] = records.size();
		if (docStatus && docStatus[ d] != 0) continue;		// (a finished batch has no results of a failed document)
		occ.clear();
		bool valid = true;
		for (uint64_t i=docOffsets[ d]; valid && i<docOffsets[ d+1]; ++i)
		{
			const sp_result_t& r = results[ i];
			valid = r.handle >= 1 && r.handle < handleBound;
			const Occurrence o = { r.handle, r.ordpos, r.ordend };
			occ.push_back( o);
		}
		if (!valid) { out->doc_freq_status[ d] = FREQ_ERR_RANGE; continue; }
		std::sort( occ.begin(), occ.end());
		for (size_t i=0; i<occ.size(); ++i)
		{
			if (i == 0 || occ[ i].handle != occ[ i-1].handle)
			{
				const sp_pattern_freq_t rec = { occ[ i].handle, 0, 0xFFFFFFFFu, 0 };
				records.push_back( rec);
			}
			sp_pattern_freq_t& rec = records.back();
			rec.count += 1;
			rec.first_ordpos = std::min( rec.first_ordpos, occ[ i].ordpos);
			rec.last_ordend = std::max( rec.last_ordend, occ[ i].ordend);
		}
	}
	out->doc_offsets[ ndocs] = records.size();
	allocPatternFreqRecords( out, records.size());
	if (!records.empty()) std::memcpy( out->records, records.data(), records.size() * sizeof(sp_pattern_freq_t));
	for (const sp_pattern_freq_t& rec : records)
	{
		out->handle_results[ rec.handle] += rec.count;
		out->handle_docs[ rec.handle] += 1;
	}
}

} // namespace

extern "C" void sp_pattern_freq_batch_free( sp_pattern_freq_batch_t* b)
{
	std::free( b->records); std::free( b->doc_offsets); std::free( b->doc_freq_status);
	std::free( b->handle_results); std::free( b->handle_docs);
	std::memset( b, 0, sizeof(*b));
}

extern "C" int sp_match_batch_pattern_freq( const sp_match_batch_t* mb, uint32_t handle_bound, sp_pattern_freq_batch_t* out, char* err, size_t errsize)
{
	return spa::hostProduct( out, sp_pattern_freq_batch_free, err, errsize, [&]{
		if (!mb) throw std::runtime_error( "no batch");
		spa::patternFreq( mb->results, mb->nresults, mb->doc_result_offsets, mb->doc_status, mb->ndocs, handle_bound, out);
	});
}
