// Index terms of a finished batch over host arrays (match_terms.hpp): host only, no device needed.
#include "match_terms.hpp"
#include "finished_host.hpp"
#include <algorithm>
#include <vector>

namespace spa {

namespace {
enum {TERM_ERR_RANGE = SP_DOC_ERR_RANGE};
const uint32_t NO_TERM = 0xFFFFFFFFu;

// a result of one document with its term value
struct Occurrence
{
	uint32_t index, handle, ordpos, ordend;
	const char* bytes; uint64_t size;
};

int compareValue( const Occurrence& a, const Occurrence& b)
{
	if (a.handle != b.handle) return a.handle < b.handle ? -1 : 1;
	if (a.size != b.size) return a.size < b.size ? -1 : 1;
	return a.size ? std::memcmp( a.bytes, b.bytes, (size_t)a.size) : 0;
}

} // namespace

void allocMatchTerms( sp_match_terms_t* out, size_t ndocs, uint64_t nresults, uint32_t handleBound, uint32_t flags)
{
	out->ndocs = ndocs; out->nresults = (size_t)nresults; out->nrecords = 0; out->handle_bound = handleBound; out->flags = flags;
	out->totals[ 0] = 0;
	out->doc_term_offsets = filledArray<uint64_t>( ndocs + 1, 0);
	out->doc_term_status = filledArray<int32_t>( ndocs + 1, 0);
	out->result_term = filledArray<uint32_t>( nresults, 0xFF);
}

void allocMatchTermRecords( sp_match_terms_t* out, uint64_t nrecords)
{
	out->records = filledArray<sp_match_term_t>( nrecords, 0);
	out->nrecords = (size_t)nrecords; out->totals[ 0] = nrecords;
}

void matchTerms( const sp_result_t* results, uint64_t nresults, const uint64_t* docOffsets, const int32_t* docStatus,
		 const uint32_t* resultFormat, size_t ndocs, const TermSource (&source)[ 2], uint32_t handleBound, uint32_t flags,
		 sp_match_terms_t* out)
{
	if (!flags || (flags & ~(uint32_t)(SP_TERM_VALUES | SP_TERM_TEXT))) throw std::runtime_error( "unknown or no term flags");
	if (!handleBound) throw std::runtime_error( "a handle bound of 0 leaves no valid handle");
	if (!docOffsets) throw std::runtime_error( "batch without document offsets");
	if (nresults && !results) throw std::runtime_error( "batch without results");
	checkDocOffsets( docOffsets, ndocs, nresults);
	for (size_t d=0; d<ndocs; ++d)
	{
		if (docOffsets[ d+1] - docOffsets[ d] >= NO_TERM) throw std::runtime_error( "a document of 2^32 results or more");
	}
	if (flags & SP_TERM_VALUES) checkTermSource( source[ 0], nresults, "values");
	if (flags & SP_TERM_TEXT) checkTermSource( source[ 1], nresults, "text");

	allocMatchTerms( out, ndocs, nresults, handleBound, flags);
	std::vector<sp_match_term_t> records;
	std::vector<Occurrence> occ;
	for (size_t d=0; d<ndocs; ++d)
	{
		out->doc_term_offsets[ d] = records.size();
		if (docStatus && docStatus[ d] != 0) continue;		// (a finished batch has no results of a failed document)
		const uint64_t r0 = docOffsets[ d], r1 = docOffsets[ d+1];
		if (r0 == r1) continue;
		bool valid = true;
		for (int s=0; s<2; ++s) if ((flags & (1u << s)) && source[ s].docStatus && source[ s].docStatus[ d] != 0) valid = false;
		occ.clear();
		for (uint64_t i=r0; valid && i<r1; ++i)
		{
			const sp_result_t& r = results[ i];
			valid = r.handle >= 1 && r.handle < handleBound;
			const TermSource& S = source[ termSourceIndex( flags, resultFormat, i)];
			const Occurrence o = { (uint32_t)(i - r0), r.handle, r.ordpos, r.ordend, S.bytes + S.offsets[ i], S.offsets[ i+1] - S.offsets[ i] };
			occ.push_back( o);
		}
		if (!valid) { out->doc_term_status[ d] = TERM_ERR_RANGE; continue; }
		// equal terms as neighbours, the smallest index first
		std::sort( occ.begin(), occ.end(), []( const Occurrence& a, const Occurrence& b) {
			const int c = compareValue( a, b);
			return c ? c < 0 : a.index < b.index;
		});
		std::vector<sp_match_term_t> terms;
		std::vector<uint32_t> termOf( occ.size());		// index in `terms`, by position in `occ`
		for (size_t i=0; i<occ.size(); ++i)
		{
			if (i == 0 || compareValue( occ[ i-1], occ[ i]) != 0)
			{
				if (occ[ i].size > 0xFFFFFFFFull) throw std::runtime_error( "a term value of 2^32 bytes or more");
				const sp_match_term_t rec = { occ[ i].handle, 0, 0xFFFFFFFFu, 0, occ[ i].index, (uint32_t)occ[ i].size };
				terms.push_back( rec);
			}
			sp_match_term_t& rec = terms.back();
			rec.count += 1;
			rec.first_ordpos = std::min( rec.first_ordpos, occ[ i].ordpos);
			rec.last_ordend = std::max( rec.last_ordend, occ[ i].ordend);
			termOf[ i] = (uint32_t)(terms.size() - 1);
		}
		// the order of the records: handle, then first_result
		std::vector<uint32_t> order( terms.size()), rank( terms.size());
		for (size_t t=0; t<terms.size(); ++t) order[ t] = (uint32_t)t;
		std::sort( order.begin(), order.end(), [&]( uint32_t a, uint32_t b) {
			return terms[ a].handle != terms[ b].handle ? terms[ a].handle < terms[ b].handle : terms[ a].first_result < terms[ b].first_result;
		});
		for (size_t k=0; k<order.size(); ++k) { rank[ order[ k]] = (uint32_t)k; records.push_back( terms[ order[ k]]); }
		for (size_t i=0; i<occ.size(); ++i) out->result_term[ r0 + occ[ i].index] = rank[ termOf[ i]];
	}
	out->doc_term_offsets[ ndocs] = records.size();
	allocMatchTermRecords( out, records.size());
	if (!records.empty()) std::memcpy( out->records, records.data(), records.size() * sizeof(sp_match_term_t));
}

} // namespace

extern "C" void sp_match_terms_free( sp_match_terms_t* t)
{
	std::free( t->records); std::free( t->doc_term_offsets); std::free( t->result_term); std::free( t->doc_term_status);
	std::memset( t, 0, sizeof(*t));
}

extern "C" int sp_match_batch_terms( const sp_match_batch_t* mb, const sp_match_values_t* values, const sp_match_text_t* text,
				     uint32_t handle_bound, uint32_t flags, sp_match_terms_t* out, char* err, size_t errsize)
{
	return spa::hostProduct( out, sp_match_terms_free, err, errsize, [&]{
		if (!mb) throw std::runtime_error( "no batch");
		spa::TermSource source[ 2] = {};
		spa::termSources( *mb, values, text, flags, source);
		spa::matchTerms( mb->results, mb->nresults, mb->doc_result_offsets, mb->doc_status, mb->result_format, mb->ndocs,
				 source, handle_bound, flags, out);
	});
}
