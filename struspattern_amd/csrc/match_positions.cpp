// Posting positions of a finished batch, its terms and their postings over host arrays (match_positions.hpp): host only, no
// device needed.
#include "match_positions.hpp"
#include "finished_host.hpp"
#include <algorithm>
#include <vector>

namespace spa {

void allocMatchPositions( sp_match_positions_t* out, size_t ndocs, uint64_t nterms, uint64_t nocc)
{
	out->ndocs = ndocs; out->nterms = (size_t)nterms; out->nocc = (size_t)nocc;
	out->totals[ 0] = nocc;
	out->occurrences = filledArray<sp_occurrence_t>( nocc, 0xFF);
	out->posting_offsets = filledArray<uint64_t>( nterms + 1, 0);
	out->posting_positions = filledArray<uint32_t>( nterms, 0);
}

void matchPositions( const sp_result_t* results, uint64_t nresults, const uint64_t* docOffsets, size_t ndocs,
		     const uint32_t* resultTerm, const uint64_t* docTermOffsets, uint64_t nterms,
		     const sp_posting_t* postings, const uint32_t* recordPosting, sp_match_positions_t* out)
{
	const uint32_t NONE = 0xFFFFFFFFu;
	static const uint64_t noDocuments[ 1] = { 0};
	if (!ndocs && !docOffsets) docOffsets = noDocuments;		// (a batch of no documents need not have offsets)
	if (!docOffsets) throw std::runtime_error( "batch without document offsets");
	if (!docTermOffsets) throw std::runtime_error( "terms without document offsets");
	if (nresults && (!results || !resultTerm)) throw std::runtime_error( "results without records or without result_term");
	if (nterms && (!postings || !recordPosting)) throw std::runtime_error( "postings without records or without record_posting");
	if (nresults >= 0xFFFFFFFFull) throw std::runtime_error( "2^32 - 1 results or more");
	if (nterms >= 0xFFFFFFFFull) throw std::runtime_error( "2^32 - 1 term records or more");
	if (ndocs > 0xFFFFFFFFull) throw std::runtime_error( "2^32 documents or more");
	checkDocOffsets( docOffsets, ndocs, nresults);
	if (docTermOffsets[ 0] != 0) throw std::runtime_error( "term offsets do not start at the first record");
	for (size_t d=0; d<ndocs; ++d)
	{
		if (docTermOffsets[ d] > docTermOffsets[ d+1] || docTermOffsets[ d+1] > nterms) throw std::runtime_error( "term offsets do not ascend inside the records");
	}
	if (docTermOffsets[ ndocs] != nterms) throw std::runtime_error( "term offsets do not cover the records");

	// count: the participating results of every posting are its count
	std::vector<uint64_t> next( (size_t)nterms + 1, 0);
	uint64_t nocc = 0;
	for (size_t d=0; d<ndocs; ++d)
	{
		const uint64_t t0 = docTermOffsets[ d], nrecords = docTermOffsets[ d+1] - t0;
		for (uint64_t r=docOffsets[ d]; r<docOffsets[ d+1]; ++r)
		{
			if (resultTerm[ r] == NONE) continue;
			if (resultTerm[ r] >= nrecords) throw std::runtime_error( "a result_term entry outside the term records of its document");
			const uint32_t p = recordPosting[ t0 + resultTerm[ r]];
			if (p >= nterms) throw std::runtime_error( "a record_posting entry outside the postings");
			next[ p] += 1; ++nocc;
		}
	}
	for (uint64_t p=0; p<nterms; ++p)
	{
		if (postings[ p].count != next[ p]) throw std::runtime_error( "a posting whose count is not the number of its results");
	}
	allocMatchPositions( out, ndocs, nterms, nocc);
	// offsets, then place in result order: every list ascends by (document, result), here by result (a posting has one document)
	uint64_t sum = 0;
	for (uint64_t p=0; p<nterms; ++p) { out->posting_offsets[ p] = sum; sum += next[ p]; next[ p] = out->posting_offsets[ p]; }
	out->posting_offsets[ nterms] = sum;
	for (size_t d=0; d<ndocs; ++d)
	{
		const uint64_t t0 = docTermOffsets[ d];
		for (uint64_t r=docOffsets[ d]; r<docOffsets[ d+1]; ++r)
		{
			if (resultTerm[ r] == NONE) continue;
			const sp_occurrence_t occ = { results[ r].ordpos, (uint32_t)(r - docOffsets[ d]) };
			out->occurrences[ next[ recordPosting[ t0 + resultTerm[ r]]]++] = occ;
		}
	}
	// by position inside every list, equal positions in result order; the distinct positions
	uint64_t positions = 0;
	for (uint64_t p=0; p<nterms; ++p)
	{
		sp_occurrence_t* first = out->occurrences + out->posting_offsets[ p];
		sp_occurrence_t* last = out->occurrences + out->posting_offsets[ p+1];
		std::stable_sort( first, last, []( const sp_occurrence_t& a, const sp_occurrence_t& b) { return a.ordpos < b.ordpos; });
		uint32_t distinct = 0;
		for (sp_occurrence_t* o=first; o<last; ++o) if (o == first || o[ -1].ordpos != o->ordpos) ++distinct;
		out->posting_positions[ p] = distinct;
		positions += distinct;
	}
	out->totals[ 1] = positions;
}

} // namespace

extern "C" void sp_match_positions_free( sp_match_positions_t* p)
{
	std::free( p->occurrences); std::free( p->posting_offsets); std::free( p->posting_positions);
	std::memset( p, 0, sizeof(*p));
}

extern "C" int sp_match_batch_positions( const sp_match_batch_t* mb, const sp_match_terms_t* terms, const sp_match_postings_t* postings,
					 sp_match_positions_t* out, char* err, size_t errsize)
{
	return spa::hostProduct( out, sp_match_positions_free, err, errsize, [&]{
		if (!mb) throw std::runtime_error( "no batch");
		if (!terms) throw std::runtime_error( "no terms");
		if (!postings) throw std::runtime_error( "no postings");
		if (mb->ndocs != terms->ndocs || terms->ndocs != postings->ndocs || mb->nresults != terms->nresults || terms->nrecords != postings->nterms)
			throw std::runtime_error( "the terms are not those of the batch, or the postings not those of the terms: other counts of documents, results or term records");
		spa::matchPositions( mb->results, mb->nresults, mb->doc_result_offsets, mb->ndocs, terms->result_term, terms->doc_term_offsets,
				     terms->nrecords, postings->postings, postings->record_posting, out);
	});
}
