// Posting positions of a finished batch, its terms and their postings over host arrays: the definition that the device passes
// (l2_positions.h) are measured against, and the entry point for batches already fetched to the host
// (sp_match_batch_positions).  Host only: no HIP header and no HIP call in here.
//
// The rule (include/strus_pattern_amd.h "posting positions"; the project's own, unpinned by a reference vector).  Result r of
// document d participates iff result_term[r] is not 0xFFFFFFFF; its posting is p(r) = record_posting[doc_term_offsets[d] +
// result_term[r]].  Every participating result gets one occurrence {ordpos, r - doc_offsets[d]}; the occurrences of posting p
// lie at [posting_offsets[p], posting_offsets[p+1]), the exclusive prefix sums of the postings' count, ascending by ordpos
// (unsigned) and, at equal positions, by result; posting_positions[p] is the number of distinct ordpos of the list.
// A counting sort by posting, then a stable sort by ordpos inside each list.
#ifndef SPA_MATCH_POSITIONS_HPP
#define SPA_MATCH_POSITIONS_HPP
#include "match_postings.hpp"

namespace spa {

// the host arrays of the positions of `nocc` occurrences of `nterms` postings: offsets and posting_positions zeroed, the
// occurrences all 0xFFFFFFFF words (sp_match_positions_free)
void allocMatchPositions( sp_match_positions_t* out, size_t ndocs, uint64_t nterms, uint64_t nocc);

// The positions on the host.  Throws std::runtime_error for arguments that make no finished batch with its terms and postings.
void matchPositions( const sp_result_t* results, uint64_t nresults, const uint64_t* docOffsets, size_t ndocs,
		     const uint32_t* resultTerm, const uint64_t* docTermOffsets, uint64_t nterms,
		     const sp_posting_t* postings, const uint32_t* recordPosting, sp_match_positions_t* out);

} // namespace
#endif
