// Batch postings of a terms batch and its dictionary over host arrays: the definition that the device passes (l2_postings.h)
// are measured against, and the entry point for batches already fetched to the host (sp_match_batch_postings).
// Host only: no HIP header and no HIP call in here.
//
// The rule (include/strus_pattern_amd.h "batch postings"; the project's own, unpinned by a reference vector).  Term record i
// of document d, at index t inside d's block, has the entry term_dict[i] of the dictionary (match_dict.hpp).  Its posting is
// {d, t, count, first_ordpos}; the postings of entry e lie at [entry_offsets[e], entry_offsets[e+1]), the exclusive prefix
// sums of doc_freq, in ascending order of i, and record_posting[i] is the index of i's posting.  A counting sort.
#ifndef SPA_MATCH_POSTINGS_HPP
#define SPA_MATCH_POSTINGS_HPP
#include "match_dict.hpp"

namespace spa {

// the host arrays of the postings of `nterms` term records and `ndict` entries: postings and offsets zeroed, record_posting
// all 0xFFFFFFFF (sp_match_postings_free)
void allocMatchPostings( sp_match_postings_t* out, size_t ndocs, uint64_t nterms, uint64_t ndict);

// The postings on the host.  Throws std::runtime_error for arguments that make no terms batch with its dictionary.
void matchPostings( const sp_match_term_t* records, uint64_t nrecords, const uint64_t* docTermOffsets, size_t ndocs,
		    const sp_dict_term_t* entries, uint64_t ndict, const uint32_t* termDict, sp_match_postings_t* out);

} // namespace
#endif
