// Index terms of a finished batch over host arrays: the definition that the device passes (l2_terms.h) are measured
// against, and the entry point for batches already fetched to the host (sp_match_batch_terms).
// Host only: no HIP header and no HIP call in here.
//
// The rule (include/strus_pattern_amd.h "index terms"; the project's own, unpinned by a reference vector).  A term of a
// document is a pair (handle, value bytes); the value of result r is its range in one of up to two sources (bytes plus
// nresults+1 offsets parallel to the results), chosen per result.  A document gives one 24-byte record per distinct term,
// ascending by (handle, first_result), and every result the index of its term inside the document's block.  A document
// with a source status or with a handle outside 1 .. handleBound-1 has term status SP_DOC_ERR_RANGE, no records and
// result_term 0xFFFFFFFF throughout.
#ifndef SPA_MATCH_TERMS_HPP
#define SPA_MATCH_TERMS_HPP
#include "../../include/strus_pattern_amd.h"
#include <cstddef>
#include <cstdint>

namespace spa {

// one source of term values: NULL offsets = not given
struct TermSource
{
	const char* bytes;
	const uint64_t* offsets;	// nresults+1
	uint64_t total;			// bytes of `bytes`
	const int32_t* docStatus;	// ndocs, may be NULL
};

// the host arrays of the terms of `ndocs` documents and `nresults` results, everything but the records: offsets and status
// zeroed, result_term all 0xFFFFFFFF (sp_match_terms_free)
void allocMatchTerms( sp_match_terms_t* out, size_t ndocs, uint64_t nresults, uint32_t handleBound, uint32_t flags);
// the records, once their number is known
void allocMatchTermRecords( sp_match_terms_t* out, uint64_t nrecords);

// the terms of a batch on the host: source[0] the values, source[1] the text; resultFormat may be NULL; throws
// std::runtime_error for arguments that make no batch
void matchTerms( const sp_result_t* results, uint64_t nresults, const uint64_t* docOffsets, const int32_t* docStatus,
		 const uint32_t* resultFormat, size_t ndocs, const TermSource (&source)[ 2], uint32_t handleBound, uint32_t flags,
		 sp_match_terms_t* out);

} // namespace
#endif
