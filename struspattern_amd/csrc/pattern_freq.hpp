// Pattern frequencies of a finished batch over host arrays: the definition that the device passes (l2_freq.h) are measured
// against, and the entry point for batches already fetched to the host (sp_match_batch_pattern_freq).
// Host only: no HIP header and no HIP call in here.
//
// The rule (DESIGN.md 5 "Pattern frequencies"; the project's own, unpinned by a reference vector).  Valid handles are
// 1 .. handleBound-1.  A document whose results all carry a valid handle gives one record per distinct handle, ascending by
// handle: (handle, count of its results, minimum of their ordpos, maximum of their ordend), all unsigned.  A document with
// a handle of 0 or of handleBound and more has frequency status SP_DOC_ERR_RANGE and no records.  A document without results
// (one the matcher failed among them) has no records and status 0.  handleResults[h] is the sum of the counts of the records
// with handle h, handleDocs[h] their number; index 0 stays 0.
#ifndef SPA_PATTERN_FREQ_HPP
#define SPA_PATTERN_FREQ_HPP
#include "../../include/strus_pattern_amd.h"
#include <cstddef>
#include <cstdint>

namespace spa {

// the host arrays of the frequencies of `ndocs` documents under `handleBound`, everything but the records, zeroed
// (sp_pattern_freq_batch_free)
void allocPatternFreq( sp_pattern_freq_batch_t* out, size_t ndocs, uint32_t handleBound);
// the records, once their number is known
void allocPatternFreqRecords( sp_pattern_freq_batch_t* out, uint64_t nrecords);

// the frequencies of a batch on the host: the results of document d are [docOffsets[d], docOffsets[d+1]); docStatus may be
// NULL; throws std::runtime_error for arguments that make no batch
void patternFreq( const sp_result_t* results, uint64_t nresults, const uint64_t* docOffsets, const int32_t* docStatus,
		  size_t ndocs, uint32_t handleBound, sp_pattern_freq_batch_t* out);

} // namespace
#endif
