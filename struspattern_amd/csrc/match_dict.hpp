// Batch dictionary of a terms batch over host arrays: the definition that the device passes (l2_dict.h) are measured against,
// and the entry point for batches already fetched to the host (sp_match_batch_dictionary).
// Host only: no HIP header and no HIP call in here.
//
// The rule (include/strus_pattern_amd.h "batch dictionary"; the project's own, unpinned by a reference vector).  A term record
// (match_terms.hpp) names its value through first_result: the range of that result in the source that the flags select.
// The dictionary has one 32-byte entry per distinct (handle, value bytes) of all records, in the order of the first record
// with the term, and for every record the index of its entry; doc_freq counts the records, count sums and max_count
// maximises their per-document counts.
#ifndef SPA_MATCH_DICT_HPP
#define SPA_MATCH_DICT_HPP
#include "match_terms.hpp"

namespace spa {

// the host arrays of a dictionary of `ndocs` documents and `nterms` term records, everything but the records: offsets and
// handle_terms zeroed, term_dict all 0xFFFFFFFF (sp_match_dictionary_free)
void allocMatchDictionary( sp_match_dictionary_t* out, size_t ndocs, uint64_t nterms, uint32_t handleBound, uint32_t flags);
// the records (zeroed), once their number is known
void allocMatchDictionaryRecords( sp_match_dictionary_t* out, uint64_t ndict);

// The dictionary of the term records on the host: source[0] the values, source[1] the text (those that `flags` selects are
// read); resultFormat may be NULL.  Throws std::runtime_error for arguments that make no terms batch.
void matchDictionary( const sp_match_term_t* records, uint64_t nrecords, const uint64_t* docTermOffsets, const uint64_t* docOffsets,
		      uint64_t nresults, const uint32_t* resultFormat, size_t ndocs, const TermSource (&source)[ 2], uint32_t handleBound,
		      uint32_t flags, sp_match_dictionary_t* out);

} // namespace
#endif
