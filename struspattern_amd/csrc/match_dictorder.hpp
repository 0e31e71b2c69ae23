// Dictionary order of a terms batch and its dictionary over host arrays: the definition that the device passes
// (l2_dictorder.h) are measured against, and the entry point for batches already fetched to the host
// (sp_match_batch_dictionary_order).  Host only: no HIP header and no HIP call in here.
//
// The rule (include/strus_pattern_amd.h "dictionary order"; the project's own, unpinned by a reference vector).  The value of
// entry e of the dictionary (match_dict.hpp) is that of term record first_term of document first_doc: the range of its
// first_result in the source that the flags select.  order lists the entries ascending by (handle, value bytes) -- handles
// unsigned, bytes as memcmp does, a prefix before what it is a prefix of --, rank is its inverse, prefix_bytes[k] the leading
// bytes that the values at k-1 and k share inside one handle, handle_offsets the exclusive prefix sums of handle_terms.
#ifndef SPA_MATCH_DICTORDER_HPP
#define SPA_MATCH_DICTORDER_HPP
#include "match_dict.hpp"
#include <string_view>
#include <vector>

namespace spa {

// the host arrays of the order of `ndict` entries under `handleBound` handles: order, rank and prefix_bytes all 0xFFFFFFFF,
// the offsets zeroed (sp_match_dictionary_order_free)
void allocMatchDictionaryOrder( sp_match_dictionary_order_t* out, uint64_t ndict, uint32_t handleBound);

// The value of every entry of a dictionary, a view into its source: source[0] the values, source[1] the text (those that `flags`
// selects are read); resultFormat may be NULL.  Throws std::runtime_error for arguments that make no terms batch with its
// dictionary: what matchDictionaryOrder refuses but two entries with the same (handle, bytes).
std::vector<std::string_view> dictionaryValues( const sp_match_term_t* records, uint64_t nrecords, const uint64_t* docTermOffsets, const uint64_t* docOffsets,
						uint64_t nresults, const uint32_t* resultFormat, size_t ndocs, const TermSource (&source)[ 2], uint32_t handleBound,
						uint32_t flags, const sp_dict_term_t* entries, uint64_t ndict, const uint32_t* handleTerms);

// The order on the host: source[0] the values, source[1] the text (those that `flags` selects are read); resultFormat may be
// NULL.  Throws std::runtime_error for arguments that make no terms batch with its dictionary.
void matchDictionaryOrder( const sp_match_term_t* records, uint64_t nrecords, const uint64_t* docTermOffsets, const uint64_t* docOffsets,
			   uint64_t nresults, const uint32_t* resultFormat, size_t ndocs, const TermSource (&source)[ 2], uint32_t handleBound,
			   uint32_t flags, const sp_dict_term_t* entries, uint64_t ndict, const uint32_t* handleTerms,
			   sp_match_dictionary_order_t* out);

} // namespace
#endif
