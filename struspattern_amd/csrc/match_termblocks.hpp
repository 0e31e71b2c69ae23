// Term blocks of a dictionary and its order over host arrays: the definition that the device passes (l2_termblocks.h) are
// measured against, the entry point for batches already fetched to the host (sp_match_batch_term_blocks), the reader of the
// format (sp_match_term_blocks_decode_block) and the block size that both sides code with.  Host only: no HIP header and no HIP
// call in here.
//
// The rule (include/strus_pattern_amd.h "term blocks"; the project's own, unpinned by a reference vector).  Block j covers the
// sorted positions [jB, min((j+1)B, ndict)).  The code of position k is the five varints hdelta, shared, suffix, doc_freq,
// count and the suffix bytes of the value of order[k]; hdelta and shared are 0 at the head of a block, so that a block decodes
// from its own bytes and block_handles[j].  term_block_code.h composes a code, for this file and for the device alike.
#ifndef SPA_MATCH_TERMBLOCKS_HPP
#define SPA_MATCH_TERMBLOCKS_HPP
#include "match_dictorder.hpp"

namespace spa {

// B: TERM_BLOCK_ENTRIES unless sp_test_term_block_entries chose another
uint32_t termBlockEntries();

// the host arrays of `nblocks` blocks of B positions over `ndict` entries, without the bytes: the offsets zeroed, the handles
// all 0xFFFFFFFF (sp_match_term_blocks_free) ...
void allocMatchTermBlocks( sp_match_term_blocks_t* out, uint64_t ndict, uint64_t nblocks, uint32_t blockEntries);
// ... and the bytes, one more than nbytes
void allocMatchTermBlockBytes( sp_match_term_blocks_t* out, uint64_t nbytes);

// The blocks on the host: value[e] the value of entry e (dictionaryValues), order and prefixBytes those of the dictionary's
// order.  Throws std::runtime_error for an order that is none of this dictionary.
void matchTermBlocks( const sp_dict_term_t* entries, uint64_t ndict, const std::vector<std::string_view>& value, const uint32_t* order,
		      const uint32_t* prefixBytes, uint32_t blockEntries, sp_match_term_blocks_t* out);

} // namespace
#endif
