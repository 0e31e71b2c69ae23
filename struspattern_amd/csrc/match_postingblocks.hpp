// Posting blocks of a dictionary, its order, its postings and their positions over host arrays: the definition that the device
// passes (l2_postingblocks.h) are measured against, the entry point for arrays already fetched to the host
// (sp_match_batch_posting_blocks) and the reader of the format (sp_match_posting_blocks_decode_block).  Host only: no HIP
// header and no HIP call in here.  It needs no batch and no source.
//
// The rule (include/strus_pattern_amd.h "posting blocks"; the project's own, unpinned by a reference vector).  Block j covers the
// sorted positions [jB, min((j+1)B, ndict)), B that of the term blocks.  The code of position k is the varint `body` and, for
// every posting of the list of order[k], the varints ddelta, count, npos and npos position gaps; occurrences that repeat a
// position give no byte.  posting_block_code.h composes what an occurrence adds, for this file and for the device alike.
#ifndef SPA_MATCH_POSTINGBLOCKS_HPP
#define SPA_MATCH_POSTINGBLOCKS_HPP
#include "match_termblocks.hpp"
#include "match_positions.hpp"

namespace spa {

// the host arrays of `nblocks` blocks of B positions over `ndict` entries, without the bytes: the offsets zeroed
// (sp_match_posting_blocks_free) ...
void allocMatchPostingBlocks( sp_match_posting_blocks_t* out, uint64_t ndict, uint64_t nblocks, uint32_t blockEntries);
// ... and the bytes, one more than nbytes
void allocMatchPostingBlockBytes( sp_match_posting_blocks_t* out, uint64_t nbytes);

// The blocks on the host.  Throws std::runtime_error for arrays that are not an order, postings and positions of one dictionary.
void matchPostingBlocks( const sp_dict_term_t* entries, uint64_t ndict, const uint32_t* order, const sp_posting_t* postings,
			 const uint64_t* entryOffsets, uint64_t nterms, const sp_occurrence_t* occurrences, const uint64_t* postingOffsets,
			 const uint32_t* postingPositions, uint64_t nocc, uint32_t blockEntries, sp_match_posting_blocks_t* out);

} // namespace
#endif
