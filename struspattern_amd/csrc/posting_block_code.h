// The code of one posting list of a posting block (include/strus_pattern_amd.h "posting blocks"): one copy of the rule for the
// device-free twin (match_postingblocks.cpp), the reader (sp_match_posting_blocks_decode_block) and the device passes
// (l2_postingblocks_kernel.hip).  The varints are those of term_block_code.h.  No HIP header in here.
//
// The code of a list is the varint `body` -- the bytes of the posting codes that follow, 64 bits -- and per posting the header
// ddelta, count, npos (three varints of 32 bits, 15 bytes at most) and npos position gaps (5 bytes at most each).  The bytes of a
// list are the pieces of its OCCURRENCES one behind the other: the first occurrence of the first posting carries `body`, the
// first occurrence of a posting carries its header, and every occurrence with a new ordpos carries its gap; an occurrence that
// repeats the ordpos before it carries nothing.  So one occurrence gives at most 10 + 15 + 5 = 30 bytes: a term-block header row.
// A posting without an occurrence (none of this library has one) has nobody to carry its header and costs nothing.
// The sizing pass and the emitting pass of the device, and the twin, all go through postingOccurrenceBytes: there is one
// statement of what a posting costs, the sum of it over the posting's occurrences.
#ifndef SPA_POSTING_BLOCK_CODE_H
#define SPA_POSTING_BLOCK_CODE_H
#include "term_block_code.h"

namespace spa {

enum { POSTING_BLOCK_HEADER_MAX = 15 };		// ddelta, count, npos
enum { POSTING_BLOCK_GAP_MAX = 5 };
enum { POSTING_BLOCK_OCCURRENCE_MAX = TERM_BLOCK_VARINT_MAX + POSTING_BLOCK_HEADER_MAX + POSTING_BLOCK_GAP_MAX };	// 30

// the three fields in front of the positions of a posting
struct PostingBlockHeader
{
	uint32_t ddelta;	// the document for the first posting of a list, otherwise the document less the one before
	uint32_t count;		// the term frequency: the number of occurrences
	uint32_t npos;		// the number of distinct ordinal positions: the gaps that follow
};

// (documents that do not ascend, which no postings of this library have, wrap in 32 bits)
SPA_TB_HD PostingBlockHeader postingBlockHeader( bool firstOfList, uint32_t doc, uint32_t docBefore, uint32_t count, uint32_t npos)
{
	PostingBlockHeader h;
	h.ddelta = firstOfList ? doc : doc - docBefore;
	h.count = count;
	h.npos = npos;
	return h;
}

SPA_TB_HD uint32_t postingHeaderBytes( const PostingBlockHeader& h) { return varintBytes( h.ddelta) + varintBytes( h.count) + varintBytes( h.npos); }

// the bytes of the gap of an occurrence at `ordpos` whose posting had `ordposBefore` before it: the position as it is for the
// first occurrence of a posting, nothing for a repeated position, else the difference (positions that descend wrap in 32 bits)
SPA_TB_HD uint32_t positionGapBytes( bool firstOfPosting, uint32_t ordpos, uint32_t ordposBefore)
{
	if (firstOfPosting) return varintBytes( ordpos);
	return ordpos == ordposBefore ? 0u : varintBytes( ordpos - ordposBefore);
}

// what one occurrence adds to the code of its posting: the header with the first, and its gap
SPA_TB_HD uint32_t postingOccurrenceBytes( bool firstOfPosting, const PostingBlockHeader& h, uint32_t ordpos, uint32_t ordposBefore)
{
	return (firstOfPosting ? postingHeaderBytes( h) : 0u) + positionGapBytes( firstOfPosting, ordpos, ordposBefore);
}

// Writes the up to three pieces of one occurrence to dst (room for POSTING_BLOCK_OCCURRENCE_MAX bytes): `body` if it is the first
// of its list, the header if it is the first of its posting, its gap if its position is new.  Returns their bytes:
// (firstOfList ? varintBytes( body) : 0) + postingOccurrenceBytes( ..).
SPA_TB_HD uint32_t writePostingOccurrence( uint8_t* dst, bool firstOfList, uint64_t body, bool firstOfPosting, const PostingBlockHeader& h,
					    uint32_t ordpos, uint32_t ordposBefore)
{
	uint32_t n = 0;
	if (firstOfList) n += writeVarint( dst, body);
	if (firstOfPosting)
	{
		n += writeVarint( dst + n, h.ddelta);
		n += writeVarint( dst + n, h.count);
		n += writeVarint( dst + n, h.npos);
		n += writeVarint( dst + n, ordpos);
	}
	else if (ordpos != ordposBefore) n += writeVarint( dst + n, ordpos - ordposBefore);
	return n;
}

// the bytes of a whole list: `body` in front of its posting codes
SPA_TB_HD uint64_t postingListBytes( uint64_t body) { return (uint64_t)varintBytes( body) + body; }

} // namespace
#endif
