// Posting blocks of a finished device batch (l2_postingblocks_kernel.hip): behind l2_dictorder.h, l2_postings.h and l2_positions.h
// on the output side of the matcher, the posting lists of the batch in the sorted order of the dictionary, cut into the blocks of
// the term blocks and delta-coded with varints -- the second product that owns its bytes.  The rule is that of
// match_postingblocks.hpp (its device-free twin; include/strus_pattern_amd.h "posting blocks" states it); what an occurrence
// adds to the code of its posting and how its bytes are composed is posting_block_code.h, the one copy for both sides.
// All launches go on one stream; kernel boundaries are the only ordering between waves, nobody spins on a flag; no atomic
// decides where a byte goes (the one global atomic adds to the number of position varints, the LDS atomics add to the bytes of
// a posting: sums).  No source byte is read.
//   lists    one workgroup: scanDocumentCounts over the length of the list of order[k] (the difference of two entry offsets)
//            into listOffsets[ndict+1].  Sorted posting s then numbers the postings in output order: those of sorted position k are
//            [listOffsets[k], listOffsets[k+1]).
//   sizes    a wave takes the 64 sorted postings [64w, 64w+64).  A lane bisects listOffsets for its k, takes
//            p = entry_offsets[order[k]] + (s - listOffsets[k]) and reads the posting, its occurrence range, posting_positions[p]
//            and the document of the posting before it in the list.  The wave then walks the concatenated occurrences of its 64
//            postings in trips of 64: the owner of an occurrence is found by bisecting the in-wave prefix of the occurrence
//            counts (LDS); the ordpos before comes from the lane below, at the edge of a trip from a load.  Every lane adds
//            postingOccurrenceBytes to its owner (an LDS add).  The result is postingBytes[s], 64 bits.
//   prefix   one workgroup: the exclusive prefix of postingBytes in 64 bits, in place (N+1 values).
//   blocks   a lane per sorted position k: body[k] is the difference of two prefix values, the list costs
//            varintBytes( body) + body; the start of the list inside its block and blockSize[j] come from one 64-bit wave scan,
//            as in the sizes launch of the term blocks.
//   offsets  one workgroup: block_offsets and the totals.  The host waits here, once, for nbytes.
//   emit     the waves and the walk of `sizes`.  The start of posting s is block_offsets[k/B] + the start of list k in its block
//            + varintBytes( body[k]) + its prefix inside the list, so the output of a wave is one contiguous run and that of a
//            trip one contiguous span: every lane composes the at most 30 bytes of its occurrence into its LDS row beside its
//            start (a wave scan of the lengths behind the bytes of the trips before), and the wave writes the span a lane per
//            aligned output dword, the owner of a byte found by bisecting the 64 starts -- the last lane that starts at or
//            before the byte, which skips the lanes that own nothing.  The bytes of a dword at an unaligned edge of the span are
//            written as bytes: the trip or the wave before or behind writes the others.
// Whatever the arrays hold: an entry is compared against ndict, a posting against N, an occurrence against nocc and a document
// against ndocs before use (a posting that fails one of these has no occurrences and costs nothing); the bytes of an occurrence
// are cut to the range of its block, and that to the capacity of `bytes`.  A byte that no code reaches -- there is none for the
// arrays of this library -- keeps what the buffer held.
// Working memory (the context's, it only grows): 8 bytes a posting (postingBytes, then its prefix), 16 a sorted position
// (listOffsets, the start of the list in its block) and 8 a block (blockSize).
#ifndef SPA_L2_POSTINGBLOCKS_H
#define SPA_L2_POSTINGBLOCKS_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>

namespace spa {

struct PostingBlocksParams
{
	// the order, the postings and the positions of one dictionary
	const uint32_t* order;			// ndict
	const uint64_t* entryOffsets;		// ndict+1
	const uint32_t* postings;		// 4 words a posting (sp_posting_t), N
	const uint64_t* postingOffsets;		// N+1
	const uint32_t* postingPositions;	// N
	const uint32_t* occurrences;		// 2 words an occurrence (sp_occurrence_t), nocc
	uint32_t ndict;
	uint32_t ndocs;
	uint64_t nterms;			// N
	uint64_t nocc;
	uint32_t blockEntries;			// B: 1, 2, 4, .. 64
	uint32_t nblocks;			// ceil( ndict / B)
	// working memory
	uint64_t* listOffsets;			// ndict+1
	uint64_t* listStart;			// ndict: where the list starts inside its block
	uint64_t* postingBytes;			// N+1: the bytes of every sorted posting, then their exclusive prefix
	uint64_t* blockSize;			// nblocks
	// the blocks
	uint8_t* bytes;				// capacity; set after the host's wait
	uint64_t capacity;			// nbytes as the host read it
	uint64_t* blockOffsets;			// nblocks+1
	uint64_t* totals;			// 4, zeroed: nblocks, nbytes, B, the position varints written
};

// lists, sizes, prefix, blocks and offsets: what the host waits for
hipError_t launchL2PostingBlocksCount( const PostingBlocksParams& P, unsigned numCUs, hipStream_t stream);
// emit
hipError_t launchL2PostingBlocksPlace( const PostingBlocksParams& P, unsigned numCUs, hipStream_t stream);

} // namespace
#endif
