// Term blocks of a finished device batch (l2_termblocks_kernel.hip): behind l2_dictorder.h on the output side of the matcher, the
// sorted dictionary written as front-coded blocks -- the first product that owns its bytes.  The rule is that of
// match_termblocks.hpp (its device-free twin; include/strus_pattern_amd.h "term blocks" states it); what a position costs and
// how its header is composed is term_block_code.h, the one copy for both sides.
// All launches go on one stream; kernel boundaries are the only ordering between waves, nobody spins on a flag.
//   sizes    a lane per sorted position k, 64 positions a wave: a wave covers 64 / B whole blocks.  The lane reads order[k],
//            prefix_bytes[k] and the dictionary record; the handle of the position before comes from the lane below, lane 0
//            loads it.  Where the value lies and how long it is stays what the order's keys launch left in its working memory
//            (valueAt, valueLen), compared against both sources again: nobody walks entry -> term record -> result -> source a
//            second time.  The code lengths of a block are summed inside the wave (a scan, and the difference of two lanes) to
//            blockSize[j]; the head lane writes block_handles[j]; the sum of value_bytes is reduced in the wave and added with
//            one atomic a wave (a sum: deterministic).
//   offsets  one workgroup: scanDocumentCounts over blockSize in 64 bits (the low and the high word as two counts), and the
//            totals.  The host waits here, once, for nbytes.
//   emit     the same assignment of waves to positions.  The start of a code is block_offsets of its block plus the codes before
//            it in the block, so the output of a wave is one contiguous span.  Every lane composes its header (30 bytes at most)
//            into LDS beside its start and the address of its suffix; then the whole wave writes the span, a lane per aligned
//            output dword: the owner of a byte is found by bisecting the 64 starts, header bytes come from LDS, suffix bytes
//            from the source (copyRange<true> of l2_text_kernel.hip).  The bytes of a dword at an unaligned edge of the span
//            are written as bytes: the neighbouring wave writes the others.
// Whatever the records and the working arrays hold: an entry index is compared against ndict, a source range against its source
// (storedValue), the bytes written for block j are cut to [block_offsets[j], block_offsets[j+1]) and that to the capacity of
// `bytes`; a byte of that range that no code reaches is written as zero.
#ifndef SPA_L2_TERMBLOCKS_H
#define SPA_L2_TERMBLOCKS_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>
#include "l2_terms.h"

namespace spa {

struct TermBlocksParams
{
	// the dictionary, its order and the order's working memory
	const uint32_t* dictRecords;	// 8 words an entry (sp_dict_term_t)
	const uint32_t* order;		// ndict
	const uint32_t* prefixBytes;	// ndict
	const uint64_t* valueAt;	// ndict: the address of the value's first byte
	const uint32_t* valueLen;	// ndict
	uint32_t flags;			// those of the terms call
	TermSourceDevice source[ 2];	// values, text: what valueAt may point into
	uint32_t ndict;
	uint32_t blockEntries;		// B: 1, 2, 4, .. 64
	uint32_t nblocks;		// ceil( ndict / B)
	// working memory
	uint64_t* blockSize;		// nblocks
	// the blocks
	uint8_t* bytes;			// capacity; set after the host's wait
	uint64_t capacity;		// nbytes as the host read it
	uint64_t* blockOffsets;		// nblocks+1
	uint32_t* blockHandles;		// nblocks
	uint64_t* totals;		// 4, zeroed: nblocks, nbytes, B, the sum of value_bytes
};

inline uint64_t l2TermBlocksCount( uint64_t ndict, uint32_t blockEntries) { return (ndict + blockEntries - 1) / blockEntries; }

// sizes and offsets: what the host waits for
hipError_t launchL2TermBlocksCount( const TermBlocksParams& P, unsigned numCUs, hipStream_t stream);
// emit
hipError_t launchL2TermBlocksPlace( const TermBlocksParams& P, unsigned numCUs, hipStream_t stream);

} // namespace
#endif
