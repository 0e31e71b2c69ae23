// One pass of a stable LSD radix partition of 8-byte pairs (key in the low word, payload in the high one) over fixed tiles,
// shared by the products that partition something of a finished batch (l2_postings.h: term records by entry; l2_positions.h:
// results by position, then by posting).  Three launches on one stream (radix_passes_kernel.hip):
//   histogram  the pairs are cut into fixed tiles, tile k = the pairs [k*TILE, (k+1)*TILE) of the pass's source buffer; a wave
//              takes a tile from the cursor, counts its digits in LDS and writes hist[digit][tile];
//   scan       one workgroup: the exclusive prefix of hist in (digit-major, tile-minor) order, in 32 bits (count < 2^32 - 1);
//   scatter    the same tiles, in trips of 64 in pair order.  The rank of a lane is its tile's base for its digit + the wave's
//              running count of that digit in LDS + the lower lanes of the trip with the same digit (digitBits ballots); the
//              pair goes to the other buffer.
// The data sees no atomic in HBM and nobody spins on a flag: kernel boundaries are the only ordering between waves, and what
// a wave does depends on its tile alone, never on which wave it is.  So the order that a pass leaves is a function of its
// source buffer: pairs of equal digit keep their order.
// RADIX_TILE: 2048 pairs = 32 trips of a wave.  The passes are copies at heart: they run 16 waves per CU as every
// wave-per-document pass does (wavePerDocumentBlocks), and a wave's 256 digit counters are 1 KiB of LDS, 16 KiB per CU of its
// 160 KiB, so LDS does not bound the residency.  What the tile sets is the size of hist, 256 words per tile = count/8 words,
// which ONE workgroup scans per pass: an eighth of a word per pair, against the four words per pair that the scatter moves; a
// smaller tile makes the scan the longest launch of a pass, a larger one leaves CUs without a tile at a count near 10^5.
// Whatever the buffers hold: a rank is compared against the count before the store, a digit is masked to the counters of the wave.
#ifndef SPA_RADIX_PASSES_H
#define SPA_RADIX_PASSES_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>

namespace spa {

const uint32_t RADIX_TILE = 2048;		// pairs per tile, a multiple of 64
const uint32_t RADIX_MAX_DIGIT_BITS = 8;	// the digit counters of a wave in LDS: 2^8 words

struct RadixPass
{
	const uint64_t* src;		// count pairs
	uint64_t* dst;			// count pairs, another buffer than src
	uint64_t count;			// below 2^32 - 1
	uint32_t tiles;			// radixTiles( count)
	uint32_t digitBits;		// 1..8
	uint32_t shift;			// the digit is (key >> shift) & (2^digitBits - 1)
	uint32_t* hist;			// 2^digitBits x tiles, written whole by the histogram launch
	uint32_t* cursor;		// two zeroed words of this pass: histogram, scatter
};

inline uint32_t radixTiles( uint64_t count) { return (uint32_t)((count + RADIX_TILE - 1) / RADIX_TILE); }
// the words of hist for `count` pairs, whatever the digit
inline size_t radixHistWords( uint64_t count) { return ((size_t)radixTiles( count) + 1) << RADIX_MAX_DIGIT_BITS; }
// the passes that order keys up to `largestKey`: the digits of its bit width
inline uint32_t radixPasses( uint64_t largestKey, uint32_t digitBits)
{
	uint32_t width = 0;
	for (uint64_t k = largestKey; k; k >>= 1) ++width;
	return (width + digitBits - 1) / digitBits;
}
// enqueue the three launches of one pass (count >= 1)
hipError_t launchRadixPass( const RadixPass& R, unsigned numCUs, hipStream_t stream);
// the same with an event after each of the three launches (diagnostics: ev[0..2]); ev == 0: none
hipError_t launchRadixPass( const RadixPass& R, unsigned numCUs, hipStream_t stream, hipEvent_t* ev);

} // namespace

#ifdef __HIP__
// ---- the device side of a pass, for the kernels of radix_passes_kernel.hip (workgroups of 4 waves; the scan: 1024 threads)
#include "doc_passes.h"

namespace spa {

// The lanes of a wave hand values to each other through the wave's own counters in LDS: what was written before this point is
// read behind it.  The LDS serves the instructions of one wave in order; the fence keeps the compiler from moving them.
__device__ __forceinline__ void radixWaveSync()
{
	__builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ u32 radixDigitOf( const RadixPass& R, u64 pair) { return ((u32)pair >> R.shift) & ((1u << R.digitBits) - 1u); }

// the pairs [r0, r1) of a tile, wave-uniform (tile < R.tiles, so r0 < count)
__device__ __forceinline__ void radixTilePairs( u64 count, u32 tile, u64& r0, u64& r1)
{
	r0 = (u64)tile * RADIX_TILE;
	r1 = r0 + RADIX_TILE < count ? r0 + RADIX_TILE : count;
}

// ---- histogram: the digits of every tile, hist[digit][tile]
__device__ __forceinline__ void radixCountDigits( const RadixPass& R)
{
	__shared__ u32 counters[ 4][ 1u << RADIX_MAX_DIGIT_BITS];
	u32* mine = counters[ threadIdx.x >> 6];
	const u32 ndigits = 1u << R.digitBits;
	for (;;)
	{
		const u32 tile = nextDocument( R.cursor);
		if (tile >= R.tiles) break;
		u64 r0, r1;
		radixTilePairs( R.count, tile, r0, r1);
		for (u32 d=LANE; d<ndigits; d+=64) mine[ d] = 0;
		radixWaveSync();
		for (u64 r=r0+LANE; r<r1; r+=64) atomicAdd( &mine[ radixDigitOf( R, R.src[ r])], 1u);	// (LDS: a sum, whatever the order)
		radixWaveSync();
		for (u32 d=LANE; d<ndigits; d+=64) R.hist[ (u64)d*R.tiles + tile] = mine[ d];
		radixWaveSync();
	}
}

// ---- scan: every count of hist becomes the number of pairs in front of it, digit-major, tile-minor
__device__ __forceinline__ void radixScanHistogram( const RadixPass& R)
{
	scanDocumentCounts<u32, 1>( (u64)R.tiles << R.digitBits,
		[&]( u64 k) { return DocCounts<1>{{ R.hist[ k]}}; },
		[&]( u64 k, const DocCounts<1>&, const DocSums<1>& at) { R.hist[ k] = (u32)at.v[ 0]; });
}

// ---- scatter: every pair to its rank in the other buffer
__device__ __forceinline__ void radixScatterPairs( const RadixPass& R)
{
	__shared__ u32 counters[ 4][ 1u << RADIX_MAX_DIGIT_BITS];
	u32* mine = counters[ threadIdx.x >> 6];
	const u32 ndigits = 1u << R.digitBits;
	for (;;)
	{
		const u32 tile = nextDocument( R.cursor + 1);
		if (tile >= R.tiles) break;
		u64 r0, r1;
		radixTilePairs( R.count, tile, r0, r1);
		for (u32 d=LANE; d<ndigits; d+=64) mine[ d] = R.hist[ (u64)d*R.tiles + tile];
		radixWaveSync();
		for (u64 t=r0; t<r1; t+=64)
		{
			const u64 at = t + LANE;
			const bool active = at < r1;
			const u64 pair = active ? R.src[ at] : 0;
			const u32 d = radixDigitOf( R, pair);
			// the lanes of this trip with the same digit
			u64 peers = __ballot( active);
			for (u32 b=0; b<R.digitBits; ++b)
			{
				const bool bit = (d >> b) & 1u;
				const u64 set = __ballot( active && bit);
				peers &= bit ? set : ~set;
			}
			const u32 lower = (u32)__popcll( peers & ((1ull << LANE) - 1ull));
			u32 rank = 0xFFFFFFFFu;
			if (active) rank = mine[ d] + lower;
			radixWaveSync();
			if (active && lower == 0) mine[ d] = rank + (u32)__popcll( peers);	// (the lowest lane of a digit read its count itself)
			radixWaveSync();
			if (rank < R.count) R.dst[ rank] = pair;
		}
	}
}

} // namespace
#endif
#endif
