// Postings passes of a finished device batch (l2_postings.h): keys, offsets, per radix pass histogram / scan / scatter, place.
#include <hip/hip_runtime.h>
#include "doc_passes.h"
#include "l2_postings.h"

using namespace spa;

namespace {

const u32 NONE = 0xFFFFFFFFu;

// The lanes of a wave hand values to each other through the wave's own counters in LDS: what was written before this point is
// read behind it.  The LDS serves the instructions of one wave in order; the fence keeps the compiler from moving them.
__device__ __forceinline__ void waveSync()
{
	__builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
}

// a pair: the key in the low word, the record index in the high one
__device__ __forceinline__ u32 keyOf( u64 pair) { return (u32)pair; }
__device__ __forceinline__ u32 recordOf( u64 pair) { return (u32)(pair >> 32); }
__device__ __forceinline__ u32 digitOf( const PostingsParams& P, u64 pair, u32 pass)
{
	return (keyOf( pair) >> (pass * P.digitBits)) & ((1u << P.digitBits) - 1u);
}

// the pairs [r0, r1) of a tile, wave-uniform (tile < P.tiles, so r0 < N)
__device__ __forceinline__ void tileRecords( const PostingsParams& P, u32 tile, u64& r0, u64& r1)
{
	r0 = (u64)tile * POSTINGS_TILE;
	r1 = r0 + POSTINGS_TILE < P.nterms ? r0 + POSTINGS_TILE : P.nterms;
}

// the 2^digitBits counters of this wave
__device__ __forceinline__ u32* waveCounters( u32 (*counters)[ 1u << POSTINGS_MAX_DIGIT_BITS]) { return counters[ threadIdx.x >> 6]; }

// ---- keys: the document and the pair of every record
__device__ void writeKeys( const PostingsParams& P)
{
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor);
		if (doc >= P.ndocs) break;
		const u64 t0 = uni64( P.docTermOffsets[ doc]), t1 = uni64( P.docTermOffsets[ (u64)doc+1]);
		if (!(t0 < t1 && t1 <= P.nterms)) continue;
		for (u64 t=t0+LANE; t<t1; t+=64)
		{
			u32 key = P.termDict[ t];
			if (key >= P.ndict) key = P.ndict - 1;		// (N >= 1 here and the host launches this for ndict >= 1 only)
			P.docOf[ t] = doc;
			P.pairs[ 0][ t] = ((u64)(u32)t << 32) | key;	// (N < 2^32 - 1)
		}
	}
}

// ---- offsets: where the list of every entry starts
__device__ void scanEntries( const PostingsParams& P)
{
	const u64 total = scanDocumentCounts<u64, 1>( P.ndict,
		[&]( u64 e) { return DocCounts<1>{{ P.dictRecords[ 8*e + 4]}}; },
		[&]( u64 e, const DocCounts<1>&, const DocSums<1>& at) { P.entryOffsets[ e] = at.v[ 0]; }).v[ 0];
	if (threadIdx.x == 0) { P.entryOffsets[ P.ndict] = total; *P.total = total; }
}

// ---- histogram: the digits of every tile, hist[digit][tile]
__device__ void countDigits( const PostingsParams& P, u32 pass)
{
	__shared__ u32 counters[ 4][ 1u << POSTINGS_MAX_DIGIT_BITS];
	u32* mine = waveCounters( counters);
	const u32 ndigits = 1u << P.digitBits;
	const u64* src = P.pairs[ pass & 1];
	for (;;)
	{
		const u32 tile = nextDocument( P.cursor + 2 + 2*pass);
		if (tile >= P.tiles) break;
		u64 r0, r1;
		tileRecords( P, tile, r0, r1);
		for (u32 d=LANE; d<ndigits; d+=64) mine[ d] = 0;
		waveSync();
		for (u64 r=r0+LANE; r<r1; r+=64) atomicAdd( &mine[ digitOf( P, src[ r], pass)], 1u);	// (LDS: a sum, whatever the order)
		waveSync();
		for (u32 d=LANE; d<ndigits; d+=64) P.hist[ (u64)d*P.tiles + tile] = mine[ d];
		waveSync();
	}
}

// ---- scan: every count of hist becomes the number of pairs in front of it, digit-major, tile-minor
__device__ void scanHistogram( const PostingsParams& P)
{
	scanDocumentCounts<u32, 1>( (u64)P.tiles << P.digitBits,
		[&]( u64 k) { return DocCounts<1>{{ P.hist[ k]}}; },
		[&]( u64 k, const DocCounts<1>&, const DocSums<1>& at) { P.hist[ k] = (u32)at.v[ 0]; });
}

// ---- scatter: every pair to its rank in the other buffer
__device__ void scatterPairs( const PostingsParams& P, u32 pass)
{
	__shared__ u32 counters[ 4][ 1u << POSTINGS_MAX_DIGIT_BITS];
	u32* mine = waveCounters( counters);
	const u32 ndigits = 1u << P.digitBits;
	const u64* src = P.pairs[ pass & 1];
	u64* dst = P.pairs[ (pass & 1) ^ 1];
	for (;;)
	{
		const u32 tile = nextDocument( P.cursor + 3 + 2*pass);
		if (tile >= P.tiles) break;
		u64 r0, r1;
		tileRecords( P, tile, r0, r1);
		for (u32 d=LANE; d<ndigits; d+=64) mine[ d] = P.hist[ (u64)d*P.tiles + tile];
		waveSync();
		for (u64 t=r0; t<r1; t+=64)
		{
			const u64 at = t + LANE;
			const bool active = at < r1;
			const u64 pair = active ? src[ at] : 0;
			const u32 d = digitOf( P, pair, pass);
			// the lanes of this trip with the same digit
			u64 peers = __ballot( active);
			for (u32 b=0; b<P.digitBits; ++b)
			{
				const bool bit = (d >> b) & 1u;
				const u64 set = __ballot( active && bit);
				peers &= bit ? set : ~set;
			}
			const u32 lower = (u32)__popcll( peers & ((1ull << LANE) - 1ull));
			u32 rank = NONE;
			if (active) rank = mine[ d] + lower;
			waveSync();
			if (active && lower == 0) mine[ d] = rank + (u32)__popcll( peers);	// (the lowest lane of a digit read its count itself)
			waveSync();
			if (rank < P.nterms) dst[ rank] = pair;
		}
	}
}

// ---- place: the posting of every sorted position, and the way back from its record
__device__ void placePostings( const PostingsParams& P)
{
	const u64* src = P.pairs[ P.passes & 1];
	for (;;)
	{
		const u32 tile = nextDocument( P.cursor + 1);
		if (tile >= P.tiles) break;
		u64 r0, r1;
		tileRecords( P, tile, r0, r1);
		for (u64 p=r0+LANE; p<r1; p+=64)
		{
			const u32 i = recordOf( src[ p]);
			u32x4 posting = { NONE, NONE, NONE, NONE};
			if (i < P.nterms)
			{
				const u32 doc = P.docOf[ i];
				if (doc < P.ndocs)
				{
					const u32* rec = P.terms + 6*(u64)i;
					posting.x = doc; posting.y = i - (u32)P.docTermOffsets[ doc]; posting.z = rec[ 1]; posting.w = rec[ 2];
					P.recordPosting[ i] = (u32)p;
				}
			}
			*(u32x4*)(P.postings + 4*p) = posting;		// (a posting is 16 bytes and the postings are 256-byte aligned)
		}
	}
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l2_postings_keys_kernel( PostingsParams P) { writeKeys( P); }
extern "C" __global__ __launch_bounds__(1024) void spa_l2_postings_offsets_kernel( PostingsParams P) { scanEntries( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_postings_histogram_kernel( PostingsParams P, u32 pass) { countDigits( P, pass); }
extern "C" __global__ __launch_bounds__(1024) void spa_l2_postings_scan_kernel( PostingsParams P) { scanHistogram( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_postings_scatter_kernel( PostingsParams P, u32 pass) { scatterPairs( P, pass); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_postings_place_kernel( PostingsParams P) { placePostings( P); }

namespace spa {

hipError_t launchL2Postings( const PostingsParams& P, unsigned numCUs, hipStream_t stream)
{
	hipError_t e;
	const bool records = P.nterms && P.ndict;	// (without records there are no entries: the offsets are the single 0 and the total)
	const dim3 perTile( wavePerDocumentBlocks( P.tiles, numCUs));
	if (records)
	{
		hipLaunchKernelGGL( spa_l2_postings_keys_kernel, dim3( wavePerDocumentBlocks( P.ndocs, numCUs)), dim3( 256), 0, stream, P);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	hipLaunchKernelGGL( spa_l2_postings_offsets_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess || !records) return e;
	for (u32 pass=0; pass<P.passes; ++pass)
	{
		hipLaunchKernelGGL( spa_l2_postings_histogram_kernel, perTile, dim3( 256), 0, stream, P, pass);
		if ((e = hipGetLastError()) != hipSuccess) return e;
		hipLaunchKernelGGL( spa_l2_postings_scan_kernel, dim3( 1), dim3( 1024), 0, stream, P);
		if ((e = hipGetLastError()) != hipSuccess) return e;
		hipLaunchKernelGGL( spa_l2_postings_scatter_kernel, perTile, dim3( 256), 0, stream, P, pass);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	hipLaunchKernelGGL( spa_l2_postings_place_kernel, perTile, dim3( 256), 0, stream, P);
	return hipGetLastError();
}

}
