// What the post-passes over the documents of a batch share (l2_finish_kernel.hip, l2_text_kernel.hip, l1_stitch_kernel.hip).
// Each of them is count / offsets / place: pass A counts what every document gives, a wave per document; pass B turns the
// counts into offsets, one workgroup; pass C writes every document to its offset, a wave per document again.
#ifndef SPA_DOC_PASSES_H
#define SPA_DOC_PASSES_H
#include <stddef.h>
#include "wave_scan.h"

namespace spa {

const u64 MAX32 = 0xFFFFFFFFull;
typedef u32x4 u32x4u __attribute__((aligned(4)));	// a 16-byte load from a 4-byte aligned address (records are 36 and 28 bytes)

// ---- 64-bit values in a wave
__device__ __forceinline__ u64 uni64( u64 v) { return ((u64)uni( (u32)(v >> 32)) << 32) | uni( (u32)v); }
// inclusive prefix sum of 64 values of 32 bits in 64 bits: the two 16-bit halves cannot overflow the 32-bit scans
__device__ __forceinline__ u64 waveScanAdd64( u32 v) { return ((u64)waveScanAdd( v >> 16) << 16) + waveScanAdd( v & 0xFFFFu); }
// the value of one lane, wave-uniform (lane 63 of an inclusive scan: its sum)
__device__ __forceinline__ u64 waveLane64( u64 v, int lane)
{
	return ((u64)uni( (u32)__shfl( (int)(u32)(v >> 32), lane)) << 32) | uni( (u32)__shfl( (int)(u32)v, lane));
}

// ---- passes A and C: the next document of a wave, from the device cursor.
// The two wave barriers keep the lane-0 branch here apart from the code around the call.  The callers loop
// "for (;;) { doc = nextDocument(..); .. if (LANE == 0) write the document's counts; }": without the barriers the compiler
// may merge the lane-0 branch at the end of the loop body with the one here into a single lane-0 region that spans the
// back edge.  The other lanes would then go round without ever taking a new document.  The first barrier separates the
// ticket from what comes before it (the end of the previous trip), the second from what follows.
__device__ __forceinline__ u32 nextDocument( u32* cursor)
{
	__builtin_amdgcn_wave_barrier();
	u32 doc = 0;
	if (LANE == 0) doc = atomicAdd( cursor, 1u);
	__builtin_amdgcn_wave_barrier();
	return uni( doc);
}

// The workgroups (of 4 waves) of a wave-per-document pass: a wave for every document up to 16 waves per CU.  The passes
// that walk results or lexems are copies at heart, and 16 waves per CU keep enough 16-byte accesses in flight for them.
inline unsigned wavePerDocumentBlocks( size_t ndocs, unsigned numCUs)
{
	const size_t slots = (size_t)numCUs * 16;
	const unsigned waves = (unsigned)(ndocs < slots ? (ndocs ? ndocs : 1) : slots);
	return (waves + 3) / 4;
}

// ---- pass B: exclusive prefix sums of N counts per document, for one workgroup of 1024 threads (16 waves).
// A tile of 1024 documents per round, a thread per document: a scan inside every wave, the sums of the waves through LDS
// (two barriers per tile, paid once for all N counts), the sums of the tiles before carried in 64 bits.
//   T                  the width of the sums inside a tile: u64, or u32 where the caller knows that the sum of all its
//                      counts fits 32 bits (half the scans and half the LDS traffic; profiles/doc_passes_refactor_perf.json)
//   load( d)           the counts of document d (what a document that does not count gives is the caller's: zeros)
//   store( d, k, at)   gets the counts back with their exclusive offsets
// Returns the totals, to every thread.
template <int N> struct DocCounts { u32 v[ N]; };
template <int N> struct DocSums { u64 v[ N]; };

template <class T> __device__ __forceinline__ T waveScanAddAs( u32 v);
template <> __device__ __forceinline__ u32 waveScanAddAs<u32>( u32 v) { return waveScanAdd( v); }
template <> __device__ __forceinline__ u64 waveScanAddAs<u64>( u32 v) { return waveScanAdd64( v); }

template <class T, int N, class LOAD, class STORE>
__device__ __forceinline__ DocSums<N> scanDocumentCounts( u64 ndocs, LOAD load, STORE store)
{
	__shared__ T waveSum[ N][ 16];
	const u32 wave = threadIdx.x >> 6;
	DocSums<N> base = {};
	for (u64 t0=0; t0<ndocs; t0+=1024)
	{
		const u64 d = t0 + threadIdx.x;
		DocCounts<N> k = {};
		if (d < ndocs) k = load( d);
		T incl[ N], before[ N], tile[ N];
		for (int i=0; i<N; ++i) { incl[ i] = waveScanAddAs<T>( k.v[ i]); before[ i] = 0; tile[ i] = 0; }
		if (LANE == 63) for (int i=0; i<N; ++i) waveSum[ i][ wave] = incl[ i];
		__syncthreads();
		for (u32 w=0; w<16; ++w) for (int i=0; i<N; ++i)
		{
			const T a = waveSum[ i][ w];
			before[ i] += w < wave ? a : (T)0;	// (a select, not a branch: the compiler keeps the 16-byte LDS reads)
			tile[ i] += a;
		}
		DocSums<N> at;
		for (int i=0; i<N; ++i) at.v[ i] = base.v[ i] + before[ i] + (incl[ i] - k.v[ i]);
		if (d < ndocs) store( d, k, at);
		for (int i=0; i<N; ++i) base.v[ i] += tile[ i];
		__syncthreads();
	}
	return base;
}

} // namespace
#endif
