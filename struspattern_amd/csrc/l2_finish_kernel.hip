// Finishing passes of a device batch (l2_finish.h): count, offsets, place.
#include <hip/hip_runtime.h>
#include "l2_device.h"
#include "l2_finish.h"

using namespace spa;

namespace {

typedef u32x4 u32x4u __attribute__((aligned(4)));	// a 16-byte load from a 4-byte aligned address (records are 36 and 28 bytes)

__device__ __forceinline__ u64 uni64( u64 v) { return ((u64)uni( (u32)(v >> 32)) << 32) | uni( (u32)v); }

// The next document of a wave, from the device cursor.  The wave barriers keep the lane-0 branch here apart from a lane-0
// branch at the end of the caller's loop body: merged with it, the other lanes would go round without a new document.
__device__ __forceinline__ u32 nextDocument( u32* cursor)
{
	__builtin_amdgcn_wave_barrier();
	u32 doc = 0;
	if (LANE == 0) doc = atomicAdd( cursor, 1u);
	__builtin_amdgcn_wave_barrier();
	return uni( doc);
}

// The raw blocks of document d: results [first, first+count), items [itemFirst, itemFirst+itemCount).  False when the
// document counts as empty: it failed, its range does not fit the buffer (the two conditions of copyOutBatch), or it has no results.
__device__ __forceinline__ bool docBlocks( const FinishParams& P, u32 d, u64& first, u64& count, u64& itemFirst, u64& itemCount)
{
	const u64 devResults = P.nofResults, devItems = P.nofItems;
	first = P.docRange[ 2*(u64)d]; count = P.docRange[ 2*(u64)d+1];
	itemFirst = 0; itemCount = 0;
	if (P.docStatus[ d] != 0 || count == 0 || count > devResults || first > devResults - count) return false;
	// one item block per document, item_begin = block start + item counts before (l2_finish.h)
	const u32* r0 = P.results + 9*first;
	const u32* rl = P.results + 9*(first + count - 1);
	itemFirst = r0[ 7];
	itemCount = (u32)(rl[ 7] + rl[ 8] - r0[ 7]);
	return itemCount <= devItems && itemFirst <= devItems - itemCount;
}

// ---- pass A without `exclusive`: every result of a good document survives; a thread per document
__device__ void countDocuments( const FinishParams& P)
{
	for (u64 d = (u64)blockIdx.x*blockDim.x + threadIdx.x; d < P.ndocs; d += (u64)gridDim.x*blockDim.x)
	{
		u64 first, count, itemFirst, itemCount;
		const bool ok = docBlocks( P, (u32)d, first, count, itemFirst, itemCount);
		P.kept[ 2*d] = ok ? (u32)count : 0u;
		P.kept[ 2*d+1] = ok ? (u32)itemCount : 0u;
	}
}

// ---- pass A with `exclusive`: a wave per document marks the covered results (src/patternMatcher.cpp:192-246), a lane
// per result ai walking ni = ai, ai+1, .. to the reference's break condition.  The marks are idempotent and depend on
// the two records only, so all ai at once give the flags of the sequential loop.
__device__ void markDocuments( const FinishParams& P)
{
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor);
		if (doc >= P.ndocs) break;
		u64 first, count, itemFirst, itemCount;
		const bool ok = uni( docBlocks( P, doc, first, count, itemFirst, itemCount) ? 1u : 0u) != 0;
		u32 kept = 0, keptItems = 0;
		if (ok)
		{
			first = uni64( first);
			const u32 n = uni( (u32)count);
			const u32* R = P.results + 9*first;
			uint8_t* C = P.covered + first;
			for (u32 base=0; base<n; base+=64)
			{
				const u32 ai = base + LANE;
				if (ai >= n) continue;
				const u32* r = R + 9*(u64)ai;
				const u32 rseg = r[ 3], rpos = r[ 4], rendseg = r[ 5], rend = r[ 6];
				bool cov = false;
				for (u32 ni=ai; ni<n; ++ni)
				{
					const u32* f = R + 9*(u64)ni;
					const u32 fseg = f[ 3], fpos = f[ 4], fendseg = f[ 5], fend = f[ 6];
					if (fseg > rendseg || fpos >= rend + P.maxResultSize) break;
					const bool differ = (fendseg != rendseg || fend != rend || fseg != rseg || fpos != rpos);
					if (fseg <= rseg && fpos <= rpos && fendseg >= rendseg && fend >= rend && differ) cov = true;
					if (fseg >= rseg && fpos >= rpos && fendseg <= rendseg && fend <= rend && differ) C[ ni] = 1;
				}
				if (cov) C[ ai] = 1;
			}
			__threadfence();		// the flags of the other lanes, before they are counted
			for (u32 base=0; base<n; base+=64)
			{
				const u32 ri = base + LANE;
				const bool keep = ri < n && C[ ri] == 0;
				const u32 ic = keep ? R[ 9*(u64)ri + 8] : 0u;
				kept += (u32)__popcll( __ballot( keep));
				keptItems += uni( (u32)__shfl( (int)waveScanAdd( ic), 63));
			}
		}
		if (LANE == 0) { P.kept[ 2*(u64)doc] = kept; P.kept[ 2*(u64)doc+1] = keptItems; }
	}
}

// ---- pass B: exclusive prefix sums over the documents; one workgroup of 16 waves, a tile of 1024 documents per round.
// (The sums of a batch fit 32 bits, as the buffers hold at most 2^32-1 records; the offsets are 64 bit by contract.)
__device__ void scanDocuments( const FinishParams& P)
{
	__shared__ u32 waveSum[ 2][ 16];
	const u32 wave = threadIdx.x >> 6;
	u64 rbase = 0, ibase = 0;
	for (u64 t0=0; t0<P.ndocs; t0+=1024)
	{
		const u64 d = t0 + threadIdx.x;
		u32 k = 0, it = 0;
		if (d < P.ndocs) { const uint2 v = ((const uint2*)P.kept)[ d]; k = v.x; it = v.y; }
		const u32 ki = waveScanAdd( k), ii = waveScanAdd( it);
		if (LANE == 63) { waveSum[ 0][ wave] = ki; waveSum[ 1][ wave] = ii; }
		__syncthreads();
		u32 kb = 0, ib = 0, kt = 0, itot = 0;
		for (u32 w=0; w<16; ++w)
		{
			const u32 a = waveSum[ 0][ w], b = waveSum[ 1][ w];
			if (w < wave) { kb += a; ib += b; }
			kt += a; itot += b;
		}
		if (d < P.ndocs) { P.docResultOffsets[ d] = rbase + kb + (ki - k); P.docItemOffsets[ d] = ibase + ib + (ii - it); }
		rbase += kt; ibase += itot;
		__syncthreads();
	}
	if (threadIdx.x == 0)
	{
		P.docResultOffsets[ P.ndocs] = rbase; P.docItemOffsets[ P.ndocs] = ibase;
		P.totals[ 0] = rbase; P.totals[ 1] = ibase;
	}
}

// ---- pass C
// The word of a result record that is its item_begin gets `delta` added; r = (index of v.x in the block) mod 9
__device__ __forceinline__ void rebase( u32x4& v, u32 r, u32 delta)
{
	if (r == 7) v.x += delta; else if (r == 6) v.y += delta; else if (r == 5) v.z += delta; else if (r == 4) v.w += delta;
}
__device__ __forceinline__ u32 mod9( u32 r) { return r >= 9 ? r - 9 : r; }

// Streaming copy of n words by one wave: 16-byte stores to the aligned part of dst, 16-byte loads from wherever that
// leaves src (blocks are 4-byte aligned only), up to 3 single words at the head and at the tail.  REBASE: the block is a
// run of result records starting with a whole one, and word 7 of every 9 gets `delta` added.
template <bool REBASE>
__device__ __forceinline__ void copyWords( u32* dst, const u32* src, u64 n, u32 delta)
{
	u32 head = (4u - (u32)(((uintptr_t)dst >> 2) & 3u)) & 3u;
	if (head > n) head = (u32)n;
	if (LANE < head) dst[ LANE] = src[ LANE];		// (words 0..2 of a record: nothing to rebase)
	const u64 nvec = (n - head) >> 2;
	const u32x4u* s = (const u32x4u*)(src + head);
	u32x4* t = (u32x4*)(dst + head);
	u32 r = (head + 4*LANE) % 9;			// 64 vectors on: 256 words = 4 mod 9
	u64 v = LANE;
	for (; v + 192 < nvec; v += 256)
	{
		u32x4 a = s[ v], b = s[ v+64], c = s[ v+128], d = s[ v+192];
		if (REBASE)
		{
			const u32 r1 = mod9( r + 4), r2 = mod9( r1 + 4), r3 = mod9( r2 + 4);
			rebase( a, r, delta); rebase( b, r1, delta); rebase( c, r2, delta); rebase( d, r3, delta);
			r = mod9( r3 + 4);
		}
		t[ v] = a; t[ v+64] = b; t[ v+128] = c; t[ v+192] = d;
	}
	for (; v < nvec; v += 64)
	{
		u32x4 a = s[ v];
		if (REBASE) { rebase( a, r, delta); r = mod9( r + 4); }
		t[ v] = a;
	}
	const u64 done = head + 4*nvec;
	if (LANE < (u32)(n - done))
	{
		u32 x = src[ done + LANE];
		if (REBASE && (done + LANE) % 9 == 7) x += delta;
		dst[ done + LANE] = x;
	}
}

__device__ void placeDocuments( const FinishParams& P)
{
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor + 1);
		if (doc >= P.ndocs) break;
		const u64 rp = uni64( P.docResultOffsets[ doc]), nk = uni64( P.docResultOffsets[ doc+1]) - rp;
		const u64 ip = uni64( P.docItemOffsets[ doc]), nki = uni64( P.docItemOffsets[ doc+1]) - ip;
		if (nk == 0) continue;
		if (rp + nk > P.nofResults || ip + nki > P.nofItems) continue;	// (the survivors are a subset: what the host sized holds them)
		const u64 first = uni64( P.docRange[ 2*(u64)doc]);
		const u32* R = P.results + 9*first;
		if (!P.exclusive)
		{
			// every result survives: two blocks move as they are, item_begin rebased by the document's constant
			const u64 itemFirst = uni( R[ 7]);
			copyWords<true>( P.outResults + 9*rp, R, 9*nk, (u32)ip - (u32)itemFirst);
			copyWords<false>( P.outItems + 7*ip, P.items + 7*itemFirst, 7*nki, 0);
			if (P.withFormats)
			{
				copyWords<false>( P.outResultFormat + rp, P.resultFormat + first, nk, 0);
				copyWords<false>( P.outItemFormat + 2*ip, P.itemFormat + 2*itemFirst, 2*nki, 0);
			}
		}
		else
		{
			// a lane per result: the survivors keep their order, rank by ballot, items by prefix sum of their counts
			const u32 n = uni( (u32)P.docRange[ 2*(u64)doc+1]);
			const uint8_t* C = P.covered + first;
			u64 rat = rp, iat = ip;
			for (u32 base=0; base<n; base+=64)
			{
				const u32 ri = base + LANE;
				const bool keep = ri < n && C[ ri] == 0;
				const u32* r = R + 9*(u64)ri;
				const u32 ib = keep ? r[ 7] : 0u, ic = keep ? r[ 8] : 0u;
				const u64 mask = __ballot( keep);
				const u32 iincl = waveScanAdd( ic);
				if (keep)
				{
					const u64 mine = rat + (u32)__popcll( mask & ((1ull << LANE) - 1ull));
					const u64 myItems = iat + (iincl - ic);
					u32* o = P.outResults + 9*mine;
					for (u32 k=0; k<7; ++k) o[ k] = r[ k];
					o[ 7] = (u32)myItems; o[ 8] = ic;
					const u32* si = P.items + 7*(u64)ib;
					u32* di = P.outItems + 7*myItems;
					for (u32 k=0; k<7*ic; ++k) di[ k] = si[ k];
					if (P.withFormats)
					{
						P.outResultFormat[ mine] = P.resultFormat[ first + ri];
						for (u32 k=0; k<2*ic; ++k) P.outItemFormat[ 2*myItems + k] = P.itemFormat[ 2*(u64)ib + k];
					}
				}
				rat += (u32)__popcll( mask);
				iat += uni( (u32)__shfl( (int)iincl, 63));
			}
		}
	}
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l2_finish_count_kernel( FinishParams P) { countDocuments( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_finish_mark_kernel( FinishParams P) { markDocuments( P); }
extern "C" __global__ __launch_bounds__(1024) void spa_l2_finish_offsets_kernel( FinishParams P) { scanDocuments( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_finish_place_kernel( FinishParams P) { placeDocuments( P); }

namespace spa {
hipError_t launchL2Finish( const FinishParams& P, unsigned numCUs, hipStream_t stream, hipEvent_t* ev)
{
	// a wave per document in the passes that walk results; 16 waves per CU keep enough 16-byte accesses in flight for the copy
	const size_t slots = (size_t)numCUs * 16;
	const unsigned waves = (unsigned)(P.ndocs < slots ? (P.ndocs ? P.ndocs : 1) : slots);
	hipError_t e;
	if (ev && (e = hipEventRecord( ev[ 0], stream)) != hipSuccess) return e;
	if (P.exclusive) hipLaunchKernelGGL( spa_l2_finish_mark_kernel, dim3( (waves + 3) / 4), dim3( 256), 0, stream, P);
	else
	{
		unsigned blocks = P.ndocs / 256 + 1;		// a thread per document, grid-stride beyond 1024 workgroups
		if (blocks > 1024) blocks = 1024;
		hipLaunchKernelGGL( spa_l2_finish_count_kernel, dim3( blocks), dim3( 256), 0, stream, P);
	}
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (ev && (e = hipEventRecord( ev[ 1], stream)) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l2_finish_offsets_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (ev && (e = hipEventRecord( ev[ 2], stream)) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l2_finish_place_kernel, dim3( (waves + 3) / 4), dim3( 256), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (ev && (e = hipEventRecord( ev[ 3], stream)) != hipSuccess) return e;
	return hipSuccess;
}
}
