// Dictionary order passes of a finished device batch (l2_dictorder.h): keys, tiles, merge levels, place, offsets.
#include <hip/hip_runtime.h>
#include "doc_passes.h"
#include "l2_dictorder.h"
#include "l2_term_value.h"

using namespace spa;

namespace {

const u32 NONE = TERM_NONE;		// no entry: the index of a padding entry of a tile, a slot that no valid entry reaches
const u64 PAD_KEY = ~0ull;		// the key of a padding entry: no key is larger
const u32 TILE_THREADS = 256;

// ---- the value of an entry

// The value of entry e (e < P.ndict) by the records: the range of the first_result of term record (first_doc, first_term) in the
// selected source.  Not ok, and empty: a first_doc, first_term or first_result outside its bound, or a range outside the source.
__device__ __forceinline__ TermValue valueOfEntry( const DictOrderParams& P, u32 e)
{
	TermValue v;
	v.p = 0; v.len = 0; v.ok = false;
	const u32* entry = P.dictRecords + 8*(u64)e;
	const u32 doc = entry[ 2], term = entry[ 3];
	if (doc >= P.ndocs) return v;
	const u64 t0 = P.docTermOffsets[ doc], t1 = P.docTermOffsets[ (u64)doc+1];
	if (!(t0 <= t1 && t1 <= P.nterms && term < t1 - t0)) return v;
	const u32 first = P.terms[ 6*(t0 + term) + 4];
	const u64 r0 = P.docOffsets[ doc], r1 = P.docOffsets[ (u64)doc+1];
	if (!(r0 <= r1 && r1 <= P.nresults && first < r1 - r0)) return v;
	v = valueOf( P, r0 + first);
	if (!v.ok) { v.p = 0; v.len = 0; }
	return v;
}

// ---- the comparator: (key, entry) a lies before (key, entry) b.  Total whatever the arrays hold: the key, then -- for two valid
// entries -- the bytes and the length, then the index.
__device__ __forceinline__ bool entryBefore( const DictOrderParams& P, u64 ka, u32 ia, u64 kb, u32 ib)
{
	if (ka != kb) return ka < kb;
	if (ia == ib) return false;
	if (ia < P.ndict && ib < P.ndict)
	{
		const TermValue a = storedValue( P, ia), b = storedValue( P, ib);
		const u32 n = a.len < b.len ? a.len : b.len;
		const u32 same = commonBytes( a.p, b.p, n);
		if (same < n) return a.p[ same] < b.p[ same];
		if (a.len != b.len) return a.len < b.len;
	}
	return ia < ib;
}

// ---- keys: the sort entry of every dictionary entry, and where its value lies
__device__ void writeKeys( const DictOrderParams& P)
{
	const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= P.ndict) return;
	const u32 handle = P.dictRecords[ 8*e];
	const TermValue v = valueOfEntry( P, (u32)e);
	u32 head = 0;
	for (u32 i=0; i<4 && i<v.len; ++i) head |= (u32)v.p[ i] << (24 - 8*i);
	P.keys[ 0][ e] = ((u64)handle << 32) | head;
	P.index[ 0][ e] = (u32)e;
	P.valueAt[ e] = (u64)(size_t)v.p;
	P.valueLen[ e] = v.len;
}

// ---- tiles: every tile of buffer 0 sorted in place
__device__ void sortTiles( const DictOrderParams& P)
{
	__shared__ u64 K[ DICTORDER_TILE];
	__shared__ u32 I[ DICTORDER_TILE];
	__shared__ u32 sTile;
	for (;;)
	{
		__syncthreads();			// (the tile before is written out, sTile is read)
		if (threadIdx.x == 0) sTile = atomicAdd( P.cursor, 1u);
		__syncthreads();
		const u32 tile = sTile;
		if (tile >= P.tiles) break;
		const u64 base = (u64)tile * DICTORDER_TILE;
		const u32 count = (u32)(P.ndict - base < DICTORDER_TILE ? P.ndict - base : DICTORDER_TILE);
		u32 width = 64;				// the network: the next power of two of the entries, at most the tile
		while (width < count) width <<= 1;
		for (u32 i=threadIdx.x; i<width; i+=TILE_THREADS)
		{
			const bool real = i < count;
			K[ i] = real ? P.keys[ 0][ base + i] : PAD_KEY;
			I[ i] = real ? P.index[ 0][ base + i] : NONE;
		}
		__syncthreads();
		for (u32 k=2; k<=width; k<<=1)
		{
			for (u32 j=k>>1; j; j>>=1)
			{
				for (u32 p=threadIdx.x; p<width/2; p+=TILE_THREADS)
				{
					const u32 lo = ((p & ~(j - 1)) << 1) | (p & (j - 1)), hi = lo + j;
					const u64 ka = K[ lo], kb = K[ hi];
					const u32 ia = I[ lo], ib = I[ hi];
					const bool ascending = (lo & k) == 0;
					// ascending: the upper entry before the lower one is out of order; descending: the other way round
					if (entryBefore( P, ascending ? kb : ka, ascending ? ib : ia, ascending ? ka : kb, ascending ? ia : ib))
					{
						K[ lo] = kb; I[ lo] = ib; K[ hi] = ka; I[ hi] = ia;
					}
				}
				__syncthreads();
			}
		}
		// (a padding entry follows every real one: the first `count` slots are the tile)
		for (u32 i=threadIdx.x; i<count; i+=TILE_THREADS)
		{
			P.keys[ 0][ base + i] = K[ i];
			P.index[ 0][ base + i] = I[ i];
		}
	}
}

// ---- one merge level: runs of `width` entries of buffer `from` merged in pairs into the other buffer
__device__ void mergeRuns( const DictOrderParams& P, u32 from, u64 width)
{
	const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= P.ndict) return;
	const u64* keys = P.keys[ from];
	const u32* index = P.index[ from];
	const u64 n = P.ndict;
	const u64 base = p & ~(2*width - 1);		// (the width is a power of two)
	const u64 mid = base + width < n ? base + width : n, end = base + 2*width < n ? base + 2*width : n;
	const bool left = p < mid;
	const u64 key = keys[ p];
	const u32 idx = index[ p];
	// the entries of the partner run that lie before this one: all before `lo`, none from `hi` on
	u64 lo = left ? mid : base, hi = left ? end : mid;
	const u64 first = lo;
	while (lo < hi)
	{
		const u64 at = lo + (hi - lo)/2;
		if (entryBefore( P, keys[ at], index[ at], key, idx)) lo = at + 1; else hi = at;
	}
	const u64 to = base + (p - (left ? base : mid)) + (lo - first);
	if (to < n)					// (inside [base, end) for any total order; compared all the same)
	{
		P.keys[ from ^ 1][ to] = key;
		P.index[ from ^ 1][ to] = idx;
	}
}

// ---- place: the order, its inverse and the shared prefixes
__device__ void placeOrder( const DictOrderParams& P)
{
	const u64* keys = P.keys[ P.levels & 1];
	const u32* index = P.index[ P.levels & 1];
	const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;	// (whole waves get here: the lane below is asked for its entry)
	const bool active = k < P.ndict;
	u32 e = NONE, handle = 0;
	if (active) { e = index[ k]; handle = (u32)(keys[ k] >> 32); }
	u32 before = (u32)__shfl_up( (int)e, 1), handleBefore = (u32)__shfl_up( (int)handle, 1);
	if (LANE == 0 && active && k) { before = index[ k-1]; handleBefore = (u32)(keys[ k-1] >> 32); }
	if (!active) return;
	u32 prefix = NONE;
	if (e < P.ndict)
	{
		prefix = 0;
		if (k && before < P.ndict && handleBefore == handle)
		{
			const TermValue a = storedValue( P, before), b = storedValue( P, e);
			prefix = commonBytes( a.p, b.p, a.len < b.len ? a.len : b.len);
		}
		P.rank[ e] = (u32)k;
	}
	P.order[ k] = e < P.ndict ? e : NONE;
	P.prefixBytes[ k] = prefix;
}

// ---- offsets: where the entries of every handle start
__device__ void scanHandles( const DictOrderParams& P)
{
	const u64 total = scanDocumentCounts<u64, 1>( P.handleBound,
		[&]( u64 h) { return DocCounts<1>{{ P.handleTerms[ h]}}; },
		[&]( u64 h, const DocCounts<1>&, const DocSums<1>& at) { P.handleOffsets[ h] = at.v[ 0]; }).v[ 0];
	if (threadIdx.x == 0) { P.handleOffsets[ P.handleBound] = total; *P.total = P.ndict; }
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l2_dictorder_keys_kernel( DictOrderParams P) { writeKeys( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_dictorder_tiles_kernel( DictOrderParams P) { sortTiles( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_dictorder_merge_kernel( DictOrderParams P, uint32_t from, uint64_t width) { mergeRuns( P, from, width); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_dictorder_place_kernel( DictOrderParams P) { placeOrder( P); }
extern "C" __global__ __launch_bounds__(1024) void spa_l2_dictorder_offsets_kernel( DictOrderParams P) { scanHandles( P); }

namespace spa {

hipError_t launchL2DictOrder( const DictOrderParams& P, unsigned numCUs, hipStream_t stream)
{
	hipError_t e;
	hipLaunchKernelGGL( spa_l2_dictorder_offsets_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess || !P.ndict) return e;
	const dim3 perEntry( (unsigned)(((u64)P.ndict + 255u) / 256u));
	hipLaunchKernelGGL( spa_l2_dictorder_keys_kernel, perEntry, dim3( 256), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (P.ndict > 1)
	{
		// six workgroups of a tile's LDS share a CU
		const unsigned slots = numCUs * 6u;
		hipLaunchKernelGGL( spa_l2_dictorder_tiles_kernel, dim3( P.tiles < slots ? P.tiles : slots), dim3( TILE_THREADS), 0, stream, P);
		if ((e = hipGetLastError()) != hipSuccess) return e;
		u64 width = DICTORDER_TILE;
		for (u32 level=0; level<P.levels; ++level, width<<=1)
		{
			hipLaunchKernelGGL( spa_l2_dictorder_merge_kernel, perEntry, dim3( 256), 0, stream, P, level & 1u, width);
			if ((e = hipGetLastError()) != hipSuccess) return e;
		}
	}
	hipLaunchKernelGGL( spa_l2_dictorder_place_kernel, perEntry, dim3( 256), 0, stream, P);
	return hipGetLastError();
}

}
