// Posting-block passes of a finished device batch (l2_postingblocks.h): lists, sizes, prefix, blocks, offsets, emit.
#include <hip/hip_runtime.h>
#include "doc_passes.h"
#include "l2_span.h"
#include "l2_postingblocks.h"
#include "posting_block_code.h"

using namespace spa;

namespace {

const u32 ROW = 32;		// bytes of a lane's row in LDS: POSTING_BLOCK_OCCURRENCE_MAX and two to spare

__device__ __forceinline__ u64 least( u64 a, u64 b) { return a < b ? a : b; }

// inclusive prefix sum of 64 values in 64 bits
__device__ __forceinline__ u64 waveScanBytes( u64 v) { return waveScanAdd64( (u32)v) + ((u64)waveScanAdd( (u32)(v >> 32)) << 32); }
// the value of another lane, which differs between lanes
__device__ __forceinline__ u64 laneValue64( u64 v, u32 lane)
{
	return ((u64)(u32)__shfl( (int)(u32)(v >> 32), (int)lane) << 32) | (u32)__shfl( (int)(u32)v, (int)lane);
}

// ---- lists: where the postings of every sorted position start in output order
__device__ void scanLists( const PostingBlocksParams& P)
{
	const u64 N = P.nterms;
	const DocSums<1> sum = scanDocumentCounts<u64, 1>( P.ndict,
		[&]( u64 k) {
			const u32 e = P.order[ k];
			u64 a = 0, b = 0;
			if (e < P.ndict) { a = least( P.entryOffsets[ e], N); b = least( P.entryOffsets[ (u64)e+1], N); }
			return DocCounts<1>{{ b > a ? (u32)(b - a) : 0u}};
		},
		[&]( u64 k, const DocCounts<1>&, const DocSums<1>& at) { P.listOffsets[ k] = at.v[ 0]; });
	if (threadIdx.x == 0) P.listOffsets[ P.ndict] = sum.v[ 0];
}

// ---- sorted posting s: the one reading of the sizing and the emitting pass
struct SortedPosting
{
	PostingBlockHeader h;
	u64 k;			// its sorted position
	u64 listFirst;		// the first sorted posting of its list, cut to N
	u64 listEnd;		// ... and the one behind its last
	u64 occ0;		// its first occurrence
	u32 nocc;		// its occurrences; 0 for a posting that is none
	bool firstOfList;
};

__device__ __forceinline__ SortedPosting readPosting( const PostingBlocksParams& P, u64 s)
{
	const u64 N = P.nterms;
	SortedPosting q;
	q.h.ddelta = q.h.count = q.h.npos = 0;
	q.k = 0; q.listFirst = q.listEnd = 0; q.occ0 = 0; q.nocc = 0; q.firstOfList = false;
	if (s >= N || !P.ndict) return q;
	// the last k with listOffsets[k] <= s (listOffsets[0] is 0): a list without postings is skipped
	u32 lo = 0, hi = P.ndict;
	while (hi - lo > 1)
	{
		const u32 mid = lo + ((hi - lo) >> 1);
		if (P.listOffsets[ mid] <= s) lo = mid; else hi = mid;
	}
	const u64 a = P.listOffsets[ lo];
	q.k = lo; q.listFirst = least( a, N); q.listEnd = least( P.listOffsets[ (u64)lo+1], N);
	const u32 e = P.order[ lo];
	if (e >= P.ndict || a > s) return q;
	const u64 eo = P.entryOffsets[ e];
	if (eo >= N || s - a >= N - eo) return q;
	const u64 p = eo + (s - a);
	const uint4 posting = ld4( P.postings + 4*p);		// doc, term, count, first_ordpos
	if (posting.x >= P.ndocs) return q;
	q.firstOfList = s == a;
	const u32 docBefore = q.firstOfList ? 0u : P.postings[ 4*(p-1)];	// (p-1 >= eo)
	const u64 o1 = least( P.postingOffsets[ p+1], P.nocc), o0 = least( P.postingOffsets[ p], o1);
	q.occ0 = o0; q.nocc = (u32)least( o1 - o0, MAX32);
	q.h = postingBlockHeader( q.firstOfList, posting.x, docBefore, posting.z, P.postingPositions[ p]);
	return q;
}

// ---- The concatenated occurrences of the 64 postings of a wave in trips of 64, a lane an occurrence.  occPrefix (65) and occAt
// (64) are this wave's LDS.  perTrip( active, owner, firstOfPosting, ordpos, ordposBefore) runs with all lanes: `owner` is the
// lane whose posting the occurrence belongs to.  What the caller wrote to LDS before the call is visible inside perTrip.
template <class FN>
__device__ __forceinline__ void walkOccurrences( const PostingBlocksParams& P, const SortedPosting& q, u64* occPrefix, u64* occAt, FN perTrip)
{
	const u64 incl = waveScanAdd64( q.nocc);
	occPrefix[ LANE] = incl - q.nocc;
	if (LANE == 63) occPrefix[ 64] = incl;
	occAt[ LANE] = q.occ0;
	waveLdsSync();
	const u64 total = waveLane64( incl, 63);
	for (u64 c0=0; c0<total; c0+=64)
	{
		const u64 c = c0 + LANE;
		const bool active = c < total;
		u32 owner = 0, ordpos = 0;
		u64 i = 0;
		if (active)
		{
			// the last lane whose occurrences start at or before c: a posting without occurrences is skipped
			for (u32 step=32; step; step>>=1) if (occPrefix[ owner+step] <= c) owner += step;
			i = c - occPrefix[ owner];
			ordpos = P.occurrences[ 2*(occAt[ owner] + i)];		// (occAt + i lies below the posting's end, which is at most nocc)
		}
		// the position before it in its posting: that of the lane below, at the edge of a trip a load
		u32 before = (u32)__shfl_up( (int)ordpos, 1);
		if (LANE == 0 && active && i) before = P.occurrences[ 2*(occAt[ owner] + i - 1)];
		perTrip( active, owner, i == 0, ordpos, before);
	}
}

// ---- sizes: the bytes of every sorted posting, the number of position varints
__device__ void sizePostings( const PostingBlocksParams& P)
{
	__shared__ u64 sOccPrefix[ 4][ 66];
	__shared__ u64 sOccAt[ 4][ 64];
	__shared__ u64 sBytes[ 4][ 64];
	__shared__ PostingBlockHeader sHeader[ 4][ 64];
	const u32 wave = threadIdx.x >> 6;
	const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	const SortedPosting q = readPosting( P, s);
	sBytes[ wave][ LANE] = 0;
	sHeader[ wave][ LANE] = q.h;
	u32 gaps = 0;
	walkOccurrences( P, q, sOccPrefix[ wave], sOccAt[ wave], [&]( bool active, u32 owner, bool firstOfPosting, u32 ordpos, u32 before) {
		if (!active) return;
		const u32 n = postingOccurrenceBytes( firstOfPosting, sHeader[ wave][ owner], ordpos, before);
		if (n) atomicAdd( (unsigned long long*)&sBytes[ wave][ owner], (unsigned long long)n);		// (a sum)
		gaps += positionGapBytes( firstOfPosting, ordpos, before) ? 1u : 0u;
	});
	waveLdsSync();
	if (s < P.nterms) P.postingBytes[ s] = sBytes[ wave][ LANE];
	const u64 sum = waveLane64( waveScanAdd64( gaps), 63);
	if (LANE == 0 && sum) atomicAdd( (unsigned long long*)(P.totals + 3), (unsigned long long)sum);
}

// ---- prefix: the bytes of the sorted postings before every one, in place
__device__ void scanPostings( const PostingBlocksParams& P)
{
	const DocSums<2> sum = scanDocumentCounts<u64, 2>( P.nterms,
		[&]( u64 s) { const u64 n = P.postingBytes[ s]; return DocCounts<2>{{ (u32)n, (u32)(n >> 32)}}; },
		[&]( u64 s, const DocCounts<2>&, const DocSums<2>& at) { P.postingBytes[ s] = at.v[ 0] + (at.v[ 1] << 32); });
	if (threadIdx.x == 0) P.postingBytes[ P.nterms] = sum.v[ 0] + (sum.v[ 1] << 32);
}

// the bytes of the posting codes of the list [a, b) of sorted postings (a <= b <= N): what its `body` says
__device__ __forceinline__ u64 listBody( const PostingBlocksParams& P, u64 a, u64 b) { return b > a ? P.postingBytes[ b] - P.postingBytes[ a] : 0; }

// ---- blocks: the bytes of every list, where it starts inside its block, the bytes of every block
__device__ void sizeBlocks( const PostingBlocksParams& P)
{
	const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	const bool active = k < P.ndict;
	u64 bytes = 0;
	if (active) bytes = postingListBytes( listBody( P, least( P.listOffsets[ k], P.nterms), least( P.listOffsets[ k+1], P.nterms)));
	const u32 B = P.blockEntries, headLane = LANE & ~(B - 1);
	const u64 incl = waveScanBytes( bytes);
	const u64 beforeBlock = laneValue64( incl - bytes, headLane);
	const u64 j = k >> __builtin_ctz( B);
	if (active && j < P.nblocks)
	{
		P.listStart[ k] = incl - bytes - beforeBlock;
		if ((k & (B - 1)) == B - 1 || k == (u64)P.ndict - 1) P.blockSize[ j] = incl - beforeBlock;
	}
}

// ---- offsets: where every block starts, and the totals
__device__ void scanBlocks( const PostingBlocksParams& P)
{
	const DocSums<2> sum = scanDocumentCounts<u64, 2>( P.nblocks,
		[&]( u64 j) { const u64 n = P.blockSize[ j]; return DocCounts<2>{{ (u32)n, (u32)(n >> 32)}}; },
		[&]( u64 j, const DocCounts<2>&, const DocSums<2>& at) { P.blockOffsets[ j] = at.v[ 0] + (at.v[ 1] << 32); });
	if (threadIdx.x == 0)
	{
		const u64 nbytes = sum.v[ 0] + (sum.v[ 1] << 32);
		P.blockOffsets[ P.nblocks] = nbytes;
		P.totals[ 0] = P.nblocks; P.totals[ 1] = nbytes; P.totals[ 2] = P.blockEntries;
	}
}

// ---- emit: the codes of 64 sorted postings by the whole wave, a trip of 64 occurrences at a time
__device__ void emitPostings( const PostingBlocksParams& P)
{
	__shared__ uint8_t sRow[ 4][ 64][ ROW];
	__shared__ u64 sStart[ 4][ 66];
	__shared__ u64 sOccPrefix[ 4][ 66];
	__shared__ u64 sOccAt[ 4][ 64];
	__shared__ u64 sBody[ 4][ 64];
	__shared__ u64 sBlock0[ 4][ 64];
	__shared__ u64 sBlock1[ 4][ 64];
	__shared__ PostingBlockHeader sHeader[ 4][ 64];
	__shared__ uint8_t sFirstOfList[ 4][ 64];
	const u32 wave = threadIdx.x >> 6;
	const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	const SortedPosting q = readPosting( P, s);
	// the range of the posting's block, cut to the capacity; where the first byte of the posting's first occurrence goes: at the
	// start of the list for its first posting (the occurrence carries `body`), else behind `body` and the postings before
	u64 b0 = 0, b1 = 0, start = 0, body = 0;
	if (q.nocc)
	{
		const u64 j = q.k >> __builtin_ctz( P.blockEntries);
		if (j < P.nblocks) { b0 = P.blockOffsets[ j]; b1 = P.blockOffsets[ j+1]; }
		if (b1 > P.capacity) b1 = P.capacity;
		if (b0 > b1) b0 = b1;
		body = listBody( P, q.listFirst, q.listEnd);
		start = b0 + P.listStart[ q.k] + (P.postingBytes[ s] - P.postingBytes[ q.listFirst]) + (q.firstOfList ? 0u : varintBytes( body));
	}
	const u64 have = __ballot( q.nocc != 0);
	if (!have) return;
	// the output of the wave is one run from the start of its first posting: the codes lie one behind the other across lists and blocks
	u64 cursor = waveLane64( start, __ffsll( (unsigned long long)have) - 1);
	sBody[ wave][ LANE] = body; sBlock0[ wave][ LANE] = b0; sBlock1[ wave][ LANE] = b1;
	sHeader[ wave][ LANE] = q.h; sFirstOfList[ wave][ LANE] = q.firstOfList ? 1 : 0;
	const u64* starts = sStart[ wave];
	walkOccurrences( P, q, sOccPrefix[ wave], sOccAt[ wave], [&]( bool active, u32 owner, bool firstOfPosting, u32 ordpos, u32 before) {
		u32 n = 0;
		if (active)
		{
			n = writePostingOccurrence( sRow[ wave][ LANE], firstOfPosting && sFirstOfList[ wave][ owner], sBody[ wave][ owner], firstOfPosting,
						    sHeader[ wave][ owner], ordpos, before);
		}
		const u32 incl = waveScanAdd( n);
		const u64 at = cursor + (incl - n);
		const u64 g0 = cursor, g1 = cursor + uni( (u32)__shfl( (int)incl, 63));
		// every byte of an occurrence lies inside the range of its block (and that inside the capacity): a trip one of whose
		// occurrences does not -- none of the arrays of this library -- writes nothing
		const bool outside = active && n && (at < sBlock0[ wave][ owner] || at > sBlock1[ wave][ owner] || n > sBlock1[ wave][ owner] - at);
		const bool inside = __ballot( outside) == 0;
		sStart[ wave][ LANE] = at;			// (a lane behind the last occurrence starts at g1 and owns nothing)
		if (LANE == 63) sStart[ wave][ 64] = g1;
		waveLdsSync();
		// a lane per aligned output dword; byte x is byte x - starts[i] of the row of the last lane i with starts[i] <= x
		if (inside) for (u64 d = (g0 >> 2) + LANE; d < ((g1 + 3) >> 2); d += 64)
		{
			const u64 a = d << 2;
			const u32 first = a < g0 ? (u32)(g0 - a) : 0u, last = a + 4 > g1 ? (u32)(g1 - a) : 4u;	// the bytes [first, last) of the dword are the span's
			u64 x = a + first;
			u32 i = 0, v = 0;
			for (u32 step=32; step; step>>=1) if (starts[ i+step] <= x) i += step;
			for (u32 b=first; b<last; ++b, ++x)
			{
				while (i < 63 && starts[ i+1] <= x) ++i;
				v |= (u32)sRow[ wave][ i][ (x - starts[ i]) & (ROW - 1)] << (8*b);
			}
			// (an edge dword is shared with the trip or the wave before or behind: bytes, never a read-modify-write)
			if (first == 0 && last == 4) *(u32*)(P.bytes + a) = v;
			else for (u32 b=first; b<last; ++b) P.bytes[ a + b] = (uint8_t)(v >> (8*b));
		}
		cursor = g1;
		waveLdsSync();					// (the rows and the starts are the next trip's)
	});
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(1024) void spa_l2_postingblocks_lists_kernel( PostingBlocksParams P) { scanLists( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_postingblocks_sizes_kernel( PostingBlocksParams P) { sizePostings( P); }
extern "C" __global__ __launch_bounds__(1024) void spa_l2_postingblocks_prefix_kernel( PostingBlocksParams P) { scanPostings( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_postingblocks_blocks_kernel( PostingBlocksParams P) { sizeBlocks( P); }
extern "C" __global__ __launch_bounds__(1024) void spa_l2_postingblocks_offsets_kernel( PostingBlocksParams P) { scanBlocks( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_postingblocks_emit_kernel( PostingBlocksParams P) { emitPostings( P); }

namespace spa {

hipError_t launchL2PostingBlocksCount( const PostingBlocksParams& P, unsigned, hipStream_t stream)
{
	if (!P.ndict || !P.nterms || P.nterms >= MAX32 || !termBlockEntriesValid( P.blockEntries)) return hipErrorInvalidValue;
	const dim3 perPosting( (unsigned)((P.nterms + 255u) / 256u)), perPosition( (unsigned)(((u64)P.ndict + 255u) / 256u));
	hipError_t e;
	hipLaunchKernelGGL( spa_l2_postingblocks_lists_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l2_postingblocks_sizes_kernel, perPosting, dim3( 256), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l2_postingblocks_prefix_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l2_postingblocks_blocks_kernel, perPosition, dim3( 256), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l2_postingblocks_offsets_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	return hipGetLastError();
}

hipError_t launchL2PostingBlocksPlace( const PostingBlocksParams& P, unsigned, hipStream_t stream)
{
	if (!P.ndict || !P.nterms || !P.capacity) return hipSuccess;
	hipLaunchKernelGGL( spa_l2_postingblocks_emit_kernel, dim3( (unsigned)((P.nterms + 255u) / 256u)), dim3( 256), 0, stream, P);
	return hipGetLastError();
}

}
