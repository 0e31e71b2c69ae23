// Stitching passes of a segmented lexer batch (l1_stitch.h): count, offsets, place.
#include <hip/hip_runtime.h>
#include "doc_passes.h"
#include "l1_stitch.h"

using namespace spa;

namespace {

enum {STITCH_ERR_RANGE=5, STITCH_ERR_OUTPUT=9};		// SP_DOC_ERR_RANGE, SP_DOC_ERR_OUTPUT (include/strus_pattern_amd.h)

// what of the lexer batch's output lies inside its buffer
__device__ __forceinline__ u64 deviceLexems( const StitchParams& P)
{
	const u64 counted = uni64( *P.lexemCounter);
	return counted < P.lexemCapacity ? counted : P.lexemCapacity;
}

// ---- pass A: a wave per document, its segments in rounds of 64, a lane per segment.  The destination offset of a segment
// is the exclusive prefix sum of the lexem counts, its ordpos base the exclusive prefix sum of the ordpos of the last
// lexem of every segment before it (an empty segment adds nothing): both carried from round to round in 64 bits.
__device__ void countDocuments( const StitchParams& P)
{
	const u64 dev = deviceLexems( P);
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor);
		if (doc >= P.ndocs) break;
		const u64 s0 = uni64( P.docSegOffsets[ doc]), s1 = uni64( P.docSegOffsets[ (u64)doc+1]);
		u32 status = 0;
		u64 total = 0, base = 0;
		bool wide = false;
		if (s0 > s1 || s1 > P.nseg) status = STITCH_ERR_RANGE;
		else for (u64 r=s0; r<s1; r+=64)
		{
			const u64 seg = r + LANE;
			const bool active = seg < s1;
			const int st = active ? P.segStatus[ seg] : 0;
			const u64 failed = __ballot( st != 0);
			if (failed)
			{
				// the first failing segment gives the document its status; its (first, count) is never read
				status = uni( (u32)__shfl( st, __ffsll( (unsigned long long)failed) - 1));
				break;
			}
			u64 first = 0, count = 0;
			if (active)
			{
				first = P.segRange[ 2*seg]; count = P.segRange[ 2*seg+1];
				if (count > dev || first > dev - count) count = 0;	// (what sp_lexer_ctx_batch_fetch_docs returns for such a range)
			}
			if (__ballot( count > MAX32)) wide = true;
			const u32 cnt = (u32)count;
			const u32 last = count ? P.lexems[ 4*(first + count - 1) + 1] : 0u;
			const u64 ci = waveScanAdd64( cnt), oi = waveScanAdd64( last);
			if (active)
			{
				P.segWork[ 2*seg] = (u32)(total + ci - cnt);
				P.segWork[ 2*seg+1] = (u32)(base + oi - last);
			}
			total += waveLane64( ci, 63); base += waveLane64( oi, 63);
		}
		if (!status && (wide || total > MAX32 || base > MAX32)) status = STITCH_ERR_RANGE;
		if (LANE == 0) { P.docCount[ doc] = status ? 0u : (u32)total; P.docStatus[ doc] = (int32_t)status; }
	}
}

// ---- pass B: the offsets of the documents' lexems (doc_passes.h), with the capacity rule applied where they are stored.
// The sum of the counts cannot exceed the lexem capacity when the segment ranges of the documents are disjoint (an
// ascending docSegOffsets); with ranges that share segments it can, and the documents that end beyond the capacity --
// from the first such on, all that have lexems -- fail with STITCH_ERR_OUTPUT and are empty, at the end of what fits.
__device__ void scanDocuments( const StitchParams& P)
{
	__shared__ unsigned long long sFit;
	__shared__ u32 sFailed, sOver;
	const u64 NOWHERE = ~0ull;
	if (threadIdx.x == 0) { sFit = 0; sFailed = 0; sOver = 0; }
	__syncthreads();
	u64 fit = 0;
	u32 failed = 0;
	bool over = false;
	scanDocumentCounts<u64, 1>( P.ndocs,
		[&]( u64 d) { return DocCounts<1>{{ P.docCount[ d]}}; },
		[&]( u64 d, const DocCounts<1>& count, const DocSums<1>& offset) {
			const u32 k = count.v[ 0];
			const u64 at = offset.v[ 0];
			int32_t st = P.docStatus[ d];
			if (at + k <= P.lexemCapacity)
			{
				P.docOffsets[ d] = at;
				if (at + k > fit) fit = at + k;
			}
			else
			{
				P.docOffsets[ d] = NOWHERE; over = true;
				if (k) { st = STITCH_ERR_OUTPUT; P.docStatus[ d] = st; P.docCount[ d] = 0; }
			}
			if (st != 0) ++failed;
		});
	atomicMax( &sFit, (unsigned long long)fit);
	atomicAdd( &sFailed, failed);
	if (over) sOver = 1;
	__syncthreads();
	const u64 end = sFit;
	if (sOver) for (u64 d=threadIdx.x; d<P.ndocs; d+=1024)		// (every thread meets the documents it wrote above)
	{
		if (P.docOffsets[ d] == NOWHERE) P.docOffsets[ d] = end;
	}
	if (threadIdx.x == 0) { P.docOffsets[ P.ndocs] = end; P.totals[ 0] = end; P.totals[ 1] = sFailed; }
}

// ---- pass C: a wave per document, a lane per stitched lexem j = 0, 1, .. of the document: its segment is the last one
// whose destination offset is <= j (the empty segments in front of it share that offset), found by bisection from the
// segment of the lane's lexem before.  Whatever the work array holds, no index leaves the document's range in the
// stitched buffers or the part of the lexer's buffer that the batch wrote.
__device__ void placeDocuments( const StitchParams& P)
{
	const u64 dev = deviceLexems( P);
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor + 1);
		if (doc >= P.ndocs) break;
		const u64 at = uni64( P.docOffsets[ doc]);
		const u64 n = uni64( P.docOffsets[ (u64)doc+1]) - at;
		const u64 s0 = uni64( P.docSegOffsets[ doc]), s1 = uni64( P.docSegOffsets[ (u64)doc+1]);
		if (n == 0 || n > MAX32 || at > P.lexemCapacity || n > P.lexemCapacity - at) continue;
		if (s0 >= s1 || s1 > P.nseg) continue;
		u64 seg = s0;
		for (u64 j=LANE; j<n; j+=64)
		{
			u64 hi = s1;
			while (hi - seg > 1)
			{
				const u64 mid = (seg + hi) >> 1;
				if (P.segWork[ 2*mid] <= j) seg = mid; else hi = mid;
			}
			const uint2 w = ((const uint2*)P.segWork)[ seg];
			const u64 off = j - w.x;
			const u64 first = P.segRange[ 2*seg], count = P.segRange[ 2*seg+1];
			if (w.x > j || off >= count || count > dev || first > dev - count) continue;
			u32x4 v = *(const u32x4*)(P.lexems + 4*(first + off));
			v.y += w.y;
			*(u32x4*)(P.outLexems + 4*(at + j)) = v;
			P.outOrigseg[ at + j] = (u32)(seg - s0);
		}
	}
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l1_stitch_count_kernel( StitchParams P) { countDocuments( P); }
extern "C" __global__ __launch_bounds__(1024) void spa_l1_stitch_offsets_kernel( StitchParams P) { scanDocuments( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l1_stitch_place_kernel( StitchParams P) { placeDocuments( P); }

namespace spa {
hipError_t launchL1Stitch( const StitchParams& P, unsigned numCUs, hipStream_t stream, hipEvent_t* ev)
{
	const dim3 perDocument( wavePerDocumentBlocks( P.ndocs, numCUs));
	hipError_t e;
	if (ev && (e = hipEventRecord( ev[ 0], stream)) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l1_stitch_count_kernel, perDocument, dim3( 256), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l1_stitch_offsets_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l1_stitch_place_kernel, perDocument, dim3( 256), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (ev && (e = hipEventRecord( ev[ 1], stream)) != hipSuccess) return e;
	return hipSuccess;
}
}
