// Text passes of a finished device batch (l2_text.h): count, offsets, place, per family of spans.
#include <hip/hip_runtime.h>
#include "l2_span.h"
#include "l2_text.h"

using namespace spa;

namespace {

enum {TEXT_ERR_RANGE=5};		// SP_DOC_ERR_RANGE (include/strus_pattern_amd.h)
enum {TEXT_RESULTS=1, TEXT_ITEMS=2};	// SP_TEXT_RESULTS, SP_TEXT_ITEMS

// ---- pass A: a wave per document, its spans in rounds of 64, a lane per span.  The offset of a span inside its document
// is the exclusive prefix sum of the lengths, carried from round to round in 64 bits.
template <int STRIDE>
__device__ void countSpans( const TextParams& P, const TextFamily& F)
{
	for (;;)
	{
		const u32 doc = nextDocument( F.cursor);
		if (doc >= P.ndocs) break;
		const u64 r0 = uni64( F.docOffsets[ doc]), r1 = uni64( F.docOffsets[ (u64)doc+1]);
		u64 total = 0;
		bool failed = false;
		if (r0 < r1 && r1 <= F.nrecords)
		{
			u64 d0, d1;
			docSegments( P, doc, d0, d1);
			for (u64 r=r0; r<r1; r+=64)
			{
				const u64 i = r + LANE;
				const bool active = i < r1;
				u64 begin = 0, length = 0;
				bool ok = true;
				if (active) ok = spanRange( P, d0, d1, F.records + STRIDE*i, begin, length) && length <= MAX32;
				if (__ballot( !ok)) { failed = true; break; }
				const u32 len = (u32)length;
				const u64 ci = waveScanAdd64( len);
				if (active) F.spanWork[ i] = (u32)(total + ci - len);
				total += waveLane64( ci, 63);
				if (total > MAX32) { failed = true; break; }
			}
		}
		if (LANE == 0)
		{
			F.docBytes[ doc] = failed ? 0 : total;
			if (failed) P.docStatus[ doc] = TEXT_ERR_RANGE;
		}
	}
}

// ---- pass B: the offsets of the documents' bytes (doc_passes.h).  A document that failed, in this family or the other, counts 0.
__device__ void scanDocuments( const TextParams& P, const TextFamily& F)
{
	const u64 total = scanDocumentCounts<u64, 1>( P.ndocs,
		[&]( u64 d) {
			const u64 b = P.docStatus[ d] == 0 ? F.docBytes[ d] : 0;
			return DocCounts<1>{{ b <= MAX32 ? (u32)b : 0u}};
		},
		[&]( u64 d, const DocCounts<1>&, const DocSums<1>& at) { F.docTextOffsets[ d] = at.v[ 0]; }).v[ 0];
	if (threadIdx.x == 0) { F.docTextOffsets[ P.ndocs] = total; F.spanOffsets[ F.nrecords] = total; *F.total = total; }
}

// ---- pass C
// Copies the bytes [lo, hi) of the document's block (which starts at byte `at` of the output) with the whole wave: a
// lane per aligned output dword.  SEARCH: the byte at offset x of the block is byte x - sOff[i] of the span i, the last
// of the round with sOff[i] <= x, whose text starts at sSrc[i] (sOff[0] <= lo); else all bytes are of the one span at
// offset `off` whose text starts at `src`.  The caller has made sure that at + hi lies inside the output.
template <bool SEARCH>
__device__ __forceinline__ void copyRange( const TextParams& P, const TextFamily& F, u64 at, u32 lo, u32 hi, const u32* sOff, const u64* sSrc, u32 off, u64 src)
{
	if (lo >= hi) return;
	const u64 g0 = at + lo, g1 = at + hi;
	for (u64 q = (g0 >> 2) + LANE; q < ((g1 + 3) >> 2); q += 64)
	{
		const u64 p = q << 2;
		const u32 first = p < g0 ? (u32)(g0 - p) : 0u, last = p + 4 > g1 ? (u32)(g1 - p) : 4u;	// the bytes [first, last) of the dword are the range's
		u32 x = (u32)(p + first - at);
		u32 i = 0;
		if (SEARCH)
		{
			for (u32 step=32; step; step>>=1) if (sOff[ i+step] <= x) i += step;
			off = sOff[ i]; src = sSrc[ i];
		}
		const bool whole = first == 0 && last == 4;
		bool oneSpan = whole;
		if (SEARCH && whole) oneSpan = (u64)sOff[ i+1] >= (u64)x + 4;
		u32 v = 0;
		if (oneSpan)
		{
			// the dword lies inside one span
			const u64 s = src + (u32)(x - off);
			if (s + 4 <= P.nbytes) v = *(const u32b*)(P.text + s);
			else for (u32 b=0; b<4; ++b) v |= textByte( P, s + b) << (8*b);
		}
		else for (u32 b=first; b<last; ++b, ++x)
		{
			if (SEARCH)
			{
				while (i < 63 && sOff[ i+1] <= x) ++i;
				off = sOff[ i]; src = sSrc[ i];
			}
			v |= textByte( P, src + (u32)(x - off)) << (8*b);
		}
		if (whole) *(u32*)(F.outText + p) = v;
		else for (u32 b=first; b<last; ++b) F.outText[ p + b] = (uint8_t)(v >> (8*b));
	}
}

// A wave per document: the offsets of its spans, and its bytes round by round.  Whatever the work array and the records
// hold, every byte written lies inside the document's block [docTextOffsets[d], docTextOffsets[d+1]) and that inside
// the output, and every byte read inside the text.
template <int STRIDE>
__device__ void placeSpans( const TextParams& P, const TextFamily& F, u32* sOff, u64* sSrc)
{
	for (;;)
	{
		const u32 doc = nextDocument( F.cursor + 1);
		if (doc >= P.ndocs) break;
		const u64 r0 = uni64( F.docOffsets[ doc]), r1 = uni64( F.docOffsets[ (u64)doc+1]);
		if (r0 >= r1 || r1 > F.nrecords) continue;
		const u64 at = uni64( F.docTextOffsets[ doc]), end = uni64( F.docTextOffsets[ (u64)doc+1]);
		const bool failed = uni( (u32)P.docStatus[ doc]) != 0;
		if (failed || end < at || end > F.outCapacity || end - at > MAX32)
		{
			// "fails and is empty": all spans on the document's offset
			for (u64 i=r0+LANE; i<r1; i+=64) F.spanOffsets[ i] = at;
			continue;
		}
		const u32 n = (u32)(end - at);
		u64 d0, d1;
		docSegments( P, doc, d0, d1);
		for (u64 r=r0; r<r1; r+=64)
		{
			const u64 i = r + LANE;
			const bool active = i < r1;
			u64 begin = 0, length = 0;
			u32 w = 0;
			if (active)
			{
				w = F.spanWork[ i];
				if (!spanRange( P, d0, d1, F.records + STRIDE*i, begin, length)) length = 0;
				if (w > n) w = n;
				if (length > n - w) length = n - w;
				F.spanOffsets[ i] = at + w;
			}
			const u32 len = (u32)length;
			// the round's range of the block: from the first span to the end of the last
			const u32 lo = uni( (u32)__shfl( (int)w, 0));
			const u32 hi = uni( (u32)__shfl( (int)waveScanMax( active ? w + len : 0u), 63));
			if (!active) w = hi;
			if (lo >= hi) continue;
			sOff[ LANE] = w; sSrc[ LANE] = begin;
			if (LANE == 63) sOff[ 64] = hi;
			waveLdsSync();
			// long spans by the whole wave on their own, what lies between them through the search
			u64 longSpans = __ballot( active && len >= (u32)TEXT_LONG_SPAN);
			u32 cur = lo;
			while (longSpans)
			{
				const int j = __ffsll( (unsigned long long)longSpans) - 1;
				longSpans &= longSpans - 1;
				const u32 oj = uni( (u32)__shfl( (int)w, j)), lj = uni( (u32)__shfl( (int)len, j));
				const u64 sj = waveLane64( begin, j);
				copyRange<true>( P, F, at, cur, oj, sOff, sSrc, 0, 0);
				copyRange<false>( P, F, at, oj, oj + lj, sOff, sSrc, oj, sj);
				if (oj + lj > cur) cur = oj + lj;
			}
			copyRange<true>( P, F, at, cur, hi, sOff, sSrc, 0, 0);
			waveLdsSync();		// (the next round overwrites what this one searched)
		}
	}
}

template <int STRIDE>
__device__ __forceinline__ void placeFamily( const TextParams& P, const TextFamily& F)
{
	__shared__ u32 sOff[ 4][ 66];
	__shared__ u64 sSrc[ 4][ 64];
	const u32 wave = threadIdx.x >> 6;
	placeSpans<STRIDE>( P, F, sOff[ wave], sSrc[ wave]);
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l2_text_count_results_kernel( TextParams P) { countSpans<9>( P, P.family[ 0]); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_text_count_items_kernel( TextParams P) { countSpans<7>( P, P.family[ 1]); }
extern "C" __global__ __launch_bounds__(1024) void spa_l2_text_offsets_kernel( TextParams P, u32 family) { scanDocuments( P, P.family[ family]); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_text_place_results_kernel( TextParams P) { placeFamily<9>( P, P.family[ 0]); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_text_place_items_kernel( TextParams P) { placeFamily<7>( P, P.family[ 1]); }

namespace spa {

hipError_t launchL2TextCount( const TextParams& P, unsigned numCUs, hipStream_t stream)
{
	const dim3 grid( wavePerDocumentBlocks( P.ndocs, numCUs));
	hipError_t e;
	if (P.families & TEXT_RESULTS)
	{
		hipLaunchKernelGGL( spa_l2_text_count_results_kernel, grid, dim3( 256), 0, stream, P);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	if (P.families & TEXT_ITEMS)
	{
		hipLaunchKernelGGL( spa_l2_text_count_items_kernel, grid, dim3( 256), 0, stream, P);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	for (uint32_t f=0; f<2; ++f) if (P.families & (1u << f))
	{
		hipLaunchKernelGGL( spa_l2_text_offsets_kernel, dim3( 1), dim3( 1024), 0, stream, P, f);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	return hipSuccess;
}

hipError_t launchL2TextPlace( const TextParams& P, unsigned numCUs, hipStream_t stream)
{
	const dim3 grid( wavePerDocumentBlocks( P.ndocs, numCUs));
	hipError_t e;
	if (P.families & TEXT_RESULTS)
	{
		hipLaunchKernelGGL( spa_l2_text_place_results_kernel, grid, dim3( 256), 0, stream, P);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	if (P.families & TEXT_ITEMS)
	{
		hipLaunchKernelGGL( spa_l2_text_place_items_kernel, grid, dim3( 256), 0, stream, P);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	return hipSuccess;
}

}
