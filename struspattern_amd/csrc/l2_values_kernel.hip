// Value passes of a finished device batch (l2_values.h): count, offsets, place, per family of records.
#include <hip/hip_runtime.h>
#include "l2_span.h"
#include "l2_values.h"
#include "value_walk.h"

using namespace spa;

namespace {

enum {VALUE_ERR_RANGE=5};		// SP_DOC_ERR_RANGE (include/strus_pattern_amd.h)
enum {VALUE_RESULTS=1, VALUE_ITEMS=2};	// SP_VALUE_RESULTS, SP_VALUE_ITEMS
const u64 PIECE_TEXT = 1ull << 63;	// in the source word of a piece in LDS: bytes of the text, not of the pool

// the walk's stack of one lane: word k of level l of all 64 lanes side by side (no bank conflicts)
struct LaneStack
{
	u32* base;
	__device__ __forceinline__ u32& word( u32 level, u32 k) { return base[ (level*VALUE_FRAME_WORDS + k)*64 + LANE]; }
};

// the items of one document [first, first + count) in a document of the segments [d0, d1), indices relative to `first`;
// the walk forms only indices inside the lists it was started on, which valueOf has checked against the document
struct DocItems
{
	const ValuesParams& P; u64 first, d0, d1;
	__device__ __forceinline__ u32 variable( u32 i) const { return P.items[ 7*(first + i)]; }
	__device__ __forceinline__ void format( u32 i, u32& fmt, u32& nsub) const { fmt = P.itemFormat[ 2*(first + i)]; nsub = P.itemFormat[ 2*(first + i) + 1]; }
	__device__ __forceinline__ bool span( u32 i, u64& begin, u64& length) const { return spanRange( P, d0, d1, P.items + 7*(first + i), begin, length); }
};

// the items of a document: false when its range does not lie inside the finished items or holds 2^32 records or more
__device__ __forceinline__ bool docItemRange( const ValuesParams& P, u32 doc, u64& i0, u64& i1)
{
	i0 = uni64( P.docItemOffsets[ doc]); i1 = uni64( P.docItemOffsets[ (u64)doc+1]);
	return i0 <= i1 && i1 <= P.nitems && i1 - i0 <= MAX32;
}

// Whether record i of the family has a value: its format and its list [b, e), relative to the document's items [i0, i1).
// ok = false: the record makes the document fail.
template <int ITEMS>
__device__ __forceinline__ bool valueOf( const ValuesParams& P, const ValuesFamily& F, u64 i, bool itemsOk, u64 i0, u64 i1, u32& fmt, u32& b, u32& e, bool& ok)
{
	u64 lb, le;
	if (ITEMS) { fmt = F.format[ 2*i]; lb = i + 1; le = lb + F.format[ 2*i + 1]; }
	else { fmt = F.format[ i]; lb = F.records[ 9*i + 7]; le = lb + F.records[ 9*i + 8]; }
	ok = true; b = 0; e = 0;
	if (!fmt) return false;
	ok = itemsOk && fmt <= P.formatCount && lb >= i0 && le <= i1;
	if (ok) { b = (u32)(lb - i0); e = (u32)(le - i0); }
	return ok;
}

// ---- pass A: a wave per document, its records in rounds of 64, a lane per record.  The offset of a value inside its
// document is the exclusive prefix sum of the lengths, carried from round to round in 64 bits.
template <int ITEMS>
__device__ void countValues( const ValuesParams& P, const ValuesFamily& F, u32* stackBase)
{
	const ValueFormats T = { P.fmtParts, P.parts, P.formatCount };
	LaneStack stack = { stackBase };
	for (;;)
	{
		const u32 doc = nextDocument( F.cursor);
		if (doc >= P.ndocs) break;
		const u64 r0 = uni64( F.docOffsets[ doc]), r1 = uni64( F.docOffsets[ (u64)doc+1]);
		u64 total = 0;
		bool failed = false;
		if (r0 < r1 && r1 <= F.nrecords)
		{
			u64 i0, i1, d0, d1;
			const bool itemsOk = docItemRange( P, doc, i0, i1);
			docSegments( P, doc, d0, d1);
			const DocItems items = { P, i0, d0, d1 };
			for (u64 r=r0; r<r1; r+=64)
			{
				const u64 i = r + LANE;
				const bool active = i < r1;
				u64 length = 0;
				bool ok = true;
				u32 fmt, b, e;
				if (active && valueOf<ITEMS>( P, F, i, itemsOk, i0, i1, fmt, b, e, ok))
				{
					ValueWalk<LaneStack, DocItems> walk( T, stack, items);
					walk.start( fmt, b, e);
					ValuePiece p;
					while (length <= MAX32 && walk.next( p)) length += p.len;
					ok = !walk.failed && length <= MAX32;
				}
				if (__ballot( !ok)) { failed = true; break; }
				const u32 len = (u32)length;
				const u64 ci = waveScanAdd64( len);
				if (active) F.valueWork[ i] = (u32)(total + ci - len);
				total += waveLane64( ci, 63);
				if (total > MAX32) { failed = true; break; }
			}
		}
		if (LANE == 0)
		{
			F.docBytes[ doc] = failed ? 0 : total;
			if (failed) P.docStatus[ doc] = VALUE_ERR_RANGE;
		}
	}
}

// ---- pass B: the offsets of the documents' bytes (doc_passes.h).  A document that failed, in this family or the other, counts 0.
__device__ void scanDocuments( const ValuesParams& P, const ValuesFamily& F)
{
	const u64 total = scanDocumentCounts<u64, 1>( P.ndocs,
		[&]( u64 d) {
			const u64 b = P.docStatus[ d] == 0 ? F.docBytes[ d] : 0;
			return DocCounts<1>{{ b <= MAX32 ? (u32)b : 0u}};
		},
		[&]( u64 d, const DocCounts<1>&, const DocSums<1>& at) { F.docValueOffsets[ d] = at.v[ 0]; }).v[ 0];
	if (threadIdx.x == 0) { F.docValueOffsets[ P.ndocs] = total; F.valueOffsets[ F.nrecords] = total; *F.total = total; }
}

// ---- pass C: a wave per document: the offsets of its values, and its bytes step by step.  Whatever the work array and the
// records hold, every byte written lies inside the document's block [docValueOffsets[d], docValueOffsets[d+1]) and that
// inside the output, and every byte read inside the text or the pool.
template <int ITEMS>
__device__ void placeValues( const ValuesParams& P, const ValuesFamily& F, u32* stackBase, u64* sOff, u64* sSrc, u32* sDst)
{
	const ValueFormats T = { P.fmtParts, P.parts, P.formatCount };
	LaneStack stack = { stackBase };
	for (;;)
	{
		const u32 doc = nextDocument( F.cursor + 1);
		if (doc >= P.ndocs) break;
		const u64 r0 = uni64( F.docOffsets[ doc]), r1 = uni64( F.docOffsets[ (u64)doc+1]);
		if (r0 >= r1 || r1 > F.nrecords) continue;
		const u64 at = uni64( F.docValueOffsets[ doc]), end = uni64( F.docValueOffsets[ (u64)doc+1]);
		const bool failed = uni( (u32)P.docStatus[ doc]) != 0;
		if (failed || end < at || end > F.outCapacity || end - at > MAX32)
		{
			// "fails and is empty": all values on the document's offset
			for (u64 i=r0+LANE; i<r1; i+=64) F.valueOffsets[ i] = at;
			continue;
		}
		const u32 n = (u32)(end - at);
		u64 i0, i1, d0, d1;
		const bool itemsOk = docItemRange( P, doc, i0, i1);
		docSegments( P, doc, d0, d1);
		const DocItems items = { P, i0, d0, d1 };
		for (u64 r=r0; r<r1; r+=64)
		{
			const u64 i = r + LANE;
			ValueWalk<LaneStack, DocItems> walk( T, stack, items);
			bool walking = false;
			u32 pos = 0, room = 0;		// where the lane's next piece goes inside the block, and what is left of the block behind it
			if (i < r1)
			{
				pos = F.valueWork[ i];
				if (pos > n) pos = n;
				room = n - pos;
				F.valueOffsets[ i] = at + pos;
				u32 fmt, b, e;
				bool ok;
				if (valueOf<ITEMS>( P, F, i, itemsOk, i0, i1, fmt, b, e, ok)) { walk.start( fmt, b, e); walking = true; }
			}
			// a step: one piece of every lane that still has one, copied by the whole wave
			for (;;)
			{
				ValuePiece p;
				p.kind = 0; p.src = 0; p.len = 0;
				if (walking) walking = walk.next( p);
				if (!__ballot( walking)) break;
				if (!walking) p.len = 0;
				if (p.len > room) p.len = room;
				room -= p.len;
				const u64 ci = waveScanAdd64( p.len);
				sOff[ LANE] = ci - p.len; sSrc[ LANE] = p.src | (p.kind == VALUE_PIECE_TEXT ? PIECE_TEXT : 0); sDst[ LANE] = pos;
				pos += p.len;
				waveLdsSync();
				const u64 bytes = waveLane64( ci, 63);
				for (u64 t=LANE; t<bytes; t+=64)
				{
					// byte t of the step is byte t - sOff[j] of the piece j, the last with sOff[j] <= t
					u32 j = 0;
					for (u32 step=32; step; step>>=1) if (sOff[ j+step] <= t) j += step;
					const u32 k = (u32)(t - sOff[ j]);
					const u64 src = sSrc[ j];
					u32 v = 0;
					if (src & PIECE_TEXT) v = textByte( P, (src & ~PIECE_TEXT) + k);
					else if (P.poolBytes) { const u64 s = src + k; v = P.pool[ s < P.poolBytes ? s : P.poolBytes - 1]; }
					F.outValues[ at + sDst[ j] + k] = (uint8_t)v;
				}
				waveLdsSync();		// (the next step overwrites what this one searched)
			}
		}
	}
}

__device__ __forceinline__ u32* waveStack()
{
	__shared__ u32 sStack[ 4][ VALUE_MAX_DEPTH*VALUE_FRAME_WORDS*64];
	return sStack[ threadIdx.x >> 6];
}

template <int ITEMS>
__device__ __forceinline__ void placeFamily( const ValuesParams& P, const ValuesFamily& F)
{
	__shared__ u64 sOff[ 4][ 64];
	__shared__ u64 sSrc[ 4][ 64];
	__shared__ u32 sDst[ 4][ 64];
	const u32 wave = threadIdx.x >> 6;
	placeValues<ITEMS>( P, F, waveStack(), sOff[ wave], sSrc[ wave], sDst[ wave]);
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l2_values_count_results_kernel( ValuesParams P) { countValues<0>( P, P.family[ 0], waveStack()); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_values_count_items_kernel( ValuesParams P) { countValues<1>( P, P.family[ 1], waveStack()); }
extern "C" __global__ __launch_bounds__(1024) void spa_l2_values_offsets_kernel( ValuesParams P, u32 family) { scanDocuments( P, P.family[ family]); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_values_place_results_kernel( ValuesParams P) { placeFamily<0>( P, P.family[ 0]); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_values_place_items_kernel( ValuesParams P) { placeFamily<1>( P, P.family[ 1]); }

namespace spa {

hipError_t launchL2ValuesCount( const ValuesParams& P, unsigned numCUs, hipStream_t stream)
{
	const dim3 grid( wavePerDocumentBlocks( P.ndocs, numCUs));
	hipError_t e;
	if (P.families & VALUE_RESULTS)
	{
		hipLaunchKernelGGL( spa_l2_values_count_results_kernel, grid, dim3( 256), 0, stream, P);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	if (P.families & VALUE_ITEMS)
	{
		hipLaunchKernelGGL( spa_l2_values_count_items_kernel, grid, dim3( 256), 0, stream, P);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	for (uint32_t f=0; f<2; ++f) if (P.families & (1u << f))
	{
		hipLaunchKernelGGL( spa_l2_values_offsets_kernel, dim3( 1), dim3( 1024), 0, stream, P, f);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	return hipSuccess;
}

hipError_t launchL2ValuesPlace( const ValuesParams& P, unsigned numCUs, hipStream_t stream)
{
	const dim3 grid( wavePerDocumentBlocks( P.ndocs, numCUs));
	hipError_t e;
	if (P.families & VALUE_RESULTS)
	{
		hipLaunchKernelGGL( spa_l2_values_place_results_kernel, grid, dim3( 256), 0, stream, P);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	if (P.families & VALUE_ITEMS)
	{
		hipLaunchKernelGGL( spa_l2_values_place_items_kernel, grid, dim3( 256), 0, stream, P);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	return hipSuccess;
}

}
