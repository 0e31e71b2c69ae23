// Term-block passes of a finished device batch (l2_termblocks.h): sizes, offsets, emit.
#include <hip/hip_runtime.h>
#include "doc_passes.h"
#include "l2_span.h"
#include "l2_termblocks.h"
#include "l2_term_value.h"
#include "term_block_code.h"

using namespace spa;

namespace {

const u32 NONE = TERM_NONE;
const u32 HEADER_SLOT = 32;		// bytes of a lane's header in LDS: TERM_BLOCK_HEADER_MAX, and its length in the last byte

// ---- what position k codes: the one reading of the sizing and the emitting pass
struct Position
{
	TermBlockEntry code;
	const uint8_t* suffixAt;	// the first byte stored
	u64 bytes;			// termBlockCodeBytes; 0 behind the last position
	u32 handle;
	u32 valueBytes;
};

// Whole waves get here: the lane below is asked for its handle.  A position whose order[k] is no entry (no order of this
// library leaves one) codes the handle 0 with an empty value.
__device__ __forceinline__ Position readPosition( const TermBlocksParams& P, u64 k)
{
	const bool active = k < P.ndict;
	u32 e = NONE, handle = 0, prefix = 0, docFreq = 0;
	u64 count = 0;
	TermValue v;
	v.p = 0; v.len = 0; v.ok = false;
	if (active) e = P.order[ k];
	if (e < P.ndict)
	{
		const u32* rec = P.dictRecords + 8*(u64)e;
		handle = rec[ 0]; docFreq = rec[ 4]; count = rec[ 6] | ((u64)rec[ 7] << 32);
		v = storedValue( P, e);
		prefix = P.prefixBytes[ k];
	}
	u32 handleBefore = (u32)__shfl_up( (int)handle, 1);
	if (LANE == 0 && active && k)
	{
		const u32 before = P.order[ k-1];
		handleBefore = before < P.ndict ? P.dictRecords[ 8*(u64)before] : 0u;
	}
	Position p;
	p.code = termBlockEntry( (k & (P.blockEntries - 1)) == 0, handle, handleBefore, prefix, v.len, docFreq, count);
	p.suffixAt = v.p + p.code.shared;
	p.bytes = active ? termBlockCodeBytes( p.code) : 0;
	p.handle = handle;
	p.valueBytes = v.len;
	return p;
}

// inclusive prefix sum of 64 code lengths (each below 2^33) in 64 bits
__device__ __forceinline__ u64 waveScanBytes( u64 v) { return waveScanAdd64( (u32)v) + ((u64)waveScanAdd( (u32)(v >> 32)) << 32); }
// the value of another lane, which differs between lanes
__device__ __forceinline__ u64 laneValue64( u64 v, u32 lane)
{
	return ((u64)(u32)__shfl( (int)(u32)(v >> 32), (int)lane) << 32) | (u32)__shfl( (int)(u32)v, (int)lane);
}

// ---- sizes: the bytes and the handle of every block, the sum of value_bytes
__device__ void sizeBlocks( const TermBlocksParams& P)
{
	const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	const Position p = readPosition( P, k);
	const bool active = k < P.ndict;
	const u32 B = P.blockEntries, headLane = LANE & ~(B - 1);
	const u64 incl = waveScanBytes( p.bytes);
	const u64 beforeBlock = laneValue64( incl - p.bytes, headLane);
	const u64 j = k >> __builtin_ctz( B);
	if (active && j < P.nblocks)
	{
		if ((k & (B - 1)) == B - 1 || k == (u64)P.ndict - 1) P.blockSize[ j] = incl - beforeBlock;
		if (LANE == headLane) P.blockHandles[ j] = p.handle;
	}
	const u64 values = waveLane64( waveScanAdd64( active ? p.valueBytes : 0u), 63);
	if (LANE == 0 && values) atomicAdd( (unsigned long long*)(P.totals + 3), (unsigned long long)values);
}

// ---- offsets: where every block starts, and the totals
__device__ void scanBlocks( const TermBlocksParams& P)
{
	const DocSums<2> sum = scanDocumentCounts<u64, 2>( P.nblocks,
		[&]( u64 j) { const u64 s = P.blockSize[ j]; return DocCounts<2>{{ (u32)s, (u32)(s >> 32)}}; },
		[&]( u64 j, const DocCounts<2>&, const DocSums<2>& at) { P.blockOffsets[ j] = at.v[ 0] + (at.v[ 1] << 32); });
	if (threadIdx.x == 0)
	{
		const u64 nbytes = sum.v[ 0] + (sum.v[ 1] << 32);
		P.blockOffsets[ P.nblocks] = nbytes;
		P.totals[ 0] = P.nblocks; P.totals[ 1] = nbytes; P.totals[ 2] = P.blockEntries;
	}
}

// ---- emit: the codes of 64 positions by the whole wave
__device__ void emitBlocks( const TermBlocksParams& P)
{
	__shared__ uint8_t sHeader[ 4][ 64][ HEADER_SLOT];
	__shared__ u64 sStart[ 4][ 66];
	__shared__ u64 sSuffixAt[ 4][ 64];
	__shared__ u32 sSuffix[ 4][ 64];
	const u32 wave = threadIdx.x >> 6;
	const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	const Position p = readPosition( P, k);
	const bool active = k < P.ndict;
	const u32 B = P.blockEntries, headLane = LANE & ~(B - 1);
	const u64 incl = waveScanBytes( p.bytes);
	const u64 beforeBlock = laneValue64( incl - p.bytes, headLane);
	const u64 j = k >> __builtin_ctz( B);
	// the range of the position's block, cut to the capacity; the position's own range, cut to that
	u64 b0 = 0, b1 = 0;
	if (active && j < P.nblocks) { b0 = P.blockOffsets[ j]; b1 = P.blockOffsets[ j+1]; }
	if (b1 > P.capacity) b1 = P.capacity;
	if (b0 > b1) b0 = b1;
	u64 start = b0 + (incl - p.bytes - beforeBlock);
	if (start < b0 || start > b1) start = b1;
	// the span of the wave: from the first block of lane 0 to the end of the block of the last position
	const u64 nactive = __popcll( __ballot( active));
	if (!nactive) return;
	const u64 g0 = waveLane64( b0, 0), g1 = waveLane64( b1, (int)nactive - 1);
	if (!active) start = g1;
	uint8_t* header = sHeader[ wave][ LANE];
	header[ HEADER_SLOT - 1] = active ? (uint8_t)writeTermBlockHeader( header, p.code) : (uint8_t)0;
	sStart[ wave][ LANE] = start;
	if (LANE == 63) sStart[ wave][ 64] = g1;
	sSuffixAt[ wave][ LANE] = (u64)(size_t)p.suffixAt;
	sSuffix[ wave][ LANE] = active ? p.code.suffix : 0u;
	waveLdsSync();
	const u64* starts = sStart[ wave];
	// a lane per aligned output dword; byte x is byte x - starts[i] of the code of the last lane i with starts[i] <= x
	for (u64 q = (g0 >> 2) + LANE; q < ((g1 + 3) >> 2); q += 64)
	{
		const u64 a = q << 2;
		const u32 first = a < g0 ? (u32)(g0 - a) : 0u, last = a + 4 > g1 ? (u32)(g1 - a) : 4u;	// the bytes [first, last) of the dword are the span's
		u64 x = a + first;
		u32 i = 0;
		for (u32 step=32; step; step>>=1) if (starts[ i+step] <= x) i += step;
		const bool whole = first == 0 && last == 4;
		u32 v = 0;
		const u64 at = x - starts[ i];
		const u32 headerBytes = sHeader[ wave][ i][ HEADER_SLOT - 1];
		if (whole && at >= headerBytes && at - headerBytes + 4 <= sSuffix[ wave][ i])
		{
			// the dword lies inside one suffix
			v = *(const u32b*)((const uint8_t*)(size_t)sSuffixAt[ wave][ i] + (at - headerBytes));
		}
		else for (u32 b=first; b<last; ++b, ++x)
		{
			while (i < 63 && starts[ i+1] <= x) ++i;
			const u64 o = x - starts[ i];
			const u32 h = sHeader[ wave][ i][ HEADER_SLOT - 1];
			u32 byte = 0;			// (a byte of a block that no code reaches)
			if (o < h) byte = sHeader[ wave][ i][ o];
			else if (o - h < sSuffix[ wave][ i]) byte = ((const uint8_t*)(size_t)sSuffixAt[ wave][ i])[ o - h];
			v |= byte << (8*b);
		}
		// (an edge dword is shared with the neighbouring wave: bytes, never a read-modify-write)
		if (whole) *(u32*)(P.bytes + a) = v;
		else for (u32 b=first; b<last; ++b) P.bytes[ a + b] = (uint8_t)(v >> (8*b));
	}
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l2_termblocks_sizes_kernel( TermBlocksParams P) { sizeBlocks( P); }
extern "C" __global__ __launch_bounds__(1024) void spa_l2_termblocks_offsets_kernel( TermBlocksParams P) { scanBlocks( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_termblocks_emit_kernel( TermBlocksParams P) { emitBlocks( P); }

namespace spa {

hipError_t launchL2TermBlocksCount( const TermBlocksParams& P, unsigned, hipStream_t stream)
{
	if (!P.ndict || !termBlockEntriesValid( P.blockEntries)) return hipErrorInvalidValue;
	hipLaunchKernelGGL( spa_l2_termblocks_sizes_kernel, dim3( (unsigned)(((u64)P.ndict + 255u) / 256u)), dim3( 256), 0, stream, P);
	const hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l2_termblocks_offsets_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	return hipGetLastError();
}

hipError_t launchL2TermBlocksPlace( const TermBlocksParams& P, unsigned, hipStream_t stream)
{
	if (!P.ndict || !P.capacity) return hipSuccess;
	hipLaunchKernelGGL( spa_l2_termblocks_emit_kernel, dim3( (unsigned)(((u64)P.ndict + 255u) / 256u)), dim3( 256), 0, stream, P);
	return hipGetLastError();
}

}
