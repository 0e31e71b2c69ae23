// Lookup passes over an index segment (l2_segment.h): find, runs, sizes, offsets, emit.
#include <hip/hip_runtime.h>
#include "doc_passes.h"
#include "l2_segment.h"

using namespace spa;

namespace {

__device__ __forceinline__ u64 least( u64 a, u64 b) { return a < b ? a : b; }

// ---- find: the run of every query
__device__ void findRuns( const SegmentLookupParams& P)
{
	const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= P.nq) return;
	// the bytes of the query, cut to what was uploaded
	const u64 a = least( P.queryOffsets[ i], P.queryNbytes), b = least( P.queryOffsets[ i+1], P.queryNbytes);
	const SegmentRun run = segmentFind( P.segment, P.queryHandles[ i], P.queryBytes + a, b > a ? b - a : 0, P.prefix != 0);
	P.qFirst[ i] = run.first; P.qCount[ i] = run.count; P.qStatus[ i] = run.status;
}

// ---- runs: where the run of every query starts in the selection
__device__ void scanRuns( const SegmentLookupParams& P)
{
	const DocSums<1> sum = scanDocumentCounts<u64, 1>( P.nq,
		[&]( u64 i) { return DocCounts<1>{{ P.qCount[ i]}}; },
		[&]( u64 i, const DocCounts<1>&, const DocSums<1>& at) { P.qSelOffsets[ i] = at.v[ 0]; });
	if (threadIdx.x == 0) { P.qSelOffsets[ P.nq] = sum.v[ 0]; P.totals[ 0] = sum.v[ 0]; }
}

// the sorted position of selection s and its query; false for a position outside the segment (no run of `find` holds one)
__device__ __forceinline__ bool selectedPosition( const SegmentLookupParams& P, u64 s, u32& query, u32& k)
{
	query = selectionQuery( P.qSelOffsets, P.nq, s);
	const u64 at = P.qSelOffsets[ query], position = (u64)P.qFirst[ query] + (s - at);
	k = (u32)position;
	return at <= s && position < P.segment.ndict;
}

// ---- sizes: the record and the counts of every selected position
__device__ void sizeSelections( const SegmentLookupParams& P)
{
	const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= least( P.totals[ 0], P.selCapacity)) return;
	u32 query = 0, k = 0;
	SelectionSizes z = { SEG_ERR_RANGE, 0, 0, 0, 0, 0, 0};
	if (selectedPosition( P, s, query, k))
	{
		CountingSink counting;
		z = walkSelection( P.segment, k, counting);
	}
	u32* record = P.selections + 6*s;
	record[ 0] = k; record[ 1] = z.handle; record[ 2] = z.docFreq; record[ 3] = z.valueBytes;
	record[ 4] = (u32)z.count; record[ 5] = (u32)(z.count >> 32);
	P.selStatus[ s] = z.status;
	P.selValueOffsets[ s] = z.valueBytes; P.selPostingOffsets[ s] = z.npostings; P.selPositionOffsets[ s] = z.npositions;
	if (z.status) atomicMax( P.qStatus + query, z.status);		// (a maximum: the same whatever the order)
}

// ---- offsets: the exclusive prefixes of the three counts, in place; every count is below 2^32
__device__ void scanSelections( const SegmentLookupParams& P)
{
	const u64 nsel = least( P.totals[ 0], P.selCapacity);
	const DocSums<3> sum = scanDocumentCounts<u64, 3>( nsel,
		[&]( u64 s) { return DocCounts<3>{{ (u32)P.selValueOffsets[ s], (u32)P.selPostingOffsets[ s], (u32)P.selPositionOffsets[ s]}}; },
		[&]( u64 s, const DocCounts<3>&, const DocSums<3>& at) {
			P.selValueOffsets[ s] = at.v[ 0]; P.selPostingOffsets[ s] = at.v[ 1]; P.selPositionOffsets[ s] = at.v[ 2];
		});
	if (threadIdx.x == 0)
	{
		P.selValueOffsets[ nsel] = sum.v[ 0]; P.selPostingOffsets[ nsel] = sum.v[ 1]; P.selPositionOffsets[ nsel] = sum.v[ 2];
		P.totals[ 1] = sum.v[ 1]; P.totals[ 2] = sum.v[ 2]; P.totals[ 3] = sum.v[ 0];
	}
}

// ---- emit: the value, the postings and the positions of every selected position, cut to what `sizes` counted
__device__ void emitSelections( const SegmentLookupParams& P)
{
	const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= P.nsel) return;
	// (the end of the last posting's positions is nobody's to write but the last lane's)
	if (s == P.nsel - 1) P.postingPositionOffsets[ P.npostings] = least( P.selPositionOffsets[ P.nsel], P.npositions);
	if (P.selStatus[ s]) return;
	u32 query = 0, k = 0;
	if (!selectedPosition( P, s, query, k)) return;
	const u64 v0 = P.selValueOffsets[ s], v1 = P.selValueOffsets[ s+1], p0 = P.selPostingOffsets[ s], p1 = P.selPostingOffsets[ s+1];
	const u64 x0 = P.selPositionOffsets[ s], x1 = P.selPositionOffsets[ s+1];
	// the ranges that `offsets` laid out lie inside what the host allocated for its totals
	if (v0 > v1 || v1 > P.nvalueBytes || v1 - v0 > MAX32 || p0 > p1 || p1 > P.npostings || x0 > x1 || x1 > P.npositions) return;
	WritingSink writing = { P.values + v0, (u32)(v1 - v0), P.postings + 4*p0, P.postingPositionOffsets + p0, p1 - p0, P.positions + x0, x1 - x0, x0 };
	walkSelection( P.segment, k, writing);
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l2_segment_find_kernel( SegmentLookupParams P) { findRuns( P); }
extern "C" __global__ __launch_bounds__(1024) void spa_l2_segment_runs_kernel( SegmentLookupParams P) { scanRuns( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_segment_sizes_kernel( SegmentLookupParams P) { sizeSelections( P); }
extern "C" __global__ __launch_bounds__(1024) void spa_l2_segment_offsets_kernel( SegmentLookupParams P) { scanSelections( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_segment_emit_kernel( SegmentLookupParams P) { emitSelections( P); }

namespace spa {

hipError_t launchL2SegmentFind( const SegmentLookupParams& P, hipStream_t stream)
{
	if (!P.nq || !P.segment.ndict || !termBlockEntriesValid( P.segment.blockEntries)) return hipErrorInvalidValue;
	hipLaunchKernelGGL( spa_l2_segment_find_kernel, dim3( (unsigned)(((u64)P.nq + 255u) / 256u)), dim3( 256), 0, stream, P);
	hipError_t e;
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l2_segment_runs_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	return hipGetLastError();
}

hipError_t launchL2SegmentCount( const SegmentLookupParams& P, hipStream_t stream)
{
	if (!P.selCapacity || P.selCapacity >= MAX32) return hipErrorInvalidValue;
	hipLaunchKernelGGL( spa_l2_segment_sizes_kernel, dim3( (unsigned)((P.selCapacity + 255u) / 256u)), dim3( 256), 0, stream, P);
	hipError_t e;
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l2_segment_offsets_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	return hipGetLastError();
}

hipError_t launchL2SegmentPlace( const SegmentLookupParams& P, hipStream_t stream)
{
	if (!P.nsel) return hipSuccess;
	if (P.nsel > P.selCapacity) return hipErrorInvalidValue;
	hipLaunchKernelGGL( spa_l2_segment_emit_kernel, dim3( (unsigned)((P.nsel + 255u) / 256u)), dim3( 256), 0, stream, P);
	return hipGetLastError();
}

}
