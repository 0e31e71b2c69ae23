// Frequency passes of a finished device batch (l2_freq.h): count, offsets, place, totals.
#include <hip/hip_runtime.h>
#include "doc_passes.h"
#include "l2_freq.h"

using namespace spa;

namespace {

enum {FREQ_ERR_RANGE=5};		// SP_DOC_ERR_RANGE (include/strus_pattern_amd.h)
enum {WORDS = FREQ_WINDOW/32};		// bitmap words of a window; a trip of the rank scan takes 64 of them
static_assert( FREQ_WINDOW % 2048 == 0, "the rank scan walks the bitmap 64 words a trip");
static_assert( FREQ_WINDOW <= 65536, "the running popcounts of a window are kept in 16 bits");

// What one lane wrote is read by the other lanes of its wave only across this: the bitmap and the ranks in LDS, and the
// initialised records in HBM before the atomics of other lanes go to them (the release is of agent scope, so that the
// stores have arrived where the atomics are executed).
__device__ __forceinline__ void waveSync()
{
	__builtin_amdgcn_fence( __ATOMIC_RELEASE, "agent");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool validHandle( const FreqParams& P, u32 h) { return h - 1u < P.handleBound - 1u; }	// 1 <= h < handleBound
__device__ __forceinline__ u32 waveMax( u32 v) { return uni( (u32)__shfl( (int)waveScanMax( v), 63)); }

// The distinct handles of the window [base, base + FREQ_WINDOW) among the results [r0, r1), as bits of the wave's bitmap
// (cleared here).  A handle indexes the bitmap only after it was found inside the bound and inside the window.
__device__ __forceinline__ void markWindow( const FreqParams& P, u64 r0, u64 r1, u32 base, u32* bitmap)
{
	waveSync();		// (lanes may still be reading the bitmap of the window before)
	for (u32 k=LANE; k<(u32)WORDS; k+=64) bitmap[ k] = 0;
	waveSync();
	for (u64 r=r0; r<r1; r+=64)
	{
		const u64 i = r + LANE;
		if (i >= r1) continue;
		const u32 h = P.results[ 9*i];
		if (!validHandle( P, h)) continue;
		const u32 b = h - base;
		if (b < (u32)FREQ_WINDOW) atomicOr( &bitmap[ b >> 5], 1u << (b & 31u));
	}
	waveSync();
}

// ---- pass A: a wave per document
__device__ void countHandles( const FreqParams& P, u32* bitmap, u32* occ)
{
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor);
		if (doc >= P.ndocs) break;
		const u64 r0 = uni64( P.docOffsets[ doc]), r1 = uni64( P.docOffsets[ (u64)doc+1]);
		u32 count = 0, lo = 0xFFFFFFFFu, hi = 0;
		u64 windows = 0;
		bool failed = false;
		if (r0 < r1 && r1 <= P.nresults)
		{
			// the bound check, the range of the handles and the windows they touch (bit: window index modulo 64)
			waveSync();
			if (LANE < 2) occ[ LANE] = 0;
			waveSync();
			for (u64 r=r0; r<r1; r+=64)
			{
				const u64 i = r + LANE;
				const bool active = i < r1;
				const u32 h = active ? P.results[ 9*i] : 0u;
				if (__ballot( active && !validHandle( P, h))) { failed = true; break; }
				if (active)
				{
					lo = h < lo ? h : lo; hi = h > hi ? h : hi;
					const u32 win = h / (u32)FREQ_WINDOW;
					atomicOr( &occ[ (win >> 5) & 1u], 1u << (win & 31u));
				}
			}
			if (!failed)
			{
				waveSync();
				hi = waveMax( hi); lo = ~waveMax( ~lo);
				windows = ((u64)uni( occ[ 1]) << 32) | uni( occ[ 0]);
				for (u32 win=lo/(u32)FREQ_WINDOW; win<=hi/(u32)FREQ_WINDOW; ++win)
				{
					if (!((windows >> (win & 63u)) & 1u)) continue;
					markWindow( P, r0, r1, win*(u32)FREQ_WINDOW, bitmap);
					for (u32 k=LANE; k<(u32)WORDS; k+=64) count += (u32)__popc( bitmap[ k]);
				}
				count = uni( (u32)__shfl( (int)waveScanAdd( count), 63));
			}
		}
		if (LANE == 0)
		{
			P.docCount[ doc] = failed ? 0u : count;
			P.docStatus[ doc] = failed ? FREQ_ERR_RANGE : 0;
			u32* meta = P.docMeta + 4*(u64)doc;
			meta[ 0] = lo; meta[ 1] = hi; meta[ 2] = (u32)windows; meta[ 3] = (u32)(windows >> 32);
		}
	}
}

// ---- pass B: the offsets of the documents' records (doc_passes.h).  A document with a range status counts 0.
__device__ void scanDocuments( const FreqParams& P)
{
	const u64 total = scanDocumentCounts<u64, 1>( P.ndocs,
		[&]( u64 d) { return DocCounts<1>{{ P.docStatus[ d] == 0 ? P.docCount[ d] : 0u}}; },
		[&]( u64 d, const DocCounts<1>&, const DocSums<1>& at) { P.docFreqOffsets[ d] = at.v[ 0]; }).v[ 0];
	if (threadIdx.x == 0) { P.docFreqOffsets[ P.ndocs] = total; *P.total = total; }
}

// ---- pass C: a wave per document.  Whatever the results and the working arrays hold, every record written lies inside
// the document's block [docFreqOffsets[d], docFreqOffsets[d+1]) and that inside the output.
__device__ void placeHandles( const FreqParams& P, u32* bitmap, uint16_t* rank)
{
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor + 1);
		if (doc >= P.ndocs) break;
		const u64 r0 = uni64( P.docOffsets[ doc]), r1 = uni64( P.docOffsets[ (u64)doc+1]);
		if (r0 >= r1 || r1 > P.nresults) continue;
		if (uni( (u32)P.docStatus[ doc]) != 0) continue;
		const u64 at = uni64( P.docFreqOffsets[ doc]), end = uni64( P.docFreqOffsets[ (u64)doc+1]);
		if (end <= at || end > P.capacity) continue;
		const u64 n = end - at;
		const u32* meta = P.docMeta + 4*(u64)doc;
		const u32 lo = uni( meta[ 0]), hi = uni( meta[ 1]);
		const u64 windows = ((u64)uni( meta[ 3]) << 32) | uni( meta[ 2]);
		u64 done = 0;		// records of the windows before
		for (u32 win=lo/(u32)FREQ_WINDOW; win<=hi/(u32)FREQ_WINDOW; ++win)
		{
			if (!((windows >> (win & 63u)) & 1u)) continue;
			const u32 base = win*(u32)FREQ_WINDOW;
			markWindow( P, r0, r1, base, bitmap);
			// the set bits below every bitmap word, and the records of the window: a lane per word, 64 words a trip
			u32 carry = 0;
			for (u32 t=0; t<(u32)WORDS; t+=64)
			{
				const u32 k = t + LANE;
				u32 bits = bitmap[ k];
				const u32 incl = waveScanAdd( (u32)__popc( bits));
				const u32 below = carry + incl - (u32)__popc( bits);
				rank[ k] = (uint16_t)below;
				u64 idx = done + below;
				while (bits)
				{
					const u32 bit = (u32)__ffs( (int)bits) - 1u;
					bits &= bits - 1u;
					if (idx < n)
					{
						const u32x4 init = { base + 32u*k + bit, 0u, 0xFFFFFFFFu, 0u };
						*(u32x4*)(P.records + 4*(at + idx)) = init;
					}
					++idx;
				}
				carry += uni( (u32)__shfl( (int)incl, 63));
			}
			waveSync();
			// count, minimum and maximum per result
			for (u64 r=r0; r<r1; r+=64)
			{
				const u64 i = r + LANE;
				if (i >= r1) continue;
				const u32x4 w = *(const u32x4u*)(P.results + 9*i);	// handle, ordpos, ordend
				if (!validHandle( P, w.x)) continue;
				const u32 b = w.x - base;
				if (b >= (u32)FREQ_WINDOW) continue;
				const u32 bits = bitmap[ b >> 5];
				const u64 idx = done + rank[ b >> 5] + (u32)__popc( bits & ((1u << (b & 31u)) - 1u));
				if (idx >= n) continue;
				u32* rec = P.records + 4*(at + idx);
				atomicAdd( rec + 1, 1u);
				atomicMin( rec + 2, w.y);
				atomicMax( rec + 3, w.z);
			}
			done += carry;
		}
	}
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l2_freq_count_kernel( FreqParams P)
{
	__shared__ u32 bitmap[ 4][ WORDS];
	__shared__ u32 occ[ 4][ 2];
	const u32 wave = threadIdx.x >> 6;
	countHandles( P, bitmap[ wave], occ[ wave]);
}

extern "C" __global__ __launch_bounds__(1024) void spa_l2_freq_offsets_kernel( FreqParams P) { scanDocuments( P); }

extern "C" __global__ __launch_bounds__(256) void spa_l2_freq_place_kernel( FreqParams P)
{
	__shared__ u32 bitmap[ 4][ WORDS];
	__shared__ uint16_t rank[ 4][ WORDS];
	const u32 wave = threadIdx.x >> 6;
	placeHandles( P, bitmap[ wave], rank[ wave]);
}

// ---- pass D: every record of the batch once to the sums of its handle (the records are complete: pass C has ended)
extern "C" __global__ __launch_bounds__(256) void spa_l2_freq_totals_kernel( FreqParams P)
{
	for (u64 j=(u64)blockIdx.x*256 + threadIdx.x; j<P.capacity; j+=(u64)gridDim.x*256)
	{
		const u32x4 rec = *(const u32x4*)(P.records + 4*j);
		if (!validHandle( P, rec.x)) continue;
		atomicAdd( (unsigned long long*)(P.handleResults + rec.x), (unsigned long long)rec.y);
		atomicAdd( P.handleDocs + rec.x, 1u);
	}
}

namespace spa {

hipError_t launchL2FreqCount( const FreqParams& P, unsigned numCUs, hipStream_t stream)
{
	hipError_t e;
	hipLaunchKernelGGL( spa_l2_freq_count_kernel, dim3( wavePerDocumentBlocks( P.ndocs, numCUs)), dim3( 256), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l2_freq_offsets_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	return hipGetLastError();
}

hipError_t launchL2FreqPlace( const FreqParams& P, unsigned numCUs, hipStream_t stream)
{
	hipError_t e;
	hipLaunchKernelGGL( spa_l2_freq_place_kernel, dim3( wavePerDocumentBlocks( P.ndocs, numCUs)), dim3( 256), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	// a thread per record up to 8 workgroups per CU, the rest by grid stride
	const uint64_t want = (P.capacity + 255) / 256, most = (uint64_t)numCUs * 8;
	const unsigned blocks = (unsigned)(want < most ? (want ? want : 1) : most);
	hipLaunchKernelGGL( spa_l2_freq_totals_kernel, dim3( blocks), dim3( 256), 0, stream, P);
	return hipGetLastError();
}

}
