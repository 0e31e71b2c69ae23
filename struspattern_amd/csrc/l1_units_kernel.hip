// Units kernel of the lexer: one wave cuts the documents of a batch into scan units before any of them is scanned.
#include <hip/hip_runtime.h>
#include "l1_device.h"
#include "wave_scan.h"
#include "l1_launch.h"

using namespace spa;

namespace {

// UNITS: one wave counts the chunks of every document: unitStart[], the number of units, whether any document has more than
// one; and clears the per-document flags
__device__ void countUnits( const L1Params& P)
{
	u32 running = 0, chunked = 0;
	for (u32 base=0; base<P.ndocs; base+=64)
	{
		const u32 d = base + LANE;
		u32 n = 0;
		if (d < P.ndocs)
		{
			const u64 len = P.docOffsets[ d+1] - P.docOffsets[ d];
			n = len ? (u32)((len + P.chunkBytes - 1) / P.chunkBytes) : 1u;
			P.docStatus[ d] = 0; P.docSequential[ d] = 0;
		}
		const u32 incl = waveScanAdd( n);
		if (d < P.ndocs) P.unitStart[ d] = running + incl - n;
		running += uni( (u32)__shfl( (int)incl, 63));
		if (__ballot( n > 1u)) chunked = 1;
	}
	if (LANE == 0)
	{
		P.unitStart[ P.ndocs] = running;
		*(u32*)&P.counters[ L1C_UNITS] = running;
		*(u32*)&P.counters[ L1C_CHUNKED] = chunked;
	}
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(64) void spa_l1_units_kernel( L1Params P) { countUnits( P); }

namespace spa {
hipError_t launchL1Units( const L1Params& P, hipStream_t stream)
{
	hipLaunchKernelGGL( spa_l1_units_kernel, dim3( 1), dim3( 64), 0, stream, P);
	return hipGetLastError();
}
} // namespace
