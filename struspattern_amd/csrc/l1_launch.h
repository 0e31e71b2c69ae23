// Host entry points of the lexer kernels: launchL1Lex (l1_launch.cpp) enqueues a batch; the launch of each kernel family is
// defined behind its kernels (l1_*_kernel.hip).
#ifndef SPA_L1_LAUNCH_H
#define SPA_L1_LAUNCH_H
#include <hip/hip_runtime_api.h>
#include "l1_image.hpp"

namespace spa {

// Enqueues the kernels of a batch as the plan says.  PS: the parameters of the scan kernel (its table image holds the scanned passes
// only); PW: of the words kernel (the passes it walks + the shape table; offsets biased); P: of the other kernels (all passes, read
// from global memory).  The two events are recorded behind the scan kernels and behind the words kernel.
hipError_t launchL1Lex( const L1LaunchPlan& plan, const L1Params& PS, const L1Params& PW, const L1Params& P, hipStream_t stream, hipEvent_t betweenKernels, hipEvent_t afterWords);

// ---- the kernel families, as launchL1Lex calls them
// the units of the batch (l1_units_kernel.hip)
hipError_t launchL1Units( const L1Params& P, hipStream_t stream);
// approximate literal table: one kernel, one wave per workgroup (l1_approx_kernel.hip)
hipError_t launchL1Approx( const L1LaunchPlan& plan, const L1Params& P, hipStream_t stream);
// a lane per stream (l1_scan_lanes_kernel.hip); enqueues only: an error of this launch is the next hipGetLastError's
void launchL1ScanLanes( const L1LaunchPlan& plan, const L1Params& PS, hipStream_t stream);
// the instance of plan.scanPasses passes, every set a batch may need, with the sequential pass (S) behind it; and the sequential
// pass of the one-pass instance alone, behind the lane-per-stream kernel (l1_scan_kernel.hip)
hipError_t launchL1ScanPasses( const L1LaunchPlan& plan, const L1Params& PS, const L1Params& S, hipStream_t stream);
hipError_t launchL1ScanSequential( const L1LaunchPlan& plan, const L1Params& S, hipStream_t stream);
// whole-word literals and word shapes (l1_words_kernel.hip)
hipError_t launchL1Words( const L1LaunchPlan& plan, const L1Params& PW, hipStream_t stream);
// post-processing: the _cp instance, or the plain and the _ch instance (l1_post_kernel.hip)
hipError_t launchL1Post( const L1LaunchPlan& plan, const L1Params& P, hipStream_t stream);

// one launch; more dynamic LDS than the static limit has to be allowed first
inline hipError_t launchL1Kernel( const void* kernel, unsigned grid, unsigned threads, size_t lds, hipStream_t stream, const L1Params& params)
{
	if (lds > L1_STATIC_LDS_LIMIT)
	{
		hipError_t e = hipFuncSetAttribute( kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) return e;
	}
	void* args[ 1] = {(void*)&params};
	return hipLaunchKernel( kernel, dim3( grid), dim3( threads), args, lds, stream);
}

} // namespace
#endif
