// Host entry point of l1_kernel.hip.
#ifndef SPA_L1_LAUNCH_H
#define SPA_L1_LAUNCH_H
#include <hip/hip_runtime_api.h>
#include "l1_image.hpp"

namespace spa {

// Enqueues the kernels of a batch as the plan says.  PS: the parameters of the scan kernel (its table image holds the scanned passes
// only); PW: of the words kernel (the passes it walks + the shape table; offsets biased); P: of the other kernels (all passes, read
// from global memory).  The two events are recorded behind the scan kernels and behind the words kernel.
hipError_t launchL1Lex( const L1LaunchPlan& plan, const L1Params& PS, const L1Params& PW, const L1Params& P, hipStream_t stream, hipEvent_t betweenKernels, hipEvent_t afterWords);

} // namespace
#endif
