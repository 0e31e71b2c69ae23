// The launch of a lexer batch, as its plan says (l1_image.hpp): the sequence of the kernel families of l1_launch.h.  Host code
// only, no device header.
#include "l1_launch.h"

namespace spa {

hipError_t launchL1Lex( const L1LaunchPlan& plan, const L1Params& PS, const L1Params& PW, const L1Params& P, hipStream_t stream, hipEvent_t betweenKernels, hipEvent_t afterWords)
{
	hipError_t e;
	if (plan.route == L1_ROUTE_APPROX)
	{
		e = launchL1Approx( plan, P, stream);
		if (e != hipSuccess) return e;
		if (betweenKernels) { e = hipEventRecord( betweenKernels, stream); if (e != hipSuccess) return e; }
		return afterWords ? hipEventRecord( afterWords, stream) : hipSuccess;
	}
	// the units of the batch (chunks of long documents), then BOTH sets of instances: which one a batch needs is known on
	// the device only (classes by code point: here; chunked documents: after the units kernel) -- the other one leaves at once
	e = launchL1Units( P, stream);
	if (e != hipSuccess) return e;
	L1Params S = PS;
	S.sequentialPass = 1;
	if (plan.route == L1_ROUTE_LANES)
	{
		// a lane per stream (scanUnitLanes); the documents a piece of which could not be joined go through the sequential pass
		// of the one-pass instance behind it
		launchL1ScanLanes( plan, PS, stream);
		e = launchL1ScanSequential( plan, S, stream);
		if (e != hipSuccess) return e;
	}
	else if (plan.route == L1_ROUTE_PASSES)
	{
		e = launchL1ScanPasses( plan, PS, S, stream);
		if (e != hipSuccess) return e;
	}
	// (L1_ROUTE_NONE: nothing to scan, the caller has cleared the report counts)
	e = hipGetLastError();
	if (e != hipSuccess) return e;
	if (betweenKernels) { e = hipEventRecord( betweenKernels, stream); if (e != hipSuccess) return e; }
	if (plan.wordsKernel)
	{
		e = launchL1Words( plan, PW, stream);
		if (e != hipSuccess) return e;
	}
	if (afterWords) { e = hipEventRecord( afterWords, stream); if (e != hipSuccess) return e; }
	return launchL1Post( plan, P, stream);
}
}
