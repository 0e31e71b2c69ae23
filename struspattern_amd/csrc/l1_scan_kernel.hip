// Scan kernel of the lexer (l1_scan.h): the instance for tables of up to 16 passes, and the launch of whichever instance a
// plan names (the others: l1_scan_kernel_p1_4.hip, l1_scan_kernel_p5_8.hip, l1_scan_kernel_p32.hip).
#include <cstring>
#include "l1_scan.h"
#include "l1_launch.h"

SPA_L1_KERNEL( p16, 16, 256)

namespace spa {
const ScanInstance g_scanInstanceP16 = SPA_L1_SCAN_INSTANCE( 16, 256);

namespace {
// the instance that runs `passes` passes (1..32)
const ScanInstance& scanInstance( unsigned passes)
{
	return passes <= 4 ? g_scanInstancesP1[ passes-1] : passes <= 8 ? g_scanInstancesP5[ passes-5] : passes <= 16 ? g_scanInstanceP16 : g_scanInstanceP32;
}
}

hipError_t launchL1ScanPasses( const L1LaunchPlan& plan, const L1Params& PS, const L1Params& S, hipStream_t stream)
{
	hipError_t e;
	const size_t lds = plan.scanLdsBytes();
	if (plan.scanPasses < 1 || plan.scanPasses > 32) return hipErrorInvalidValue;
	const ScanInstance& si = scanInstance( plan.scanPasses);
	// (the name reported is the plan's: the instance launched is the one of that name, or nothing is launched)
	if (std::strcmp( si.name, plan.scanKernelName) != 0 || plan.scanThreads > si.maxThreads) return hipErrorInvalidValue;
	if (plan.cp)
	{
		if ((e = launchL1Kernel( si.cp, plan.scanGrid, plan.scanThreads, lds, stream, PS)) != hipSuccess) return e;
		if ((e = launchL1Kernel( si.cp, plan.scanGrid, plan.scanThreads, lds, stream, S)) != hipSuccess) return e;
	}
	else
	{
		if ((e = launchL1Kernel( si.plain, plan.scanGrid, plan.scanThreads, lds, stream, PS)) != hipSuccess) return e;
		if ((e = launchL1Kernel( si.ch, plan.scanGrid, plan.scanThreads, lds, stream, PS)) != hipSuccess) return e;
		if ((e = launchL1Kernel( si.ch, plan.scanGrid, plan.scanThreads, lds, stream, S)) != hipSuccess) return e;
	}
	return hipSuccess;
}

hipError_t launchL1ScanSequential( const L1LaunchPlan& plan, const L1Params& S, hipStream_t stream)
{
	return launchL1Kernel( scanInstance( 1).ch, plan.scanGrid, plan.scanThreads, plan.scanLdsBytes(), stream, S);
}
} // namespace
