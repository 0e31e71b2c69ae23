// The three launches of one pass of the stable radix partition of pairs (radix_passes.h): one copy for every product that
// partitions (l2_postings_kernel.hip, l2_positions_kernel.hip).
#include <hip/hip_runtime.h>
#include "radix_passes.h"

using namespace spa;

extern "C" __global__ __launch_bounds__(256) void spa_radix_histogram_kernel( RadixPass R) { radixCountDigits( R); }
extern "C" __global__ __launch_bounds__(1024) void spa_radix_scan_kernel( RadixPass R) { radixScanHistogram( R); }
extern "C" __global__ __launch_bounds__(256) void spa_radix_scatter_kernel( RadixPass R) { radixScatterPairs( R); }

namespace spa {

hipError_t launchRadixPass( const RadixPass& R, unsigned numCUs, hipStream_t stream, hipEvent_t* ev)
{
	hipError_t e;
	const dim3 perTile( wavePerDocumentBlocks( R.tiles, numCUs));
	hipLaunchKernelGGL( spa_radix_histogram_kernel, perTile, dim3( 256), 0, stream, R);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (ev && (e = hipEventRecord( ev[ 0], stream)) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_radix_scan_kernel, dim3( 1), dim3( 1024), 0, stream, R);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (ev && (e = hipEventRecord( ev[ 1], stream)) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_radix_scatter_kernel, perTile, dim3( 256), 0, stream, R);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (ev && (e = hipEventRecord( ev[ 2], stream)) != hipSuccess) return e;
	return hipSuccess;
}

hipError_t launchRadixPass( const RadixPass& R, unsigned numCUs, hipStream_t stream) { return launchRadixPass( R, numCUs, stream, 0); }

}
