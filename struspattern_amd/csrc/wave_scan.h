// Wavefront helpers shared by the kernels: lane index, wave-uniform values and loads, prefix scans.
#ifndef SPA_WAVE_SCAN_H
#define SPA_WAVE_SCAN_H
#include <stdint.h>

namespace spa {

typedef uint32_t u32;
typedef uint64_t u64;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

#define LANE ((u32)(threadIdx.x & 63u))

// wave-uniform value: lane 0's, in a scalar register
__device__ __forceinline__ u32 uni( u32 v) { return __builtin_amdgcn_readfirstlane( v); }
// Wave-uniform load: every lane reads the same address; the value is moved to a scalar register so
// that everything computed from it (indices, loop bounds, branch conditions) stays scalar and the
// control flow is made of scalar branches, not exec-masked vector loops.
__device__ __forceinline__ u32 ldu( const u32* p) { return __builtin_amdgcn_readfirstlane( *p); }
// 16-byte load: one memory instruction moves a quarter/third/half of a record
__device__ __forceinline__ uint4 ld4( const void* p) { const u32x4 v = *(const u32x4*)p; return make_uint4( v.x, v.y, v.z, v.w); }

// Inclusive prefix operations over the 64 lanes of a wavefront with DPP row shifts / row broadcasts
// (6 VALU instructions, no LDS traffic; a shuffle-based scan is 6 dependent ds_bpermute round trips).
// All 64 lanes must be active.
__device__ __forceinline__ uint32_t waveScanAdd( uint32_t v)
{
	v += (uint32_t)__builtin_amdgcn_update_dpp( 0, (int)v, 0x111, 0xF, 0xF, true);	// row_shr:1
	v += (uint32_t)__builtin_amdgcn_update_dpp( 0, (int)v, 0x112, 0xF, 0xF, true);	// row_shr:2
	v += (uint32_t)__builtin_amdgcn_update_dpp( 0, (int)v, 0x114, 0xF, 0xF, true);	// row_shr:4
	v += (uint32_t)__builtin_amdgcn_update_dpp( 0, (int)v, 0x118, 0xF, 0xF, true);	// row_shr:8
	v += (uint32_t)__builtin_amdgcn_update_dpp( 0, (int)v, 0x142, 0xA, 0xF, false);	// row_bcast:15 into rows 1,3
	v += (uint32_t)__builtin_amdgcn_update_dpp( 0, (int)v, 0x143, 0xC, 0xF, false);	// row_bcast:31 into rows 2,3
	return v;
}

__device__ __forceinline__ uint32_t waveScanMax( uint32_t v)		// unsigned maximum (identity 0)
{
	uint32_t t;
	t = (uint32_t)__builtin_amdgcn_update_dpp( 0, (int)v, 0x111, 0xF, 0xF, true); v = t > v ? t : v;
	t = (uint32_t)__builtin_amdgcn_update_dpp( 0, (int)v, 0x112, 0xF, 0xF, true); v = t > v ? t : v;
	t = (uint32_t)__builtin_amdgcn_update_dpp( 0, (int)v, 0x114, 0xF, 0xF, true); v = t > v ? t : v;
	t = (uint32_t)__builtin_amdgcn_update_dpp( 0, (int)v, 0x118, 0xF, 0xF, true); v = t > v ? t : v;
	t = (uint32_t)__builtin_amdgcn_update_dpp( 0, (int)v, 0x142, 0xA, 0xF, false); v = t > v ? t : v;
	t = (uint32_t)__builtin_amdgcn_update_dpp( 0, (int)v, 0x143, 0xC, 0xF, false); v = t > v ? t : v;
	return v;
}

} // namespace
#endif
