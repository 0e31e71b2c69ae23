// The span rule on the device (span_text.hpp states it): what the text passes (l2_text_kernel.hip) and the value passes
// (l2_values_kernel.hip) share.  PARAMS has the text source: text, nbytes, segOffsets, nseg, docSegOffsets.
#ifndef SPA_L2_SPAN_H
#define SPA_L2_SPAN_H
#include "doc_passes.h"

namespace spa {

typedef u32 u32b __attribute__((aligned(1)));		// a 4-byte load from any address of the text

// what one lane wrote to LDS is read by the other lanes of its wave (and the other way round) only across this
__device__ __forceinline__ void waveLdsSync()
{
	__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront");
}

// the segments [d0, d1) of a document
template <class PARAMS>
__device__ __forceinline__ void docSegments( const PARAMS& P, u32 doc, u64& d0, u64& d1)
{
	d0 = doc; d1 = (u64)doc + 1;
	if (P.docSegOffsets) { d0 = uni64( P.docSegOffsets[ doc]); d1 = uni64( P.docSegOffsets[ (u64)doc+1]); }
}

// The rule (span_text.hpp): the byte range of the span of record `rec` in a document of the segments [d0, d1); false for
// an invalid span.  Every index into segOffsets is at most nseg when it is formed.
template <class PARAMS>
__device__ __forceinline__ bool spanRange( const PARAMS& P, u64 d0, u64 d1, const u32* rec, u64& begin, u64& length)
{
	const u32x4 w = *(const u32x4u*)(rec + 3);
	const u64 origseg = w.x, origpos = w.y, origendseg = w.z, origend = w.w;
	begin = 0; length = 0;
	if (d0 > d1 || d1 > P.nseg) return false;
	if (origseg > origendseg || origendseg >= d1 - d0) return false;
	const u64 s0 = d0 + origseg, s1 = d0 + origendseg;
	const u64 a = P.segOffsets[ s0], b = P.segOffsets[ s0+1], c = P.segOffsets[ s1], e = P.segOffsets[ s1+1];
	if (a > b || c > e || (s0 != s1 && b > c)) return false;
	if (origpos > b - a || origend > e - c) return false;
	const u64 end = c + origend;
	begin = a + origpos;
	if (begin > end || end > P.nbytes) return false;
	length = end - begin;
	return true;
}

// one byte of the text, the index clamped into it
template <class PARAMS>
__device__ __forceinline__ u32 textByte( const PARAMS& P, u64 src)
{
	if (!P.nbytes) return 0;
	return P.text[ src < P.nbytes ? src : P.nbytes - 1];
}

} // namespace
#endif
