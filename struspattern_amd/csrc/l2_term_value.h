// What the term passes (l2_terms_kernel.hip), the dictionary passes (l2_dict_kernel.hip) and the order passes
// (l2_dictorder_kernel.hip) share on the device: the value of a result in the selected source, the hash of a term, the byte
// compares (the same bytes? how many leading bytes?), and the read of a word that other lanes write.
// The collision rule of both: a hash chooses where the probing starts and decides nothing else; two values are one term
// only after sameBytes.  Device code only: included by .hip files behind doc_passes.h and l2_terms.h.
#ifndef SPA_L2_TERM_VALUE_H
#define SPA_L2_TERM_VALUE_H
#include "doc_passes.h"
#include "l2_terms.h"

namespace spa {

const u32 TERM_NONE = 0xFFFFFFFFu;		// an empty slot, no slot, no term

// a word that other lanes have written with a store or an atomic, read where the atomics are executed
__device__ __forceinline__ u32 loadShared( const u32* p) { return __hip_atomic_load( p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// 1 <= h < handleBound
template <class PARAMS>
__device__ __forceinline__ bool validHandle( const PARAMS& P, u32 h) { return h - 1u < P.handleBound - 1u; }

// the value of result r (r < P.nresults): its range in the source that the flags and the format of the result select.
// ok: the range lies inside the source and is shorter than 2^32 bytes; nothing outside [p, p + len) is read.
// PARAMS names flags, resultFormat and source[2] as TermsParams does.
struct TermValue { const uint8_t* p; u32 len; bool ok; };

template <class PARAMS>
__device__ __forceinline__ TermValue valueOf( const PARAMS& P, u64 r)
{
	bool text = !(P.flags & 1u);
	if (P.flags == 3u) text = !(P.resultFormat && P.resultFormat[ r] != 0);
	const u64* offsets = text ? P.source[ 1].offsets : P.source[ 0].offsets;
	const uint8_t* bytes = text ? P.source[ 1].bytes : P.source[ 0].bytes;
	const u64 total = text ? P.source[ 1].total : P.source[ 0].total;
	const u64 b = offsets[ r], e = offsets[ r+1];
	TermValue v;
	v.ok = b <= e && e <= total && e - b <= MAX32;
	v.len = v.ok ? (u32)(e - b) : 0u;
	v.p = bytes + (v.ok ? b : 0);
	return v;
}

// [p, p + len) lies inside the bytes of source s
template <class PARAMS>
__device__ __forceinline__ bool insideSource( const PARAMS& P, int s, u64 p, u32 len)
{
	const u64 at = p - (u64)(size_t)P.source[ s].bytes;		// (wraps to a large number for an address before the bytes)
	return p >= (u64)(size_t)P.source[ s].bytes && at <= P.source[ s].total && len <= P.source[ s].total - at;
}

// The value of entry e (e < P.ndict) as the keys pass of the order left it in working memory (valueAt, valueLen of
// l2_dictorder.h), compared against both sources again: the order passes, and the term-block passes that run on the same memory.
template <class PARAMS>
__device__ __forceinline__ TermValue storedValue( const PARAMS& P, u32 e)
{
	TermValue v;
	const u64 p = P.valueAt[ e];
	v.len = P.valueLen[ e];
	v.ok = v.len == 0 || insideSource( P, 0, p, v.len) || insideSource( P, 1, p, v.len);
	if (!v.ok) v.len = 0;
	v.p = (const uint8_t*)(size_t)p;
	return v;
}

__device__ __forceinline__ u32 termHashMix( u32 h, u32 w)
{
	h = (h ^ w) * 0x9E3779B1u;
	return h ^ (h >> 15);
}

// Hash of (handle, length, bytes): the bytes as little-endian words counted from the start of the value, the last one
// filled up with zeros, so that the hash does not depend on where the value lies.  16-byte loads for a value that starts
// on a 16-byte address, 4-byte loads for one on a 4-byte address, bytes otherwise and for the tail.
__device__ __forceinline__ u32 hashTerm( u32 handle, const TermValue& v)
{
	u32 h = termHashMix( termHashMix( 0x811C9DC5u, handle), v.len);
	const uint8_t* p = v.p;
	u32 i = 0;
	if (((size_t)p & 15u) == 0)
	{
		for (; i+16<=v.len; i+=16)
		{
			const u32x4 w = *(const u32x4*)(p + i);
			h = termHashMix( termHashMix( termHashMix( termHashMix( h, w.x), w.y), w.z), w.w);
		}
	}
	if (((size_t)p & 3u) == 0)
	{
		for (; i+4<=v.len; i+=4) h = termHashMix( h, *(const u32*)(p + i));
	}
	for (; i<v.len; i+=4)
	{
		u32 w = p[ i];
		if (i+1 < v.len) w |= (u32)p[ i+1] << 8;
		if (i+2 < v.len) w |= (u32)p[ i+2] << 16;
		if (i+3 < v.len) w |= (u32)p[ i+3] << 24;
		h = termHashMix( h, w);
	}
	return termHashMix( h, h >> 16);
}

// the same length: the same bytes?
__device__ __forceinline__ bool sameBytes( const uint8_t* p, const uint8_t* q, u32 len)
{
	u32 i = 0;
	if ((((size_t)p | (size_t)q) & 15u) == 0)
	{
		for (; i+16<=len; i+=16)
		{
			const u32x4 a = *(const u32x4*)(p + i), b = *(const u32x4*)(q + i);
			if (a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w) return false;
		}
	}
	if ((((size_t)p | (size_t)q) & 3u) == 0)
	{
		for (; i+4<=len; i+=4) if (*(const u32*)(p + i) != *(const u32*)(q + i)) return false;
	}
	for (; i<len; ++i) if (p[ i] != q[ i]) return false;
	return true;
}

// the bytes before the first byte of a word that differs from the same word of the other value (the words are little-endian)
__device__ __forceinline__ u32 equalBytesOfWord( u32 a, u32 b) { return (u32)__builtin_ctz( a ^ b) >> 3; }

// the leading bytes that p and q share among their first `len`: `len` when they are the same there.  The alignment cases are
// those of sameBytes.
__device__ __forceinline__ u32 commonBytes( const uint8_t* p, const uint8_t* q, u32 len)
{
	u32 i = 0;
	if ((((size_t)p | (size_t)q) & 15u) == 0)
	{
		for (; i+16<=len; i+=16)
		{
			const u32x4 a = *(const u32x4*)(p + i), b = *(const u32x4*)(q + i);
			if (a.x != b.x) return i + equalBytesOfWord( a.x, b.x);
			if (a.y != b.y) return i + 4 + equalBytesOfWord( a.y, b.y);
			if (a.z != b.z) return i + 8 + equalBytesOfWord( a.z, b.z);
			if (a.w != b.w) return i + 12 + equalBytesOfWord( a.w, b.w);
		}
	}
	if ((((size_t)p | (size_t)q) & 3u) == 0)
	{
		for (; i+4<=len; i+=4)
		{
			const u32 a = *(const u32*)(p + i), b = *(const u32*)(q + i);
			if (a != b) return i + equalBytesOfWord( a, b);
		}
	}
	for (; i<len; ++i) if (p[ i] != q[ i]) return i;
	return len;
}

} // namespace
#endif
