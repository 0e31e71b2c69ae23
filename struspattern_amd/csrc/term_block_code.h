// The code of one position of a front-coded term block (include/strus_pattern_amd.h "term blocks"): one copy of the rule for the
// device-free twin (match_termblocks.cpp), the reader (sp_match_term_blocks_decode_block) and the device passes
// (l2_termblocks_kernel.hip).  No HIP header in here: SPA_TB_HD is empty for a host compiler.
//
// A code is five unsigned LEB128 varints -- hdelta, shared, suffix, doc_freq, count -- followed by the `suffix` bytes of the
// value behind the `shared` ones.  A varint is seven bits a byte, low bits first, the high bit set on every byte but the last,
// in minimal length: at most five bytes for 32 bits and ten for 64, so a header is at most 5+5+5+5+10 = 30 bytes.
// The sizing pass and the emitting pass of the device both go through termBlockEntry and termBlockCodeBytes: there is one
// statement of what a position costs.
#ifndef SPA_TERM_BLOCK_CODE_H
#define SPA_TERM_BLOCK_CODE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define SPA_TB_HD __host__ __device__ __forceinline__
#else
#define SPA_TB_HD inline
#endif

namespace spa {

enum { TERM_BLOCK_ENTRIES = 16 };		// positions a block by default (sp_matcher_term_block_entries)
enum { TERM_BLOCK_MAX_ENTRIES = 64 };		// ... and at most: a wave trip of the device covers whole blocks
enum { TERM_BLOCK_HEADER_MAX = 30 };
enum { TERM_BLOCK_VARINT_MAX = 10 };

// 1, 2, 4, 8, 16, 32 or 64
SPA_TB_HD bool termBlockEntriesValid( uint32_t n) { return n >= 1 && n <= TERM_BLOCK_MAX_ENTRIES && (n & (n - 1)) == 0; }

SPA_TB_HD uint32_t varintBytes( uint64_t v)
{
	uint32_t n = 1;
	for (; v >= 128; v >>= 7) ++n;
	return n;
}

// writes v to dst (varintBytes( v) bytes) and returns their number
SPA_TB_HD uint32_t writeVarint( uint8_t* dst, uint64_t v)
{
	uint32_t n = 0;
	for (; v >= 128; v >>= 7) dst[ n++] = (uint8_t)(v | 128);
	dst[ n++] = (uint8_t)v;
	return n;
}

// Reads the varint at src[ at..end) into v and moves `at` behind it.  False: it runs past `end`, is longer than ten bytes or
// does not fit 64 bits.
SPA_TB_HD bool readVarint( const uint8_t* src, uint64_t& at, uint64_t end, uint64_t& v)
{
	v = 0;
	for (uint32_t n=0; n<TERM_BLOCK_VARINT_MAX; ++n)
	{
		if (at >= end) return false;
		const uint8_t b = src[ at++];
		if (n == TERM_BLOCK_VARINT_MAX - 1 && b > 1) return false;
		v |= (uint64_t)(b & 127) << (7*n);
		if (!(b & 128)) return true;
	}
	return false;
}

// the five fields of a position
struct TermBlockEntry
{
	uint32_t hdelta;	// 0 at a head, otherwise the handle less the handle of the position before
	uint32_t shared;	// 0 at a head, otherwise the leading bytes shared with the value before: they are not stored
	uint32_t suffix;	// the bytes stored: value_bytes - shared
	uint32_t docFreq;
	uint64_t count;
};

// The fields of a position whose value has valueBytes bytes and shares prefixBytes of them with the one before.  (What no
// order of this library leaves: a prefix longer than the value is cut to it, a handle below the one before wraps in 32 bits.)
SPA_TB_HD TermBlockEntry termBlockEntry( bool head, uint32_t handle, uint32_t handleBefore, uint32_t prefixBytes, uint32_t valueBytes,
					  uint32_t docFreq, uint64_t count)
{
	TermBlockEntry e;
	e.hdelta = head ? 0u : handle - handleBefore;
	e.shared = head ? 0u : (prefixBytes < valueBytes ? prefixBytes : valueBytes);
	e.suffix = valueBytes - e.shared;
	e.docFreq = docFreq;
	e.count = count;
	return e;
}

SPA_TB_HD uint32_t termBlockHeaderBytes( const TermBlockEntry& e)
{
	return varintBytes( e.hdelta) + varintBytes( e.shared) + varintBytes( e.suffix) + varintBytes( e.docFreq) + varintBytes( e.count);
}

// the bytes of the whole code: header and suffix
SPA_TB_HD uint64_t termBlockCodeBytes( const TermBlockEntry& e) { return (uint64_t)termBlockHeaderBytes( e) + e.suffix; }

// writes the header to dst (room for TERM_BLOCK_HEADER_MAX bytes) and returns termBlockHeaderBytes( e)
SPA_TB_HD uint32_t writeTermBlockHeader( uint8_t* dst, const TermBlockEntry& e)
{
	uint32_t n = writeVarint( dst, e.hdelta);
	n += writeVarint( dst + n, e.shared);
	n += writeVarint( dst + n, e.suffix);
	n += writeVarint( dst + n, e.docFreq);
	n += writeVarint( dst + n, e.count);
	return n;
}

} // namespace
#endif
