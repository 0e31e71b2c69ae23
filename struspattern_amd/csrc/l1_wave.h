// Level-1 pattern lexer on gfx950: one wavefront per document, one 64-bit automaton word per lane.
// This header: what every kernel family of the lexer uses -- the wave's state, the table image, class and context of a
// byte, the queue slices and the bounds of a document.  Device code only; included by the l1_*_kernel.hip files
// (stages 2-4: l1_handler.h; the launch sequence: l1_launch.cpp).
//
// What it replaces (reference, CPU): hs_scan (Intel Hyperscan, src/patternLexer.cpp:875-879), the
// per-match callback PatternLexerContext::match_event_handler (:717-826) and the ordinal-position
// pass of PatternLexerContext::match (:893-945).
//
// Two kernels per batch (round 2; one fused kernel before): the SCAN kernel runs stage 1 and leaves the raw
// reports of a document in its slice of a report queue in HBM (16 B per report, ~3 B per text byte); the
// POST kernel runs stages 1b-4 on them.  Fused, the two halves shared one register allocation: 106 scalar
// registers of the byte loop were spilled and every step reloaded kernel arguments.
// Stages per document:
//  1. SCAN   bit-parallel position automaton (tables: l1_tables.h).  Lane l owns word l of every
//            pass; the document byte is wave-uniform, the table row of its byte class is one
//            coalesced 512-byte read; a report is detected with one __ballot per pass and byte.
//            Reports are appended to a queue in (end offset, pattern index) order = the order in
//            which the reference's handler is called.
//  1b. LITERALS  \bWORD\b patterns are no automaton bits: per 64-byte tile the runs of word characters come out
//            of one ballot, their hashes out of one segmented scan, and every lane where a run has ended probes
//            the literal table by itself; the literal reports are merged with the automaton's by (end offset,
//            pattern index).
//  2. SOM    start of match: one lane per queued report runs the pattern's automaton BACKWARDS from
//            the end offset (predecessor sets from the same shift/self/exception tables) and keeps
//            the smallest offset at which a start position is live = leftmost start.
//  3. HANDLER the reference's supersede / ignore / sorted-insert logic, executed in report order on
//            the wave's event array (wave-uniform control flow, scalarised loads).
//  4. ORDPOS ordinal positions and the output records, once per document.
// Integer/byte work, HBM-streaming input: no MFMA.
#ifndef SPA_L1_WAVE_H
#define SPA_L1_WAVE_H
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>
#include "l1_tables.h"
#include "l1_device.h"
#include "wave_scan.h"

using namespace spa;

namespace {

#ifdef SPA_PROF
#define PROF_T() __builtin_amdgcn_s_memtime()
#define PROF_ACC( SLOT, T0) do { w.prof[ SLOT] += __builtin_amdgcn_s_memtime() - (T0); } while (0)
#else
#define PROF_T() 0ull
#define PROF_ACC( SLOT, T0) do { (void)(T0); } while (0)
#endif

enum {L1D_OK=0, L1D_ERR_ARENA=2, L1D_ERR_LEXEMSIZE=7, L1D_ERR_INTERNAL=8, L1D_ERR_OUTPUT=9,
      L1D_CHUNK_UNPROVEN=100};	// (internal: the document goes to the sequential re-scan)

struct Event { u32 id, origpos, origsize, levelBind; };	// levelBind = level | posbind<<8   (MatchEvent, patternLexer.cpp:665-679)

// hot tables: one image [charMask][acceptMask][startMask][shiftDst][selfLoop][exSrc][exDst], read either
// from the workgroup's LDS copy (ds_read, LDS=true) or from global memory (LDS=false)
extern __shared__ u64 ldsImage[];
template <bool LDS>
struct LexTab
{
	const u64* g;		// global image
	u32 oChar, oAccept, oStart, oShift, oSelf, oExSrc, oExDst;	// (offsets may be biased, modulo 2^32, by the passes an image leaves out: the words kernel's)
	__device__ __forceinline__ u64 at( u32 off) const { if (LDS) return ldsImage[ off]; else return g[ off]; }
};

struct EventLanes { u32 id, pos, size, lb; };	// one event per lane

struct LexWave
{
	u32* queue;		// raw reports: 4 words {to, pattern, accLo, accHi}; after SOM word 2 holds `from`
	Event* events;
	u32 nQueue, nEvents, err, queueCap;
	EventLanes e; u32 cnt;	// the cnt most recent events, lane L holds event nEvents-1-L
	u32 tailPos, tailEnd;	// start and end of the last event (lane 0), valid while cnt > 0
	u32 unit0, unit, unitEnd; u64 docBegin;	// post-processing of a chunked document: the unit whose reports are being read, one behind its last unit
	const unsigned char* doc;
	u32 docLen;
#ifdef SPA_PROF
	u64 prof[4];
#endif
};

// class by code point of the well-formed multi-byte character that begins at `at` (L1Params::cpBlocks), 0xFF = none:
// the byte is classed as a byte then
__device__ __forceinline__ u32 cpClassAt( const L1Params& P, const unsigned char* doc, u32 len, u32 at)
{
	const u32 c = doc[ at];
	const u32 want = (c >= 0xC2u && c <= 0xDFu) ? 2u : (c >= 0xE0u && c <= 0xEFu) ? 3u : (c >= 0xF0u && c <= 0xF4u) ? 4u : 1u;
	if (want == 1u || at + want > len) return 0xFFu;
	u32 v = c & (0xFFu >> (want+1u));
	for (u32 i=1; i<want; ++i)
	{
		const u32 x = doc[ at+i];
		if ((x & 0xC0u) != 0x80u) return 0xFFu;
		v = (v << 6) | (x & 0x3Fu);
	}
	if (want == 2u ? v < 0x80u : want == 3u ? v < 0x800u : (v < 0x10000u || v > 0x10FFFFu)) return 0xFFu;		// overlong / out of range
	return P.cpPages[ (u32)P.cpBlocks[ v >> 6]*64u + (v & 63u)];
}

// class and context of the byte at `pos`: the lead byte of a well-formed character by its code point when the tables
// have such classes; with UCP a continuation byte by whether its character is a word character (twin classes 256..319)
__device__ __forceinline__ void classCtxAt( const L1Params& P, const unsigned char* doc, u32 len, long pos, u32& cls, int& ctx)
{
	if (pos < 0 || pos >= (long)len) { cls = 0; ctx = CTX_EDGE; return; }
	const u32 b = doc[ pos];
	cls = P.byteClass[ b]; ctx = P.classCtx[ cls];
	if (!P.cpBlocks || b < 0x80u) return;
	if (b >= 0xC2u)
	{
		const u32 c = cpClassAt( P, doc, len, (u32)pos);
		if (c != 0xFFu) { cls = c; ctx = P.classCtx[ c]; }
		return;
	}
	if (!P.ucp || b > 0xBFu) return;
	for (long d=1; d<=3 && pos-d >= 0; ++d)
	{
		const u32 l = doc[ pos-d];
		if (l >= 0xC2u && l <= 0xF4u)
		{
			const u32 want = l <= 0xDFu ? 2u : l <= 0xEFu ? 3u : 4u;
			if (want > (u32)d)
			{
				const u32 c = cpClassAt( P, doc, len, (u32)(pos-d));
				if (c != 0xFFu && P.classCtx[ c] == (u32)CTX_WORD) { cls = P.byteClass[ 256u + (b - 0x80u)]; ctx = CTX_WORD; }
			}
			return;
		}
		if ((l & 0xC0u) != 0x80u) return;
	}
}
template <bool CP>
__device__ __forceinline__ int ctxAt( const L1Params& P, const unsigned char* doc, u32 len, long pos)
{
	if (pos < 0 || pos >= (long)len) return CTX_EDGE;
	if (CP && P.ucp) { u32 cls; int ctx; classCtxAt( P, doc, len, pos, cls, ctx); return ctx; }
	return P.classCtx[ P.byteClass[ doc[ pos]]];
}
// UCP: which of the bytes q, q+1, q+2 are continuation bytes of a word character that begins before q (the carry a scan
// starting at q takes over from the tile before)
__device__ __forceinline__ u64 wordCarryAt( const L1Params& P, const unsigned char* doc, u32 len, u32 q)
{
	u64 carry = 0;
	for (u32 d=0; d<3u && q+d<len; ++d)
	{
		const u32 pos = q + d;
		if ((doc[ pos] & 0xC0u) != 0x80u) break;
		for (u32 back=1; back<=3u && back<=pos; ++back)
		{
			const u32 l = doc[ pos-back];
			if (l >= 0xC2u && l <= 0xF4u)
			{
				const u32 want = l <= 0xDFu ? 2u : l <= 0xEFu ? 3u : 4u;
				if (pos-back < q && want > back)
				{
					const u32 c = cpClassAt( P, doc, len, pos-back);
					if (c != 0xFFu && P.classCtx[ c] == (u32)CTX_WORD) carry |= 1ull << d;
				}
				break;
			}
			if ((l & 0xC0u) != 0x80u) break;
		}
	}
	return carry;
}
// class | context << 8 of the byte of my lane in the 64-byte tile at `tile` (`mine`), from the in-register byte tables and
// -- in the kernel instances for tables with classes by code point (CP) -- from the decoded character; wcarry: continuation
// bytes at the start of the next tile that belong to a word character of this one (UCP)
template <bool CP>
__device__ __forceinline__ u32 tileClassCtx( const L1Params& P, const unsigned char* doc, u32 len, u32 tile, u32 mine, u32 clsReg, u32 ctxReg, u64& wcarry)
{
	const u32 shm = (mine & 3u)*8;
	const u32 clsL = ((u32)__builtin_amdgcn_ds_bpermute( (int)((mine >> 2) << 2), (int)clsReg) >> shm) & 0xFFu;
	const u32 ctxL = ((u32)__builtin_amdgcn_ds_bpermute( (int)((mine >> 2) << 2), (int)ctxReg) >> shm) & 0xFFu;
	u32 ccv = clsL | (ctxL << 8);
	if (CP && P.cpBlocks)
	{
		u32 n = 0; bool word = false;
		if (mine >= 0xC2u && mine <= 0xF4u && tile + LANE < len)
		{
			const u32 c = cpClassAt( P, doc, len, tile + LANE);
			if (c != 0xFFu)
			{
				u32 ctx = ctxL;
				if (P.ucp) { ctx = P.classCtx[ c]; word = ctx == (u32)CTX_WORD; n = mine <= 0xDFu ? 2u : mine <= 0xEFu ? 3u : 4u; }
				ccv = c | (ctx << 8);
			}
		}
		if (P.ucp)
		{
			const u64 m2 = __ballot( word && n >= 2u), m3 = __ballot( word && n >= 3u), m4 = __ballot( word && n >= 4u);
			const u64 covered = (m2 << 1) | (m3 << 2) | (m4 << 3) | wcarry;
			wcarry = (m2 >> 63) | (m3 >> 62) | (m4 >> 61);
			if (((covered >> LANE) & 1ull) && mine >= 0x80u && mine <= 0xBFu && tile + LANE < len)
			{
				ccv = (u32)P.byteClass[ 256u + (mine - 0x80u)] | ((u32)CTX_WORD << 8);
			}
		}
	}
	return ccv;
}

// the leftmost start of the matches of one pattern (p0 = {id, word, levelBind, prefixLen}, mask = its bits) that end at `to`, R = the
// positions that consumed byte to-1 and accept there; `to` itself when there is none (a candidate that does not confirm).
// (stage 2's backward walk: here because the words kernel confirms its candidates with it too)
template <bool LDS, bool CP>
__device__ __forceinline__ u32 leftmostStart( const unsigned char* doc, u32 docLen, const L1Params& P, const LexTab<LDS>& T, u32 word, u64 mask, u32 to, u64 R)
{
	const u32 pass = word >> 6, ln = word & 63u;
	const u64 shiftDst = T.at( T.oShift + pass*64 + ln), selfLoop = T.at( T.oSelf + pass*64 + ln);
	const u32 nEx = P.exCount[ pass];
	u32 from = to;
	long j = (long)to;			// R = positions that consumed byte j-1
	while (R && j > 0)
	{
		int prevctx = ctxAt<CP>( P, doc, docLen, j-2);
		if (R & T.at( T.oStart + (pass*CTX_COUNT + prevctx)*64 + ln)) from = (u32)(j-1);
		if (j-1 == 0) break;
		u64 Rp = ((R & shiftDst) >> 1) | (R & selfLoop);
		for (u32 e=0; e<nEx; ++e)
		{
			const u32 at = (pass*P.maxExceptions + e)*64 + ln;
			const u64 es = T.at( T.oExSrc + at), ed = T.at( T.oExDst + at);
			Rp |= (R & ed) ? es : 0ull;
		}
		u32 cls = P.byteClass[ doc[ j-2]];
		if (CP && P.cpBlocks && doc[ j-2] >= 0x80u) { int cx; classCtxAt( P, doc, docLen, j-2, cls, cx); }
		R = Rp & mask & T.at( T.oChar + (pass*P.nofClasses + cls)*64 + ln);
		--j;
	}
	return from;
}

__device__ __forceinline__ u32 ld32u( const unsigned char* p) { u32 v; __builtin_memcpy( &v, p, 4); return v; }
__device__ __forceinline__ uint4 ld128u( const unsigned char* p) { uint4 v; __builtin_memcpy( &v, p, 16); return v; }

// the 16-byte records of scan unit `unit`, whose text begins at byte `bytePos` of the batch, start here in either queue
__device__ __forceinline__ u64 queueBase( const L1Params& P, u64 bytePos, u32 unit) { return ((bytePos * P.queueMul) >> 4) + 64ull*unit; }

__device__ __forceinline__ void docBounds( const L1Params& P, u32 doc, u64& beg, u64& end)
{
	beg = ((u64)ldu( (const u32*)&P.docOffsets[ doc]+1) << 32) | ldu( (const u32*)&P.docOffsets[ doc]);
	end = ((u64)ldu( (const u32*)&P.docOffsets[ doc+1]+1) << 32) | ldu( (const u32*)&P.docOffsets[ doc+1]);
}

template <bool LDS>
__device__ __forceinline__ void stageTables( const L1Params& P, LexTab<LDS>& T)
{
	T.g = P.tableImage; T.oChar = P.ldsChar; T.oAccept = P.ldsAccept; T.oStart = P.ldsStart; T.oShift = P.ldsShift; T.oSelf = P.ldsSelf;
	T.oExSrc = P.ldsExSrc; T.oExDst = P.ldsExDst;
	if (LDS)
	{
		// the workgroup stages the hot tables once
		for (u32 k=threadIdx.x; k<P.ldsWords; k+=blockDim.x) ldsImage[ k] = P.tableImage[ k];
		__syncthreads();
	}
}

} // anonymous namespace
#endif
