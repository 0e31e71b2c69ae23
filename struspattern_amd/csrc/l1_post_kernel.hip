// Post-processing kernel of the lexer (stages 1b-4 of l1_wave.h): the queued reports of a document through the handler
// (l1_handler.h) -- one queue with the literals found here, two queues merged, or a cluster of reports per lane -- and out.
#include "l1_handler.h"
#include "l1_launch.h"

namespace {

// The literals of one 64-byte tile, all lanes at once.  Lane l holds byte tile+l: the runs of word characters of
// the tile come out of one ballot, their hashes out of one segmented scan (polynomial hash, l1_tables.h), and every
// lane where a run has just ended looks its word up in the literal table by itself.  A run that crosses the tile
// boundary is carried (hash, length and start so far).
struct LitCarry { bool in; u32 hash, len, start; };
__device__ __forceinline__ void tileLiterals(  const LexWave& w, const L1Params& P, u32 tile, u32 mine, bool isW, LitCarry& c,
						u64& endMask, u32& litFrom, u32& litBegin, u32& litCount, u32& litPi0, u32& litId0, u32& litLb0)
{
	const u64 wm = __ballot( isW);
	const u64 prevW = (wm << 1) | (c.in ? 1ull : 0ull);
	const u64 startM = wm & ~prevW;
	endMask = ~wm & prevW;				// bit e: the run that ended just before byte tile+e
	const u64 sb = startM & (((1ull << LANE) - 1ull) | (1ull << LANE));
	const int ss = sb ? 63 - (int)__builtin_clzll( sb) : -1;	// start of my run inside the tile (-1: it began in an earlier tile)
	u32 H = isW ? mine + 1u : 0u, M = (u32)L1_LITHASH_MUL;
#pragma unroll
	for (int d=1; d<64; d<<=1)
	{
		const u32 Hs = (u32)__shfl_up( (int)H, d), Ms = (u32)__shfl_up( (int)M, d);
		const bool take = isW && (int)LANE >= d && (int)LANE - d >= ss;
		if (take) { H = Hs * M + H; M = Ms * M; }
	}
	const bool carried = isW && ss < 0;
	const u32 Htot = carried ? c.hash * M + H : H;		// (M = MUL^(lane+1) for a carried run)
	u32 runLen = isW ? (carried ? c.len + LANE + 1u : LANE - (u32)ss + 1u) : 0u;
	if (runLen > 65u) runLen = 65u;
	const u32 from = carried ? c.start : tile + (u32)(ss < 0 ? 0 : ss);
	// the run that ended before me = the values of the lane before me
	u32 pH = (u32)__shfl_up( (int)Htot, 1), pLen = (u32)__shfl_up( (int)runLen, 1), pFrom = (u32)__shfl_up( (int)from, 1);
	if (LANE == 0) { pH = c.hash; pLen = c.len; pFrom = c.start; }
	litFrom = pFrom; litBegin = 0; litCount = 0; litPi0 = 0; litId0 = 0; litLb0 = 0;
	if (((endMask >> LANE) & 1ull) && pLen >= 1u && pLen <= 64u)
	{
		const u32 h = literalHashFinish( pH);
		u32 slot = h & P.literalMask;
		// the word's first 16 bytes, read once beside the first probe (the table entry carries its own first 16)
		uint4 dw = make_uint4( 0, 0, 0, 0);
		if (pFrom + 16u <= w.docLen) dw = ld128u( w.doc + pFrom);
		else
		{
			u32 d[ 4] = {0,0,0,0};
			for (u32 q=0; q<16u && pFrom+q<w.docLen; ++q) d[ q>>2] |= (u32)w.doc[ pFrom + q] << (8*(q&3u));
			dw = make_uint4( d[0], d[1], d[2], d[3]);
		}
		const u32 m0 = pLen >= 4u ? 0xFFFFFFFFu : ((1u << (8*pLen)) - 1u);
		const u32 m1 = pLen >= 8u ? 0xFFFFFFFFu : (pLen > 4u ? ((1u << (8*(pLen-4u))) - 1u) : 0u);
		const u32 m2 = pLen >= 12u ? 0xFFFFFFFFu : (pLen > 8u ? ((1u << (8*(pLen-8u))) - 1u) : 0u);
		const u32 m3 = pLen >= 16u ? 0xFFFFFFFFu : (pLen > 12u ? ((1u << (8*(pLen-12u))) - 1u) : 0u);
		for (u32 probes=0; probes<=P.literalMask; ++probes)
		{
			const uint4* ep = (const uint4*)&P.literals[ slot];
			const uint4 e0 = ep[ 0], e1 = ep[ 1], tx = ep[ 2];	// {hash, len, patBegin, patCount} {pat0, id0, levelBind0, textOffset} {text}
			if (!e0.x) break;
			if (e0.x == h && e0.y == pLen)
			{
				bool same = (((dw.x ^ tx.x) & m0) | ((dw.y ^ tx.y) & m1) | ((dw.z ^ tx.z) & m2) | ((dw.w ^ tx.w) & m3)) == 0;
				for (u32 k=16; k<pLen && same; k+=4)		// (a word beyond 16 bytes: the rest from the text pool)
				{
					const u32 rem = pLen - k;
					u32 a;
					if (pFrom + k + 4u <= w.docLen) a = ld32u( w.doc + pFrom + k);
					else
					{
						a = 0;
						for (u32 q=0; q<rem && q<4u; ++q) a |= (u32)w.doc[ pFrom + k + q] << (8*q);
					}
					const u32 b = ld32u( P.literalText + e1.w + k);
					const u32 mask = rem >= 4u ? 0xFFFFFFFFu : ((1u << (8*rem)) - 1u);
					same = ((a ^ b) & mask) == 0;
				}
				if (same)
				{
					litBegin = e0.z; litCount = e0.w; litPi0 = e1.x; litId0 = e1.y; litLb0 = e1.z;
					break;
				}
			}
			slot = (slot+1) & P.literalMask;
		}
	}
	// carry the run that reaches the end of the tile
	c.in = (wm >> 63) & 1ull;
	if (c.in)
	{
		c.hash = uni( (u32)__shfl( (int)Htot, 63)); c.len = uni( (u32)__shfl( (int)runLen, 63)); c.start = uni( (u32)__shfl( (int)from, 63));
	}
}

// the reports of a chunked document lie in one slice of the report queue per chunk: on to the next slice that holds any
__device__ __forceinline__ void sliceOf( LexWave& w, const L1Params& P)
{
	w.queue = P.reportQueue + 4*(((w.docBegin + (u64)(w.unit - w.unit0) * P.chunkBytes) * P.queueMul >> 4) + 64ull*w.unit);
	w.nQueue = ldu( &P.reportCount[ w.unit]);
}
__device__ __forceinline__ bool nextSlice( LexWave& w, const L1Params& P)
{
	while (w.unit + 1u < w.unitEnd)
	{
		++w.unit;
		sliceOf( w, P);
		if (w.nQueue) return true;
	}
	return false;
}

// ---------------------------------------------------------------- stages 1b-3: literals, start of match, handler
// The document's raw reports (scan kernel) and its literal reports (found here, tile by tile) go through the
// reference's handler in the order the reference's callback sees them: ascending end offset, ascending pattern
// index inside one end offset.
template <bool LDS, bool CP, bool CH>
__device__ void postDocument( LexWave& w, const L1Params& P, const LexTab<LDS>& T)
{
	const u32 len = w.docLen;
	u32 ctxReg = 0, clsReg = 0;		// byte -> context, class: lane l keeps the entries of bytes 4l..4l+3
	for (u32 k=0; k<4; ++k) { const u32 c = P.byteClass[ 4*LANE + k]; clsReg |= c << (8*k); ctxReg |= (u32)P.classCtx[ c] << (8*k); }
	u64 wcarry = 0;
	LitCarry carry; carry.in = false; carry.hash = 0; carry.len = 0; carry.start = 0;
	u32 nq = w.nQueue;
	u32 qi = 0, qb = 0, qn = 0;		// next report; the batch [qb, qb+qn) is resolved in lr
	LaneReport lr;
	lr.to = 0; lr.from = 0; lr.id = 0; lr.levelBind = 0; lr.prefixLen = 0; lr.suffixLen = 0; lr.pi = 0; lr.def = 0; lr.skip = 0;
	if (nq) nextBatch<LDS,CP>( w.queue, w.doc, w.docLen, P, T, nq, 0, qn, lr);
	u32 ahead = (LANE < len) ? w.doc[ LANE] : 0u;		// the next tile's bytes are loaded one tile ahead
	for (u32 tile=0; tile<=len && !w.err; tile+=64)
	{
		const u32 mine = ahead;
		ahead = (tile + 64 + LANE < len) ? w.doc[ tile + 64 + LANE] : 0u;
		const u32 inTile = (len - tile) < 64 ? (len - tile) : 64;
		u64 litEnds = 0; u32 litFrom = 0, litBegin = 0, litCount = 0, litPi0 = 0, litId0 = 0, litLb0 = 0;
		if (P.nofLiterals)
		{
			u32 ctxL;
			if (CP && P.ucp) ctxL = tileClassCtx<true>( P, w.doc, len, tile, mine, clsReg, ctxReg, wcarry) >> 8;
			else { const u32 shm = (mine & 3u)*8; ctxL = ((u32)__builtin_amdgcn_ds_bpermute( (int)((mine >> 2) << 2), (int)ctxReg) >> shm) & 0xFFu; }
			const u64 tLit = PROF_T();
			tileLiterals( w, P, tile, mine, LANE < inTile && ctxL == (u32)CTX_WORD, carry, litEnds, litFrom, litBegin, litCount, litPi0, litId0, litLb0);
			PROF_ACC( 1, tLit);
			litEnds &= __ballot( litCount != 0);
		}
		// every report that ends inside this tile: end offsets tile .. tile+63 (a full tile) or .. len (the last one).
		// Two sorted streams -- the automaton's reports (lanes of lr) and the tile's literals (lanes of lit*, one
		// pattern after the other where a literal defines several) -- merged by (end offset, pattern index).
		const u32 lastTo = (tile + 64 > len) ? len : tile + 63u;
		const u64 NOKEY = ~0ull;
		u32 kL = 64, pb = 0, pc = 0, lj = 0, lfrom = 0, lid = 0, llb = 0;
		u64 keyL = NOKEY;
		auto literalAt = [&]()			// the first literal end of litEnds becomes the current literal
		{
			keyL = NOKEY;
			if (!litEnds) return;
			kL = (u32)__builtin_ctzll( litEnds);
			pb = (u32)__builtin_amdgcn_readlane( litBegin, kL); pc = (u32)__builtin_amdgcn_readlane( litCount, kL);
			lfrom = (u32)__builtin_amdgcn_readlane( litFrom, kL);
			lid = (u32)__builtin_amdgcn_readlane( litId0, kL); llb = (u32)__builtin_amdgcn_readlane( litLb0, kL);
			lj = 0;
			keyL = ((u64)(tile + kL) << 32) | (u32)__builtin_amdgcn_readlane( litPi0, kL);
		};
		literalAt();
		while (!w.err)
		{
			const u32 x = qi - qb;
			u64 keyA = NOKEY;
			if (qi < nq) keyA = ((u64)(u32)__builtin_amdgcn_readlane( lr.to, x) << 32) | (u32)__builtin_amdgcn_readlane( lr.pi, x);
			const bool lit = keyL < keyA;
			const u64 key = lit ? keyL : keyA;
			const u32 toNext = (u32)(key >> 32);
			if (toNext > lastTo) break;		// (also when both streams are at their end)
			const u32 hid = lit ? lid : (u32)__builtin_amdgcn_readlane( lr.id, x);
			const u32 hlb = lit ? llb : (u32)__builtin_amdgcn_readlane( lr.levelBind, x);
			const u32 hpre = lit ? 0u : (u32)__builtin_amdgcn_readlane( lr.prefixLen, x);
			const u32 hsuf = lit ? 0u : (u32)__builtin_amdgcn_readlane( lr.suffixLen, x);
			const u32 hfrom = lit ? lfrom : (u32)__builtin_amdgcn_readlane( lr.from, x);
			const u64 tH = PROF_T();
			if (lit || !__builtin_amdgcn_readlane( lr.skip, x)) handleReport( w, P, hid, hlb, hpre, hsuf, hfrom, toNext);
			PROF_ACC( 3, tH);
			if (lit)
			{
				++lj;
				if (lj < pc)
				{
					const u32 lpi = ldu( &P.litPats[ pb + lj]);
					const DevLexPattern* pat = &P.patterns[ lpi];
					lid = ldu( &pat->id); llb = ldu( &pat->levelBind);
					keyL = ((u64)toNext << 32) | lpi;
				}
				else { litEnds &= litEnds - 1; literalAt(); }
			}
			else
			{
				++qi;
				if (qi == qb + qn && qi < nq)
				{
					qb = qi;
					const u64 tR = PROF_T();
					nextBatch<LDS,CP>( w.queue, w.doc, w.docLen, P, T, nq, qb, qn, lr);
					PROF_ACC( 2, tR);
				}
				else if (CH && qi == nq && nextSlice( w, P))
				{
					// (a chunked document: the reports of its next chunk)
					nq = w.nQueue; qi = 0; qb = 0;
					nextBatch<LDS,CP>( w.queue, w.doc, w.docLen, P, T, nq, qb, qn, lr);
				}
			}
		}
	}
	if (!w.err && qi != nq) w.err = L1D_ERR_INTERNAL;
}

// ---------------------------------------------------------------- stages 2-3 with the words kernel: two queues, merged
// The automaton's reports (scan kernel) and the word reports (words kernel) of a document, both in (end offset, pattern) order,
// go through the reference's handler in the order the reference's callback sees them.  Each queue is read 64 records at a time
// (the automaton's get their leftmost starts on the way, nextBatch); a chunked document has one slice per chunk in either queue.
struct ReportStream
{
	const u32* queue; u32 nq, qi, qb, qn, unit;
	LaneReport lr;
};
template <bool LDS, bool CP, bool CH, bool WORDS>
__device__ __forceinline__ void streamSlice( ReportStream& s, const LexWave& w, const L1Params& P)
{
	const u64 qbase = ((w.docBegin + (u64)(s.unit - w.unit0) * P.chunkBytes) * P.queueMul >> 4) + 64ull*s.unit;
	s.queue = (WORDS ? P.wordQueue : P.reportQueue) + 4*qbase;
	s.nq = ldu( WORDS ? &P.wordCount[ s.unit] : &P.reportCount[ s.unit]);
	s.qi = 0; s.qb = 0; s.qn = 0;
}
template <bool LDS, bool CP, bool CH, bool WORDS>
__device__ __forceinline__ void streamFill( ReportStream& s, const LexWave& w, const L1Params& P, const LexTab<LDS>& T)
{
	// the next batch of the current slice, or of the next slice that holds any
	while (s.qi == s.nq)
	{
		if (!CH || s.unit + 1u >= w.unitEnd) return;
		++s.unit;
		streamSlice<LDS,CP,CH,WORDS>( s, w, P);
	}
	s.qb = s.qi;
	if (WORDS)
	{
		s.qn = (s.nq - s.qb) < 64u ? (s.nq - s.qb) : 64u;
		resolveStarts<LDS,CP>( s.queue, w.doc, w.docLen, P, T, s.qb, s.qn, s.lr);
	}
	else nextBatch<LDS,CP>( s.queue, w.doc, w.docLen, P, T, s.nq, s.qb, s.qn, s.lr);
}
template <bool LDS, bool CP, bool CH>
__device__ void postDocumentMerged( LexWave& w, const L1Params& P, const LexTab<LDS>& T)
{
	ReportStream A, B;
	A.unit = w.unit0; B.unit = w.unit0;
	A.lr.to = 0; A.lr.from = 0; A.lr.id = 0; A.lr.levelBind = 0; A.lr.prefixLen = 0; A.lr.suffixLen = 0; A.lr.pi = 0; A.lr.def = 0; A.lr.skip = 0;
	B.lr = A.lr;
	streamSlice<LDS,CP,CH,false>( A, w, P); streamFill<LDS,CP,CH,false>( A, w, P, T);
	streamSlice<LDS,CP,CH,true>( B, w, P); streamFill<LDS,CP,CH,true>( B, w, P, T);
	const u64 NOKEY = ~0ull;
	while (!w.err)
	{
		const u32 xa = A.qi - A.qb, xb = B.qi - B.qb;
		u64 keyA = NOKEY, keyB = NOKEY;
		if (A.qi < A.nq) keyA = ((u64)(u32)__builtin_amdgcn_readlane( A.lr.to, xa) << 32) | (u32)__builtin_amdgcn_readlane( A.lr.pi, xa);
		if (B.qi < B.nq) keyB = ((u64)(u32)__builtin_amdgcn_readlane( B.lr.to, xb) << 32) | (u32)__builtin_amdgcn_readlane( B.lr.pi, xb);
		if (keyA == NOKEY && keyB == NOKEY) break;
		if (keyB < keyA)
		{
			if (!__builtin_amdgcn_readlane( B.lr.skip, xb))
			{
				handleReport( w, P, (u32)__builtin_amdgcn_readlane( B.lr.id, xb), (u32)__builtin_amdgcn_readlane( B.lr.levelBind, xb),
					(u32)__builtin_amdgcn_readlane( B.lr.prefixLen, xb), (u32)__builtin_amdgcn_readlane( B.lr.suffixLen, xb),
					(u32)__builtin_amdgcn_readlane( B.lr.from, xb), (u32)(keyB >> 32));
			}
			++B.qi;
			if (B.qi == B.qb + B.qn || B.qi == B.nq) streamFill<LDS,CP,CH,true>( B, w, P, T);
		}
		else
		{
			if (!__builtin_amdgcn_readlane( A.lr.skip, xa))
			{
				handleReport( w, P, (u32)__builtin_amdgcn_readlane( A.lr.id, xa), (u32)__builtin_amdgcn_readlane( A.lr.levelBind, xa),
					(u32)__builtin_amdgcn_readlane( A.lr.prefixLen, xa), (u32)__builtin_amdgcn_readlane( A.lr.suffixLen, xa),
					(u32)__builtin_amdgcn_readlane( A.lr.from, xa), (u32)(keyA >> 32));
			}
			++A.qi;
			if (A.qi == A.qb + A.qn || A.qi == A.nq) streamFill<LDS,CP,CH,false>( A, w, P, T);
		}
	}
}

// ---------------------------------------------------------------- stage 3, a cluster of reports per lane (round 3)
// The reference's handler (patternLexer.cpp:727-822) looks at its event array from the back only: the delete pass stops at the first event
// that starts left of the new match, the ignore pass at the first that ends left of its end, the insertion at the first that does not
// start right of it.  Take the reports in callback order r0 r1 ... and say there is a BOUNDARY before ri when every report from ri on
// starts right of every earlier report's start and ends right of every earlier report's end: then none of the three scans of a report
// behind the boundary ever gets past the events the reports behind the boundary have left -- the handler works on the events of its own
// CLUSTER (the reports between two boundaries) as if the array began there, and what a cluster leaves is appended to the array as it is.
// A window of 64 merged reports has its boundaries found with two prefix maxima and two suffix minima; every complete cluster of the
// window is then run through the handler by ONE LANE on a little event array of its own in LDS, all clusters at once, and the survivors
// are appended to the wave's event array with one prefix sum.  What the lanes cannot take goes through handleReport one report after
// the other, as before: the reports in front of the window's first boundary (they may reach into the array), a cluster that leaves more
// than LOC_CAP events or holds a symbol lookup, a cluster as long as the window.  The last cluster of a window waits for the next one
// unless the input has ended (its last reports may still be to come).
#ifndef SPA_L1_POST_LOC_CAP
#define SPA_L1_POST_LOC_CAP 6
#endif
enum {WIN_CAP=192, LOC_CAP=SPA_L1_POST_LOC_CAP, REC_SYMBOL=1u<<16, REC_SIZEERR=1u<<31};

__device__ __forceinline__ u32 waveSuffixMin( u32 v)		// inclusive, identity ~0
{
	u32 t;
	t = (u32)__builtin_amdgcn_update_dpp( -1, (int)v, 0x101, 0xF, 0xF, false); v = t < v ? t : v;	// row_shl:1
	t = (u32)__builtin_amdgcn_update_dpp( -1, (int)v, 0x102, 0xF, 0xF, false); v = t < v ? t : v;
	t = (u32)__builtin_amdgcn_update_dpp( -1, (int)v, 0x104, 0xF, 0xF, false); v = t < v ? t : v;
	t = (u32)__builtin_amdgcn_update_dpp( -1, (int)v, 0x108, 0xF, 0xF, false); v = t < v ? t : v;
	const u32 m1 = (u32)__builtin_amdgcn_readlane( v, 16), m2 = (u32)__builtin_amdgcn_readlane( v, 32), m3 = (u32)__builtin_amdgcn_readlane( v, 48);
	const u32 s2 = m2 < m3 ? m2 : m3, s1 = m1 < s2 ? m1 : s2;
	const u32 behind = LANE < 16u ? s1 : (LANE < 32u ? s2 : (LANE < 48u ? m3 : ~0u));
	return behind < v ? behind : v;
}

// the record of a resolved report as the handler takes it: {end, start, lexem id, level|posbind<<8|flags}, sub expression selection
// applied (patternLexer.cpp:731-741); false: the report is dropped
__device__ __forceinline__ bool preparedRecord( const LaneReport& lr, uint4& rec)
{
	u32 from = lr.from, to = lr.to;
	u32 fl = lr.levelBind & 0x1FFFFu;
	if (to - from >= 65535u) fl |= (u32)REC_SIZEERR;						// :727-730, raised when the handler gets there
	bool live = !lr.skip;
	if (lr.levelBind & (1u<<17))
	{
		if (lr.prefixLen + lr.suffixLen > to - from) live = (fl & (u32)REC_SIZEERR) != 0;
		else { from += lr.prefixLen; to -= lr.suffixLen; }
	}
	rec = make_uint4( to, from, lr.id, fl);
	return live;
}

// ranks of the live records of two sorted batches in their merge (keys are distinct: a pattern reports through one of the queues only)
__device__ __forceinline__ void mergeRanks( u64 liveX, u32 xHi, u32 xLo, u32& rankX, bool isLiveY, u32 yHi, u32 yLo, u32& rankY)
{
	const u64 keyY = ((u64)yHi << 32) | yLo;
	while (liveX)
	{
		const u32 x = (u32)__builtin_ctzll( liveX);
		liveX &= liveX - 1;
		const u64 kx = ((u64)(u32)__builtin_amdgcn_readlane( xHi, x) << 32) | (u32)__builtin_amdgcn_readlane( xLo, x);
		const bool less = isLiveY && keyY < kx;
		const u32 c = (u32)__builtin_popcountll( __ballot( less));
		if (LANE == x) rankX += c;
		if (isLiveY && !less) ++rankY;
	}
}

template <bool LDS, bool CP, bool CH>
__device__ void postDocumentClusters( LexWave& w, const L1Params& P, const LexTab<LDS>& T)
{
	__shared__ uint4 postWin[ 4][ WIN_CAP];
	__shared__ uint4 postLoc[ 4][ LOC_CAP*64];
	uint4* win = postWin[ (threadIdx.x >> 6) & 3u];
	uint4* loc = postLoc[ (threadIdx.x >> 6) & 3u] + LANE;		// event j of this lane's cluster: loc[ 64*j]
	ReportStream A, B;
	A.unit = w.unit0; B.unit = w.unit0;
	A.lr.to = 0; A.lr.from = 0; A.lr.id = 0; A.lr.levelBind = 0; A.lr.prefixLen = 0; A.lr.suffixLen = 0; A.lr.pi = 0; A.lr.def = 0; A.lr.skip = 0;
	B.lr = A.lr;
	streamSlice<LDS,CP,CH,false>( A, w, P); streamFill<LDS,CP,CH,false>( A, w, P, T);
	streamSlice<LDS,CP,CH,true>( B, w, P); streamFill<LDS,CP,CH,true>( B, w, P, T);
	u32 wi = 0, wn = 0;			// the window: win[ wi .. wn)
	u32 carryF = 0, carryT = 0;		// 1 + the greatest start / end of the reports handled so far (0: none)
	bool exhausted = false;
	const u64 NOKEY = ~0ull;
	auto sequential = [&]( const uint4& rec, u32 s, u32 e)
	{
		if (w.cnt == 0 && w.nEvents) { __builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront"); reloadLanes( w); readTail( w); }
		for (u32 x=s; x<e && !w.err; ++x)
		{
			const u32 fl = (u32)__builtin_amdgcn_readlane( rec.w, x);
			if (fl & (u32)REC_SIZEERR) { w.err = L1D_ERR_LEXEMSIZE; break; }
			handleReport( w, P, (u32)__builtin_amdgcn_readlane( rec.z, x), fl & 0x1FFFFu, 0, 0, (u32)__builtin_amdgcn_readlane( rec.y, x), (u32)__builtin_amdgcn_readlane( rec.x, x));
		}
	};
	while (!w.err)
	{
		// ---- refill: what is left of the window moves to its front, the next records of the two queues are merged in behind it
		while (wn - wi < 64u && !exhausted)
		{
			const bool haveA = A.qi < A.nq, haveB = B.qi < B.nq;
			if (!haveA && !haveB) { exhausted = true; break; }
			const u32 left = wn - wi;
			uint4 keep = make_uint4( 0, 0, 0, 0);
			if (LANE < left) keep = win[ wi + LANE];
			const u32 xa = A.qi - A.qb, xb = B.qi - B.qb;
			// nothing behind a batch's last key is known yet: records up to the smaller of the two last keys are taken
			u64 limit = NOKEY;
			if (haveA && (A.qb + A.qn < A.nq || (CH && A.unit + 1u < w.unitEnd)))
				limit = ((u64)(u32)__builtin_amdgcn_readlane( A.lr.to, A.qn-1) << 32) | (u32)__builtin_amdgcn_readlane( A.lr.pi, A.qn-1);
			if (haveB && (B.qb + B.qn < B.nq || (CH && B.unit + 1u < w.unitEnd)))
			{
				const u64 lb = ((u64)(u32)__builtin_amdgcn_readlane( B.lr.to, B.qn-1) << 32) | (u32)__builtin_amdgcn_readlane( B.lr.pi, B.qn-1);
				if (lb < limit) limit = lb;
			}
			const bool takeA = haveA && LANE >= xa && LANE < A.qn && ((((u64)A.lr.to << 32) | A.lr.pi) <= limit);
			const bool takeB = haveB && LANE >= xb && LANE < B.qn && ((((u64)B.lr.to << 32) | B.lr.pi) <= limit);
			uint4 recA, recB;
			const bool liveA = preparedRecord( A.lr, recA) && takeA, liveB = preparedRecord( B.lr, recB) && takeB;
			const u64 liveAm = __ballot( liveA), liveBm = __ballot( liveB);
			u32 rankA = (u32)__builtin_amdgcn_mbcnt_hi( (u32)(liveAm >> 32), __builtin_amdgcn_mbcnt_lo( (u32)liveAm, 0));
			u32 rankB = (u32)__builtin_amdgcn_mbcnt_hi( (u32)(liveBm >> 32), __builtin_amdgcn_mbcnt_lo( (u32)liveBm, 0));
			if (liveAm && liveBm)
			{
				if (__builtin_popcountll( liveAm) <= __builtin_popcountll( liveBm)) mergeRanks( liveAm, A.lr.to, A.lr.pi, rankA, liveB, B.lr.to, B.lr.pi, rankB);
				else mergeRanks( liveBm, B.lr.to, B.lr.pi, rankB, liveA, A.lr.to, A.lr.pi, rankA);
			}
			__builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront");
			if (LANE < left) win[ LANE] = keep;
			if (liveA) win[ left + rankA] = recA;
			if (liveB) win[ left + rankB] = recB;
			__builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront");
			wi = 0; wn = left + (u32)__builtin_popcountll( liveAm) + (u32)__builtin_popcountll( liveBm);
			const u32 tookA = (u32)__builtin_popcountll( __ballot( takeA)), tookB = (u32)__builtin_popcountll( __ballot( takeB));
			if (tookA) { A.qi += tookA; if (A.qi == A.qb + A.qn || A.qi == A.nq) streamFill<LDS,CP,CH,false>( A, w, P, T); }
			if (tookB) { B.qi += tookB; if (B.qi == B.qb + B.qn || B.qi == B.nq) streamFill<LDS,CP,CH,true>( B, w, P, T); }
			if (!tookA && !tookB) { w.err = L1D_ERR_INTERNAL; break; }
		}
		if (w.err) break;
		const u32 avail = (wn - wi) < 64u ? (wn - wi) : 64u;
		if (!avail) break;
		const bool valid = LANE < avail;
		uint4 rec = make_uint4( 0, 0, 0, 0);
		if (valid) rec = win[ wi + LANE];
		// ---- boundaries
		const u32 inclF = waveScanMax( valid ? rec.y + 1u : 0u), inclT = waveScanMax( valid ? rec.x + 1u : 0u);
		u32 exclF = laneFromBelow( inclF), exclT = laneFromBelow( inclT);
		exclF = exclF > carryF ? exclF : carryF; exclT = exclT > carryT ? exclT : carryT;
		const u32 sufF = waveSuffixMin( valid ? rec.y + 1u : ~0u), sufT = waveSuffixMin( valid ? rec.x + 1u : ~0u);
		const u64 bounds = __ballot( valid && sufF > exclF && sufT > exclT);
		const u32 first = bounds ? (u32)__builtin_ctzll( bounds) : 64u;
		auto carryTo = [&]( u32 upTo)		// the reports [0, upTo) of the view are done
		{
			if (!upTo) return;
			const u32 f = (u32)__builtin_amdgcn_readlane( inclF, upTo-1), t = (u32)__builtin_amdgcn_readlane( inclT, upTo-1);
			carryF = f > carryF ? f : carryF; carryT = t > carryT ? t : carryT;
		};
		if (first)
		{
			// the reports in front of the first boundary may reach into the array
			const u32 e = first < avail ? first : avail;
			sequential( rec, 0, e);
			carryTo( e); wi += e;
			continue;
		}
		const bool final = exhausted && avail == wn - wi;
		const u32 lastB = 63u - (u32)__builtin_clzll( bounds);
		const u32 procEnd = final ? avail : lastB;
		if (procEnd == 0)
		{
			// one cluster as long as the view
			sequential( rec, 0, avail);
			carryTo( avail); wi += avail;
			continue;
		}
		// ---- every complete cluster through the handler, one lane each
		const bool head = ((bounds >> LANE) & 1ull) != 0 && LANE < procEnd;
		u32 len = 0;
		{
			const u64 above = (bounds >> LANE) >> 1;
			const u32 nextB = above ? LANE + 1u + (u32)__builtin_ctzll( above) : 64u;
			len = (nextB < procEnd ? nextB : procEnd) - LANE;
		}
		u32 n = 0;
		bool hard = false;
		for (u32 k=0; __ballot( head && !hard && k < len) != 0; ++k)
		{
			if (head && !hard && k < len)
			{
				const uint4 r = win[ wi + LANE + k];
				if (r.w & ((u32)REC_SYMBOL | (u32)REC_SIZEERR)) hard = true;
				else
				{
					const u32 level = r.w & 0xFFu, from = r.y, lastPos = r.x;
					u32 nofDeletes = 0;
					// delete pass (:757-777)
					for (u32 q=n; q>0; --q)
					{
						const uint4 m = loc[ 64*(q-1)];
						if (!(m.y >= from)) break;
						const u32 mlevel = m.w & 0xFFu;
						if ((r.z == m.x && m.y == from && mlevel == level) || (mlevel < level && m.y + m.z <= lastPos))
						{
							for (u32 t=q-1; t+1<n; ++t) loc[ 64*t] = loc[ 64*(t+1)];
							--n; ++nofDeletes;
						}
					}
					bool ignored = false;
					if (!nofDeletes)
					{
						// ignore pass (:778-792)
						for (u32 q=n; q>0; --q)
						{
							const uint4 m = loc[ 64*(q-1)];
							if (!(m.y + m.z >= lastPos)) break;
							if ((m.w & 0xFFu) > level && m.y <= from) { ignored = true; break; }
						}
					}
					if (!ignored)
					{
						if (n == (u32)LOC_CAP) hard = true;
						else
						{
							// insert (:793-822)
							u32 at = n;
							for (; at>0; --at)
							{
								const uint4 m = loc[ 64*(at-1)];
								if (!(m.y > from)) break;
								loc[ 64*at] = m;
							}
							loc[ 64*at] = make_uint4( r.z, from, lastPos - from, r.w & 0xFFFFu);
							++n;
						}
					}
				}
			}
		}
		const u64 hardm = __ballot( head && hard);
		const u32 firstHard = hardm ? (u32)__builtin_ctzll( hardm) : 64u;
		// ---- what the clusters in front of the first one that has to go the slow way have left is appended
		const bool mine = head && LANE < firstHard;
		const u32 cnt = mine ? n : 0u;
		const u32 incl = waveScanAdd( cnt);
		const u32 total = (u32)__builtin_amdgcn_readlane( incl, 63);
		if (w.nEvents + total + 2u > P.eventCap)
		{
			if (LANE == 0) atomicAdd( (unsigned long long*)&P.counters[ L1C_OVER_EVENTS], 1ull);
			w.err = L1D_ERR_ARENA; break;
		}
		if (total)
		{
			if (w.cnt) spillLanes( w, 0);
			uint4* dst = (uint4*)w.events + w.nEvents + (incl - cnt);
			for (u32 j=0; j<(u32)LOC_CAP; ++j)
			{
				if (j < cnt) dst[ j] = loc[ 64*j];
			}
			w.nEvents += total;
		}
		if (firstHard < 64u)
		{
			const u32 hlen = (u32)__builtin_amdgcn_readlane( len, firstHard);
			if (total) __builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront");
			carryTo( firstHard);
			sequential( rec, firstHard, firstHard + hlen);
			carryTo( firstHard + hlen); wi += firstHard + hlen;
		}
		else { carryTo( procEnd); wi += procEnd; }
	}
	if (!w.err && (A.qi != A.nq || B.qi != B.nq)) w.err = L1D_ERR_INTERNAL;
}

// POST: literals, start of match, handler, ordinal positions, lexems
template <bool LDS, bool CP, bool CH>
__device__ void postDocuments( const L1Params& P)
{
	// (the same three sets of instances as the scan kernel's)
	const u32 chunked = ldu( (const u32*)&P.counters[ L1C_CHUNKED]);
	if (CP != (P.cpBlocks != 0 || P.nofNullable != 0) || (!CP && CH != (chunked != 0))) return;
	LexTab<LDS> T;
	stageTables( P, T);
	const u32 waveSlot = uni( blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
	LexWave w;
	w.events = (Event*)(P.arenaBase + (u64)waveSlot * P.arenaWords);
#ifdef SPA_PROF
	for (int k=0; k<4; ++k) w.prof[ k] = 0;
#endif
	for (u32 round=0; round<=P.ndocs; ++round)
	{
		// every document comes from the device-side cursor (a workgroup that only becomes resident when others have
		// finished finds it exhausted and leaves at once: no document waits for a particular wave)
		u32 doc = 0;
		if (LANE == 0) doc = atomicAdd( (u32*)&P.counters[ L1C_CURSOR2], 1u);
		doc = uni( doc);
		if (doc >= P.ndocs) break;
		u64 beg, end;
		docBounds( P, doc, beg, end);
		w.doc = P.text + beg; w.docLen = (u32)(end - beg);
		if (ldu( (const u32*)&P.docStatus[ doc]) != 0)
		{
			// failed in the scan kernel
			if (LANE == 0)
			{
				P.docRange[ 2*(u64)doc] = 0; P.docRange[ 2*(u64)doc+1] = 0;
				atomicAdd( (unsigned long long*)&P.counters[ L1C_BYTES], (unsigned long long)w.docLen);
				atomicAdd( (unsigned long long*)&P.counters[ L1C_FAILED], 1ull);
			}
			continue;
		}
		w.docBegin = beg;
		w.unit0 = chunked ? ldu( &P.unitStart[ doc]) : doc;
		w.unitEnd = chunked ? ldu( &P.unitStart[ doc+1]) : doc + 1u;
		w.unit = w.unit0;
		w.nEvents = 0; w.err = 0; w.cnt = 0; w.tailPos = 0; w.tailEnd = 0;
		w.e.id = 0; w.e.pos = 0; w.e.size = 0; w.e.lb = 0;
		const u64 tDoc = PROF_T();
		if (!CP && P.wordsKernel && P.postClusters) postDocumentClusters<LDS,CP,CH>( w, P, T);
		else if (!CP && P.wordsKernel) postDocumentMerged<LDS,CP,CH>( w, P, T);
		else
		{
			sliceOf( w, P);
			if (CH && !w.nQueue) (void)nextSlice( w, P);
			w.queueCap = w.nQueue;
			postDocument<LDS,CP,CH>( w, P, T);
		}
		spillLanes( w, 0);
		__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront");
		if (!w.err) emitLexems( w, P, doc);
		else if (LANE == 0) { P.docRange[ 2*(u64)doc] = 0; P.docRange[ 2*(u64)doc+1] = 0; }
		PROF_ACC( 0, tDoc);
		if (LANE == 0)
		{
			P.docStatus[ doc] = (int32_t)w.err;
			atomicAdd( (unsigned long long*)&P.counters[ L1C_BYTES], (unsigned long long)w.docLen);
			if (w.err) atomicAdd( (unsigned long long*)&P.counters[ L1C_FAILED], 1ull);
		}
	}
#ifdef SPA_PROF
	if (LANE == 0) for (int k=0; k<4; ++k) atomicAdd( (unsigned long long*)&P.counters[ 4+k], (unsigned long long)w.prof[ k]);
#endif
}

} // anonymous namespace

enum {POST_WAVES=4};
// The post-processing kernel is bound by the latency of its dependent chains, not by issue slots: it gains from
// more resident waves as long as the register budget does not spill much.  Measured on 12288 x 64 KiB documents
// (tests/micro/sweep_l1_post.py): 100 registers / 16 waves per CU 72 ms, 96 / 20: 65 ms, 80 / 24: 59.4 ms,
// 72 / 28: 58.9 ms, 64 / 32: 100 ms (60 spills).
#ifndef SPA_L1_POST_WAVES_PER_EU
#define SPA_L1_POST_WAVES_PER_EU 6
#endif
#define SPA_L1_POST_OCC __attribute__((amdgpu_waves_per_eu( SPA_L1_POST_WAVES_PER_EU, SPA_L1_POST_WAVES_PER_EU)))
// (the two instances with the cluster-per-lane handler hold 9 KB of LDS per wave: 16 waves per CU)
#ifndef SPA_L1_POST_CLUSTER_WAVES_PER_EU
#define SPA_L1_POST_CLUSTER_WAVES_PER_EU 4
#endif
#define SPA_L1_POST_OCC4 __attribute__((amdgpu_waves_per_eu( SPA_L1_POST_CLUSTER_WAVES_PER_EU, SPA_L1_POST_CLUSTER_WAVES_PER_EU)))
extern "C" __global__ __launch_bounds__(64*POST_WAVES) SPA_L1_POST_OCC4 void spa_l1_post_kernel( L1Params P) { postDocuments<false,false,false>( P); }
extern "C" __global__ __launch_bounds__(64*POST_WAVES) SPA_L1_POST_OCC4 void spa_l1_post_kernel_ch( L1Params P) { postDocuments<false,false,true>( P); }
extern "C" __global__ __launch_bounds__(64*POST_WAVES) SPA_L1_POST_OCC void spa_l1_post_kernel_cp( L1Params P) { postDocuments<false,true,true>( P); }

namespace spa {
static_assert( (int)POST_WAVES == (int)L1_POST_WAVES, "workgroup size of the post-processing kernel");

hipError_t launchL1Post( const L1LaunchPlan& plan, const L1Params& P, hipStream_t stream)
{
	// its own number of waves (one event array each), in workgroups of POST_WAVES
	if (plan.cp) hipLaunchKernelGGL( spa_l1_post_kernel_cp, dim3( plan.postGrid()), dim3( 64*POST_WAVES), 0, stream, P);
	else
	{
		hipLaunchKernelGGL( spa_l1_post_kernel, dim3( plan.postGrid()), dim3( 64*POST_WAVES), 0, stream, P);
		hipLaunchKernelGGL( spa_l1_post_kernel_ch, dim3( plan.postGrid()), dim3( 64*POST_WAVES), 0, stream, P);
	}
	return hipGetLastError();
}
} // namespace
