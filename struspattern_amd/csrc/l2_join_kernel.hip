// Result-set mode, the non-materialising rule automaton (l2_join.h): lane-parallel over the lexems of a document, no state.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "l2_join.h"
#include "l2_tables.h"
#include "l2_device.h"
#include "wave_scan.h"

using namespace spa;

namespace {
__shared__ u32 pairFilter[ JOIN_FILTER_WORDS];
__device__ __forceinline__ bool maybeKey( u32 first, u32 second)
{
	const u32 bit = (joinHash( first, second) >> 8) % (JOIN_FILTER_WORDS*32u);
	return (pairFilter[ bit >> 5] >> (bit & 31u)) & 1u;
}

// the matches that end at lexem j (lane-private loop over the lexems of the last maxRange positions); WRITE: store them
// from `out` on, else count
// records are word aligned only: multi-word stores through memcpy (one request per 16 / 12 bytes instead of one per word --
// the kernel is bound by the number of store requests of its lanes, not by their bytes)
__device__ __forceinline__ void st4( u32* p, u32 a, u32 b, u32 c, u32 d) { const u32 v[ 4] = {a, b, c, d}; __builtin_memcpy( p, v, 16); }
__device__ __forceinline__ void st3( u32* p, u32 a, u32 b, u32 c) { const u32 v[ 3] = {a, b, c}; __builtin_memcpy( p, v, 12); }
__device__ __forceinline__ void putItem( const JoinParams& P, u64 at, u32 variable, uint4 t, u32 st)
{
	u32* io = P.io.items + at*7;
	st4( io, variable, t.y, t.y + 1u, st); st3( io+4, t.z, st, t.z + t.w);
	if (P.io.withFormats) { P.io.itemFormat[ 2*at] = 0; P.io.itemFormat[ 2*at+1] = 0; }
}
// how many times the pair (i, j) matches for a rule of a moved key reference (JOIN_ALT_* in l2_join.h); the caller has checked
// ordpos(i) < ordpos(j) <= ordpos(i) + range and the delimiter between them.  Lane-private scans over the few lexems of the
// last 2 x range positions (range <= the optimizer's maxRange, 5 by default), read through the cache like the main look-back.
__device__ __forceinline__ u32 altMatches( const JoinParams& P, const uint4* lex, u32 i, u32 j, u32 a, u32 b, u32 pi, u32 pj, u32 range, u32 flags, bool taken)
{
	if (flags & JOIN_ALT_LINGER)
	{
		if (taken) return 0;
		for (u32 k=i; k-- > 0;)
		{
			const uint2 lk = make_uint2( lex[ k].x, lex[ k].y);
			if (lk.y + range < pi) break;
			if (lk.x == b) return 0;		// the instance at i replayed that b (or gave up on it) instead of waiting
		}
		return 1;
	}
	// the replay of the instance installed at j: i must be the latest a before j
	u32 m = 1, nb = 0;
	for (u32 k=i+1; k<j; ++k)
	{
		const u32 x = lex[ k].x;
		if (x == a) { m = 0; break; }
		if (x == b && lex[ k].y == pi) ++nb;		// (JOIN_ALT_SEQ: a b beside i that replayed i and waited for a later b)
	}
	if (!(flags & JOIN_ALT_SEQ) || taken) return m;
	m += nb;
	// instances of earlier bs without a replay (no a within range before them) that took i as their first a
	u32 lim = 0; bool prevA = false;
	for (u32 k=i; k-- > 0;)
	{
		const uint2 lk = make_uint2( lex[ k].x, lex[ k].y);
		if (lk.y + 2u*range < pj) break;
		if (lk.x == a) { lim = lk.y + range; prevA = true; break; }
	}
	for (u32 k=i; k-- > 0;)
	{
		const uint2 lk = make_uint2( lex[ k].x, lex[ k].y);
		if (lk.y + range < pj || (prevA && lk.y <= lim)) break;
		if ((flags & JOIN_STRUCT) && lk.x == P.delimiter) break;
		if (lk.x == b) ++m;
	}
	return m;
}

// `times` more matches of `ni` items each: the count stops at JOIN_COUNT_MAX + 1, so it cannot wrap whatever the rule set and
// the document hold (below that the items are at most twice the matches: they fit the high half); no branch per match
__device__ __forceinline__ void countMatches( u32& cnt, u32& icnt, u32 times, u32 ni)
{
	const u32 lim = (u32)JOIN_COUNT_MAX + 1u, t = times < lim ? times : lim;
	cnt = cnt + t < lim ? cnt + t : lim; icnt += ni*t;
}

// returns matches | items << 16 -- or, counting, JOIN_COUNT_OVERFLOW when the matches exceed JOIN_COUNT_MAX (the count
// saturates there: the low half never carries into the item half, and two items per match at most fit the high one).  The
// writing instantiation is entered only with a count the counting one has returned, so it stores exactly that many records.
template <bool WRITE>
__device__ __forceinline__ u32 matchesEndingAt( const JoinParams& P, const uint4* lex, const u32* seg, u32 j, uint4 lj, u32* out, u32* fmtOut, u64 itemAt)
{
	u32 cnt = 0, icnt = 0;
	const u32 e = lj.x;
	if (!e) return 0;
	// any( .., e, .. ): the lexem alone
	if (maybeKey( JOIN_SELF, e))
	{
		u32 slot = joinHash( JOIN_SELF, e) & P.keymask;
		for (u32 probes=0; probes<=P.keymask; ++probes)
		{
			const JoinKey k = P.keytab[ slot];
			if (!k.first) break;
			if (k.first == (u32)JOIN_SELF && k.second == e)
			{
				for (u32 r=0; r<k.count; ++r)
				{
					const JoinRule rule = P.rules[ k.begin + r];
					// (any( e, e ): both triggers of the instance take the lexem, the second field is the one that fired first)
					const u32 vj = P.io.withItems ? (rule.flags >> 16) & 0xFFu : 0u, vi = P.io.withItems ? (rule.flags >> 8) & 0xFFu : 0u;
					const u32 ni = (vj ? 1u : 0u) + (vi ? 1u : 0u);
					if (WRITE)
					{
						u32* o = out + 9*(u64)cnt;
						const u32 sj = seg ? seg[ j] : 0u;
						st4( o, rule.resultHandle, lj.y, lj.y + 1u, sj); st4( o+4, lj.z, sj, lj.z + lj.w, P.io.withItems ? (u32)(itemAt + icnt) : 0u); o[8] = ni;
						if (fmtOut) fmtOut[ cnt] = rule.formatHandle;
						if (vj) putItem( P, itemAt + icnt, vj, lj, sj);
						if (vi) putItem( P, itemAt + icnt + (vj ? 1u : 0u), vi, lj, sj);
					}
					countMatches( cnt, icnt, 1, ni);
				}
				break;
			}
			slot = (slot+1) & P.keymask;
		}
	}
	u32 takenPos = 0;		// position of the latest occurrence of e seen so far: it has taken every instance that began at an earlier position
	bool delimited = false;		// a delimiter lexem lies between i and j
	for (u32 i=j; i-- > 0;)
	{
		const uint4 li = lex[ i];
		if (lj.y - li.y > P.maxRange) break;		// every instance that old has expired
		const bool taken = takenPos > li.y;		// this one and all earlier ones were completed by that occurrence
		if (taken && !P.altRules) break;		// (the replays of moved key references are not)
		if (li.x && lj.y > li.y && maybeKey( li.x, e))
		{
			u32 slot = joinHash( li.x, e) & P.keymask;
			for (u32 probes=0; probes<=P.keymask; ++probes)
			{
				const JoinKey k = P.keytab[ slot];
				if (!k.first) break;
				if (k.first == li.x && k.second == e)
				{
					for (u32 r=0; r<k.count; ++r)
					{
						const JoinRule rule = P.rules[ k.begin + r];
						if (lj.y - li.y > rule.range || (delimited && (rule.flags & JOIN_STRUCT))) continue;
						u32 times = 1;
						if (rule.flags & JOIN_ALT) times = altMatches( P, lex, i, j, li.x, e, li.y, lj.y, rule.range, rule.flags, taken);
						else if (taken) continue;
						// captured items, latest first (as the reference lists them): the completing lexem's, then the first one's
						const u32 vi = P.io.withItems ? (rule.flags >> 8) & 0xFFu : 0u, vj = P.io.withItems ? (rule.flags >> 16) & 0xFFu : 0u;
						const u32 ni = (vi ? 1u : 0u) + (vj ? 1u : 0u);
						if (!WRITE) countMatches( cnt, icnt, times, ni);
						else for (u32 t=0; t<times; ++t)
						{
							u32* o = out + 9*(u64)cnt;
							const u32 si = seg ? seg[ i] : 0u, sj = seg ? seg[ j] : 0u;
							st4( o, rule.resultHandle, li.y, lj.y + 1u, si); st4( o+4, li.z, sj, lj.z + lj.w, P.io.withItems ? (u32)(itemAt + icnt) : 0u); o[8] = ni;
							if (fmtOut) fmtOut[ cnt] = rule.formatHandle;
							if (vj) putItem( P, itemAt + icnt, vj, lj, sj);
							if (vi) putItem( P, itemAt + icnt + (vj ? 1u : 0u), vi, li, si);
							++cnt; icnt += ni;
						}
					}
					break;
				}
				slot = (slot+1) & P.keymask;
			}
		}
		if (li.x == e && li.y > takenPos) takenPos = li.y;
		if (P.delimiter && li.x == P.delimiter) delimited = true;
	}
	if (!WRITE && cnt > (u32)JOIN_COUNT_MAX) return JOIN_COUNT_OVERFLOW;
	return cnt | (icnt << 16);
}

__device__ void joinDocuments( const JoinParams& P)
{
	for (u32 k=threadIdx.x; k<(u32)JOIN_FILTER_WORDS; k+=blockDim.x) pairFilter[ k] = P.filter[ k];
	__syncthreads();
	for (u32 round=0; round<=P.io.ndocs; ++round)
	{
		u32 doc = 0;
		if (LANE == 0) doc = atomicAdd( P.io.docCursor, 1u);
		doc = uni( doc);
		if (doc >= P.io.ndocs) break;
		// (docLexems of l2_device.h reads the range into scalar registers: 5 more SGPR spills here than this vector read)
		u64 beg, n64;
		if (P.io.docRangesIn) { beg = P.io.docRangesIn[ 2*(u64)doc]; n64 = P.io.docRangesIn[ 2*(u64)doc+1]; }
		else { beg = P.io.docOffsets[ doc]; n64 = P.io.docOffsets[ doc+1] - beg; }
		beg = ((u64)uni( (u32)(beg >> 32)) << 32) | uni( (u32)beg);
		const u32 n = uni( (u32)n64);
		const uint4* lex = (const uint4*)P.io.lexems + beg;
		const u32* seg = P.io.origseg ? P.io.origseg + beg : 0;
		u32 err = 0;
		if (n64 >= (1ull << 32)) err = SPD_ERR_RANGE;
		const bool stored = beg + n64 <= P.countsCapacity;
		// checks of putInput (patternMatcher.cpp:131-162), the matches counted
		u32 total = 0, itotal = 0;
		if (!err)
		{
			// the first offending lexem decides the status, as in a sequential feed: a descending position shows at the later
			// lexem and before that lexem's own range checks; the origpos / origsize checks sit in the else-if chain behind the
			// position compares, so they see only a lexem that stays on the current position (0 before the first lexem)
			u32 firstBad = ~0u, firstOrder = ~0u;		// (lane-private: the lexem index)
			bool wrapped = false;
			for (u32 base=0; base<n; base+=64)
			{
				const u32 j = base + LANE;
				u32 c = 0;
				if (j < n)
				{
					const uint4 lj = lex[ j];
					bool bad = lj.x >= (1u<<29);
					if ((lj.z >= 0x7FFFFFFFu || lj.w >= 0x7FFFFFFFu) && (j ? lex[ j-1].y : 0u) == lj.y) bad = true;
					if (j + 1 < n && lex[ j+1].y < lj.y && firstOrder == ~0u) firstOrder = j + 1;
					c = matchesEndingAt<false>( P, lex, seg, j, lj, 0, 0, 0);
					if (c == (u32)JOIN_COUNT_OVERFLOW) { bad = true; c = 0; }	// more than JOIN_COUNT_MAX matches end at this lexem
					if (bad && firstBad == ~0u) firstBad = j;
					if (stored) P.counts[ beg + j] = c;
				}
				const u32 incl = waveScanAdd( c & 0xFFFFu), iincl = waveScanAdd( c >> 16);
				// (a chunk adds at most 64 x 0x7FFF matches and twice as many items: a sum that wrapped is smaller than what was added)
				const u32 add = uni( (u32)__shfl( (int)incl, 63)), iadd = uni( (u32)__shfl( (int)iincl, 63));
				total += add; itotal += iadd;
				if (total < add || itotal < iadd) wrapped = true;
			}
			if (__ballot( (firstOrder & firstBad) != ~0u))
			{
				const u32 o = ~uni( (u32)__shfl( (int)waveScanMax( ~firstOrder), 63)), b = ~uni( (u32)__shfl( (int)waveScanMax( ~firstBad), 63));
				err = o <= b ? SPD_ERR_ORDER : SPD_ERR_RANGE;
			}
			else if (wrapped) err = SPD_ERR_RANGE;		// 2^32 results or items in one document: its sums are 32 bit
		}
		// both reservations are made even when the first one does not fit: the counters say what the whole batch needs
		u64 resBase = 0, itemBase = 0;
		if (!err && total)
		{
			bool fits = reserveOutput( P.io, SPC_RESULTS, total, resBase);
			if (itotal && !reserveOutput( P.io, SPC_ITEMS, itotal, itemBase)) fits = false;
			if (!fits) { err = SPD_ERR_OUTPUT; total = 0; }
		}
		if (!err && total)
		{
			u32 at = 0, iat = 0;
			for (u32 base=0; base<n; base+=64)
			{
				const u32 j = base + LANE;
				uint4 lj = make_uint4( 0, 0, 0, 0);
				u32 c = 0;
				if (j < n)
				{
					if (stored) { c = P.counts[ beg + j]; if (c) lj = lex[ j]; }
					else { lj = lex[ j]; c = matchesEndingAt<false>( P, lex, seg, j, lj, 0, 0, 0); }
				}
				const u32 cm = c & 0xFFFFu, ci = c >> 16;
				const u32 incl = waveScanAdd( cm), iincl = waveScanAdd( ci);
				if (cm)
				{
					const u64 mine = resBase + at + incl - cm;
					(void)matchesEndingAt<true>( P, lex, seg, j, lj, P.io.results + 9*mine, P.io.withFormats ? P.io.resultFormat + mine : 0, itemBase + iat + iincl - ci);
				}
				at += uni( (u32)__shfl( (int)incl, 63));
				iat += uni( (u32)__shfl( (int)iincl, 63));
			}
		}
		finishDocument( P.io, doc, resBase, err ? 0 : total, 0, 0, 0, 0, err, err ? 0 : n);
	}
}
} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l2_join_kernel( JoinParams P) { joinDocuments( P); }

namespace spa {
hipError_t launchL2Join( const JoinParams& P, unsigned nwaves, hipStream_t stream)
{
	hipLaunchKernelGGL( spa_l2_join_kernel, dim3( (nwaves + 3) / 4), dim3( 256), 0, stream, P);
	return hipGetLastError();
}
}
