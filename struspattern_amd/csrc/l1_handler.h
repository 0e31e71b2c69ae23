// Stages 2-4 of the lexer (l1_wave.h): the leftmost start of a batch of queued reports, the reference's handler on the wave's
// event array, ordinal positions and output.  Device code only; included by the kernels that produce lexems
// (l1_post_kernel.hip, l1_approx_kernel.hip), never by the scan kernels.
#ifndef SPA_L1_HANDLER_H
#define SPA_L1_HANDLER_H
#include "l1_wave.h"

namespace {

// ---------------------------------------------------------------- stage 2: leftmost start per report
// lane-parallel: lane i resolves report base+i
struct LaneReport { u32 to, from, id, levelBind, prefixLen, suffixLen, pi, def, skip; };	// one queued report per lane, pattern attributes attached

template <bool LDS, bool CP>
__device__ __forceinline__ void resolveStarts( const u32* queue, const unsigned char* doc, u32 docLen, const L1Params& P, const LexTab<LDS>& T, u32 base, u32 count, LaneReport& out)
{
	u32 i = base + LANE;
	out.to = 0; out.from = 0; out.id = 0; out.levelBind = 0; out.prefixLen = 0; out.suffixLen = 0; out.pi = 0; out.def = 0; out.skip = 0;
	if (LANE < count)
	{
		const uint4 q = *(const uint4*)(queue + 4*(u64)i);	// {to, pattern, accLo|from, accHi}
		u32 to = q.x, pi = q.y & ~(u32)(L1_LITERAL_FLAG | L1_DEAD_FLAG);
		const uint4 p0 = *(const uint4*)&P.patterns[ pi], p1 = *((const uint4*)&P.patterns[ pi] + 1);	// {id,word,levelBind,prefixLen} {suffixLen,maskLo,maskHi,-}
		out.to = to; out.id = p0.x; out.levelBind = p0.z; out.prefixLen = p0.w; out.suffixLen = p1.x; out.pi = pi; out.def = p1.w;
		if (q.y & L1_DEAD_FLAG) out.skip = 1;				// (words kernel: a candidate that did not confirm)
		if (q.y & L1_LITERAL_FLAG) { out.from = q.z; return; }		// whole-word literal / word shape: start already known
		out.from = leftmostStart<LDS,CP>( doc, docLen, P, T, p0.y, ((u64)p1.z << 32) | p1.y, to, ((u64)q.w << 32) | q.z);
	}
}

// The next batch of up to 64 reports with their starts.  An expression cut into several patterns entries reports
// once per entry: the reports of one expression and one end offset are adjacent; the last of them takes the
// leftmost start of the group, the others are marked to be skipped, and a group is never cut by a batch boundary.
template <bool LDS, bool CP>
__device__ __forceinline__ void nextBatch( const u32* queue, const unsigned char* doc, u32 docLen, const L1Params& P, const LexTab<LDS>& T, u32 nq, u32 qb, u32& qn, LaneReport& lr)
{
	qn = (nq - qb) < 64u ? (nq - qb) : 64u;
	resolveStarts<LDS,CP>( queue, doc, docLen, P, T, qb, qn, lr);
	if (!P.splitPatterns) return;
	if (qb + qn < nq)
	{
		const u32 nto = ldu( queue + 4*(u64)(qb+qn)), npi = ldu( queue + 4*(u64)(qb+qn) + 1) & ~(u32)L1_LITERAL_FLAG;
		const u32 ndef = ldu( &P.patterns[ npi].defIndex);
		const u32 lastTo = (u32)__builtin_amdgcn_readlane( lr.to, qn-1), lastDef = (u32)__builtin_amdgcn_readlane( lr.def, qn-1);
		if (nto == lastTo && ndef == lastDef)
		{
			const u32 g = (u32)__builtin_popcountll( __ballot( LANE < qn && lr.to == lastTo && lr.def == lastDef));
			if (g < qn) qn -= g;
		}
	}
	for (u32 d=1; d<64; d<<=1)
	{
		const u32 pf = (u32)__shfl_up( (int)lr.from, d), pt = (u32)__shfl_up( (int)lr.to, d), pd = (u32)__shfl_up( (int)lr.def, d);
		if (LANE >= d && LANE < qn && pt == lr.to && pd == lr.def && pf < lr.from) lr.from = pf;
	}
	const u32 nt = (u32)__shfl_down( (int)lr.to, 1), nd = (u32)__shfl_down( (int)lr.def, 1);
	lr.skip = (LANE + 1u < qn && nt == lr.to && nd == lr.def) ? 1u : 0u;
}

// ---------------------------------------------------------------- stage 3: the reference's handler
__device__ __forceinline__ void ldEvent( Event& e, const Event* p)
{
	e.id = ldu( &p->id); e.origpos = ldu( &p->origpos); e.origsize = ldu( &p->origsize); e.levelBind = ldu( &p->levelBind);
}
__device__ __forceinline__ void stEvent( Event* p, const Event& e)
{
	p->id = e.id; p->origpos = e.origpos; p->origsize = e.origsize; p->levelBind = e.levelBind;
}

// symbol lookup (PatternTable::symbolId, patternLexer.cpp:312-317): exact text of the match
__device__ u32 lookupSymbol( const unsigned char* doc, const L1Params& P, u32 lexemId, u32 from, u32 len)
{
	u32 h = 2166136261u;
	for (u32 b=0; b<4; ++b) h = symbolHashStep( h, (lexemId >> (8*b)) & 0xFFu);
	for (u32 k=0; k<len; ++k) h = symbolHashStep( h, uni( doc[ from+k]));
	if (!h) h = 1;
	u32 slot = h & P.symbolMask;
	for (u32 probes=0; probes<=P.symbolMask; ++probes)
	{
		const DevSymbol* s = &P.symbols[ slot];
		u32 sh = ldu( &s->hash);
		if (!sh) return 0;
		if (sh == h && ldu( &s->lexemId) == lexemId && ldu( &s->len) == len)
		{
			u32 off = ldu( &s->textOffset);
			bool same = true;
			for (u32 k=0; k<len && same; ++k) same = (uni( P.symbolText[ off+k]) == uni( doc[ from+k]));
			if (same) return ldu( &s->symbolId);
		}
		slot = (slot+1) & P.symbolMask;
	}
	return 0;
}

// The reference's handler (patternLexer.cpp:727-822) edits its event array near the tail almost always.  The wave
// keeps the most recent events in registers, one per lane: lane L holds event nEvents-1-L (L < cnt), the older
// ones (indices < nEvents-cnt) are in the wave's arena in global memory.  The three scans of the handler (delete
// pass, ignore pass, insertion point) become ballots over the lanes, element moves become wave shifts.  A scan
// that would run past the registers into the arena is rare; it goes through handleReportArena on the whole array
// in global memory, a literal restatement of the reference's loops.
__device__ __forceinline__ u32 laneFromAbove( u32 v) { return (u32)__builtin_amdgcn_update_dpp( 0, (int)v, 0x130, 0xF, 0xF, false); }	// wave_shl:1, lane i <- lane i+1
__device__ __forceinline__ u32 laneFromBelow( u32 v) { return (u32)__builtin_amdgcn_update_dpp( 0, (int)v, 0x138, 0xF, 0xF, false); }	// wave_shr:1, lane i <- lane i-1
__device__ __forceinline__ u64 lowMask( u32 n) { return n ? (~0ull >> (64u - n)) : 0ull; }		// n <= 64

// stage 0: the whole handler; stage 1: insertion only (the delete pass has already removed something)
// returns the new number of events
__device__ __noinline__ u32 handleReportArena( Event* events, u32 n, u32 stage, u32 id, u32 patternid, u32 levelBind, u32 from, u32 to)
{
	struct { Event* events; Event tail; bool tailValid; } w;
	w.events = events; w.tailValid = false;
	const u32 level = levelBind & 0xFFu;
	const bool twin = (patternid != id);
	Event ev; ev.id = id; ev.origpos = from; ev.origsize = to-from; ev.levelBind = levelBind;
	if (n && !w.tailValid) { ldEvent( w.tail, &w.events[ n-1]); w.tailValid = true; }
	if (n == 0)
	{
		stEvent( &w.events[0], ev); n = 1;
		if (twin) { Event t = ev; t.id = patternid; stEvent( &w.events[1], t); n = 2; }
		return n;
	}
	const u32 n0 = n;
	const u32 lastPos = from + (to-from);
	u32 nofDeletes = 0;
	if (stage == 0)
	{
		// delete pass (:757-777): from the back while origpos >= the new origpos
		for (u32 k=n; k>0; --k)
		{
			Event m;
			if (k == n0 && w.tailValid) m = w.tail; else ldEvent( m, &w.events[ k-1]);
			if (!(m.origpos >= ev.origpos)) break;
			u32 mlevel = m.levelBind & 0xFFu;
			if ((ev.id == m.id && m.origpos == ev.origpos && mlevel == level)
			||  (mlevel < level && m.origpos + m.origsize <= lastPos))
			{
				// close the gap: lanes move the tail down by one (ascending order, distinct elements)
				for (u32 t=k-1+LANE; t+1<n; t+=64)
				{
					Event x = w.events[ t+1];
					__builtin_amdgcn_wave_barrier();
					w.events[ t] = x;
				}
				--n; ++nofDeletes;
				w.tailValid = false;
			}
		}
		if (!nofDeletes)
		{
			// ignore pass (:778-792)
			for (u32 k=n; k>0; --k)
			{
				Event m;
				if (k == n0 && w.tailValid) m = w.tail; else ldEvent( m, &w.events[ k-1]);
				if (!(m.origpos + m.origsize >= lastPos)) break;
				if ((m.levelBind & 0xFFu) > level && m.origpos <= ev.origpos) return n;
			}
		}
	}
	// insert (:793-822), literal element moves of the reference (see oracle/l1_oracle.cpp for the
	// two-slot quirk of the symbol twin variant)
	const u32 newSlots = twin ? 2u : 1u;
	Event zero; zero.id = 0; zero.origpos = 0; zero.origsize = 0; zero.levelBind = 0;
	for (u32 s=0; s<newSlots; ++s) stEvent( &w.events[ n+s], zero);
	long prev = (long)n + (long)newSlots - 1, mi = (long)n - 1;
	for (; mi >= 0; prev = mi--)
	{
		Event m; ldEvent( m, &w.events[ mi]);
		if (!(m.origpos > ev.origpos)) break;
		stEvent( &w.events[ prev], m);
	}
	++mi;
	stEvent( &w.events[ mi], ev);
	if (twin) { Event t = ev; t.id = patternid; stEvent( &w.events[ mi+1], t); }
	return n + newSlots;
}

// the lanes [keep, cnt) go to the arena
__device__ __forceinline__ void spillLanes( LexWave& w, u32 keep)
{
	if (LANE >= keep && LANE < w.cnt) *(uint4*)&w.events[ w.nEvents - 1u - LANE] = make_uint4( w.e.id, w.e.pos, w.e.size, w.e.lb);
	w.cnt = keep < w.cnt ? keep : w.cnt;
}
__device__ __forceinline__ void reloadLanes( LexWave& w)
{
	enum {RELOAD=32};
	w.cnt = w.nEvents < (u32)RELOAD ? w.nEvents : (u32)RELOAD;
	uint4 x = make_uint4( 0, 0, 0, 0);
	if (LANE < w.cnt) x = *(const uint4*)&w.events[ w.nEvents - 1u - LANE];
	w.e.id = x.x; w.e.pos = x.y; w.e.size = x.z; w.e.lb = x.w;
}
__device__ __forceinline__ void pushEvent( LexWave& w, u32 at, u32 id, u32 pos, u32 size, u32 lb)
{
	// lanes above `at` take their lower neighbour's event, lane `at` the new one
	const u32 a = laneFromBelow( w.e.id), b = laneFromBelow( w.e.pos), c = laneFromBelow( w.e.size), d = laneFromBelow( w.e.lb);
	const bool up = LANE > at, here = LANE == at;
	w.e.id = up ? a : (here ? id : w.e.id);
	w.e.pos = up ? b : (here ? pos : w.e.pos);
	w.e.size = up ? c : (here ? size : w.e.size);
	w.e.lb = up ? d : (here ? lb : w.e.lb);
	++w.cnt; ++w.nEvents;
	if (at == 0) { w.tailPos = pos; w.tailEnd = pos + size; }
}
__device__ __forceinline__ void readTail( LexWave& w)
{
	w.tailPos = (u32)__builtin_amdgcn_readlane( w.e.pos, 0); w.tailEnd = w.tailPos + (u32)__builtin_amdgcn_readlane( w.e.size, 0);
}

__device__ __forceinline__ void handleReport( LexWave& w, const L1Params& P, u32 id, u32 lb, u32 pre, u32 suf, u32 from, u32 to)
{
	if (to - from >= 65535u) { w.err = L1D_ERR_LEXEMSIZE; return; }			// :727-730
	if (lb & (1u<<17))										// sub expression selection
	{
		if (pre + suf > to - from) return;
		from += pre; to -= suf;
	}
	u32 patternid = id;
	if (lb & (1u<<16))
	{
		const u32 sym = uni( lookupSymbol( w.doc, P, id, from, to-from));	// (a call's result counts as lane-varying unless told otherwise)
		if (sym) patternid = sym;
	}
	const u32 levelBind = lb & 0xFFFFu, level = lb & 0xFFu;
	const bool twin = (patternid != id);
	if (w.nEvents + 2 > P.eventCap)
	{
		// (which of the two working sets was too small is counted apart: the host grows only that one)
		if (LANE == 0) atomicAdd( (unsigned long long*)&P.counters[ L1C_OVER_EVENTS], 1ull);
		w.err = L1D_ERR_ARENA; return;
	}
	if (w.cnt >= 62u) spillLanes( w, 32);
	if (w.nEvents == 0 || (w.cnt && w.tailPos < from && w.tailEnd < to))
	{
		// most reports of a new token: the last event starts and ends before it, all three scans stop at once
		pushEvent( w, 0, id, from, to-from, levelBind);
		if (twin) pushEvent( w, 0, patternid, from, to-from, levelBind);
		return;
	}
	const bool more = w.nEvents > w.cnt;		// older events in the arena
	const u32 lastPos = to;
	u32 stage = 0;
	bool arena = false;
	{
		const u32 cnt = w.cnt;
		const u64 valid = lowMask( cnt);
		const u32 lvlL = w.e.lb & 0xFFu, endL = w.e.pos + w.e.size;
		// delete pass (:757-777): the run of events from the back with origpos >= the new origpos
		const u64 ge = __ballot( w.e.pos >= from) & valid;
		const u32 run = (u32)__builtin_ctzll( ~ge);
		if (run == cnt && more) arena = true;
		else
		{
			u64 del = __ballot( (w.e.id == id && w.e.pos == from && lvlL == level) || (lvlL < level && endL <= lastPos)) & lowMask( run);
			if (del)
			{
				stage = 1;
				while (del)
				{
					// remove the highest lane of the set: the lanes from there on take their upper neighbour's event
					const u32 d = 63u - (u32)__builtin_clzll( del);
					del &= ~(1ull << d);
					const u32 a = laneFromAbove( w.e.id), b = laneFromAbove( w.e.pos), c = laneFromAbove( w.e.size), e = laneFromAbove( w.e.lb);
					const bool dn = LANE >= d;
					w.e.id = dn ? a : w.e.id; w.e.pos = dn ? b : w.e.pos; w.e.size = dn ? c : w.e.size; w.e.lb = dn ? e : w.e.lb;
					--w.cnt; --w.nEvents;
				}
				readTail( w);
			}
			else
			{
				// ignore pass (:778-792): the run of events from the back that end at or behind the new end
				const u64 ge2 = __ballot( endL >= lastPos) & valid;
				const u32 run2 = (u32)__builtin_ctzll( ~ge2);
				if (run2 == cnt && more) arena = true;
				else if (__ballot( lvlL > level && w.e.pos <= from) & lowMask( run2)) return;
			}
		}
	}
	u32 at = 0;
	if (!arena)
	{
		// insertion point (:793-822): behind the events from the back that start to the right of the new one
		const u64 gt = __ballot( w.e.pos > from) & lowMask( w.cnt);
		at = (u32)__builtin_ctzll( ~gt);
		if ((at == w.cnt && more) || (twin && at)) arena = true;
	}
	if (arena)
	{
		spillLanes( w, 0);
		__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront");
		const u32 n = uni( handleReportArena( w.events, w.nEvents, stage, id, patternid, levelBind, from, to));
		__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront");
		w.nEvents = n;
		reloadLanes( w);
		readTail( w);
		return;
	}
	pushEvent( w, at, id, from, to-from, levelBind);
	if (twin) pushEvent( w, 0, patternid, from, to-from, levelBind);
}

// ---------------------------------------------------------------- stage 4: ordinal positions + output (:893-945)
// The reference walks the sorted event array once with a little state machine (patternLexer.cpp:893-945):
// up to the first content/unique event only successor-bound events are kept (position 1); from there on
// the ordinal position advances whenever a content/unique event starts to the right of all earlier
// ones, a unique event directly after a unique event is dropped, successor-bound events get position+1.
// Every piece of that state is a prefix quantity, so 64 events are handled per step: one coalesced
// load, a max-scan (start of the rightmost counted event so far), two sum-scans (ordinal position,
// output index), one coalesced store.  Pass A counts (the output is reserved once per document),
// pass B writes.
__device__ __forceinline__ u32 scanAdd( u32 v)
{
	return waveScanAdd( v);
}
__device__ __forceinline__ u32 scanMax( u32 v)
{
	return waveScanMax( v);
}
__device__ void emitLexems( LexWave& w, const L1Params& P, u32 doc)
{
	enum {BIND_CONTENT=0, BIND_SUCCESSOR=1, BIND_PREDECESSOR=2, BIND_UNIQUE=3};
	const u32 n = w.nEvents;
	// the first content/unique event
	u32 first = n;
	for (u32 base=0; base<n && first==n; base+=64)
	{
		const u32 i = base + LANE;
		u32 bind = 0xFFu;
		if (i < n) bind = (w.events[ i].levelBind >> 8) & 0xFFu;
		const u64 m = __ballot( bind == BIND_UNIQUE || bind == BIND_CONTENT);
		if (m) first = base + (u32)__builtin_ctzll( m);
	}
	u64 outBase = 0;
	u32 total = 0;
	if (first < n)
	{
		for (int phase=0; phase<2 && !w.err; ++phase)
		{
			u32 out = 0;			// lexems written so far
			u32 runMax = 0;			// start of the rightmost counted event so far (valid from `first` on)
			u32 runOrd = 1;			// ordinal position after the events so far
			u32 prevBind = BIND_CONTENT;	// bind of the event before this step's first one
			for (u32 base=0; base<n; base+=64)
			{
				const u32 i = base + LANE;
				uint4 e = make_uint4( 0, 0, 0, 0xFF00u);		// {id, origpos, origsize, levelBind}
				if (i < n) e = *(const uint4*)&w.events[ i];
				const u32 bind = (e.w >> 8) & 0xFFu;
				u32 pb = (u32)__shfl_up( (int)bind, 1);
				if (LANE == 0) pb = prevBind;
				const bool valid = i < n;
				const bool after = valid && i > first;			// the state machine proper
				const bool isFirst = valid && i == first;
				const bool dropped = after && bind == BIND_UNIQUE && pb == BIND_UNIQUE;
				const bool counted = (after && !dropped && (bind == BIND_UNIQUE || bind == BIND_CONTENT)) || isFirst;
				// start of the rightmost counted event strictly before me
				const u32 mine = counted ? e.y + 1u : 0u;		// +1: 0 = none
				const u32 inclMax = scanMax( mine);
				u32 exclMax = (u32)__shfl_up( (int)inclMax, 1);
				if (LANE == 0) exclMax = 0;
				if (runMax > exclMax) exclMax = runMax;
				const bool advances = counted && !isFirst && (e.y + 1u) > exclMax;
				const u32 inclOrd = scanAdd( advances ? 1u : 0u);
				const u32 ord = runOrd + inclOrd;			// ordinal position after me
				bool emit; u32 pos;
				if (!valid) { emit = false; pos = 0; }
				else if (i < first) { emit = (bind == BIND_SUCCESSOR); pos = 1; }
				else if (dropped) { emit = false; pos = 0; }
				else { emit = true; pos = (bind == BIND_SUCCESSOR) ? ord + 1u : ord; }
				const u32 inclOut = scanAdd( emit ? 1u : 0u);
				if (phase && emit)
				{
					u32* o = P.lexems + 4*(outBase + out + inclOut - 1u);
					*(uint4*)o = make_uint4( e.x, pos, e.y, e.z);
				}
				out += uni( (u32)__shfl( (int)inclOut, 63));
				runOrd += uni( (u32)__shfl( (int)inclOrd, 63));
				const u32 stepMax = uni( (u32)__shfl( (int)inclMax, 63));
				if (stepMax > runMax) runMax = stepMax;
				prevBind = uni( (u32)__shfl( (int)bind, 63));
			}
			if (!phase)
			{
				total = out;
				u64 b = 0;
				if (LANE == 0) b = atomicAdd( (unsigned long long*)&P.counters[ L1C_LEXEMS], (unsigned long long)total);
				outBase = ((u64)uni( (u32)(b >> 32)) << 32) | uni( (u32)b);
				if (outBase + total > P.lexemCapacity) { w.err = L1D_ERR_OUTPUT; total = 0; }
				if (!total) break;
			}
		}
	}
	if (LANE == 0)
	{
		P.docRange[ 2*(u64)doc] = outBase; P.docRange[ 2*(u64)doc+1] = w.err ? 0 : total;
	}
}

} // anonymous namespace
#endif
