// Words kernel of the lexer: whole-word literals and word shapes, a lane per byte (stage 1b of l1_wave.h as a kernel of its own).
#include "l1_wave.h"
#include "l1_launch.h"

namespace {

// SPA_WORDS_ABLATE (measurement builds only, never the product: the records come out wrong): bit 0 leaves out the confirming walks
// (every shape candidate stays dead), bit 1 the shape probes, bit 2 the literal probe, bit 3 the whole flush.  The instruction
// counters of two such builds differ by what the phase left out retires (the words kernel's table).
#ifndef SPA_WORDS_ABLATE
#define SPA_WORDS_ABLATE 0
#endif

// ---------------------------------------------------------------- words kernel: whole-word literals and word shapes
// A lane per byte, a wave per scan unit (a document, or a chunk of a long one): everything here is parallel over the text.
// Where a run of word characters ends, the lane behind it knows the run (start, length, polynomial hash -- one ballot and one
// segmented scan per 64-byte tile, as tileLiterals) and the run before it, and derives the candidates of that end offset:
// the literal table's entry of the whole word, and per shape variant of the table (l1_tables.h: PREFIX / SUFFIX / PREVWORD) the
// entry of the few bytes that pin the shape.  A shape candidate is confirmed by the backward walk of its automaton from the end
// offset (leftmostStart: exactly what an automaton report of that expression would go through), which also gives the leftmost
// start.  The unit's records go to its slice of the word queue in (end offset, pattern) order; a candidate that does not confirm
// keeps its record, marked dead (the lanes reserve their records before they walk).
struct WordCarry
{
	bool in; u32 hash, len, start;			// the run that reaches the end of the tile
	bool lastValid; u32 lastTo, lastHash, lastLen;	// the last run that ended so far: its end offset (= the byte behind it), hash, length
};

// start of the run of word characters that byte pos-1 belongs to (pos >= 1, byte pos-1 is a word character)
__device__ __forceinline__ u32 runStartBefore( const L1Params& P, const unsigned char* doc, u32 pos, u32 ctxReg)
{
	for (;;)
	{
		const u32 base = pos >= 64u ? pos - 64u : 0u;
		const u32 at = base + LANE;
		const u32 b = at < pos ? (u32)doc[ at] : 0u;
		const u32 ctxL = ((u32)__builtin_amdgcn_ds_bpermute( (int)((b >> 2) << 2), (int)ctxReg) >> ((b & 3u)*8)) & 0xFFu;
		const u64 nonWord = __ballot( at < pos && ctxL != (u32)CTX_WORD);
		if (nonWord) return base + 64u - (u32)__builtin_clzll( nonWord);		// behind the last byte that is none
		if (base == 0) return 0;
		pos = base;
	}
}

// The backward walk of leftmostStart for a candidate of the words kernel: class and context of the bytes it visits come from the
// wave's ring in LDS (the last 512 bytes of the text, written a tile at a time), the automaton's rows from the LDS image -- two
// LDS round trips per byte instead of four dependent global loads.  A walk that leaves the ring goes on with leftmostStart.
enum {WORD_RING=512, WORD_ENDS=96, WORD_ENDWORDS=5};
// (per wave: a ring of class | context << 8 of the last 512 bytes, wordRing, and wordEnds -- both declared in wordsDocuments, one pair
//  of arrays per workgroup size)
// the run ends that wait for their probes, {end offset, start of the run, hash of the run, hash of the word before it, length | length of
// the word before << 8} each; while a batch of them is worked on (they are in registers then) the first 1 KB holds the candidates
// {end offset, pattern | L1_LITERAL_FLAG for a literal, start of the run, -}: a lane each for the walks
static_assert( WORD_RING*2 + WORD_ENDS*WORD_ENDWORDS*4 == L1_WORDS_LDS_PER_WAVE, "static LDS of the words kernel");
static_assert( 64*WORD_ENDWORDS*4 >= 64*16, "the candidates lie over the ends of the batch");
template <bool LDS>
__device__ __forceinline__ u32 confirmWalk( const unsigned char* doc, u32 docLen, const L1Params& P, const LexTab<LDS>& T, const unsigned short* ring, u32 ringLo,
					    u32 word, u64 mask, u32 to)
{
	// ring[ q & (WORD_RING-1)] = class | context << 8 of byte q for ringLo <= q < ringLo + WORD_RING
	const u32 pass = word >> 6, ln = word & 63u;
	const u32 ccLast = ring[ (to-1u) & (WORD_RING-1)];
	const u32 nextctx = to < docLen ? ((u32)ring[ to & (WORD_RING-1)] >> 8) : (u32)CTX_EDGE;
	u64 R = mask & T.at( T.oAccept + (pass*CTX_COUNT + nextctx)*64 + ln) & T.at( T.oChar + (pass*P.nofClasses + (ccLast & 0xFFu))*64 + ln);
	if (!R) return to;
	const u64 shiftDst = T.at( T.oShift + pass*64 + ln), selfLoop = T.at( T.oSelf + pass*64 + ln);
	const u32 nEx = P.exCount[ pass];
	u32 nExWave = 0;			// the most exceptions a pass of the wave's walks has: a wave-uniform bound for the loop over them
	while (__ballot( nEx > nExWave)) ++nExWave;
	u32 from = to;
	u32 j = to;				// R = positions that consumed byte j-1
	// One loop condition and selects inside: a step costs the scalar unit the loop control alone.  The walk leaves the ring at the
	// first j with 2 <= j and j-2 < ringLo: j counts down by one from `to`, so that is j == ringLo+1 (or `to` itself when it is
	// below already), and never when ringLo is 0 or the walk begins at 1 -- jStop.  The step of j == 1 (the byte before the text is
	// the edge) goes through the transition too: what it leaves in R is not looked at again, j is 0 then.
	const u32 jStop = (ringLo > 0 && to >= 2u) ? ringLo + 1u : 0u;
	while ((R != 0) & (j > jStop))
	{
		const u32 inRing = ring[ (j-2u) & (WORD_RING-1)];
		const u32 cc = j >= 2u ? inRing : ((u32)CTX_EDGE << 8);
		from = (R & T.at( T.oStart + (pass*CTX_COUNT + (cc >> 8))*64 + ln)) ? j-1u : from;
		u64 Rp = ((R & shiftDst) >> 1) | (R & selfLoop);
		for (u32 e=0; e<nExWave; ++e)
		{
			const u32 at = (pass*P.maxExceptions + (e < nEx ? e : 0u))*64 + ln;
			const u64 es = T.at( T.oExSrc + at), ed = T.at( T.oExDst + at);
			Rp |= ((e < nEx) & ((R & ed) != 0)) ? es : 0ull;
		}
		R = Rp & mask & T.at( T.oChar + (pass*P.nofClasses + (cc & 0xFFu))*64 + ln);
		--j;
	}
	if ((R != 0) & (j > 0))			// (stopped at jStop with positions alive)
	{
		// (rare: a match longer than the ring) the rest of the walk from global memory
		const u32 f = leftmostStart<LDS,false>( doc, docLen, P, T, word, mask, j, R);
		return f < j ? f : from;
	}
	return from;
}

// One batch of up to 64 run ends, a lane each: literal probe, shape probes, the candidates ordered by (end offset, pattern) into the
// unit's queue, every candidate that is not a literal confirmed by a backward walk on a lane of its own (64 candidates a round).
template <bool LDS>
__device__ __forceinline__ void wordsFlush( LexWave& w, const L1Params& P, const LexTab<LDS>& T, const unsigned short* ring, const u32 ringLo, u32* ends, const u32 count, const u32 nVar)
{
	if (SPA_WORDS_ABLATE & 8) return;
	const u32 len = w.docLen;
	const bool emit = LANE < count;
	u32 to = 0, pFrom = 0, pH = 0, qH = 0, pLen = 0, qLen = 0;
	if (emit)
	{
		const u32* e = ends + WORD_ENDWORDS*LANE;
		to = e[ 0]; pFrom = e[ 1]; pH = e[ 2]; qH = e[ 3];
		const u32 l = e[ 4]; pLen = l & 0xFFu; qLen = l >> 8;
	}
	__builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront");		// (the candidates overwrite the batch from here on)
	// ---- candidates of my end offset: lists of patterns, ascending each
	enum {NLIST=SHAPE_MAXVARIANTS+1};
	u32 lb[ NLIST], lc[ NLIST];
#pragma unroll
	for (int k=0; k<NLIST; ++k) { lb[ k] = 0; lc[ k] = 0; }
	u32 total = 0, lit0 = 0;
	if (emit)
	{
		if (!(SPA_WORDS_ABLATE & 4) && P.nofLiterals && pLen <= 64u)
		{
			// whole-word literal (the probe of tileLiterals)
			const u32 h = literalHashFinish( pH);
			u32 slot = h & P.literalMask;
			uint4 dw = make_uint4( 0, 0, 0, 0);
			if (pFrom + 16u <= len) dw = ld128u( w.doc + pFrom);
			else
			{
				u32 d[ 4] = {0,0,0,0};
				for (u32 q=0; q<16u && pFrom+q<len; ++q) d[ q>>2] |= (u32)w.doc[ pFrom + q] << (8*(q&3u));
				dw = make_uint4( d[0], d[1], d[2], d[3]);
			}
			const u32 m0 = pLen >= 4u ? 0xFFFFFFFFu : ((1u << (8*pLen)) - 1u);
			const u32 m1 = pLen >= 8u ? 0xFFFFFFFFu : (pLen > 4u ? ((1u << (8*(pLen-4u))) - 1u) : 0u);
			const u32 m2 = pLen >= 12u ? 0xFFFFFFFFu : (pLen > 8u ? ((1u << (8*(pLen-8u))) - 1u) : 0u);
			const u32 m3 = pLen >= 16u ? 0xFFFFFFFFu : (pLen > 12u ? ((1u << (8*(pLen-12u))) - 1u) : 0u);
			for (u32 probes=0; probes<=P.literalMask; ++probes)
			{
				const uint4* ep = (const uint4*)&P.literals[ slot];
				const uint4 e0 = ep[ 0], e1 = ep[ 1], tx = ep[ 2];
				if (!e0.x) break;
				if (e0.x == h && e0.y == pLen)
				{
					bool same = (((dw.x ^ tx.x) & m0) | ((dw.y ^ tx.y) & m1) | ((dw.z ^ tx.z) & m2) | ((dw.w ^ tx.w) & m3)) == 0;
					for (u32 k=16; k<pLen && same; k+=4)
					{
						const u32 rem = pLen - k;
						u32 a;
						if (pFrom + k + 4u <= len) a = ld32u( w.doc + pFrom + k);
						else { a = 0; for (u32 q=0; q<rem && q<4u; ++q) a |= (u32)w.doc[ pFrom + k + q] << (8*q); }
						const u32 b = ld32u( P.literalText + e1.w + k);
						const u32 mask = rem >= 4u ? 0xFFFFFFFFu : ((1u << (8*rem)) - 1u);
						same = ((a ^ b) & mask) == 0;
					}
					if (same) { lb[ 0] = e0.z; lc[ 0] = e0.w; lit0 = e1.x; break; }
				}
				slot = (slot+1) & P.literalMask;
			}
		}
	}
	// ---- shape variants: the key bytes come out of two unaligned words of the text (the run's first four bytes, its last
	// four); the compact table (fingerprint, pattern or list) sits in LDS beside the automaton tables: no global round trip
	if (nVar && !(SPA_WORDS_ABLATE & 2))
	{
		u32 first4 = 0, last4 = 0;
		if (emit)
		{
			if (pFrom + 4u <= len) first4 = ld32u( w.doc + pFrom); else for (u32 i=0; i<4u && pFrom+i<len; ++i) first4 |= (u32)w.doc[ pFrom+i] << (8*i);
			if (to >= 4u) last4 = ld32u( w.doc + to - 4u); else for (u32 i=0; i<to; ++i) last4 |= (u32)w.doc[ i] << (8*(4u-to+i));
		}
		// (the key of every kind by selects on the variant's wave-uniform fields -- no branch per kind and lane; the first two
		//  probes as straight-line code, both entries requested before the first compare: the loop is entered only when a ballot
		//  says that a lane still probes)
		const u32 prevTag = (emit && qLen >= 1u && qLen <= 64u) ? ((u32)SHAPE_PREVWORD | (qLen << 8)) : 0u;
		const u32 prevKey = literalHashFinish( qH);
		const u32 shapeMask = uni( P.shapeMask), fpOffset = uni( P.shapeFpOffset), salt = uni( P.shapeSalt);
#pragma unroll
		for (int v=0; v<SHAPE_MAXVARIANTS; ++v)
		{
			if ((u32)v < nVar)
			{
				const u32 var = uni( P.shapeVariants[ v]);
				const u32 kind = var & 3u, o = (var >> 2) & 3u, k = (var >> 4) & 7u;
				const u32 kmask = k >= 4u ? 0xFFFFFFFFu : ((1u << (8*k)) - 1u);
				const bool isPrev = kind == (u32)SHAPE_PREVWORD, isPrefix = kind == (u32)SHAPE_PREFIX;
				const u32 need = isPrefix ? o + k : k;
				const u32 shift = isPrefix ? 8*o : (k >= 4u ? 0u : 8*(4u-k));
				u32 tag = isPrev ? prevTag : ((emit && pLen >= need) ? var : 0u);
				u32 key = isPrev ? prevKey : (((isPrefix ? first4 : last4) >> shift) & kmask);
				if (isPrefix && o + k > 4u)
				{
					// (a prefix key that reaches behind the run's first four bytes: byte by byte)
					key = 0;
					if (tag) for (u32 i=0; i<k; ++i) key |= (u32)w.doc[ pFrom + o + i] << (8*i);
				}
				const u32 fp = shapeFingerprint( tag, key, salt);
				u32 slot = shapeSlotHash( tag, key) & shapeMask;
				const u64 e0 = T.at( fpOffset + slot), e1 = T.at( fpOffset + ((slot+1) & shapeMask));	// fingerprint | (count << 24 | pattern or list) << 32
				const bool hit0 = tag && (u32)e0 == fp;
				const bool second = tag && (u32)e0 && (u32)e0 != fp && shapeMask >= 1u;
				const bool hit1 = second && (u32)e1 == fp;
				const bool more = second && (u32)e1 && (u32)e1 != fp && shapeMask >= 2u;
				const u32 eh = (u32)((hit0 ? e0 : e1) >> 32);
				lb[ 1+v] = (hit0 || hit1) ? (eh & 0xFFFFFFu) : 0u;
				lc[ 1+v] = (hit0 || hit1) ? (eh >> 24) : 0u;
				if (__ballot( more))
				{
					if (more)
					{
						slot = (slot+2) & shapeMask;
						for (u32 probes=2; probes<=shapeMask; ++probes)
						{
							const u64 e = T.at( fpOffset + slot);
							if (!(u32)e) break;
							if ((u32)e == fp) { lb[ 1+v] = (u32)(e >> 32) & 0xFFFFFFu; lc[ 1+v] = (u32)(e >> 56); break; }
							slot = (slot+1) & shapeMask;
						}
					}
				}
			}
		}
	}
#pragma unroll
	for (int k=0; k<NLIST; ++k) total += lc[ k];
	// ---- every lane reserves its records; 64 candidates a round get a lane each for the walk that confirms them
	const u32 incl = waveScanAdd( total);
	const u32 waveTotal = (u32)__builtin_amdgcn_readlane( incl, 63);
	if (!waveTotal) return;
	if (w.nQueue + waveTotal > w.queueCap) { w.err = L1D_ERR_ARENA; return; }
	uint4* stage = (uint4*)ends;
	// The usual lane: no list longer than one pattern, no more than four candidates.  Then its candidates are a handful of keys
	// (pattern << 1 | literal) in registers, ordered by a five-comparator network; the others merge their lists by pattern index.
	bool simple = total <= 4u;
#pragma unroll
	for (int k=0; k<NLIST; ++k) if (lc[ k] > 1u) simple = false;
	u32 c0 = 0xFFFFFFFFu, c1 = 0xFFFFFFFFu, c2 = 0xFFFFFFFFu, c3 = 0xFFFFFFFFu;
	u32 head[ NLIST];
	if (simple)
	{
		u32 nc = 0;
#pragma unroll
		for (int k=0; k<NLIST; ++k)
		{
			if (lc[ k])
			{
				const u32 key = k == 0 ? ((lit0 << 1) | 1u) : (lb[ k] << 1);
				c0 = nc == 0 ? key : c0; c1 = nc == 1 ? key : c1; c2 = nc == 2 ? key : c2; c3 = nc == 3 ? key : c3;
				++nc;
			}
		}
#define SPA_CSWAP( A, B) { const u32 lo = A < B ? A : B, hi = A < B ? B : A; A = lo; B = hi; }
		SPA_CSWAP( c0, c1) SPA_CSWAP( c2, c3) SPA_CSWAP( c0, c2) SPA_CSWAP( c1, c3) SPA_CSWAP( c1, c2)
#undef SPA_CSWAP
	}
	const bool anyGeneral = __ballot( !simple && total) != 0;
	if (anyGeneral)
	{
#pragma unroll
		for (int k=0; k<NLIST; ++k)
		{
			head[ k] = 0xFFFFFFFFu;
			if (!simple && lc[ k]) head[ k] = k == 0 ? lit0 : (lc[ k] == 1u ? lb[ k] : P.shapePats[ lb[ k]]);	// (a shape entry of one pattern holds the pattern in place of the list)
		}
	}
	const u32 base = incl - total;
	u32 produced = 0;
	for (u32 r0=0; r0<waveTotal; r0+=64)
	{
		while (produced < total && base + produced < r0 + 64u)
		{
			u32 cand;
			if (simple)
			{
				const u32 key = produced == 0 ? c0 : (produced == 1 ? c1 : (produced == 2 ? c2 : c3));
				cand = (key >> 1) | ((key & 1u) ? (u32)L1_LITERAL_FLAG : 0u);
			}
			else
			{
				u32 best = 0xFFFFFFFFu; int which = 0;
#pragma unroll
				for (int k=0; k<NLIST; ++k) if (head[ k] < best) { best = head[ k]; which = k; }
#pragma unroll
				for (int k=0; k<NLIST; ++k)
				{
					if (k == which)
					{
						if (k != 0 && lc[ k] == 1u) { lc[ k] = 0; head[ k] = 0xFFFFFFFFu; }
						else
						{
							++lb[ k]; --lc[ k];
							head[ k] = lc[ k] ? (k == 0 ? P.litPats[ lb[ 0]] : P.shapePats[ lb[ k]]) : 0xFFFFFFFFu;
						}
					}
				}
				cand = which == 0 ? (best | (u32)L1_LITERAL_FLAG) : best;
			}
			stage[ base + produced - r0] = make_uint4( to, cand, pFrom, 0u);
			++produced;
		}
		__builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront");
		const u32 nr = (waveTotal - r0) < 64u ? (waveTotal - r0) : 64u;
		if (LANE < nr)
		{
			const uint4 cnd = stage[ LANE];
			u32 fromOut = cnd.z, flags = (u32)L1_LITERAL_FLAG;
			const u32 pi = cnd.y & ~(u32)L1_LITERAL_FLAG;
			if ((SPA_WORDS_ABLATE & 1) && !(cnd.y & (u32)L1_LITERAL_FLAG)) flags |= (u32)L1_DEAD_FLAG;
			else if (!(cnd.y & (u32)L1_LITERAL_FLAG))
			{
				const uint2 pw = *(const uint2*)((const u32*)&P.patterns[ pi] + 5);	// {maskLo, maskHi}
				const u32 word = ((const u32*)&P.patterns[ pi])[ 1];
				fromOut = confirmWalk<LDS>( w.doc, len, P, T, ring, ringLo, word, ((u64)pw.y << 32) | pw.x, cnd.x);
				if (fromOut == cnd.x) flags |= (u32)L1_DEAD_FLAG;
			}
			*(uint4*)(w.queue + 4*(u64)(w.nQueue + r0 + LANE)) = make_uint4( cnd.x, pi | flags, fromOut, 0u);
		}
		__builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront");
	}
	w.nQueue += waveTotal;
}

// The runs of word characters of a unit, a lane per byte: where a run ends the lane knows the run's start, length and hash and those of
// the word before it.  Only one byte in six ends a run, so the ends are collected -- up to 64 of them, over several tiles -- before
// they are probed with a lane each (wordsFlush).
template <bool LDS>
__device__ __forceinline__ void wordsUnit( LexWave& w, const L1Params& P, const LexTab<LDS>& T, const u32 segBeg, const u32 segEnd, unsigned short* ring, u32* ends)
{
	const u32 len = w.docLen;
	u32 ctxReg = 0, clsReg = 0;		// byte -> context, class: lane l keeps the entries of bytes 4l..4l+3
	for (u32 k=0; k<4; ++k) { const u32 cl = P.byteClass[ 4*LANE + k]; clsReg |= cl << (8*k); ctxReg |= (u32)P.classCtx[ cl] << (8*k); }
	auto isWordAt = [&]( u32 pos) -> bool { return P.classCtx[ P.byteClass[ uni( (u32)w.doc[ pos])]] == (u32)CTX_WORD; };
	// where to begin: before the unit, at the start of a run (or between runs), so that every run that ends inside the unit is
	// seen from its first byte -- and one run further back when that one could be the word before a run of the unit
	u32 w0 = segBeg > 160u ? segBeg - 160u : 0u;
	if (w0 > 0 && isWordAt( w0-1)) w0 = runStartBefore( P, w.doc, w0, ctxReg);
	if (w0 >= 2 && isWordAt( w0-2)) w0 = runStartBefore( P, w.doc, w0-1, ctxReg);
	WordCarry c; c.in = false; c.hash = 0; c.len = 0; c.start = 0; c.lastValid = false; c.lastTo = 0; c.lastHash = 0; c.lastLen = 0;
	const u32 nVar = uni( P.nofShapeVariants);
	u32 nEnds = 0, firstTile = 0;		// ends that wait, the tile the oldest of them was seen in
	u32 ahead = (w0 + LANE < len) ? (u32)w.doc[ w0 + LANE] : 0u;
	u32 tile = w0;
	for (; tile<=len && tile<=segEnd && !w.err; tile+=64)
	{
		const u32 inTile = (len - tile) < 64 ? (len - tile) : 64;
		const u32 mine = ahead;			// (the next tile's bytes are requested one tile ahead)
		ahead = (tile + 64u + LANE < len) ? (u32)w.doc[ tile + 64u + LANE] : 0u;
		const u32 ctxL = ((u32)__builtin_amdgcn_ds_bpermute( (int)((mine >> 2) << 2), (int)ctxReg) >> ((mine & 3u)*8)) & 0xFFu;
		const u32 clsL = ((u32)__builtin_amdgcn_ds_bpermute( (int)((mine >> 2) << 2), (int)clsReg) >> ((mine & 3u)*8)) & 0xFFu;
		ring[ (tile + LANE) & (WORD_RING-1)] = (unsigned short)(clsL | (ctxL << 8));		// (the ring keeps the last 512 bytes)
		const bool isW = LANE < inTile && ctxL == (u32)CTX_WORD;
		// ---- the runs of the tile (as tileLiterals)
		const u64 wm = __ballot( isW);
		const u64 prevW = (wm << 1) | (c.in ? 1ull : 0ull);
		const u64 startM = wm & ~prevW;
		const u64 endMask = ~wm & prevW;			// bit e: the run that ended just before byte tile+e
		const u64 sb = startM & (((1ull << LANE) - 1ull) | (1ull << LANE));
		const int ss = sb ? 63 - (int)__builtin_clzll( sb) : -1;
		u32 H = isW ? mine + 1u : 0u, M = (u32)L1_LITHASH_MUL;
#pragma unroll
		for (int d=1; d<64; d<<=1)
		{
			const u32 Hs = (u32)__shfl_up( (int)H, d), Ms = (u32)__shfl_up( (int)M, d);
			const bool take = isW && (int)LANE >= d && (int)LANE - d >= ss;
			// (a lane that takes nothing multiplies by the neutral pair: selects, no exec-mask branch per step)
			const u32 Ht = take ? Hs : 0u, Mt = take ? Ms : 1u;
			H = Ht * M + H; M = Mt * M;
		}
		const bool carried = isW && ss < 0;
		const u32 Htot = carried ? c.hash * M + H : H;
		u32 runLen = isW ? (carried ? c.len : 0u - (u32)ss) + LANE + 1u : 0u;
		if (runLen > 65u) runLen = 65u;
		const u32 from = carried ? c.start : tile + (u32)(ss < 0 ? 0 : ss);
		u32 pH = (u32)__shfl_up( (int)Htot, 1), pLen = (u32)__shfl_up( (int)runLen, 1), pFrom = (u32)__shfl_up( (int)from, 1);
		if (LANE == 0) { pH = c.hash; pLen = c.len; pFrom = c.start; }
		const bool isEnd = (endMask >> LANE) & 1ull;
		const u32 to = tile + LANE;
		// ---- the run before mine, when it ended one byte before mine begins (PREVWORD)
		u32 qH = 0, qLen = 0;
		{
			const u32 want = pFrom - 1u;			// its end offset
			const u32 src = want - tile;			// lane that saw it end, if in this tile
			const u32 sH = (u32)__builtin_amdgcn_ds_bpermute( (int)((src & 63u) << 2), (int)pH);
			const u32 sLen = (u32)__builtin_amdgcn_ds_bpermute( (int)((src & 63u) << 2), (int)pLen);
			const bool inTile = want >= tile;
			const bool fromTile = inTile && ((endMask >> (src & 63u)) & 1ull), fromCarry = !inTile && c.lastValid && c.lastTo == want;
			const bool hasPrev = isEnd && pFrom >= 2u && (fromTile || fromCarry);
			qH = hasPrev ? (fromTile ? sH : c.lastHash) : 0u;
			qLen = hasPrev ? (fromTile ? sLen : c.lastLen) : 0u;
		}
		// ---- the ends that count go behind the ones that wait
		const bool emit = isEnd && pLen >= 1u && ((to >= segBeg && to < segEnd) || (to == segEnd && segEnd == len));
		const u64 em = __ballot( emit);
		if (em)
		{
			const u32 rank = (u32)__builtin_amdgcn_mbcnt_hi( (u32)(em >> 32), __builtin_amdgcn_mbcnt_lo( (u32)em, 0));
			if (emit)
			{
				u32* e = ends + WORD_ENDWORDS*(nEnds + rank);
				e[ 0] = to; e[ 1] = pFrom; e[ 2] = pH; e[ 3] = qH; e[ 4] = (pLen > 65u ? 65u : pLen) | ((qLen > 65u ? 65u : qLen) << 8);
			}
			if (!nEnds) firstTile = tile;
			nEnds += (u32)__builtin_popcountll( em);
		}
		__builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront");
		// ---- carry: the run that reaches the end of the tile, the last run that ended
		c.in = (wm >> 63) & 1ull;
		if (c.in)
		{
			c.hash = uni( (u32)__shfl( (int)Htot, 63)); c.len = uni( (u32)__shfl( (int)runLen, 63)); c.start = uni( (u32)__shfl( (int)from, 63));
		}
		if (endMask)
		{
			const u32 e = 63u - (u32)__builtin_clzll( endMask);
			c.lastValid = true; c.lastTo = tile + e;
			c.lastHash = (u32)__builtin_amdgcn_readlane( pH, e); c.lastLen = (u32)__builtin_amdgcn_readlane( pLen, e);
		}
		// ---- a full batch, or ends about to lose the bytes before them from the ring: probe
		const bool pressure = nEnds && tile + 64u - firstTile > (u32)WORD_RING - 192u;
		while (!w.err && (nEnds >= 64u || (pressure && nEnds)))
		{
			const u32 count = nEnds < 64u ? nEnds : 64u;
			const u32 ringLo = tile + 64u > w0 + (u32)WORD_RING ? tile + 64u - (u32)WORD_RING : w0;
			// (what is behind the batch is read before the candidates of the batch are written over it... it lies behind them: entries 64..)
			wordsFlush<LDS>( w, P, T, ring, ringLo, ends, count, nVar);
			const u32 rest = nEnds - count;
			u32 keep[ WORD_ENDWORDS];
			if (LANE < rest) { _Pragma("unroll") for (int k=0; k<WORD_ENDWORDS; ++k) keep[ k] = ends[ WORD_ENDWORDS*(64u + LANE) + k]; }
			__builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront");
			if (LANE < rest) { _Pragma("unroll") for (int k=0; k<WORD_ENDWORDS; ++k) ends[ WORD_ENDWORDS*LANE + k] = keep[ k]; }
			__builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront");
			nEnds = rest; firstTile = tile;
		}
	}
	// the ends that still wait (the ring holds the bytes up to the last tile)
	if (!w.err && nEnds)
	{
		const u32 doneTo = tile;	// (one behind the last tile's first byte + 64... the loop has stepped past it)
		const u32 ringLo = doneTo > w0 + (u32)WORD_RING ? doneTo - (u32)WORD_RING : w0;
		wordsFlush<LDS>( w, P, T, ring, ringLo, ends, nEnds, nVar);
	}
}

template <bool LDS>
__device__ __forceinline__ void wordsDocuments( const L1Params& P, unsigned short* ring, u32* ends)
{
	if (!P.wordsKernel) return;
	LexTab<LDS> T;
	stageTables( P, T);
	const u32 chunked = ldu( (const u32*)&P.counters[ L1C_CHUNKED]);
	LexWave w;
	w.events = 0; w.nEvents = 0; w.cnt = 0; w.tailPos = 0; w.tailEnd = 0;
	const u32 nunits = ldu( (const u32*)&P.counters[ L1C_UNITS]);
	for (u32 round=0; round<=nunits; ++round)
	{
		u32 unit = 0;
		if (LANE == 0) unit = atomicAdd( (u32*)&P.counters[ L1C_CURSOR4], 1u);
		unit = uni( unit);
		if (unit >= nunits) break;
		u32 doc = unit;
		if (chunked)
		{
			u32 lo = 0, hi = P.ndocs;			// last document whose first unit is <= unit
			while (hi - lo > 1u) { const u32 mid = (lo + hi) >> 1; if (ldu( &P.unitStart[ mid]) <= unit) lo = mid; else hi = mid; }
			doc = lo;
		}
		u64 beg, end;
		docBounds( P, doc, beg, end);
		w.doc = P.text + beg; w.docLen = (u32)(end - beg);
		u32 segBeg = 0, segEnd = w.docLen;
		if (chunked)
		{
			segBeg = (unit - ldu( &P.unitStart[ doc])) * P.chunkBytes;
			segEnd = (w.docLen - segBeg) < P.chunkBytes ? w.docLen : segBeg + P.chunkBytes;
		}
		const u64 qb = queueBase( P, beg + segBeg, unit);
		w.queue = P.wordQueue + 4*qb;
		w.queueCap = (u32)(queueBase( P, beg + segEnd, unit + 1) - qb);
		w.nQueue = 0; w.err = 0;
		wordsUnit<LDS>( w, P, T, segBeg, segEnd, ring, ends);
		if (LANE == 0)
		{
			P.wordCount[ unit] = w.err ? 0u : w.nQueue;
			if (w.err) P.docStatus[ doc] = (int32_t)w.err;
			if (w.err == L1D_ERR_ARENA) atomicAdd( (unsigned long long*)&P.counters[ L1C_OVER_QUEUE], 1ull);
			atomicAdd( (unsigned long long*)&P.counters[ L1C_WORDREPORTS], (unsigned long long)w.nQueue);
		}
	}
}

} // anonymous namespace

// (12 waves: the table image of a large expression set leaves room for no more; 16 waves -- what 114 registers allow -- for small sets)
#define SPA_L1_WORDS_KERNEL( NAME, WAVES) \
extern "C" __global__ __launch_bounds__(64*WAVES) void NAME( L1Params P) \
{ \
	__shared__ unsigned short wordRing[ WAVES][ WORD_RING]; \
	__shared__ __attribute__((aligned(16))) u32 wordEnds[ WAVES][ WORD_ENDS*WORD_ENDWORDS]; \
	const u32 wv = threadIdx.x >> 6; \
	if (P.ldsWords) wordsDocuments<true>( P, wordRing[ wv], wordEnds[ wv]); else wordsDocuments<false>( P, wordRing[ wv], wordEnds[ wv]); \
}
SPA_L1_WORDS_KERNEL( spa_l1_words_kernel, L1_WORD_WAVES)
SPA_L1_WORDS_KERNEL( spa_l1_words_kernel_w16, L1_WORD_WAVES_SMALL)

namespace spa {
hipError_t launchL1Words( const L1LaunchPlan& plan, const L1Params& PW, hipStream_t stream)
{
	// (its own copy of the parameters: its image staged in LDS when it fits; 16 or 12 waves per workgroup by what the image leaves)
	const bool small = plan.wordWaves == (unsigned)L1_WORD_WAVES_SMALL;
	hipError_t e = launchL1Kernel( small ? (const void*)spa_l1_words_kernel_w16 : (const void*)spa_l1_words_kernel, plan.wordGrid, 64*plan.wordWaves, (size_t)plan.wordLdsWords * 8, stream, PW);
	if (e != hipSuccess) return e;
	return hipGetLastError();
}
} // namespace
