// Stage 1 of the lexer (l1_wave.h), a wave per scan unit: the scan template, the macro that instantiates it for one pass
// count, and the host's table entry of such an instance.  The instances are spread over the l1_scan_kernel*.hip files (they are
// most of the lexer's compile time and independent of each other); l1_scan_kernel.hip picks and launches them.
#ifndef SPA_L1_SCAN_H
#define SPA_L1_SCAN_H
#include "l1_wave.h"

namespace {

// ---------------------------------------------------------------- stage 1: forward scan
// Scans the bytes [segBeg, segEnd) of the document (CH: a chunk of it; else the whole document) and queues the raw reports
// of the end offsets segBeg .. segEnd-1, and of segEnd when that is the document's end.  The state at the start of a
// later chunk comes from a warm-up over the WARM bytes before it: S = the state reached from the empty state with starts
// injected (a subset of the true state), F = the state reached from "every position live" without injection (a superset of
// whatever the true state before the warm-up contributes).  The automaton is linear in its state set, so the true state
// is S | (something inside F): F inside S proves S exact -- the usual case after a few words --, otherwise the document is
// handed to the sequential re-scan (L1D_CHUNK_UNPROVEN).
template <int PASSES, bool LDS, bool CP, bool CH>
__device__ void scanDocument( LexWave& w, const L1Params& P, const LexTab<LDS>& T, const u32 segBeg, const u32 segEnd)
{
	enum {WARM=256};
	u64 state[ PASSES];
#pragma unroll
	for (int p=0; p<PASSES; ++p) state[ p] = 0;
	const u32 len = w.docLen;
	// instances for 1..8 passes run tables of exactly that many passes; the 16 / 32 instances run anything up to it
	const u32 nofPasses = (PASSES <= 8) ? (u32)PASSES : uni( P.nofPasses);
	const u32 nofClasses = uni( P.nofClasses), maxEx = uni( P.maxExceptions);
	int prevctx = CTX_EDGE;
	// byte -> class / context without touching memory: lane l keeps the entries of bytes 4l..4l+3
	u32 clsReg = 0, ctxReg = 0;
	for (u32 k=0; k<4; ++k)
	{
		const u32 c = P.byteClass[ 4*LANE + k];
		clsReg |= c << (8*k);
		ctxReg |= (u32)P.classCtx[ c] << (8*k);
	}
	// per-pass constants in registers
	u64 shiftDst[ PASSES], selfLoop[ PASSES]; u32 nExOf[ PASSES];
#pragma unroll
	for (int p=0; p<PASSES; ++p)
	{
		const bool on = (u32)p < nofPasses;
		shiftDst[ p] = on ? T.at( T.oShift + p*64 + LANE) : 0; selfLoop[ p] = on ? T.at( T.oSelf + p*64 + LANE) : 0;
		nExOf[ p] = on ? uni( P.exCount[ p]) : 0;
	}
	u64 wcarry = 0;
	auto runRange = [&]( auto emitTag, auto injectTag, const u32 from, const u32 to, const bool withEnd)
	{
	constexpr bool EMIT = decltype(emitTag)::value, INJECT = decltype(injectTag)::value;
	for (u32 tile=from; (tile < to || (withEnd && tile == to)) && !w.err; tile+=64)
	{
		// 64 document bytes per load, one per lane; replayed byte by byte through a scalar register
		u32 mine = (tile + LANE < len) ? w.doc[ tile + LANE] : 0u;
		u32 inTile = (to - tile) < 64 ? (to - tile) : 64;	// bytes of the range in this tile
		// class and context of my byte (lane-parallel lookup in the register tables), replayed per byte with one readlane
		const u32 ccv = tileClassCtx<CP>( P, w.doc, len, tile, mine, clsReg, ctxReg, wcarry);
		// one byte step; the virtual step behind the last byte (matches that end with the document) is a
		// separate instance so that the hot one carries no end-of-document conditions
		auto step = [&]( auto atEndTag, const u32 k)
		{
			constexpr bool atEnd = decltype(atEndTag)::value;
			const u32 i = tile + k;
			const u32 cc = atEnd ? ((u32)CTX_EDGE << 8) : (u32)__builtin_amdgcn_readlane( ccv, k);
			const u32 cls = cc & 0xFFu;
			const int ctx = (int)(cc >> 8);
			const u32 groupStart = w.nQueue;	// reports of this end offset start here
			// every table row this byte needs, for all passes, before anything depends on them
			u64 accRow[ PASSES], cmRow[ PASSES], stRow[ PASSES];
#pragma unroll
			for (int p=0; p<PASSES; ++p)
			{
				// the tables end at nofPasses
				accRow[ p] = 0; cmRow[ p] = 0; stRow[ p] = 0;
				if ((u32)p < nofPasses)
				{
					accRow[ p] = T.at( T.oAccept + (p*CTX_COUNT + ctx)*64 + LANE);
					cmRow[ p] = T.at( (p*nofClasses + cls)*64 + LANE);
					stRow[ p] = T.at( T.oStart + (p*CTX_COUNT + prevctx)*64 + LANE);
				}
			}
			u64 acc[ PASSES];
			u64 anyAcc = 0;
#pragma unroll
			for (int p=0; p<PASSES; ++p)
			{
				acc[ p] = 0;
				if ((u32)p >= nofPasses) continue;
				const u64 st = state[ p];
				acc[ p] = st & accRow[ p];			// matches ending before byte i
				anyAcc |= acc[ p];
				if (!atEnd)
				{
					u64 nxt = ((st << 1) & shiftDst[ p]) | (st & selfLoop[ p]) | (INJECT ? stRow[ p] : 0ull);
					const u32 nEx = nExOf[ p];
					for (u32 e=0; e<nEx; ++e)
					{
						const u32 at = (p*maxEx + e)*64 + LANE;
						const u64 es = T.at( T.oExSrc + at), ed = T.at( T.oExDst + at);
						nxt |= (st & es) ? ed : 0ull;
					}
					state[ p] = nxt & cmRow[ p];
				}
			}
			if (EMIT && (__ballot( anyAcc != 0) || (CP && P.nofNullable)))
			{

#pragma unroll
				for (int p=0; p<PASSES; ++p)
				{
					const u64 a = acc[ p];
					if (!__ballot( a != 0)) continue;
					// per lane: which patterns packed into my word fired.  patOfBit maps an automaton bit to its
					// pattern; the pattern's mask then retires all of its bits at once (two loads per report).
					const u32 word = p*64 + LANE;
					u32 mycount = 0;
					u32 pi0 = 0, pi1 = 0; u64 m0 = 0, m1 = 0;
					{
						u64 rem = a;
						while (rem)
						{
							const u32 bit = (u32)__builtin_ctzll( rem);
							const u32 pi = P.patOfBit[ word*64 + bit];
							const DevLexPattern* pat = &P.patterns[ pi];
							const uint2 mm = *(const uint2*)&pat->maskLo;
							const u64 m = ((u64)mm.y << 32) | mm.x;
							if (mycount == 0) { pi0 = pi; m0 = m; } else if (mycount == 1) { pi1 = pi; m1 = m; }
							rem &= ~m;
							++mycount;
						}
					}
					// exclusive prefix sum of the counts over the lanes (report order = lane order)
					u32 incl = waveScanAdd( mycount);
					u32 total = (u32)__builtin_amdgcn_readlane( incl, 63);
					u32 at = w.nQueue + incl - mycount;
					if (w.nQueue + total > w.queueCap) { w.err = L1D_ERR_ARENA; break; }
					if (mycount)
					{
						u64 rem = a;
						for (u32 x=0; x<mycount; ++x)
						{
							u32 pi; u64 m;
							if (x == 0) { pi = pi0; m = m0; }
							else if (x == 1) { pi = pi1; m = m1; }
							else
							{
								const u32 bit = (u32)__builtin_ctzll( rem);
								pi = P.patOfBit[ word*64 + bit];
								const uint2 mm = *(const uint2*)&P.patterns[ pi].maskLo;
								m = ((u64)mm.y << 32) | mm.x;
							}
							*(uint4*)(w.queue + 4*(u64)at) = make_uint4( i, pi, (u32)(a & m), (u32)((a & m) >> 32));
							rem &= ~m;
							++at;
						}
					}
					w.nQueue += total;
				}
				if (CP && P.nofNullable)
				{
					// ALLOWEMPTY: an expression that matches the empty string reports (i, i) when its empty path holds between the
					// byte before and this one and nothing longer of it ends here (the leftmost start wins)
					for (u32 k=0; k<P.nofNullable && !w.err; ++k)
					{
						const u32 pi = ldu( &P.nullable[ k].pattern), ok = ldu( &P.nullable[ k].emptyOk);
						if (!((ok >> ((u32)prevctx*CTX_COUNT + (u32)ctx)) & 1u)) continue;
						const DevLexPattern* pat = &P.patterns[ pi];
						const u32 word = ldu( &pat->word);
						const u64 mask = ((u64)ldu( &pat->maskHi) << 32) | ldu( &pat->maskLo);
						u64 a = 0;
#pragma unroll
						for (int p=0; p<PASSES; ++p) if ((word >> 6) == (u32)p) a = acc[ p];
						if (__ballot( (word & 63u) == LANE && (a & mask) != 0)) continue;
						if (w.nQueue + 1u > w.queueCap) { w.err = L1D_ERR_ARENA; break; }
						if (LANE == 0) *(uint4*)(w.queue + 4*(u64)w.nQueue) = make_uint4( i, pi, 0, 0);
						++w.nQueue;
					}
				}
				if (!P.reportsOrdered && !w.err)
				{
					// the patterns are packed by size, not in definition order: bring the reports of this end
					// offset into ascending pattern index (the order the reference's handler sees them in)
					const u32 g = w.nQueue - groupStart;
					if (g > 1)
					{
						__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront");
						if (g <= 64u)
						{
							uint4 e = make_uint4( 0, 0xFFFFFFFFu, 0, 0);
							if (LANE < g) e = *(const uint4*)(w.queue + 4*(u64)(groupStart + LANE));
							u32 rank = 0;
							for (u32 j=0; j<g; ++j) { const u32 pj = (u32)__builtin_amdgcn_readlane( e.y, j); if (pj < e.y) ++rank; }
							if (LANE < g) *(uint4*)(w.queue + 4*(u64)(groupStart + rank)) = e;
						}
						else
						{
							for (u32 a=groupStart+1; a<w.nQueue; ++a)		// insertion sort, one entry at a time
							{
								const u32* src = w.queue + 4*(u64)a;
								const u32 k0 = ldu( &src[0]), k1 = ldu( &src[1]), k2 = ldu( &src[2]), k3 = ldu( &src[3]);
								u32 b = a;
								while (b > groupStart && ldu( &w.queue[ 4*(u64)(b-1)+1]) > k1)
								{
									u32* dst = w.queue + 4*(u64)b; const u32* s2 = w.queue + 4*(u64)(b-1);
									const u32 m0 = ldu( &s2[0]), m1 = ldu( &s2[1]), m2 = ldu( &s2[2]), m3 = ldu( &s2[3]);
									dst[0] = m0; dst[1] = m1; dst[2] = m2; dst[3] = m3;
									--b;
								}
								u32* dst = w.queue + 4*(u64)b;
								dst[0] = k0; dst[1] = k1; dst[2] = k2; dst[3] = k3;
							}
						}
						__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront");
					}
				}

			}
			prevctx = ctx;
		};
		for (u32 k=0; k<inTile && !w.err; ++k) step( std::false_type(), k);
		if (withEnd && tile + 64 > to && !w.err) step( std::true_type(), inTile);
	}
	};
	if (CH && segBeg)
	{
		const u32 q = segBeg > (u32)WARM ? segBeg - (u32)WARM : 0u;
		const u64 carry0 = (CP && P.ucp) ? wordCarryAt( P, w.doc, len, q) : 0ull;
		u64 F[ PASSES];
#pragma unroll
		for (int p=0; p<PASSES; ++p) state[ p] = ~0ull;
		wcarry = carry0;
		runRange( std::false_type(), std::false_type(), q, segBeg, false);
#pragma unroll
		for (int p=0; p<PASSES; ++p) { F[ p] = state[ p]; state[ p] = 0; }
		prevctx = q ? ctxAt<CP>( P, w.doc, len, (long)q - 1) : (int)CTX_EDGE;
		wcarry = carry0;
		runRange( std::false_type(), std::true_type(), q, segBeg, false);
		if (q)
		{
			u64 bad = 0;
#pragma unroll
			for (int p=0; p<PASSES; ++p) bad |= F[ p] & ~state[ p];
			if (__ballot( bad != 0)) { w.err = L1D_CHUNK_UNPROVEN; return; }
		}
	}
	if (CH) runRange( std::true_type(), std::true_type(), segBeg, segEnd, segEnd == len);
	else runRange( std::true_type(), std::true_type(), 0u, len, true);		// (the whole document: constants for the plain instance)
}

// SCAN: automaton over the bytes of a unit (a document, or a chunk of a long one), raw reports into the unit's slice of the
// report queue.  All sets of instances are launched, the ones that are not meant for the batch leave at once.
template <int PASSES, bool LDS, bool CP, bool CH>
__device__ void scanDocuments( const L1Params& P)
{
	// three sets of instances: plain (no classes by code point, no chunked document in the batch), chunks, classes by code point (+ chunks)
	const u32 chunked = ldu( (const u32*)&P.counters[ L1C_CHUNKED]);
	// (the sequential pass is launched on the _ch instance only and runs whatever the batch looks like: the lane-per-stream
	//  kernel cuts every unit into pieces, chunked batch or not)
	if (CP != (P.cpBlocks != 0 || P.nofNullable != 0) || (!CP && !P.sequentialPass && CH != (chunked != 0))) return;
	LexTab<LDS> T;
	stageTables( P, T);
	LexWave w;
	w.events = 0; w.nEvents = 0; w.cnt = 0; w.tailPos = 0; w.tailEnd = 0;
	const u32 nunits = P.sequentialPass ? P.ndocs : ldu( (const u32*)&P.counters[ L1C_UNITS]);
	// the loop is bounded so that it ends whatever the cursor holds
	for (u32 round=0; round<=nunits; ++round)
	{
		// every unit comes from the device-side cursor (a workgroup that only becomes resident when others have
		// finished finds it exhausted and leaves at once: no document waits for a particular wave)
		u32 unit = 0;
		if (LANE == 0) unit = atomicAdd( (u32*)&P.counters[ P.sequentialPass ? L1C_CURSOR3 : L1C_CURSOR], 1u);
		unit = uni( unit);
		if (unit >= nunits) break;
		u32 doc = unit, u0 = unit, u1 = unit + 1;
		if (CH && P.sequentialPass)
		{
			// the re-scan of the documents whose chunks could not be joined: in one piece, into the slices of all its units
			if (ldu( &P.docSequential[ doc]) == 0) continue;
			if (LANE == 0) atomicAdd( (unsigned long long*)&P.counters[ L1C_SEQDOCS], 1ull);
			u0 = ldu( &P.unitStart[ doc]); u1 = ldu( &P.unitStart[ doc+1]);
		}
		else if (CH && chunked)
		{
			u32 lo = 0, hi = P.ndocs;			// last document whose first unit is <= unit
			while (hi - lo > 1u) { const u32 mid = (lo + hi) >> 1; if (ldu( &P.unitStart[ mid]) <= unit) lo = mid; else hi = mid; }
			doc = lo;
		}
		u64 beg, end;
		docBounds( P, doc, beg, end);
		w.doc = P.text + beg; w.docLen = (u32)(end - beg);
		u32 segBeg = 0, segEnd = w.docLen;
		if (CH && chunked && !P.sequentialPass)
		{
			segBeg = (unit - ldu( &P.unitStart[ doc])) * P.chunkBytes;
			segEnd = (w.docLen - segBeg) < P.chunkBytes ? w.docLen : segBeg + P.chunkBytes;
		}
		const u64 qb = queueBase( P, beg + segBeg, u0);
		w.queue = P.reportQueue + 4*qb;
		w.queueCap = (u32)(queueBase( P, beg + segEnd, u1) - qb);
		w.nQueue = 0; w.err = 0;
		scanDocument<PASSES,LDS,CP,CH>( w, P, T, segBeg, segEnd);
		if (LANE == 0)
		{
			if (w.err == L1D_CHUNK_UNPROVEN) { P.docSequential[ doc] = 1; P.reportCount[ u0] = 0; }
			else
			{
				// (the re-scan replaces what the proven units of its document left in the first pass: their records leave the count of
				//  raw reports with them, or the batch would count such a document once per pass)
				u32 replaced = 0;
				if (CH && P.sequentialPass) for (u32 u=u0; u<u1; ++u) replaced += P.reportCount[ u];
				P.reportCount[ u0] = w.err ? 0u : w.nQueue;
				for (u32 u=u0+1; u<u1; ++u) P.reportCount[ u] = 0;
				// (the sequential pass decides alone about its document: a chunk of the first pass may have left an error behind)
				if (w.err || P.sequentialPass) P.docStatus[ doc] = (int32_t)w.err;
				if (w.err == L1D_ERR_ARENA) atomicAdd( (unsigned long long*)&P.counters[ L1C_OVER_QUEUE], 1ull);
				atomicAdd( (unsigned long long*)&P.counters[ L1C_RAW], (unsigned long long)(w.err ? 0u : w.nQueue) - (unsigned long long)replaced);
			}
		}
	}
}

} // anonymous namespace

// One scan instance per pass count (the per-pass rows of a byte step live in registers, so the count is a
// template parameter).
// (a second set, _cp, for batches with classes by code point -- \\p{..} sets, UCP -- or with documents scanned in chunks: the
// plain set pays nothing for either)
#define SPA_L1_KERNEL( NAME, N, T) \
extern "C" __global__ __launch_bounds__(T) void spa_l1_scan_kernel_##NAME( L1Params P) { if (P.ldsWords) scanDocuments<N,true,false,false>( P); else scanDocuments<N,false,false,false>( P); } \
extern "C" __global__ __launch_bounds__(T) void spa_l1_scan_kernel_##NAME##_ch( L1Params P) { if (P.ldsWords) scanDocuments<N,true,false,true>( P); else scanDocuments<N,false,false,true>( P); } \
extern "C" __global__ __launch_bounds__(T) void spa_l1_scan_kernel_##NAME##_cp( L1Params P) { if (P.ldsWords) scanDocuments<N,true,true,true>( P); else scanDocuments<N,false,true,true>( P); }

// ---- host part: the table entry of an instance, filled in by the file that defines its kernels
namespace spa {
typedef const void* L1Kernel;
// The scan instances: `plain` for batches of whole documents, `ch` for batches with documents scanned in chunks and for the
// sequential re-scan, `cp` for tables with classes by code point or empty matches.
struct ScanInstance { unsigned passes; L1Kernel plain, ch, cp; unsigned maxThreads; const char* name; };
#define SPA_L1_SCAN_INSTANCE( N, T) { N, (L1Kernel)spa_l1_scan_kernel_p##N, (L1Kernel)spa_l1_scan_kernel_p##N##_ch, (L1Kernel)spa_l1_scan_kernel_p##N##_cp, T, "spa_l1_scan_kernel_p" #N }
extern const ScanInstance g_scanInstancesP1[ 4];	// 1..4 passes (l1_scan_kernel_p1_4.hip)
extern const ScanInstance g_scanInstancesP5[ 4];	// 5..8 passes (l1_scan_kernel_p5_8.hip)
extern const ScanInstance g_scanInstanceP16;		// up to 16 passes (l1_scan_kernel.hip)
extern const ScanInstance g_scanInstanceP32;		// up to 32 passes (l1_scan_kernel_p32.hip)
} // namespace
#endif
