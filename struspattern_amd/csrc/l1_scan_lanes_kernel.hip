// Scan kernel of the lexer with a lane per stream (stage 1 of l1_wave.h for tables of a few automaton words).
#include "l1_wave.h"
#include "l1_launch.h"

namespace {

// ---------------------------------------------------------------- scan, a lane per stream (round 3)
// When what is left to scan fits a few automaton words (the literals and the word shapes are found by the words kernel: of the
// 10 001 expressions of the benchmark set five are left, 17 positions), a wave that steps through ONE byte per instruction
// stream wastes its lanes.  Here the unit is cut into 64 pieces and every lane runs the whole (small) automaton over its own
// piece: 64 bytes per step of the wave.  The state at the start of a piece comes from the same warm-up proof the chunks of a
// long document use (F inside S, scanDocument); a lane whose proof fails sends the document to the sequential re-scan.  The
// reports of a lane go to the lane's part of the unit's queue slice and are moved together at the end (lane order = offset order).
__shared__ unsigned short laneCc[ 256];		// byte -> class | context << 8
#ifndef SPA_L1_LANE_PARK
#define SPA_L1_LANE_PARK 4
#endif
enum {LANE_PARK=SPA_L1_LANE_PARK};		// 16-byte blocks of a lane's piece parked per refill (8 = a whole 128-byte line: 33 KB per workgroup, 8 waves per CU beside the table image; 4: 16 waves)
__shared__ uint4 laneText[ 4][ LANE_PARK*64];		// per wave: the next bytes of every lane's piece of the text
template <int W>
__device__ __forceinline__ void scanUnitLanes( LexWave& w, const L1Params& P, const LexTab<true>& T, const u32 segBeg, const u32 segEnd)
{
#ifndef SPA_L1_LANE_WARM
#define SPA_L1_LANE_WARM 256
#endif
	enum {WARM=SPA_L1_LANE_WARM};
	const u32 len = w.docLen;
	const u32 nofClasses = uni( P.nofClasses), maxEx = uni( P.maxExceptions), nEx = uni( P.exCount[ 0]);
	const u32 span = segEnd - segBeg;
	const u32 per = (((span + 63u) >> 6) + 15u) & ~15u;		// bytes per lane, a multiple of 16
	u32 b0 = segBeg + LANE*per; if (b0 > segEnd) b0 = segEnd;
	u32 b1 = b0 + per; if (b1 > segEnd) b1 = segEnd;
	u64 shiftDst[ W], selfLoop[ W];
#pragma unroll
	for (int x=0; x<W; ++x) { shiftDst[ x] = T.at( T.oShift + x); selfLoop[ x] = T.at( T.oSelf + x); }
	auto stepWords = [&]( u64* st, u32 cls, u32 prevctx, bool inject)
	{
#pragma unroll
		for (int x=0; x<W; ++x)
		{
			const u64 s0 = st[ x];
			u64 nxt = ((s0 << 1) & shiftDst[ x]) | (s0 & selfLoop[ x]) | (inject ? T.at( T.oStart + prevctx*64 + x) : 0ull);
			for (u32 e=0; e<nEx; ++e)
			{
				const u64 es = T.at( T.oExSrc + e*64 + x), ed = T.at( T.oExDst + e*64 + x);
				nxt |= (s0 & es) ? ed : 0ull;
			}
			st[ x] = nxt & T.at( cls*64 + x);
		}
	};
	u64 S[ W];
#pragma unroll
	for (int x=0; x<W; ++x) S[ x] = 0;
	u32 prevctx = (u32)CTX_EDGE;
	bool unproven = false;
	if (b0 < b1 && b0 > 0)
	{
		// warm-up over the bytes before my piece: F from "every position live" without starts, S from nothing with starts
		const u32 q = b0 > (u32)WARM ? b0 - (u32)WARM : 0u;
		u64 F[ W];
#pragma unroll
		for (int x=0; x<W; ++x) F[ x] = ~0ull;
		prevctx = q ? ((u32)laneCc[ w.doc[ q-1]] >> 8) : (u32)CTX_EDGE;
		// (16 bytes per load: a byte per load was 256 dependent global loads per lane)
#pragma unroll 1
		for (u32 i=q; i<b0; i+=16)
		{
			uint4 v = make_uint4( 0,0,0,0);
			if (i + 16u <= len) v = ld128u( w.doc + i);
			else
			{
				// (the document's last bytes: one at a time through the lane's parking place, nothing is read behind the text)
				uint4* pk = laneText[ threadIdx.x >> 6] + LANE;
				pk[ 0] = make_uint4( 0,0,0,0);
				for (u32 k=0; k<16u && i+k<len; ++k) ((unsigned char*)pk)[ k] = w.doc[ i+k];
				v = pk[ 0];
			}
#pragma unroll 1
			for (u32 dw=0; dw<4u; ++dw)
			{
				const u32 x = dw == 0 ? v.x : (dw == 1 ? v.y : (dw == 2 ? v.z : v.w));
#pragma unroll
				for (int k=0; k<4; ++k)
				{
					if (i + 4u*dw + (u32)k < b0)
					{
						const u32 cc = laneCc[ (x >> (8*k)) & 0xFFu];
						stepWords( F, cc & 0xFFu, prevctx, false);
						stepWords( S, cc & 0xFFu, prevctx, true);
						prevctx = cc >> 8;
					}
				}
			}
		}
		if (q)
		{
			u64 bad = 0;
#pragma unroll
			for (int x=0; x<W; ++x) bad |= F[ x] & ~S[ x];
			unproven = bad != 0;
		}
	}
	if (__ballot( unproven)) { w.err = L1D_CHUNK_UNPROVEN; return; }
	// my part of the unit's queue slice
	const u32 regionCap = w.queueCap >> 6;
	u32* region = w.queue + 4*(u64)(LANE*regionCap);
	u32 cnt = 0; bool full = false;
	auto emit = [&]( u32 to, const u64* st, u32 ctx)
	{
#pragma unroll
		for (int x=0; x<W; ++x)
		{
			u64 rem = st[ x] & T.at( T.oAccept + ctx*64 + x);
			while (rem)
			{
				const u32 bit = (u32)__builtin_ctzll( rem);
				const u32 pi = P.patOfBit[ (u32)x*64 + bit];
				const uint2 mm = *(const uint2*)&P.patterns[ pi].maskLo;
				const u64 m = ((u64)mm.y << 32) | mm.x;
				if (cnt < regionCap) { *(uint4*)(region + 4*(u64)cnt) = make_uint4( to, pi, (u32)(rem & m), (u32)((rem & m) >> 32)); ++cnt; } else full = true;
				rem &= ~m;
			}
		}
	};
	// 64 bytes of my piece per refill, parked in LDS (a lane's loads are 1 KB apart from its neighbours': read 16 bytes at
	// a time straight from memory, every 128-byte line of the text came in eight times -- 11 GB of traffic for 0.8 GB of text;
	// a whole line per refill is 33 KB of LDS per workgroup and 8 waves per CU: 5.7 ms instead of 4.2 on 805 MB)
	uint4* park = laneText[ threadIdx.x >> 6] + LANE;		// [LANE_PARK][64]: block q of lane l at park[ q*64]
	for (u32 i=b0; i<b1; i+=16u*(u32)LANE_PARK)
	{
#pragma unroll 1
		for (u32 q=0; q<(u32)LANE_PARK; ++q)
		{
			const u32 at = i + 16u*q;
			if (at >= b1) break;
			if (at + 16u <= len) park[ q*64] = ld128u( w.doc + at);
			else
			{
				// (the document's last bytes: one at a time, nothing is read behind the text)
				park[ q*64] = make_uint4( 0,0,0,0);
				for (u32 k=0; k<16u && at+k<len; ++k) ((unsigned char*)&park[ q*64])[ k] = w.doc[ at+k];
			}
		}
#pragma unroll 1
		for (u32 q=0; q<(u32)LANE_PARK && i + 16u*q < b1; ++q)
		{
			const uint4 v = park[ q*64];
			const u32 vv[ 4] = {v.x, v.y, v.z, v.w};
#pragma unroll
			for (int k=0; k<16; ++k)
			{
				const u32 at = i + 16u*q + (u32)k;
				if (at < b1)
				{
					const u32 cc = laneCc[ (vv[ k>>2] >> (8*(k&3))) & 0xFFu];
					emit( at, S, cc >> 8);			// matches that end before this byte
					stepWords( S, cc & 0xFFu, prevctx, true);
					prevctx = cc >> 8;
				}
			}
		}
	}
	// matches that end with the document: by the lane that holds its last byte (an empty document has none)
	if (segEnd == len && b1 == segEnd && b0 < b1) emit( len, S, (u32)CTX_EDGE);
	if (__ballot( full)) { w.err = L1D_ERR_ARENA; return; }
	// ---- the lanes' parts moved together (ascending lanes: a part only moves towards the front)
	const u32 incl = waveScanAdd( cnt);
	const u32 excl = incl - cnt;
	__builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront");
	for (u32 l=1; l<64; ++l)
	{
		const u32 n = (u32)__builtin_amdgcn_readlane( cnt, l);
		if (!n) continue;
		const u32 dst = (u32)__builtin_amdgcn_readlane( excl, l), src = l*regionCap;
		if (dst == src) continue;
		for (u32 k=0; k<n; k+=64)
		{
			uint4 rec = make_uint4( 0,0,0,0);
			if (k + LANE < n) rec = *(const uint4*)(w.queue + 4*(u64)(src + k + LANE));
			__builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront");
			if (k + LANE < n) *(uint4*)(w.queue + 4*(u64)(dst + k + LANE)) = rec;
			__builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront");
		}
	}
	w.nQueue = (u32)__builtin_amdgcn_readlane( incl, 63);
}

template <int W>
__device__ __forceinline__ void scanDocumentsLanes( const L1Params& P)
{
	LexTab<true> T;
	for (u32 k=threadIdx.x; k<256u; k+=blockDim.x) { const u32 cl = P.byteClass[ k]; laneCc[ k] = (unsigned short)(cl | ((u32)P.classCtx[ cl] << 8)); }
	stageTables( P, T);			// (the barrier inside covers laneCc too)
	const u32 chunked = ldu( (const u32*)&P.counters[ L1C_CHUNKED]);
	LexWave w;
	w.events = 0; w.nEvents = 0; w.cnt = 0; w.tailPos = 0; w.tailEnd = 0;
	const u32 nunits = ldu( (const u32*)&P.counters[ L1C_UNITS]);
	for (u32 round=0; round<=nunits; ++round)
	{
		u32 unit = 0;
		if (LANE == 0) unit = atomicAdd( (u32*)&P.counters[ L1C_CURSOR], 1u);
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
		w.queue = P.reportQueue + 4*qb;
		w.queueCap = (u32)(queueBase( P, beg + segEnd, unit + 1) - qb);
		w.nQueue = 0; w.err = 0;
		scanUnitLanes<W>( w, P, T, segBeg, segEnd);
		if (LANE == 0)
		{
			if (w.err == L1D_CHUNK_UNPROVEN) { P.docSequential[ doc] = 1; P.reportCount[ unit] = 0; }
			else
			{
				P.reportCount[ unit] = w.err ? 0u : w.nQueue;
				if (w.err) P.docStatus[ doc] = (int32_t)w.err;
				if (w.err == L1D_ERR_ARENA) atomicAdd( (unsigned long long*)&P.counters[ L1C_OVER_QUEUE], 1ull);
				atomicAdd( (unsigned long long*)&P.counters[ L1C_RAW], (unsigned long long)(w.err ? 0u : w.nQueue));
			}
		}
	}
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l1_scan_lanes_kernel( L1Params P)
{
	if (P.scanWords <= 1) scanDocumentsLanes<1>( P); else if (P.scanWords == 2) scanDocumentsLanes<2>( P); else scanDocumentsLanes<4>( P);
}

namespace spa {
void launchL1ScanLanes( const L1LaunchPlan& plan, const L1Params& PS, hipStream_t stream)
{
	hipLaunchKernelGGL( spa_l1_scan_lanes_kernel, dim3( plan.laneGrid), dim3( 256), plan.scanLdsBytes(), stream, PS);
}
} // namespace
