// Launch parameters of the level-2 kernels: the batch contract all three share, and the general kernel's (l2_kernel.hip).
#ifndef SPA_L2_DEVICE_H
#define SPA_L2_DEVICE_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>
#include "l2_tables.h"
#if defined(__HIPCC__)
#include "wave_scan.h"
#endif

namespace spa {

// per-document status codes (= SP_DOC_* of include/strus_pattern_amd.h)
enum {SPD_OK=0, SPD_ERR_ORDER=1, SPD_ERR_ARENA=2, SPD_ERR_KEYTRIGGERS=3, SPD_ERR_PASTFOLLOW=4, SPD_ERR_RANGE=5, SPD_ERR_DATAREF=6, SPD_ERR_LEXEMSIZE=7, SPD_ERR_INTERNAL=8, SPD_ERR_OUTPUT=9};
// counters[]
enum {SPC_RESULTS=0, SPC_ITEMS=1, SPC_EVENTS=2, SPC_FAILED=3, SPC_HANDOVER=4 /*documents the fast tier handed to the general kernel*/, SPC_COUNT=8};

// Per-wave arena: mutable state of the document a wavefront is working on.  Capacities in
// records, offsets in u32 words from the arena base.  Record sizes: rule 12 words, trigger 8,
// item 12, follow 12, stop-log 12, staged result 8, data reference 2, heap entry 2.
struct ArenaLayout
{
	uint32_t maxRules, maxTrigs, bucketCap, maxItems, maxRefs, maxFollow, maxDispose, maxHeap, maxGStack, maxStaged, nStop, winCap, scratchCap, winChunk, winChunks;
	uint32_t oRules, oTrigs, oBEvent, oBIdx, oBSize, oWindow, oHeap, oFollow, oDispose, oStop, oItems, oRefs, oGStack, oStaged, oRuleFree, oTrigFree, oItemFree, oRefFree, oWinArr, oScratch, oWinChunk, oWinFree;
	uint32_t totalWords;
};

// The batch contract of the three rule kernels (l2_kernel.hip, l2_fast_kernel.hip, l2_join_kernel.hip): the input they
// read and the output they all write in the same format.  The host fills one (capi_l2.cpp, batchIO) for whichever runs.
struct L2BatchIO
{
	// input
	const uint32_t* lexems;		// sp_lexem_t[]: id, ordpos, origpos, origsize
	const uint32_t* origseg;	// optional
	const uint64_t* docOffsets;	// ndocs+1 lexem indices, or NULL when docRangesIn is given
	const uint64_t* docRangesIn;	// ndocs x (first lexem, count): the lexer kernel's output layout
	uint32_t* docCursor;
	// output
	uint64_t* counters;		// SPC_*
	uint32_t* results;		// sp_result_t[resultCapacity] (9 words each)
	uint64_t resultCapacity;
	uint32_t* items;		// sp_result_item_t[itemCapacity] (7 words each)
	uint64_t itemCapacity;
	uint64_t* docRange;		// ndocs x (first result, count)
	uint64_t* docStats;		// ndocs x 4
	int32_t* docStatus;		// ndocs
	uint32_t* resultFormat;		// [resultCapacity] format handle of the result (0 = none), if withFormats
	uint32_t* itemFormat;		// [itemCapacity] x {format handle, records of the item's subtree that follow it}, if withFormats
	uint32_t ndocs;
	uint32_t withItems;
	uint32_t withFormats;		// patterns with format strings
};

struct L2Params
{
	// compiled tables (read only)
	const DevProgram* programs;
	const DevTrigDef* trigdefs;
	const DevKeyEntry* keytab;
	const DevKeyRef* keylist;
	uint32_t keymask;
	uint32_t nofStopWords;
	L2BatchIO io;
	// working memory
	uint32_t* arenaBase;
	ArenaLayout arena;
	// list mode: the documents docList[0 .. *docListCount) instead of 0..ndocs (documents the fast tier handed
	// over, l2_fast.h); the output counters continue where the fast kernel left them
	const uint32_t* docList;
	const uint32_t* docListCount;
};

// enqueue the general kernel (l2_kernel.hip): one wave per workgroup
hipError_t launchL2Match( const L2Params& P, unsigned nblocks, hipStream_t stream);

#if defined(__HIPCC__)
// ---- the per-document prologue and epilogue of the batch contract (IO: L2BatchIO in whatever address space the
// kernel reads its parameters from)

// the document's lexems [lbeg, lend), wave-uniform
template <class IO>
__device__ __forceinline__ void docLexems( const IO& io, u32 doc, u64& lbeg, u64& lend)
{
	if (io.docRangesIn)
	{
		const u32* rp = (const u32*)&io.docRangesIn[ 2*(u64)doc];
		lbeg = ((u64)ldu( rp+1) << 32) | ldu( rp);
		lend = lbeg + (((u64)ldu( rp+3) << 32) | ldu( rp+2));
	}
	else
	{
		lbeg = ((u64)ldu( (const u32*)&io.docOffsets[ doc]+1) << 32) | ldu( (const u32*)&io.docOffsets[ doc]);
		lend = ((u64)ldu( (const u32*)&io.docOffsets[ doc+1]+1) << 32) | ldu( (const u32*)&io.docOffsets[ doc+1]);
	}
}

// reserves n output records (n wave-uniform) of kind c (SPC_RESULTS or SPC_ITEMS) by adding to their counter: the first
// one's index in `base`; false when the range ends beyond the buffer (the caller fails the document with SPD_ERR_OUTPUT;
// the counter has moved on all the same)
template <class IO>
__device__ __forceinline__ bool reserveOutput( const IO& io, u32 c, u64 n, u64& base)
{
	u64 b = 0;
	if (LANE == 0) b = atomicAdd( (unsigned long long*)&io.counters[ c], (unsigned long long)n);
	base = ((u64)uni( (u32)(b >> 32)) << 32) | uni( (u32)b);
	return base + n <= (c == SPC_RESULTS ? io.resultCapacity : io.itemCapacity);		// (read after the atomic: not live across it)
}

// the document's result range, statistics and status; `events` is what the document adds to SPC_EVENTS
template <class IO>
__device__ __forceinline__ void finishDocument( const IO& io, u32 doc, u64 resBase, u64 nres, u64 st0, u64 st1, u64 st2, u64 st3, u32 err, u64 events)
{
	if (LANE == 0)
	{
		io.docRange[ 2*(u64)doc] = resBase; io.docRange[ 2*(u64)doc+1] = nres;
		u64* st = io.docStats + 4*(u64)doc;
		st[0] = st0; st[1] = st1; st[2] = st2; st[3] = st3;
		io.docStatus[ doc] = (int32_t)err;
		atomicAdd( (unsigned long long*)&io.counters[ SPC_EVENTS], (unsigned long long)events);
		if (err) atomicAdd( (unsigned long long*)&io.counters[ SPC_FAILED], 1ull);
	}
}
#endif

} // namespace
#endif
