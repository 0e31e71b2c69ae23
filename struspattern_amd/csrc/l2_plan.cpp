// Switches, arena policy, engine choice and launch plan of the level-2 rule matcher (l2_plan.hpp): host only, no device needed.
#include "l2_plan.hpp"
#include "../../include/strus_pattern_amd.h"
#include <cstdlib>
#include <cstring>
#include <stdexcept>

namespace spa {

L2Switches L2Switches::fromEnv()
{
	L2Switches sw;
	if (const char* e = getenv( "SPA_L2_FAST")) sw.fast = e[ 0] != '0';
	if (const char* e = getenv( "SPA_L2_FAST_SIZE")) sw.fastSize = e[ 0];
	if (const char* e = getenv( "SPA_L2_FAST_MAXRULES")) sw.fastMaxRules = (uint32_t)atoi( e);
	if (const char* e = getenv( "SPA_L2_FAST_MAXSTAGED")) sw.fastMaxStaged = (uint32_t)atoi( e);
	if (const char* e = getenv( "SPA_L2_JOIN")) sw.join = e[ 0] == '1';
	sw.verbose = getenv( "SPA_L2_VERBOSE") != 0;
	return sw;
}

// ------------------------------------------------------------------ arena
static uint32_t alignUp( uint32_t v, uint32_t a) { return (v + a-1) / a * a; }

ArenaLayout initialArena()
{
	ArenaLayout a;
	std::memset( &a, 0, sizeof(a));
	a.maxRules = 1024; a.maxTrigs = 1024; a.bucketCap = 256; a.maxItems = 2048;
	a.maxRefs = 1024; a.maxFollow = 256; a.maxDispose = 512; a.maxHeap = 256;
	a.maxGStack = 64; a.maxStaged = 1024; a.winCap = 128; a.scratchCap = 256;
	return a;
}

void layoutArena( ArenaLayout& L)
{
	uint32_t o = 0;
	L.oRules = o;	o += L.maxRules*32;			// 128-byte blocks: rule + its 4 trigger slots
	L.oTrigs = 0; L.oBIdx = 0; L.oTrigFree = 0;		// (unused: triggers live in the rule blocks)
	L.oBEvent = o;	o += alignUp( 2*16*L.bucketCap, 32);	// {event, trigger id} pairs
	L.oBSize = o;	o += 16;
	L.oWindow = o;	o += 64;
	L.oHeap = o;	o += alignUp( L.maxHeap*2, 4);
	L.oFollow = o;	o += alignUp( L.maxFollow*12, 4);
	L.oDispose = o;	o += alignUp( L.maxDispose, 4);
	L.oStop = o;	o += alignUp( (L.nStop?L.nStop:1)*12, 4);
	L.oItems = o;	o += alignUp( L.maxItems*12, 4);
	L.oRefs = o;	o += alignUp( L.maxRefs*2, 4);
	L.oGStack = o;	o += alignUp( L.maxGStack, 4);
	L.oStaged = o;	o += alignUp( L.maxStaged*8, 4);
	L.oRuleFree = o; o += alignUp( L.maxRules, 4);
	L.oItemFree = o; o += alignUp( L.maxItems, 4);
	L.oRefFree = o;	o += alignUp( L.maxRefs, 4);
	// expiry window: lists of up to 8 chunks per position; the pool covers every live rule plus one
	// partly filled chunk per position
	L.winChunk = L.winCap/8 < 16 ? 16 : L.winCap/8;
	L.winChunks = L.maxRules/L.winChunk + 64;
	L.oWinArr = o;	o += alignUp( L.winChunks*L.winChunk, 4);
	L.oWinChunk = o; o += 64*8;
	L.oWinFree = o;	o += alignUp( L.winChunks, 4);
	L.oScratch = o;	o += alignUp( 16*L.scratchCap, 4);
	L.totalWords = alignUp( o, 64);
}

void setArena( ArenaLayout& L, uint32_t maxRules, uint32_t maxTrigs, uint32_t bucketCap, uint32_t maxItems, uint32_t maxFollow)
{
	if (maxRules) { L.maxRules = maxRules; L.maxHeap = maxRules; L.maxDispose = maxRules; L.winCap = maxRules/4 < 64 ? 64 : maxRules/4; }
	if (maxTrigs) L.maxTrigs = maxTrigs;
	if (bucketCap) L.bucketCap = bucketCap;
	if (maxItems) { L.maxItems = maxItems; L.maxRefs = maxItems; }
	if (maxFollow) L.maxFollow = maxFollow;
}

bool growArena( ArenaLayout& L)
{
	if (L.maxRules >= (1u<<20)) return false;
	L.maxRules *= 2; L.maxTrigs *= 2; L.bucketCap *= 2; L.maxItems *= 2;
	L.maxRefs *= 2; L.maxFollow *= 2; L.maxDispose *= 2; L.maxHeap *= 2;
	L.maxStaged *= 2; L.maxGStack *= 2; L.winCap *= 2;
	if (L.scratchCap < 256) L.scratchCap = 256;
	return true;
}

ArenaWaves arenaWaves( size_t perWaveBytes, unsigned wanted, size_t fullSlots, unsigned multiple)
{
	const size_t fit = ((size_t)48 << 30) / perWaveBytes;
	const size_t maxRun = fit < 4 ? 4 : fit;
	const size_t full = fullSlots < fit ? fullSlots : fit;
	ArenaWaves w;
	w.run = wanted > maxRun ? (unsigned)(maxRun / multiple * multiple) : wanted;
	w.alloc = (w.run >= 64 && w.run < full) ? (unsigned)full : w.run;
	return w;
}

// ------------------------------------------------------------------ engine
L2Engine chooseL2Engine( const RuleCompiler& compiler, const FlatTables& ft, uint32_t ctxFlags, const L2Switches& sw)
{
	L2Engine e;
	// flat tier: eligible rule sets get the one-line-per-install table (SPA_L2_FAST=0 keeps everything on the general kernel)
	e.flat.whyNot = buildFastTables( ft, e.flat.keyinst, &e.flat.statics);
	if (!sw.fast) e.flat.whyNot = "disabled by SPA_L2_FAST=0";
	e.flat.on = e.flat.whyNot.empty();
	if (e.flat.on && e.flat.keyinst.empty()) e.flat.keyinst.resize( 1);
	e.flat.maxRules = sw.fastMaxRules > 4095 ? 4095 : sw.fastMaxRules;	// trigger ids are 14 bits (rule << 2 | slot)
	e.flat.maxStaged = sw.fastMaxStaged;
	// result-set mode: asked for by the flag, or for every context by SPA_L2_JOIN=1; ineligible rule sets stay on the
	// exact engine, whose results are a correct multiset too
	e.join.asked = (ctxFlags & SP_CTX_RESULT_SETS) != 0 || sw.join;
	if (!e.join.asked) e.join.whyNot = "result sets not asked for";
	// (`exclusive` drops the results covered by another one in a scan that follows the order of the results)
	else if (compiler.exclusive()) e.join.whyNot = "the `exclusive` option (its outcome depends on the order of the results)";
	else e.join.whyNot = buildJoinTables( ft, e.join.keytab, e.join.rules, e.join.filter, e.join.maxRange, e.join.delimiter, e.altPrograms);
	e.join.on = e.join.whyNot.empty();
	if (!e.join.on) e.altPrograms = 0;
	return e;
}

FlatPlan planFlat( const L2Engine::Flat& flat, unsigned variant, const char* kernelName, uint32_t R, uint32_t T)
{
	FlatPlan p;
	p.variant = variant; p.kernelName = kernelName; p.R = R; p.T = T;
	layoutFast( p.spill, p.bucketMeta, p.expShift, flat.keyinst, R, T, flat.maxRules, flat.maxStaged);
	return p;
}

const char* l2KernelName( L2EngineKind kind, const FlatPlan* flat)
{
	return kind == L2_JOIN ? "spa_l2_join_kernel" : kind == L2_FLAT ? flat->kernelName : "spa_l2_match_kernel";
}

// ------------------------------------------------------------------ launch
L2LaunchPlan planL2Launch( L2EngineKind kind, bool rerun, unsigned numCUs, unsigned fastBlocksPerCU, size_t docsToRun, size_t ndocs, size_t nlexems,
			   const ArenaLayout& arena, const FlatPlan* flat, uint64_t minResults, uint64_t minItems)
{
	if (ndocs >= 0xFFFFFFFFull) throw std::runtime_error( "too many documents in one batch");
	auto blocksFor = []( size_t docs, size_t slots) { return (unsigned)(docs < slots ? (docs ? docs : 1) : slots); };	// never more waves than documents
	L2LaunchPlan p;
	p.route = rerun ? L2_ROUTE_RERUN_LIST : kind == L2_JOIN ? L2_ROUTE_JOIN : kind == L2_FLAT ? L2_ROUTE_FLAT_LIST : L2_ROUTE_GENERAL;
	p.kernelName = l2KernelName( kind, flat);
	const size_t waveSlots = (size_t)numCUs * L2_WAVES_PER_CU;
	p.layout = arena;
	layoutArena( p.layout);
	p.arenaPerWaveBytes = (size_t)p.layout.totalWords * sizeof(uint32_t);
	p.arena = arenaWaves( p.arenaPerWaveBytes, blocksFor( docsToRun, waveSlots), waveSlots, 1);
	p.generalBlocks = p.arena.run;
	p.arenaAllocWaves = rerun ? p.arena.run : p.arena.alloc;
	if (p.route == L2_ROUTE_FLAT_LIST)
	{
		const size_t fslots = (size_t)numCUs * fastBlocksPerCU;
		p.fastBlocks = blocksFor( ndocs, fslots);
		p.spillAllocWaves = p.fastBlocks >= 64 ? fslots : p.fastBlocks;
		p.spillPerWaveBytes = (size_t)flat->spill.totalWords * sizeof(uint32_t);
		const unsigned listSlots = L2_LIST_BLOCKS_PER_CU * numCUs;
		p.listBlocks = p.generalBlocks < listSlots ? p.generalBlocks : listSlots;
	}
	if (p.route == L2_ROUTE_JOIN) p.joinBlocks = blocksFor( ndocs, (size_t)numCUs * L2_JOIN_WAVES_PER_CU);
	// item indices in a result record are 32 bit: a batch that needs more fails with SP_DOC_ERR_OUTPUT instead of wrapping
	auto want = []( uint64_t fromInput, uint64_t reserved) { const uint64_t n = fromInput < reserved ? reserved : fromInput; return n > 0xFFFFFFFFull ? 0xFFFFFFFFull : n; };
	p.wantResults = want( (uint64_t)nlexems*2 + 1024, minResults);
	p.wantItems = want( (uint64_t)nlexems*6 + 1024, minItems);
	return p;
}

} // namespace
