// Host side of a rule-matcher launch that needs no device: the environment switches, the arena policy, which kernel serves a
// rule set, the flat tier's layout and the launch plan of a batch (grids, capacities, allocation sizes).  No HIP function is
// called in here (hip_runtime_api.h comes in through l2_device.h for its types only): a plain C++ compiler builds l2_plan.cpp.
#ifndef SPA_L2_PLAN_HPP
#define SPA_L2_PLAN_HPP
#include <stdint.h>
#include <cstddef>
#include <string>
#include <vector>
#include "l2_compile.hpp"
#include "l2_device.h"
#include "l2_fast.h"
#include "l2_join.h"

namespace spa {

// The SPA_L2_* switches (tests and A/B runs).  fromEnv() is the one place of the rule matcher that reads the environment; a
// context reads them when it is created and keeps them.
struct L2Switches
{
	bool fast = true;		// SPA_L2_FAST: off when the value starts with 0 (everything stays on the general kernel)
	char fastSize = 0;		// SPA_L2_FAST_SIZE: the letter of the kernel instance (fastVariantNamed, l2_fast_kernel.hip); 0 = default
	uint32_t fastMaxRules = 2048;	// SPA_L2_FAST_MAXRULES: rule ids of a document on the flat tier (LDS + spill area)
	uint32_t fastMaxStaged = 32768;	// SPA_L2_FAST_MAXSTAGED: staged results of a document on the flat tier
	bool join = false;		// SPA_L2_JOIN=1: every context is created with SP_CTX_RESULT_SETS
	bool verbose = false;		// SPA_L2_VERBOSE: engine choice, arena and spill sizes, hand-overs on stderr
	static L2Switches fromEnv();
};

// ---- the per-wave arena of the general kernel (ArenaLayout, l2_device.h)
// small defaults (a document's hot state should stay cache and TLB friendly); every capacity doubles when a document
// overflows it (SP_DOC_ERR_ARENA -> growArena -> rerun)
ArenaLayout initialArena();
// the offsets and totalWords that follow from the capacities
void layoutArena( ArenaLayout& L);
// sp_matcher_ctx_set_arena: 0 keeps a capacity
void setArena( ArenaLayout& L, uint32_t maxRules, uint32_t maxTrigs, uint32_t bucketCap, uint32_t maxItems, uint32_t maxFollow);
// doubles every capacity; false (nothing changed) when the arena is at its maximum size
bool growArena( ArenaLayout& L);

// Waves of a per-wave arena of `perWaveBytes`.  `run`: the waves of this launch, as many as wanted while the arena stays
// below ~48 GiB (fewer resident waves when documents need a large working set; never fewer than 4, a multiple of `multiple` when cut).
// `alloc`: the waves to allocate when the arena has to grow: batches of 64 waves and more get the arena of the full machine (`fullSlots`
// waves) at once; a context that sees single documents (the plugin path: one context per host thread) keeps a small one -- gigabytes less.
struct ArenaWaves { unsigned run, alloc; };
ArenaWaves arenaWaves( size_t perWaveBytes, unsigned wanted, size_t fullSlots, unsigned multiple);

// ---- which kernel serves a rule set, and why not the others; the tables of the ones that do
enum L2EngineKind {L2_GENERAL=0, L2_FLAT=1, L2_JOIN=2};		// = sp_matcher_ctx_kernel_kind
struct L2Engine
{
	struct Flat
	{
		bool on = false;
		std::string whyNot;
		std::vector<FastKeyInst> keyinst;	// never empty when on
		std::vector<FastStatic> statics;
		uint32_t maxRules = 0, maxStaged = 0;
	} flat;
	struct Join
	{
		bool asked = false, on = false;		// asked: SP_CTX_RESULT_SETS or SPA_L2_JOIN=1
		std::string whyNot;
		std::vector<JoinKey> keytab; std::vector<JoinRule> rules; std::vector<uint32_t> filter;
		uint32_t maxRange = 0, delimiter = 0;
	} join;
	uint32_t altPrograms = 0;			// join: programs whose key the optimizer moved
	L2EngineKind kind() const	{return join.on ? L2_JOIN : flat.on ? L2_FLAT : L2_GENERAL;}
};
L2Engine chooseL2Engine( const RuleCompiler& compiler, const FlatTables& ft, uint32_t ctxFlags, const L2Switches& sw);

// ---- the flat tier's kernel instance and per-wave layout, fixed when a context is created.  R, T and the name come from the
// kernel table of l2_fast_kernel.hip (fastCapacities, fastKernelName), the only statement of them.
struct FlatPlan
{
	unsigned variant = 0;
	const char* kernelName = "(none)";
	uint32_t R = 0, T = 0;
	FastSpillLayout spill = {};
	uint32_t bucketMeta[ 16] = {};
	uint32_t expShift = 0;
};
FlatPlan planFlat( const L2Engine::Flat& flat, unsigned variant, const char* kernelName, uint32_t R, uint32_t T);

// name of the kernel that does the work of a context's batches
const char* l2KernelName( L2EngineKind kind, const FlatPlan* flat);

// ---- everything a launch decides, decided once
#ifndef SPA_L2_WAVES_PER_CU
#define SPA_L2_WAVES_PER_CU 12		// (a build variant may state another: tests/micro/sweep_l2_occ.sh)
#endif
enum {
	L2_WAVES_PER_CU=SPA_L2_WAVES_PER_CU,	// general kernel: one wave per workgroup, as many as keep every CU busy
	L2_JOIN_WAVES_PER_CU=32,	// join kernel: one wave per document, no LDS, few registers
	L2_LIST_BLOCKS_PER_CU=2		// general kernel behind the flat one: the few documents handed over
};
enum L2Route {L2_ROUTE_GENERAL, L2_ROUTE_FLAT_LIST /*flat kernel, then the general one in list mode*/, L2_ROUTE_JOIN, L2_ROUTE_RERUN_LIST};
struct L2LaunchPlan
{
	L2Route route = L2_ROUTE_GENERAL;
	const char* kernelName = "(none)";
	// the general kernel's arena (allocated for every engine)
	ArenaLayout layout;			// laid out: what the kernel gets
	ArenaWaves arena = {1, 1};
	unsigned generalBlocks = 1;		// = arena.run
	size_t arenaPerWaveBytes = 0;
	unsigned arenaAllocWaves = 1;		// when the arena holds fewer than arena.run waves (a rerun: what it runs)
	// flat tier
	unsigned fastBlocks = 0;
	uint64_t spillAllocWaves = 0;		// when the spill area holds fewer than fastBlocks waves (single documents: a small one, see the arena)
	size_t spillPerWaveBytes = 0;
	unsigned listBlocks = 0;
	unsigned joinBlocks = 0;
	// output capacity, sized from the input (grown by the caller on SP_DOC_ERR_OUTPUT); the buffers are grow-only
	uint64_t wantResults = 0, wantItems = 0;
};
// `docsToRun`: the documents of a rerun, else ndocs.  Throws std::runtime_error for a batch of too many documents.
L2LaunchPlan planL2Launch( L2EngineKind kind, bool rerun, unsigned numCUs, unsigned fastBlocksPerCU, size_t docsToRun, size_t ndocs, size_t nlexems,
			   const ArenaLayout& arena, const FlatPlan* flat, uint64_t minResults, uint64_t minItems);

} // namespace
#endif
