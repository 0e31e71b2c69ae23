// Stand-alone host program for a sanitizer run of the device-free host layer of the rule matcher (csrc/l2_plan.hpp): builds one
// flat and one nested rule set, chooses their engines and plans the edges of every grid and capacity.  No HIP code is linked:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       -Istruspattern_amd/csrc tests/micro/l2_plan_san.cpp struspattern_amd/csrc/l2_plan.cpp struspattern_amd/csrc/l2_compile.cpp \
//       struspattern_amd/csrc/l2_fast_tables.cpp struspattern_amd/csrc/l2_join_tables.cpp -o l2_plan_san && ./l2_plan_san
#include "l2_plan.hpp"
#include "../../include/strus_pattern_amd.h"
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

using namespace spa;

#define CHECK( COND) do { if (!(COND)) { std::fprintf( stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #COND); std::exit( 1); } } while (0)

static void flatRules( RuleCompiler& c)
{
	static const int ops[ 5] = {SP_OP_SEQUENCE, SP_OP_WITHIN, SP_OP_SEQUENCE_STRUCT, SP_OP_WITHIN_STRUCT, SP_OP_ANY};
	for (int i=0; i<40; ++i)
	{
		const int op = ops[ i % 5];
		size_t n = 2;
		if (op == SP_OP_SEQUENCE_STRUCT || op == SP_OP_WITHIN_STRUCT) { c.pushTerm( 1u << 24); ++n; }
		c.pushTerm( 1 + i % 7); c.attachVariable( "A0");
		c.pushTerm( 1 + (3*i) % 11); c.attachVariable( "A1");
		c.pushExpression( op, n, 1 + i % 5, 0);
		c.definePattern( "r" + std::to_string( i), "", true);
	}
}

static void nestedRules( RuleCompiler& c)
{
	c.pushTerm( 1); c.pushTerm( 2); c.attachVariable( "b");
	c.pushExpression( SP_OP_SEQUENCE, 2, 3, 0);
	c.pushTerm( 3);
	c.pushExpression( SP_OP_WITHIN, 2, 8, 0);
	c.definePattern( "outer", "", true);
	c.compile();
}

int main()
{
	const unsigned CUS = 256;
	const size_t edges[] = {0, 1, 63, 64, 3072, 3073, 4096, 4097, 8192, 8193, 0xFFFFFFFEull};
	RuleCompiler flat, nested;
	flatRules( flat);
	nestedRules( nested);
	FlatTables ft, nt;
	flat.flatten( ft);
	nested.flatten( nt);

	// engines
	const L2Engine general = chooseL2Engine( nested, nt, SP_CTX_RESULT_SETS, L2Switches());
	CHECK( general.kind() == L2_GENERAL && !general.flat.whyNot.empty() && !general.join.whyNot.empty());
	L2Switches sw;
	sw.fastMaxRules = 9999;
	const L2Engine fe = chooseL2Engine( flat, ft, 0, sw);
	CHECK( fe.kind() == L2_FLAT && fe.flat.maxRules == 4095 && !fe.flat.keyinst.empty() && !fe.join.asked);
	const L2Engine je = chooseL2Engine( flat, ft, SP_CTX_RESULT_SETS, L2Switches());
	CHECK( je.kind() == L2_JOIN && je.flat.on && !je.join.keytab.empty());
	sw = L2Switches(); sw.fast = false; sw.join = true;
	const L2Engine off = chooseL2Engine( flat, ft, 0, sw);
	CHECK( off.kind() == L2_JOIN && !off.flat.on && off.flat.whyNot == "disabled by SPA_L2_FAST=0");

	// flat layouts of the instances n and t (R, T as in the kernel table of l2_fast_kernel.hip)
	const FlatPlan fn = planFlat( fe.flat, 4, "n", 256, 448), ftiny = planFlat( je.flat, 3, "t", 8, 128);
	CHECK( fn.expShift == 3 && ftiny.expShift == 3 && fn.spill.totalWords % 64 == 0 && ftiny.spill.maxRules == 2048);

	// launches: every engine at every edge, new batches and reruns, the arena at every size it can take
	ArenaLayout arena = initialArena();
	for (int grows=0;; ++grows)
	{
		for (size_t ndocs : edges)
		{
			const L2LaunchPlan g = planL2Launch( L2_GENERAL, false, CUS, 0, ndocs, ndocs, 8*ndocs, arena, 0, 0, 0);
			CHECK( g.route == L2_ROUTE_GENERAL && g.generalBlocks >= 1 && g.generalBlocks <= CUS*L2_WAVES_PER_CU && g.arenaAllocWaves >= g.arena.run);
			CHECK( (uint64_t)g.arenaAllocWaves * g.arenaPerWaveBytes <= ((uint64_t)48 << 30) || g.arenaAllocWaves <= 4);
			const L2LaunchPlan f = planL2Launch( L2_FLAT, false, CUS, 16, ndocs, ndocs, 8*ndocs, arena, &fn, 0, 0);
			CHECK( f.route == L2_ROUTE_FLAT_LIST && f.fastBlocks >= 1 && f.fastBlocks <= 4096 && f.spillAllocWaves >= f.fastBlocks && f.listBlocks >= 1 && f.listBlocks <= 512);
			const L2LaunchPlan j = planL2Launch( L2_JOIN, false, CUS, 16, ndocs, ndocs, 8*ndocs, arena, &ftiny, 1, (uint64_t)1 << 40);
			CHECK( j.route == L2_ROUTE_JOIN && j.joinBlocks >= 1 && j.joinBlocks <= 8192 && j.wantItems == 0xFFFFFFFFull);
			const L2LaunchPlan r = planL2Launch( L2_FLAT, true, CUS, 16, ndocs < 100 ? ndocs : 100, ndocs, 715827883, arena, &fn, 0, 0);
			CHECK( r.route == L2_ROUTE_RERUN_LIST && r.arenaAllocWaves == r.arena.run && r.fastBlocks == 0 && r.wantItems == 0xFFFFFFFFull && r.wantResults < 0xFFFFFFFFull);
		}
		if (!growArena( arena)) { CHECK( grows == 10 && arena.maxRules == (1u << 20) && arena.scratchCap == 256); break; }
	}
	setArena( arena, 4096, 0, 512, 100, 7);
	CHECK( arena.maxRules == 4096 && arena.winCap == 1024 && arena.maxRefs == 100 && arena.maxTrigs == (1024u << 10));
	bool refused = false;
	try { planL2Launch( L2_GENERAL, false, CUS, 0, 1, 0xFFFFFFFFull, 8, arena, 0, 0, 0); }
	catch (const std::runtime_error&) { refused = true; }
	CHECK( refused);
	std::printf( "l2 plan: ok\n");
	return 0;
}
