// C-ABI of level 2 (include/strus_pattern_amd.h): rule compiler handle + GPU match context.
// No CPU fallback: a context cannot be created without a usable HIP device.
#include "l2_plan.hpp"
#include "l2_finish.h"
#include "l2_text.h"
#include "l2_freq.h"
#include "l2_values.h"
#include "l2_terms.h"
#include "match_terms.hpp"
#include "span_text.hpp"
#include "result_values.hpp"
#include "pattern_freq.hpp"
#include "capi_util.hpp"
#include <cstdio>
#include <mutex>

using namespace spa;

struct sp_matcher
{
	RuleCompiler compiler;
	bool compiled = false;	// compile() is optional for the matcher (reference: tests/randomTokenPatternMatch :317-320)
	mutable std::string lasterror;
	// the parts of the format strings (result_values.hpp): built when the rule set compiles or is loaded, else at the first values call
	mutable std::mutex formatMutex;
	mutable FormatTable formatTable;
	mutable bool haveFormatTable = false;
	mutable size_t formatTableVariables = 0;	// the variable names the table was resolved against

	// rebuild = true (every compile, every load): the definitions may have changed under the same counts
	const FormatTable& formats( bool rebuild = false) const
	{
		std::lock_guard<std::mutex> lock( formatMutex);
		const size_t nvariables = compiler.variables().names().size();
		if (rebuild || !haveFormatTable || formatTable.count != compiler.formatCount() || formatTableVariables != nvariables)
		{
			formatTableVariables = nvariables;
			formatTable = buildFormatTable( compiler.formatCount(),
				[this]( uint32_t f) { return compiler.formatString( f); },
				[this]( const std::string& name) { return compiler.variables().get( name); });
			haveFormatTable = true;
		}
		return formatTable;
	}
};

namespace {

// which kernel serves the rule set under `flags` and `sw` (l2_plan.hpp), with its tables
L2Engine engineOf( const sp_matcher* m, uint32_t flags, const L2Switches& sw, FlatTables& ft)
{
	m->compiler.flatten( ft);
	return chooseL2Engine( m->compiler, ft, flags, sw);
}

// the flat tier's kernel instance (l2_fast_kernel.hip) and layout for the rule set
FlatPlan flatPlanOf( const L2Engine& e, const L2Switches& sw)
{
	// SPA_L2_FAST_SIZE=s|m|l picks the kernel instance (LDS capacities; t = the tiny one of the tests); the spill area takes what does not fit
	const char size[ 2] = {sw.fastSize, 0};
	const unsigned variant = fastVariantNamed( size);
	uint32_t R = 0, T = 0;
	fastCapacities( variant, R, T);
	return planFlat( e.flat, variant, fastKernelName( variant), R, T);
}

// sp_matcher_*_tier: 1 when the engine chosen without any switch is `kind`, else 0 with the reason (or the error) in `why`
int tierQuery( const sp_matcher* m, uint32_t flags, L2EngineKind kind, char* why, size_t whysize, uint32_t* altPrograms)
{
	if (altPrograms) *altPrograms = 0;
	try
	{
		FlatTables ft;
		const L2Engine e = engineOf( m, flags, L2Switches(), ft);
		const std::string& reason = kind == L2_JOIN ? e.join.whyNot : e.flat.whyNot;
		copyText( why, whysize, reason.c_str());
		if (altPrograms) *altPrograms = e.altPrograms;
		return reason.empty() ? 1 : 0;
	}
	catch (const std::exception& e)
	{
		copyText( why, whysize, e.what());
		return 0;
	}
}

} // namespace

struct sp_matcher_ctx
{
	const sp_matcher* inst = 0;
	int device = 0;
	unsigned numCUs = 256;
	L2Switches sw;			// read when the context is created
	L2EngineKind kind = L2_GENERAL;
	std::string lasterror;
	// the exact engine (l2_kernel.hip): compiled tables, working memory, the documents of a launch in list mode
	struct Exact
	{
		DeviceBuffer dPrograms, dTrigdefs, dKeytab, dKeylist, dDocList;
		uint32_t keymask = 0, nofStopWords = 0;
		ArenaLayout layout = initialArena();
		CountedBuffer arena;		// count: waves; 0 forces a new layout at the next launch
	} exact;
	// flat tier (l2_fast.h): flat rule sets run with their hot state in LDS; the general kernel takes what it hands over
	struct Flat
	{
		bool on = false;
		std::string whyNot;
		DeviceBuffer dKeyinst, dStatics;
		FlatPlan plan;			// kernel instance = LDS capacities (l2_fast_kernel.hip), spill layout
		CountedBuffer spill;		// count: waves
		unsigned blocksPerCU = 0;
	} flat;
	// result-set mode (l2_join.h; SP_CTX_RESULT_SETS or SPA_L2_JOIN=1): result multisets without materialised rule instances
	struct ResultSets
	{
		bool on = false, altRules = false;
		std::string whyNot;
		uint32_t keymask = 0, maxRange = 0, delimiter = 0;
		DeviceBuffer dKeytab, dRules, dFilter, dCounts;
	} join;
	// batch buffers (grown on demand): the input of the host entry points, the output of every rule kernel
	struct BatchIO
	{
		DeviceBuffer dCursor, dCounters;
		DeviceBuffer dLexems, dOrigseg, dDocOffsets;
		CountedBuffer results, items;	// count: sp_result_t, sp_result_item_t
		DeviceBuffer dDocRange, dDocStats, dDocStatus;
		DeviceBuffer dResultFormat, dItemFormat;	// only for matchers with format strings
		bool withFormats = false, withItems = true;
		uint64_t minResults = 0, minItems = 0;
	} io;
	// the last batch finished on the device (l2_finish.h); nothing is allocated before the first sp_matcher_ctx_batch_finish_device
	struct Finished
	{
		PassRun<5> run;		// ev[4]: between the sort and the placement of a canonical finish
		DeviceBuffer dResults, dItems, dResultFormat, dItemFormat, dDocResultOffsets, dDocItemOffsets, dTotals, dKept, dCovered, dCursor;
		bool canonical = false;
		// working memory of the canonical order, allocated at the first finish that asks for it
		DeviceBuffer dSortKeys[ 2], dSortIdx[ 2], dSortCursor;
	} fin;
	// the matched text of the last finished batch (l2_text.h); nothing is allocated before the first sp_matcher_ctx_finished_text_device
	struct Text
	{
		PassRun<2> run;
		DeviceBuffer dText[ 2], dSpanOffsets[ 2], dSpanWork[ 2], dDocBytes[ 2], dDocTextOffsets[ 2];	// [0] results, [1] items
		DeviceBuffer dStatus, dTotals, dCursor;
		uint32_t flags = 0;
		size_t ndocs = 0;
		uint64_t nrecords[ 2] = {0, 0}, totals[ 2] = {0, 0};
	} txt;
	// the values of the format strings of the last finished batch (l2_values.h); nothing is allocated before the first sp_matcher_ctx_finished_values_device
	struct Values
	{
		PassRun<2> run;
		DeviceBuffer dFmtParts, dParts, dPool;		// the format table, uploaded at the first call
		bool uploaded = false;
		uint32_t poolBytes = 0;
		DeviceBuffer dValues[ 2], dValueOffsets[ 2], dValueWork[ 2], dDocBytes[ 2], dDocValueOffsets[ 2];	// [0] results, [1] items
		DeviceBuffer dStatus, dTotals, dCursor;
		uint32_t flags = 0;
		size_t ndocs = 0;
		uint64_t nrecords[ 2] = {0, 0}, totals[ 2] = {0, 0};
	} val;
	// the pattern frequencies of the last finished batch (l2_freq.h); nothing is allocated before the first sp_matcher_ctx_finished_pattern_freq_device
	struct Freq
	{
		PassRun<2> run;
		DeviceBuffer dRecords, dDocOffsets, dStatus, dHandleResults, dHandleDocs, dTotals, dDocCount, dDocMeta, dCursor;
		size_t ndocs = 0;
		uint32_t handleBound = 0;
		uint64_t total = 0;
	} frq;
	// the index terms of the last finished batch (l2_terms.h); nothing is allocated before the first sp_matcher_ctx_finished_terms_device
	struct Terms
	{
		PassRun<2> run;
		DeviceBuffer dRecords, dDocOffsets, dResultTerm, dStatus, dTotals, dLeader, dTable, dHistogram, dDocCount, dCursor;
		size_t ndocs = 0;
		uint32_t handleBound = 0, flags = 0;
		uint64_t nresults = 0, total = 0;
	} trm;
	// single-document mode
	struct SingleDoc
	{
		std::vector<sp_lexem_t> lexems;
		std::vector<uint32_t> origseg; bool hasSeg = false;
		std::vector<uint32_t> resultFormat, itemFormat;	// of the last sp_matcher_ctx_fetch_results
		sp_matcher_stats_t stats = {};
	} cur;
	// the last launch
	bool haveBatch = false;
	size_t lastNdocs = 0;
	hipStream_t lastStream = 0;
	Event evStart, evStop; bool evValid = false;
	Stream own;			// the context's own stream (non-blocking): see sp_lexer_ctx; last member: it waits for its work before anything else goes
};

extern "C" {

const char* sp_version(void) { return "struspattern_amd 0.1 (gfx950)"; }

int sp_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount( &n) != hipSuccess) return 0;
	return n;
}

void sp_free( void* p) { std::free( p); }

// test hook: device allocations of at least `bytes` fail like an out-of-memory hipMalloc (0 = off)
void sp_test_fail_alloc_above( uint64_t bytes) { allocFailureThreshold().store( bytes, std::memory_order_relaxed); }

// ------------------------------------------------------------------ instance
sp_matcher_t* sp_matcher_create(void) { try { return new sp_matcher(); } catch (...) { return 0; } }
void sp_matcher_free( sp_matcher_t* m) { delete m; }
const char* sp_matcher_last_error( const sp_matcher_t* m) { return m->lasterror.c_str(); }

#define MGUARD( CODE, BODY) return guardedCall( m->lasterror, CODE, [&]{ BODY; })

int sp_matcher_define_term_frequency( sp_matcher_t* m, uint32_t termid, double df)
{ MGUARD( SP_ERR_INVALID, m->compiler.defineTermFrequency( termid, df)); }
int sp_matcher_push_term( sp_matcher_t* m, uint32_t termid)
{ MGUARD( SP_ERR_INVALID, m->compiler.pushTerm( termid)); }
int sp_matcher_push_expression( sp_matcher_t* m, int joinop, size_t argc, uint32_t range, uint32_t cardinality)
{ MGUARD( SP_ERR_INVALID, m->compiler.pushExpression( joinop, argc, range, cardinality)); }
int sp_matcher_push_pattern( sp_matcher_t* m, const char* name)
{ MGUARD( SP_ERR_INVALID, m->compiler.pushPattern( name ? name : "")); }
int sp_matcher_attach_variable( sp_matcher_t* m, const char* name)
{ MGUARD( SP_ERR_INVALID, m->compiler.attachVariable( name ? name : "")); }
int sp_matcher_define_pattern( sp_matcher_t* m, const char* name, const char* formatstring, int visible)
{ MGUARD( SP_ERR_INVALID, m->compiler.definePattern( name ? name : "", formatstring ? formatstring : "", visible != 0)); }
int sp_matcher_define_option( sp_matcher_t* m, const char* name, double value)
{ MGUARD( SP_ERR_INVALID, m->compiler.defineOption( name ? name : "", value)); }
int sp_matcher_compile( sp_matcher_t* m)
{ MGUARD( SP_ERR_COMPILE, m->compiler.compile(); m->compiled = true; m->formats( true)); }

uint32_t sp_matcher_pattern_id( const sp_matcher_t* m, const char* name) { return m->compiler.patterns().get( name); }
const char* sp_matcher_pattern_name( const sp_matcher_t* m, uint32_t handle) { return m->compiler.patterns().key( handle); }
uint32_t sp_matcher_variable_id( const sp_matcher_t* m, const char* name) { return m->compiler.variables().get( name); }
const char* sp_matcher_variable_name( const sp_matcher_t* m, uint32_t variable) { return m->compiler.variables().key( variable); }

// np + 1: every result handle of the rule set lies in [1, handle bound)
uint32_t sp_matcher_handle_bound( const sp_matcher_t* m) { return (uint32_t)m->compiler.patterns().names().size() + 1; }

uint32_t sp_matcher_format_count( const sp_matcher_t* m) { return m->compiler.formatCount(); }
const char* sp_matcher_format_string( const sp_matcher_t* m, uint32_t format_handle) { return m->compiler.formatString( format_handle); }

// which kernel the context's batches run on: 0 = general, 1 = LDS-resident (flat rule sets), 2 = join kernel (result-set mode)
int sp_matcher_ctx_kernel_kind( const sp_matcher_ctx_t* c) { return c->kind; }
// name of the kernel that does a batch's work: the launch plan's (the instance of the LDS-resident kernel is picked by SPA_L2_FAST_SIZE, default n)
const char* sp_matcher_ctx_kernel_name( const sp_matcher_ctx_t* c) { return l2KernelName( c->kind, &c->flat.plan); }

// 1 when the compiled rule set is flat (l2_fast.h) and runs on the LDS-resident kernel, else 0 with the reason
int sp_matcher_fast_tier( const sp_matcher_t* m, char* why, size_t whysize)
{ return tierQuery( m, 0, L2_FLAT, why, whysize, 0); }

// result-set mode: 1 when a context that asks for it runs the compiled rule set on the join kernel, else 0 with the reason why it stays on the exact engine
int sp_matcher_result_set_tier( const sp_matcher_t* m, char* why, size_t whysize, uint32_t* alt_programs)
{ return tierQuery( m, SP_CTX_RESULT_SETS, L2_JOIN, why, whysize, alt_programs); }

// What a context created now with `ctx_flags` on a device of `num_cus` compute units would launch for a batch, without a device:
// key=value fields, one per line (include/strus_pattern_amd.h)
int sp_matcher_launch_plan( const sp_matcher_t* m, uint32_t ctx_flags, unsigned num_cus, unsigned fast_blocks_per_cu, size_t ndocs, size_t nlexems,
			    size_t rerun_docs, uint32_t arena_grows, uint64_t min_results, uint64_t min_items, char* buf, size_t bufsize)
{
	if (buf && bufsize) buf[ 0] = 0;
	return guardedCall( m->lasterror, SP_ERR_INVALID, [&]{
		if (ctx_flags & ~(uint32_t)SP_CTX_RESULT_SETS) throw std::runtime_error( "unknown context flags");
		const L2Switches sw = L2Switches::fromEnv();
		FlatTables ft;
		const L2Engine e = engineOf( m, ctx_flags, sw, ft);
		const FlatPlan fp = e.flat.on ? flatPlanOf( e, sw) : FlatPlan();
		ArenaLayout arena = initialArena();
		arena.nStop = ft.nofStopWords;
		for (uint32_t i=0; i<arena_grows; ++i) if (!growArena( arena)) throw std::runtime_error( "arena at its maximum size");
		const L2LaunchPlan p = planL2Launch( e.kind(), rerun_docs != 0, num_cus ? num_cus : 256u, fast_blocks_per_cu, rerun_docs ? rerun_docs : ndocs, ndocs, nlexems,
							arena, &fp, min_results, min_items);
		static const char* const engines[] = {"general", "flat", "join"};
		static const char* const routes[] = {"general", "flat+list", "join", "rerun-list"};
		int n = std::snprintf( buf, bufsize, "engine=%s\nkind=%d\nflat_why_not=%s\njoin_why_not=%s\nalt_programs=%u\nkernel=%s\nroute=%s\n"
			"general_blocks=%u\narena_run=%u\narena_alloc=%u\narena_alloc_waves=%u\narena_per_wave_bytes=%zu\narena_max_rules=%u\narena_scratch_cap=%u\nstop_words=%u\n"
			"fast_blocks=%u\nspill_alloc_waves=%llu\nspill_per_wave_bytes=%zu\nlist_blocks=%u\njoin_blocks=%u\nwant_results=%llu\nwant_items=%llu\n"
			"R=%u\nT=%u\nexp_shift=%u\nspill_words=%u\nmax_rules=%u\nmax_staged=%u\nbucket_caps=",
			engines[ e.kind()], (int)e.kind(), e.flat.whyNot.c_str(), e.join.whyNot.c_str(), e.altPrograms, p.kernelName, routes[ p.route],
			p.generalBlocks, p.arena.run, p.arena.alloc, p.arenaAllocWaves, p.arenaPerWaveBytes, p.layout.maxRules, p.layout.scratchCap, ft.nofStopWords,
			p.fastBlocks, (unsigned long long)p.spillAllocWaves, p.spillPerWaveBytes, p.listBlocks, p.joinBlocks, (unsigned long long)p.wantResults, (unsigned long long)p.wantItems,
			fp.R, fp.T, fp.expShift, fp.spill.totalWords, fp.spill.maxRules, fp.spill.maxStaged);
		for (int b=0; b<16 && n >= 0 && buf && (size_t)n < bufsize; ++b) n += std::snprintf( buf+n, bufsize-n, b ? ",%u" : "%u", fp.bucketMeta[ b] >> 16);
		if (n < 0 || !buf || (size_t)n >= bufsize) throw std::runtime_error( "buffer too small for the launch plan");
	});
}

// the rule set as a blob (tables, names, format strings, options) and back: SURVEY.md 8(f).4
int sp_matcher_serialize( const sp_matcher_t* m, void** blob, size_t* size)
{ return exportBlob( m->lasterror, blob, size, [&]( std::vector<uint8_t>& buf){ m->compiler.save( buf, m->compiled); }); }
sp_matcher_t* sp_matcher_deserialize( const void* blob, size_t size, char* err, size_t errsize)
{ return importBlob<sp_matcher>( err, errsize, [&]( sp_matcher& m){ m.compiled = m.compiler.load( blob, size); m.formats( true); }); }

size_t sp_matcher_dump_table( const sp_matcher_t* m, uint32_t** out)
{
	std::vector<uint32_t> buf = m->compiler.dump();
	*out = (uint32_t*)std::malloc( buf.size()*sizeof(uint32_t) + 4);
	if (!*out) return 0;
	std::memcpy( *out, buf.data(), buf.size()*sizeof(uint32_t));
	return buf.size();
}

// ------------------------------------------------------------------ context
sp_matcher_ctx_t* sp_matcher_ctx_create( const sp_matcher_t* m, int device) { return sp_matcher_ctx_create_ex( m, device, 0); }

sp_matcher_ctx_t* sp_matcher_ctx_create_ex( const sp_matcher_t* m, int device, uint32_t flags)
{
	sp_matcher_ctx* c = 0;
	if (flags & ~(uint32_t)SP_CTX_RESULT_SETS)
	{
		m->lasterror = "unknown context flags";
		return 0;
	}
	try
	{
		c = new sp_matcher_ctx();
		c->inst = m; c->device = device;
		int ndev = 0;
		hipError_t e = hipGetDeviceCount( &ndev);
		if (e != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
		{
			m->lasterror = "no usable HIP device: the rule automaton runs on the GPU only (no CPU fallback)";
			delete c; return 0;
		}
		HIP_CHECK( hipSetDevice( device));
		hipDeviceProp_t prop;
		HIP_CHECK( hipGetDeviceProperties( &prop, device));
		c->numCUs = prop.multiProcessorCount > 0 ? (unsigned)prop.multiProcessorCount : 256u;

		c->sw = L2Switches::fromEnv();
		FlatTables ft;
		const L2Engine engine = engineOf( m, flags, c->sw, ft);
		c->kind = engine.kind();
		c->exact.dPrograms.upload( ft.programs.data(), ft.programs.size()*sizeof(DevProgram));
		c->exact.dTrigdefs.upload( ft.trigdefs.data(), ft.trigdefs.size()*sizeof(DevTrigDef));
		c->exact.dKeytab.upload( ft.keytab.data(), ft.keytab.size()*sizeof(DevKeyEntry));
		c->exact.dKeylist.upload( ft.keylist.data(), ft.keylist.size()*sizeof(DevKeyRef));
		c->exact.keymask = (uint32_t)ft.keytab.size()-1;
		c->exact.nofStopWords = ft.nofStopWords;
		c->exact.layout.nStop = ft.nofStopWords;
		c->io.withFormats = m->compiler.formatCount() != 0;
		c->flat.on = engine.flat.on; c->flat.whyNot = engine.flat.whyNot;
		if (c->flat.on)
		{
			c->flat.dKeyinst.upload( engine.flat.keyinst.data(), engine.flat.keyinst.size()*sizeof(FastKeyInst));
			c->flat.dStatics.upload( engine.flat.statics.data(), engine.flat.statics.size()*sizeof(FastStatic));
			c->flat.plan = flatPlanOf( engine, c->sw);
			c->flat.blocksPerCU = (unsigned)fastBlocksPerCU( c->flat.plan.variant);
		}
		if (c->sw.verbose) fprintf( stderr, "[spa] fast tier: %s\n", c->flat.on ? "on" : c->flat.whyNot.c_str());
		c->join.on = engine.join.on; c->join.whyNot = engine.join.whyNot;
		if (c->join.on)
		{
			const L2Engine::Join& j = engine.join;
			c->join.dKeytab.upload( j.keytab.data(), j.keytab.size()*sizeof(JoinKey)); c->join.dRules.upload( j.rules.data(), j.rules.size()*sizeof(JoinRule)); c->join.dFilter.upload( j.filter.data(), j.filter.size()*sizeof(uint32_t));
			c->join.keymask = (uint32_t)j.keytab.size()-1; c->join.maxRange = j.maxRange; c->join.delimiter = j.delimiter;
			c->join.altRules = engine.altPrograms != 0;
		}
		if (c->sw.verbose && engine.join.asked) fprintf( stderr, "[spa] result-set mode: %s\n", c->join.on ? "join kernel" : c->join.whyNot.c_str());
		c->io.dCursor.alloc( 256);		// u32: [0] fast cursor, [1] general cursor (list mode), [2] hand-over count, [16..31] hand-over reasons, [32..47] phase profile (u64 x 8)
		c->io.dCounters.alloc( SPC_COUNT*sizeof(uint64_t));
		c->own.create( device);
		c->evStart.create(); c->evStop.create();
		return c;
	}
	catch (const std::exception& e)
	{
		m->lasterror = e.what();
		delete c;
		return 0;
	}
}

void sp_matcher_ctx_free( sp_matcher_ctx_t* c) { delete c; }	// (`own` waits for its work before it goes: Stream)
const char* sp_matcher_ctx_last_error( const sp_matcher_ctx_t* c) { return c->lasterror.c_str(); }

int sp_matcher_ctx_set_arena( sp_matcher_ctx_t* c, uint32_t max_rules, uint32_t max_triggers, uint32_t bucket_capacity,
				uint32_t max_items, uint32_t max_follow)
{
	setArena( c->exact.layout, max_rules, max_triggers, bucket_capacity, max_items, max_follow);
	c->exact.arena.count = 0;	// forces re-layout at the next launch
	return SP_OK;
}

} // extern "C"

namespace {

// the counters of the last batch (its stream has been waited for), and what of its output lies inside the buffers
struct BatchCounts { uint64_t counters[ SPC_COUNT]; uint64_t results, items; };
BatchCounts readCounts( sp_matcher_ctx* c)
{
	BatchCounts b;
	copySync( c->own, b.counters, c->io.dCounters.ptr, sizeof(b.counters), hipMemcpyDeviceToHost);
	b.results = clampCount( b.counters[ SPC_RESULTS], c->io.results.count);
	b.items = clampCount( b.counters[ SPC_ITEMS], c->io.items.count);
	return b;
}

// Host copy of the device results of the last launch for the documents [firstDoc, firstDoc+ndocs), regrouped by document with
// the `exclusive` elimination of fetchResults applied on the way: the plan, the copy segments and the regroup of batch_fetch.hpp
void copyOutBatch( sp_matcher_ctx* c, size_t firstDoc, size_t ndocs, const BatchCounts& counts, sp_match_batch_t* out)
{
	MatchBatchSource src;
	src.results = (const sp_result_t*)c->io.results.ptr(); src.nresults = counts.results;
	src.items = (const sp_result_item_t*)c->io.items.ptr(); src.nitems = counts.items;
	src.resultFormat = c->io.withFormats ? (const uint32_t*)c->io.dResultFormat.ptr : 0;
	src.itemFormat = c->io.withFormats ? (const uint32_t*)c->io.dItemFormat.ptr : 0;
	src.docRange = (const uint64_t*)c->io.dDocRange.ptr; src.docStatus = (const int32_t*)c->io.dDocStatus.ptr;
	src.docStats = (const uint64_t*)c->io.dDocStats.ptr;
	src.ndocs = c->lastNdocs;
	fetchMatchBatch( src, firstDoc, ndocs, c->inst->compiler.exclusive(), c->inst->compiler.maxResultSize(), deviceToHost( c->own), out);
}

} // namespace

extern "C" {

// copies the device results of the documents [first_doc, first_doc+ndocs) of the last batch to the host, grouped by document
int sp_matcher_ctx_batch_fetch_docs( sp_matcher_ctx_t* c, size_t first_doc, size_t ndocs, sp_match_batch_t* out)
{
	std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_DEVICE, [&]{
		HIP_CHECK( hipSetDevice( c->device));
		HIP_CHECK( hipStreamSynchronize( c->lastStream));
		copyOutBatch( c, first_doc, ndocs, readCounts( c), out);
	});
}

// the same for the whole batch
int sp_matcher_ctx_batch_fetch( sp_matcher_ctx_t* c, sp_match_batch_t* out) { return sp_matcher_ctx_batch_fetch_docs( c, 0, c->lastNdocs, out); }

int sp_matcher_ctx_batch_status( sp_matcher_ctx_t* c, int32_t* status, size_t ndocs) { return batchStatus( c, c->io.dDocStatus, status, ndocs); }

int sp_matcher_ctx_grow_arena( sp_matcher_ctx_t* c)
{
	if (!growArena( c->exact.layout)) { c->lasterror = "arena at its maximum size"; return SP_ERR_INVALID; }
	c->exact.arena.count = 0;
	return SP_OK;
}

int sp_matcher_ctx_reserve_output( sp_matcher_ctx_t* c, uint64_t results, uint64_t items)
{
	if (results > c->io.minResults) c->io.minResults = results;
	if (items > c->io.minItems) c->io.minItems = items;
	return SP_OK;
}

} // extern "C"

namespace {

// the batch contract of every rule kernel (l2_device.h): this batch's input, the context's output buffers
L2BatchIO batchIO( sp_matcher_ctx* c, const void* d_lexems, const void* d_origseg, const void* d_doc_offsets, const void* d_doc_ranges, size_t ndocs)
{
	L2BatchIO io;
	std::memset( &io, 0, sizeof(io));
	io.lexems = (const uint32_t*)d_lexems; io.origseg = (const uint32_t*)d_origseg;
	io.docOffsets = (const uint64_t*)d_doc_offsets; io.docRangesIn = (const uint64_t*)d_doc_ranges;
	io.ndocs = (uint32_t)ndocs; io.withItems = c->io.withItems ? 1u : 0u;
	io.docCursor = (uint32_t*)c->io.dCursor.ptr;
	io.counters = (uint64_t*)c->io.dCounters.ptr;
	io.results = (uint32_t*)c->io.results.ptr(); io.resultCapacity = c->io.results.count;
	io.items = (uint32_t*)c->io.items.ptr(); io.itemCapacity = c->io.items.count;
	io.docRange = (uint64_t*)c->io.dDocRange.ptr; io.docStats = (uint64_t*)c->io.dDocStats.ptr; io.docStatus = (int32_t*)c->io.dDocStatus.ptr;
	io.withFormats = c->io.withFormats ? 1u : 0u;
	io.resultFormat = (uint32_t*)c->io.dResultFormat.ptr; io.itemFormat = (uint32_t*)c->io.dItemFormat.ptr;
	return io;
}

// ---- one batch on `stream`, step by step (launchBatch below)

// the per-wave arena of the general kernel
void ensureArena( sp_matcher_ctx* c, const L2LaunchPlan& plan)
{
	if (c->exact.arena.count < plan.arena.run)
	{
		const ArenaLayout& L = plan.layout;
		if (c->sw.verbose) fprintf( stderr, "[spa] arena: rules %u bucket %u items %u refs %u staged %u winCap %u -> %.2f MB per wave, %u waves\n", L.maxRules, L.bucketCap, L.maxItems, L.maxRefs, L.maxStaged, L.winCap, L.totalWords*4/1e6, plan.arena.run);
		c->exact.arena.realloc( plan.arenaAllocWaves, plan.arenaPerWaveBytes);
	}
}

// output capacity: results are bounded by what fits; sized from the input, grown by the caller on SP_DOC_ERR_ARENA
void ensureOutput( sp_matcher_ctx* c, const L2LaunchPlan& plan, size_t ndocs)
{
	sp_matcher_ctx::BatchIO& io = c->io;
	io.results.ensure( plan.wantResults, sizeof(sp_result_t));
	io.items.ensure( plan.wantItems, sizeof(sp_result_item_t));
	if (io.withFormats)
	{
		io.dResultFormat.reserve( io.results.count*sizeof(uint32_t));
		io.dItemFormat.reserve( io.items.count*2*sizeof(uint32_t));
	}
	io.dDocRange.reserve( (ndocs+1)*2*sizeof(uint64_t));
	io.dDocStats.reserve( (ndocs+1)*4*sizeof(uint64_t));
	io.dDocStatus.reserve( (ndocs+1)*sizeof(int32_t));
}

void resetCursorAndCounters( sp_matcher_ctx* c, bool rerun, hipStream_t stream)
{
	HIP_CHECK( hipMemsetAsync( c->io.dCursor.ptr, 0, 256, stream));
	if (!rerun) HIP_CHECK( hipMemsetAsync( c->io.dCounters.ptr, 0, SPC_COUNT*sizeof(uint64_t), stream));
	else HIP_CHECK( hipMemsetAsync( (uint64_t*)c->io.dCounters.ptr + SPC_FAILED, 0, sizeof(uint64_t), stream));	// (the other counters continue)
}

L2Params generalParams( const sp_matcher_ctx* c, const L2BatchIO& io, const L2LaunchPlan& plan)
{
	L2Params P;
	std::memset( &P, 0, sizeof(P));
	P.programs = (const DevProgram*)c->exact.dPrograms.ptr;
	P.trigdefs = (const DevTrigDef*)c->exact.dTrigdefs.ptr;
	P.keytab = (const DevKeyEntry*)c->exact.dKeytab.ptr;
	P.keylist = (const DevKeyRef*)c->exact.dKeylist.ptr;
	P.keymask = c->exact.keymask; P.nofStopWords = c->exact.nofStopWords;
	P.io = io;
	P.arenaBase = (uint32_t*)c->exact.arena.ptr(); P.arena = plan.layout;
	return P;
}

// list mode of the general kernel: the documents exact.dDocList[0 .. cursor[2]), their cursor is cursor[1]
void listMode( const sp_matcher_ctx* c, L2Params& P)
{
	P.docList = (const uint32_t*)c->exact.dDocList.ptr; P.docListCount = (const uint32_t*)c->io.dCursor.ptr + 2;
	P.io.docCursor = (uint32_t*)c->io.dCursor.ptr + 1;
}

// `rerun`: only these documents of the batch already in the output buffers run again, with the working set the caller has just grown
void launchRerun( sp_matcher_ctx* c, L2Params P, const L2LaunchPlan& plan, const std::vector<uint32_t>& rerun, hipStream_t stream)
{
	const uint32_t n = (uint32_t)rerun.size();
	c->exact.dDocList.reserve( ((size_t)P.io.ndocs+1)*sizeof(uint32_t));
	HIP_CHECK( hipMemcpyAsync( c->exact.dDocList.ptr, rerun.data(), n*sizeof(uint32_t), hipMemcpyHostToDevice, stream));
	HIP_CHECK( hipMemcpyAsync( (uint32_t*)c->io.dCursor.ptr + 2, &n, sizeof(uint32_t), hipMemcpyHostToDevice, stream));
	HIP_CHECK( hipStreamSynchronize( stream));		// (the list and its count are host temporaries)
	listMode( c, P);
	HIP_CHECK( launchL2Match( P, plan.generalBlocks, stream));
}

// result-set mode: result multisets by joining positions, nothing installed (l2_join.h)
void launchJoin( sp_matcher_ctx* c, const L2BatchIO& io, const L2LaunchPlan& plan, size_t nlexems, hipStream_t stream)
{
	JoinParams J;
	std::memset( &J, 0, sizeof(J));
	c->join.dCounts.reserve( (nlexems + 64) * sizeof(uint32_t));
	J.filter = (const uint32_t*)c->join.dFilter.ptr; J.counts = (uint32_t*)c->join.dCounts.ptr; J.countsCapacity = nlexems;
	J.keytab = (const JoinKey*)c->join.dKeytab.ptr; J.keymask = c->join.keymask; J.rules = (const JoinRule*)c->join.dRules.ptr; J.maxRange = c->join.maxRange; J.delimiter = c->join.delimiter; J.altRules = c->join.altRules ? 1u : 0u;
	J.io = io;
	HIP_CHECK( launchL2Join( J, plan.joinBlocks, stream));
}

// flat rule set: the LDS-resident kernel first; the documents it hands over (exact.dDocList) go through the
// general kernel in list mode right behind it on the same stream (an empty list costs one short launch)
void launchFlat( sp_matcher_ctx* c, L2Params P, const L2LaunchPlan& plan, hipStream_t stream)
{
	sp_matcher_ctx::Flat& f = c->flat;
	const size_t ndocs = P.io.ndocs;
	if (f.spill.count < plan.fastBlocks)
	{
		f.spill.realloc( plan.spillAllocWaves, plan.spillPerWaveBytes);
		if (c->sw.verbose) fprintf( stderr, "[spa] fast tier: %u waves/CU, LDS capacities R %u T %u, spill %.2f MB per wave\n", f.blocksPerCU, f.plan.R, f.plan.T, f.plan.spill.totalWords*4/1e6);
	}
	c->exact.dDocList.reserve( (ndocs+1)*sizeof(uint32_t));
	FastParams F;
	std::memset( &F, 0, sizeof(F));
	F.keyinst = (const FastKeyInst*)f.dKeyinst.ptr; F.statics = (const FastStatic*)f.dStatics.ptr; F.keytab = (const FastKeyEntry*)c->exact.dKeytab.ptr;
	F.keymask = c->exact.keymask; F.nofStopWords = c->exact.nofStopWords;
	F.io = P.io;
	std::memcpy( F.bucketMeta, f.plan.bucketMeta, sizeof(F.bucketMeta)); F.expShift = f.plan.expShift;
	F.spill = f.plan.spill; F.spillBase = (uint32_t*)f.spill.ptr();
	F.fallbackList = (uint32_t*)c->exact.dDocList.ptr; F.fallbackCount = (uint32_t*)c->io.dCursor.ptr + 2;
	F.diag = (uint32_t*)c->io.dCursor.ptr + 16; F.prof = (uint64_t*)((uint32_t*)c->io.dCursor.ptr + 32);
	HIP_CHECK( launchL2Fast( F, f.plan.variant, plan.fastBlocks, stream));
	listMode( c, P);
	HIP_CHECK( launchL2Match( P, plan.listBlocks, stream));
}

// enqueue one batch on `stream`; all inputs are device pointers
// `rerun` (host entry points): only these documents of the batch already in the output buffers run again, on the
// general kernel in list mode -- the results of the other documents stay where they are
void launchBatch( sp_matcher_ctx* c, const void* d_lexems, const void* d_origseg, const void* d_doc_offsets,
		  size_t ndocs, size_t nlexems, hipStream_t stream, const void* d_doc_ranges=0, const std::vector<uint32_t>* rerun=0)
{
	// everything the launch decides (l2_plan.hpp); it refuses a batch of too many documents before anything is touched
	const L2LaunchPlan plan = planL2Launch( c->kind, rerun != 0, c->numCUs, c->flat.blocksPerCU, rerun ? rerun->size() : ndocs, ndocs, nlexems,
						c->exact.layout, &c->flat.plan, c->io.minResults, c->io.minItems);
	HIP_CHECK( hipSetDevice( c->device));
	c->fin.run.done = false; c->txt.run.done = false; c->val.run.done = false; c->frq.run.done = false; c->trm.run.done = false;	// (a new batch: what was finished is of the one before)
	ensureArena( c, plan);
	ensureOutput( c, plan, ndocs);
	resetCursorAndCounters( c, rerun != 0, stream);
	const L2BatchIO io = batchIO( c, d_lexems, d_origseg, d_doc_offsets, d_doc_ranges, ndocs);
	HIP_CHECK( hipEventRecord( c->evStart, stream));
	switch (plan.route)
	{
		case L2_ROUTE_RERUN_LIST: launchRerun( c, generalParams( c, io, plan), plan, *rerun, stream); break;
		case L2_ROUTE_JOIN: launchJoin( c, io, plan, nlexems, stream); break;
		case L2_ROUTE_FLAT_LIST: launchFlat( c, generalParams( c, io, plan), plan, stream); break;
		case L2_ROUTE_GENERAL: HIP_CHECK( launchL2Match( generalParams( c, io, plan), plan.generalBlocks, stream)); break;
	}
	HIP_CHECK( hipEventRecord( c->evStop, stream));
	c->evValid = true; c->lastStream = stream; c->lastNdocs = ndocs; c->haveBatch = true;
}

// where the batch just enqueued leaves its output (device entry points)
void deviceBatch( const sp_matcher_ctx* c, size_t ndocs, sp_match_device_batch_t* out)
{
	out->ndocs = ndocs;
	out->d_results = c->io.results.ptr(); out->d_items = c->io.items.ptr();
	out->d_doc_result_offsets = c->io.dDocRange.ptr;
	out->d_doc_stats = c->io.dDocStats.ptr; out->d_doc_status = c->io.dDocStatus.ptr;
	out->d_counters = c->io.dCounters.ptr;
	out->d_result_format = c->io.withFormats ? c->io.dResultFormat.ptr : 0;
	out->d_item_format = c->io.withFormats ? c->io.dItemFormat.ptr : 0;
}

// the device entry points: documents by offsets (with optional segments), or by the lexer's (first, count) ranges
int matchDevice( sp_matcher_ctx* c, const void* d_lexems, const void* d_origseg, const void* d_doc_offsets, const void* d_doc_ranges,
		 size_t ndocs, size_t nlexems, void* stream, sp_match_device_batch_t* out)
{
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		launchBatch( c, d_lexems, d_origseg, d_doc_offsets, ndocs, nlexems, (hipStream_t)stream, d_doc_ranges);
		if (out) deviceBatch( c, ndocs, out);
	});
}

} // namespace

extern "C" {

int sp_matcher_ctx_match_docs_device( sp_matcher_ctx_t* c, const void* d_lexems, const void* d_origseg, const void* d_doc_offsets,
				      size_t ndocs, size_t nlexems, void* stream, sp_match_device_batch_t* out)
{ return matchDevice( c, d_lexems, d_origseg, d_doc_offsets, 0, ndocs, nlexems, stream, out); }

int sp_matcher_ctx_match_lexed_device( sp_matcher_ctx_t* c, const void* d_lexems, const void* d_doc_ranges,
				       size_t ndocs, size_t nlexems_hint, void* stream, sp_match_device_batch_t* out)
{ return matchDevice( c, d_lexems, 0, 0, d_doc_ranges, ndocs, nlexems_hint, stream, out); }

int sp_matcher_ctx_batch_counters( sp_matcher_ctx_t* c, uint64_t counters[8])
{
	return guardedCall( c->lasterror, SP_ERR_DEVICE, [&]{
		HIP_CHECK( hipSetDevice( c->device));
		HIP_CHECK( hipStreamSynchronize( c->lastStream));
		copySync( c->own, counters, c->io.dCounters.ptr, SPC_COUNT*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (c->flat.on && c->sw.verbose)
		{
			uint32_t diag[ 16];
			copySync( c->own, diag, (const uint32_t*)c->io.dCursor.ptr + 16, sizeof(diag), hipMemcpyDeviceToHost);
#ifdef SPA_PROF
			uint64_t prof[ 12];
			copySync( c->own, prof, (const uint32_t*)c->io.dCursor.ptr + 32, sizeof(prof), hipMemcpyDeviceToHost);
			double tot = 0; for (int i=0; i<6; ++i) tot += (double)prof[ i];
			fprintf( stderr, "[spa] fast tier phases (share of wave cycles): scan+fire %.1f%% install %.1f%% deactivate %.1f%% expiry %.1f%% results %.1f%% fetch %.1f%% | inside deactivation: loads %.1f%% ranks+queue %.1f%% replay %.1f%% (%.2f replay steps, %.2f batches, %.2f rules per event); %.0f cycles per event\n",
				100*prof[0]/tot, 100*prof[1]/tot, 100*prof[2]/tot, 100*prof[3]/tot, 100*prof[4]/tot, 100*prof[5]/tot, 100*prof[6]/tot, 100*prof[7]/tot, 100*prof[11]/tot,
				(double)prof[ 8] / (double)(counters[ SPC_EVENTS] ? counters[ SPC_EVENTS] : 1), (double)prof[ 9] / (double)(counters[ SPC_EVENTS] ? counters[ SPC_EVENTS] : 1), (double)prof[ 10] / (double)(counters[ SPC_EVENTS] ? counters[ SPC_EVENTS] : 1),
				tot / (double)(counters[ SPC_EVENTS] ? counters[ SPC_EVENTS] : 1));
#endif
			if (diag[ 0])
			{
				fprintf( stderr, "[spa] fast tier handed %u of %zu documents to the general kernel; by reason:", diag[ 0], c->lastNdocs);
				for (int i=1; i<16; ++i) if (diag[ i]) fprintf( stderr, " [%d]=%u", i, diag[ i]);
				fprintf( stderr, "\n");
			}
		}
	});
}

// ---- the last device batch finished on the device: document order, `exclusive` applied, items without gaps (l2_finish.h)
int sp_matcher_ctx_batch_finish_device( sp_matcher_ctx_t* c, void* stream, sp_match_finished_batch_t* out)
{ return sp_matcher_ctx_batch_finish_device_ex( c, stream, 0, out); }

// flags: SP_FINISH_CANONICAL orders the results of every document by the tuple T of the header
int sp_matcher_ctx_batch_finish_device_ex( sp_matcher_ctx_t* c, void* stream_, uint32_t flags, sp_match_finished_batch_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		if (flags & ~(uint32_t)SP_FINISH_CANONICAL) throw std::runtime_error( "unknown finish flags");
		const bool canonical = (flags & SP_FINISH_CANONICAL) != 0;
		if (!c->haveBatch) throw std::runtime_error( "no batch to finish: no batch has run on this context");
		hipStream_t stream = (hipStream_t)stream_;
		HIP_CHECK( hipSetDevice( c->device));
		c->fin.run.done = false; c->txt.run.done = false; c->val.run.done = false; c->frq.run.done = false; c->trm.run.done = false;
		// the buffers are sized from what the batch counted: this read waits for the batch, the passes below do not
		HIP_CHECK( hipStreamSynchronize( c->lastStream));
		const BatchCounts counts = readCounts( c);
		const uint64_t devResults = counts.results, devItems = counts.items;
		const size_t ndocs = c->lastNdocs;
		const bool exclusive = c->inst->compiler.exclusive();
		c->fin.dResults.reserve( (devResults+1)*sizeof(sp_result_t));
		c->fin.dItems.reserve( (devItems+1)*sizeof(sp_result_item_t));
		if (c->io.withFormats)
		{
			c->fin.dResultFormat.reserve( (devResults+1)*sizeof(uint32_t));
			c->fin.dItemFormat.reserve( (devItems+1)*2*sizeof(uint32_t));
		}
		c->fin.dDocResultOffsets.reserve( (ndocs+1)*sizeof(uint64_t));
		c->fin.dDocItemOffsets.reserve( (ndocs+1)*sizeof(uint64_t));
		c->fin.dKept.reserve( (ndocs+1)*2*sizeof(uint32_t));
		if (!c->fin.dTotals.ptr) c->fin.dTotals.alloc( 2*sizeof(uint64_t));
		if (!c->fin.dCursor.ptr) c->fin.dCursor.alloc( 2*sizeof(uint32_t));
		if (exclusive) c->fin.dCovered.reserve( devResults+1);
		if (canonical)
		{
			for (int i=0; i<2; ++i)
			{
				c->fin.dSortKeys[ i].reserve( (devResults+1)*sizeof(uint64_t));
				c->fin.dSortIdx[ i].reserve( (devResults+1)*sizeof(uint32_t));
			}
			if (!c->fin.dSortCursor.ptr) c->fin.dSortCursor.alloc( sizeof(uint32_t));
		}
		// another stream than the batch's runs behind the batch (evStop closes every launch sequence, reruns included)
		c->fin.run.begin( stream, c->lastStream, c->evStop);
		hipEvent_t ev[ 5];
		c->fin.run.events( ev);
		HIP_CHECK( hipMemsetAsync( c->fin.dCursor.ptr, 0, 2*sizeof(uint32_t), stream));
		if (exclusive) HIP_CHECK( hipMemsetAsync( c->fin.dCovered.ptr, 0, devResults+1, stream));
		if (canonical) HIP_CHECK( hipMemsetAsync( c->fin.dSortCursor.ptr, 0, sizeof(uint32_t), stream));
		FinishParams F;
		std::memset( &F, 0, sizeof(F));
		F.results = (const uint32_t*)c->io.results.ptr(); F.items = (const uint32_t*)c->io.items.ptr();
		F.docRange = (const uint64_t*)c->io.dDocRange.ptr; F.docStatus = (const int32_t*)c->io.dDocStatus.ptr;
		F.resultFormat = (const uint32_t*)c->io.dResultFormat.ptr; F.itemFormat = (const uint32_t*)c->io.dItemFormat.ptr;
		F.nofResults = devResults; F.nofItems = devItems;
		F.ndocs = (uint32_t)ndocs; F.withFormats = c->io.withFormats ? 1u : 0u;
		F.exclusive = exclusive ? 1u : 0u; F.maxResultSize = c->inst->compiler.maxResultSize();
		F.covered = (uint8_t*)c->fin.dCovered.ptr; F.kept = (uint32_t*)c->fin.dKept.ptr; F.cursor = (uint32_t*)c->fin.dCursor.ptr;
		F.outResults = (uint32_t*)c->fin.dResults.ptr; F.outItems = (uint32_t*)c->fin.dItems.ptr;
		F.docResultOffsets = (uint64_t*)c->fin.dDocResultOffsets.ptr; F.docItemOffsets = (uint64_t*)c->fin.dDocItemOffsets.ptr;
		F.outResultFormat = (uint32_t*)c->fin.dResultFormat.ptr; F.outItemFormat = (uint32_t*)c->fin.dItemFormat.ptr;
		F.totals = (uint64_t*)c->fin.dTotals.ptr;
		if (canonical)
		{
			F.canonical = 1;
			for (int i=0; i<2; ++i) { F.sortKeys[ i] = (uint64_t*)c->fin.dSortKeys[ i].ptr; F.sortIdx[ i] = (uint32_t*)c->fin.dSortIdx[ i].ptr; }
			F.sortCursor = (uint32_t*)c->fin.dSortCursor.ptr;
		}
		HIP_CHECK( launchL2Finish( F, c->numCUs, stream, ev));
		c->fin.run.completed( stream); c->fin.canonical = canonical;
		if (out)
		{
			out->ndocs = ndocs;
			out->d_results = c->fin.dResults.ptr; out->d_items = c->fin.dItems.ptr;
			out->d_doc_result_offsets = c->fin.dDocResultOffsets.ptr; out->d_doc_item_offsets = c->fin.dDocItemOffsets.ptr;
			out->d_result_format = c->io.withFormats ? c->fin.dResultFormat.ptr : 0;
			out->d_item_format = c->io.withFormats ? c->fin.dItemFormat.ptr : 0;
			out->d_totals = c->fin.dTotals.ptr;
		}
	});
}

// plain copy of the finished buffers: nothing is regrouped or eliminated on the host
int sp_matcher_ctx_finished_fetch( sp_matcher_ctx_t* c, sp_match_batch_t* out)
{
	std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		if (!c->fin.run.done) throw std::runtime_error( "the last batch of this context has not been finished (sp_matcher_ctx_batch_finish_device)");
		HIP_CHECK( hipSetDevice( c->device));
		HIP_CHECK( hipStreamSynchronize( c->fin.run.stream));
		const size_t ndocs = c->lastNdocs;
		uint64_t totals[ 2];
		copySync( c->own, totals, c->fin.dTotals.ptr, sizeof(totals), hipMemcpyDeviceToHost);
		allocMatchBatch( out, ndocs, totals[ 0], totals[ 1], c->io.withFormats);
		if (totals[ 0]) copySync( c->own, out->results, c->fin.dResults.ptr, totals[ 0]*sizeof(sp_result_t), hipMemcpyDeviceToHost);
		if (totals[ 1]) copySync( c->own, out->items, c->fin.dItems.ptr, totals[ 1]*sizeof(sp_result_item_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->doc_result_offsets, c->fin.dDocResultOffsets.ptr, (ndocs+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (ndocs)
		{
			copySync( c->own, out->doc_stats, c->io.dDocStats.ptr, ndocs*4*sizeof(uint64_t), hipMemcpyDeviceToHost);
			copySync( c->own, out->doc_status, c->io.dDocStatus.ptr, ndocs*sizeof(int32_t), hipMemcpyDeviceToHost);
		}
		if (c->io.withFormats)
		{
			if (totals[ 0]) copySync( c->own, out->result_format, c->fin.dResultFormat.ptr, totals[ 0]*sizeof(uint32_t), hipMemcpyDeviceToHost);
			if (totals[ 1]) copySync( c->own, out->item_format, c->fin.dItemFormat.ptr, totals[ 1]*2*sizeof(uint32_t), hipMemcpyDeviceToHost);
		}
	});
}

// durations of the three passes of the last finish in milliseconds (HIP events on its stream)
int sp_matcher_ctx_last_finish_ms( sp_matcher_ctx_t* c, double* count_ms, double* offsets_ms, double* place_ms)
{
	*offsets_ms = *place_ms = -1.0;
	// (a canonical finish sorts between the offsets and the placement: the placement starts at ev[4] then)
	int rc = c->fin.run.ms( 0, 1, count_ms);
	if (rc == SP_OK) rc = c->fin.run.ms( 1, 2, offsets_ms);
	if (rc == SP_OK) rc = c->fin.run.ms( c->fin.canonical ? 4 : 2, 3, place_ms);
	return rc;
}

// duration of the sorting pass of the last finish (0.0 after a finish without SP_FINISH_CANONICAL)
int sp_matcher_ctx_last_finish_sort_ms( sp_matcher_ctx_t* c, double* sort_ms)
{
	if (c->fin.run.evValid && !c->fin.canonical) { *sort_ms = 0.0; return SP_OK; }
	return c->fin.run.ms( 2, 4, sort_ms);
}

uint32_t sp_matcher_finish_sort_tile(void) { return FINISH_SORT_TILE; }

// ---- the text that the results and items of the finished batch cover, gathered on the device (l2_text.h)
namespace {
// grow-only, a failure is SP_ERR_NOMEM (the buffer is left empty, the context usable)
void reserveOrNoMem( DeviceBuffer& buf, size_t n)
{
	try { buf.reserve( n); }
	catch (const HipError&) { (void)hipGetLastError(); throw std::bad_alloc(); }
}
}

int sp_matcher_ctx_finished_text_device( sp_matcher_ctx_t* c, const sp_text_source_t* src, uint32_t flags, void* stream_, sp_match_text_batch_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		if (!flags || (flags & ~(uint32_t)(SP_TEXT_RESULTS | SP_TEXT_ITEMS))) throw std::runtime_error( "unknown or no text flags");
		if (!src || !src->d_seg_offsets || (!src->d_text && src->nbytes)) throw std::runtime_error( "no text source");
		if (!c->fin.run.done) throw std::runtime_error( "the last batch of this context has not been finished (sp_matcher_ctx_batch_finish_device)");
		const size_t ndocs = c->lastNdocs;
		if (!src->d_doc_seg_offsets && src->nseg != ndocs) throw std::runtime_error( "without document segment offsets every document is one segment: nseg must be ndocs");
		sp_matcher_ctx::Text& t = c->txt;
		hipStream_t stream = (hipStream_t)stream_;
		HIP_CHECK( hipSetDevice( c->device));
		t.run.done = t.run.evValid = false;
		// the span arrays are sized from the totals of the finish: this read waits for it
		HIP_CHECK( hipStreamSynchronize( c->fin.run.stream));
		uint64_t records[ 2];
		copySync( c->own, records, c->fin.dTotals.ptr, sizeof(records), hipMemcpyDeviceToHost);
		for (int f=0; f<2; ++f) if (flags & (1u << f))
		{
			reserveOrNoMem( t.dSpanWork[ f], (records[ f]+1)*sizeof(uint32_t));
			reserveOrNoMem( t.dSpanOffsets[ f], (records[ f]+1)*sizeof(uint64_t));
			reserveOrNoMem( t.dDocBytes[ f], (ndocs+1)*sizeof(uint64_t));
			reserveOrNoMem( t.dDocTextOffsets[ f], (ndocs+1)*sizeof(uint64_t));
		}
		reserveOrNoMem( t.dStatus, (ndocs+1)*sizeof(int32_t));
		reserveOrNoMem( t.dTotals, 2*sizeof(uint64_t));
		reserveOrNoMem( t.dCursor, 4*sizeof(uint32_t));

		// another stream than the finish's runs behind the finish
		t.run.begin( stream, c->fin.run.stream, c->fin.run.ev[ 3]);
		HIP_CHECK( hipMemsetAsync( t.dCursor.ptr, 0, 4*sizeof(uint32_t), stream));
		HIP_CHECK( hipMemsetAsync( t.dTotals.ptr, 0, 2*sizeof(uint64_t), stream));
		HIP_CHECK( hipMemsetAsync( t.dStatus.ptr, 0, (ndocs+1)*sizeof(int32_t), stream));
		TextParams P;
		std::memset( &P, 0, sizeof(P));
		P.text = (const uint8_t*)src->d_text; P.nbytes = src->nbytes;
		P.segOffsets = (const uint64_t*)src->d_seg_offsets; P.nseg = src->nseg;
		P.docSegOffsets = (const uint64_t*)src->d_doc_seg_offsets;
		P.ndocs = (uint32_t)ndocs; P.docStatus = (int32_t*)t.dStatus.ptr; P.families = flags;
		for (int f=0; f<2; ++f) if (flags & (1u << f))
		{
			TextFamily& F = P.family[ f];
			F.records = (const uint32_t*)(f ? c->fin.dItems.ptr : c->fin.dResults.ptr);
			F.docOffsets = (const uint64_t*)(f ? c->fin.dDocItemOffsets.ptr : c->fin.dDocResultOffsets.ptr);
			F.nrecords = records[ f];
			F.spanWork = (uint32_t*)t.dSpanWork[ f].ptr; F.docBytes = (uint64_t*)t.dDocBytes[ f].ptr;
			F.docTextOffsets = (uint64_t*)t.dDocTextOffsets[ f].ptr; F.spanOffsets = (uint64_t*)t.dSpanOffsets[ f].ptr;
			F.total = (uint64_t*)t.dTotals.ptr + f; F.cursor = (uint32_t*)t.dCursor.ptr + 2*f;
		}
		HIP_CHECK( hipEventRecord( t.run.ev[ 0], stream));
		HIP_CHECK( launchL2TextCount( P, c->numCUs, stream));
		// the text buffers are sized from what the passes counted: this read waits for them, the placement below is not waited for
		HIP_CHECK( hipStreamSynchronize( stream));
		uint64_t totals[ 2];
		copySync( c->own, totals, t.dTotals.ptr, sizeof(totals), hipMemcpyDeviceToHost);
		for (int f=0; f<2; ++f) if (flags & (1u << f))
		{
			reserveOrNoMem( t.dText[ f], totals[ f] + 16);
			P.family[ f].outText = (uint8_t*)t.dText[ f].ptr; P.family[ f].outCapacity = totals[ f];
		}
		HIP_CHECK( launchL2TextPlace( P, c->numCUs, stream));
		HIP_CHECK( hipEventRecord( t.run.ev[ 1], stream));
		t.run.completed( stream); t.flags = flags; t.ndocs = ndocs;
		for (int f=0; f<2; ++f) { t.nrecords[ f] = records[ f]; t.totals[ f] = (flags & (1u << f)) ? totals[ f] : 0; }
		if (out)
		{
			out->ndocs = ndocs;
			if (flags & SP_TEXT_RESULTS) { out->d_result_text = t.dText[ 0].ptr; out->d_result_text_offsets = t.dSpanOffsets[ 0].ptr; }
			if (flags & SP_TEXT_ITEMS) { out->d_item_text = t.dText[ 1].ptr; out->d_item_text_offsets = t.dSpanOffsets[ 1].ptr; }
			out->d_doc_text_status = t.dStatus.ptr; out->d_totals = t.dTotals.ptr;
		}
	});
}

// plain copy of the text buffers
int sp_matcher_ctx_finished_text_fetch( sp_matcher_ctx_t* c, sp_match_text_t* out)
{
	std::memset( out, 0, sizeof(*out));
	const int rc = guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		const sp_matcher_ctx::Text& t = c->txt;
		if (!t.run.done) throw std::runtime_error( "no text of the last batch of this context (sp_matcher_ctx_finished_text_device)");
		HIP_CHECK( hipSetDevice( c->device));
		HIP_CHECK( hipStreamSynchronize( t.run.stream));
		allocMatchText( out, t.ndocs, t.nrecords[ 0], t.nrecords[ 1], t.flags);
		out->totals[ 0] = t.totals[ 0]; out->totals[ 1] = t.totals[ 1];
		allocMatchTextBytes( out, t.flags);
		if (t.ndocs) copySync( c->own, out->doc_text_status, t.dStatus.ptr, t.ndocs*sizeof(int32_t), hipMemcpyDeviceToHost);
		char* const text[ 2] = {out->result_text, out->item_text};
		uint64_t* const offsets[ 2] = {out->result_text_offsets, out->item_text_offsets};
		for (int f=0; f<2; ++f) if (t.flags & (1u << f))
		{
			copySync( c->own, offsets[ f], t.dSpanOffsets[ f].ptr, (t.nrecords[ f]+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
			if (t.totals[ f]) copySync( c->own, text[ f], t.dText[ f].ptr, t.totals[ f], hipMemcpyDeviceToHost);
		}
	});
	if (rc != SP_OK) sp_match_text_free( out);
	return rc;
}

// duration of the passes of the last text call in milliseconds (HIP events on its stream)
int sp_matcher_ctx_last_text_ms( sp_matcher_ctx_t* c, double* ms) { return c->txt.run.ms( 0, 1, ms); }

uint32_t sp_matcher_text_long_span(void) { return TEXT_LONG_SPAN; }

// ---- the values of the format strings of the finished batch, built on the device (l2_values.h)
int sp_matcher_ctx_finished_values_device( sp_matcher_ctx_t* c, const sp_text_source_t* src, uint32_t flags, void* stream_, sp_match_values_batch_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		if (!flags || (flags & ~(uint32_t)(SP_VALUE_RESULTS | SP_VALUE_ITEMS))) throw std::runtime_error( "unknown or no value flags");
		if (!src || !src->d_seg_offsets || (!src->d_text && src->nbytes)) throw std::runtime_error( "no text source");
		if (!c->fin.run.done) throw std::runtime_error( "the last batch of this context has not been finished (sp_matcher_ctx_batch_finish_device)");
		const size_t ndocs = c->lastNdocs;
		if (!src->d_doc_seg_offsets && src->nseg != ndocs) throw std::runtime_error( "without document segment offsets every document is one segment: nseg must be ndocs");
		const FormatTable& table = c->inst->formats();
		if (!table.error.empty()) throw std::runtime_error( table.error);
		sp_matcher_ctx::Values& v = c->val;
		hipStream_t stream = (hipStream_t)stream_;
		HIP_CHECK( hipSetDevice( c->device));
		v.run.done = v.run.evValid = false;
		if (!v.uploaded)
		{
			// the format table: once per context
			reserveOrNoMem( v.dFmtParts, (table.fmtParts.size()+1)*sizeof(uint32_t));
			reserveOrNoMem( v.dParts, (table.parts.size()+1)*sizeof(uint32_t));
			reserveOrNoMem( v.dPool, table.pool.size()+16);
			copySync( c->own, v.dFmtParts.ptr, table.fmtParts.data(), table.fmtParts.size()*sizeof(uint32_t), hipMemcpyHostToDevice);
			if (!table.parts.empty()) copySync( c->own, v.dParts.ptr, table.parts.data(), table.parts.size()*sizeof(uint32_t), hipMemcpyHostToDevice);
			if (!table.pool.empty()) copySync( c->own, v.dPool.ptr, table.pool.data(), table.pool.size(), hipMemcpyHostToDevice);
			v.poolBytes = (uint32_t)table.pool.size();
			v.uploaded = true;
		}
		// the value arrays are sized from the totals of the finish: this read waits for it
		HIP_CHECK( hipStreamSynchronize( c->fin.run.stream));
		uint64_t records[ 2];
		copySync( c->own, records, c->fin.dTotals.ptr, sizeof(records), hipMemcpyDeviceToHost);
		for (int f=0; f<2; ++f) if (flags & (1u << f))
		{
			reserveOrNoMem( v.dValueWork[ f], (records[ f]+1)*sizeof(uint32_t));
			reserveOrNoMem( v.dValueOffsets[ f], (records[ f]+1)*sizeof(uint64_t));
			reserveOrNoMem( v.dDocBytes[ f], (ndocs+1)*sizeof(uint64_t));
			reserveOrNoMem( v.dDocValueOffsets[ f], (ndocs+1)*sizeof(uint64_t));
		}
		reserveOrNoMem( v.dStatus, (ndocs+1)*sizeof(int32_t));
		reserveOrNoMem( v.dTotals, 2*sizeof(uint64_t));
		reserveOrNoMem( v.dCursor, 4*sizeof(uint32_t));

		// another stream than the finish's runs behind the finish
		v.run.begin( stream, c->fin.run.stream, c->fin.run.ev[ 3]);
		HIP_CHECK( hipMemsetAsync( v.dCursor.ptr, 0, 4*sizeof(uint32_t), stream));
		HIP_CHECK( hipMemsetAsync( v.dTotals.ptr, 0, 2*sizeof(uint64_t), stream));
		HIP_CHECK( hipMemsetAsync( v.dStatus.ptr, 0, (ndocs+1)*sizeof(int32_t), stream));
		// a matcher without format strings has no format arrays: every value is empty, the passes only lay out the offsets
		const bool withFormats = c->io.withFormats && table.count;
		for (int f=0; f<2; ++f) if ((flags & (1u << f)) && !withFormats)
		{
			HIP_CHECK( hipMemsetAsync( v.dValueOffsets[ f].ptr, 0, (records[ f]+1)*sizeof(uint64_t), stream));
		}
		ValuesParams P;
		std::memset( &P, 0, sizeof(P));
		P.text = (const uint8_t*)src->d_text; P.nbytes = src->nbytes;
		P.segOffsets = (const uint64_t*)src->d_seg_offsets; P.nseg = src->nseg;
		P.docSegOffsets = (const uint64_t*)src->d_doc_seg_offsets;
		P.fmtParts = (const uint32_t*)v.dFmtParts.ptr; P.parts = (const uint32_t*)v.dParts.ptr; P.pool = (const uint8_t*)v.dPool.ptr;
		P.formatCount = table.count; P.poolBytes = v.poolBytes;
		P.items = (const uint32_t*)c->fin.dItems.ptr; P.itemFormat = (const uint32_t*)c->fin.dItemFormat.ptr;
		P.docItemOffsets = (const uint64_t*)c->fin.dDocItemOffsets.ptr; P.nitems = records[ 1];
		P.ndocs = (uint32_t)ndocs; P.docStatus = (int32_t*)v.dStatus.ptr; P.families = withFormats ? flags : 0;
		for (int f=0; f<2; ++f) if (flags & (1u << f))
		{
			ValuesFamily& F = P.family[ f];
			F.records = (const uint32_t*)(f ? c->fin.dItems.ptr : c->fin.dResults.ptr);
			F.format = (const uint32_t*)(f ? c->fin.dItemFormat.ptr : c->fin.dResultFormat.ptr);
			F.docOffsets = (const uint64_t*)(f ? c->fin.dDocItemOffsets.ptr : c->fin.dDocResultOffsets.ptr);
			F.nrecords = records[ f];
			F.valueWork = (uint32_t*)v.dValueWork[ f].ptr; F.docBytes = (uint64_t*)v.dDocBytes[ f].ptr;
			F.docValueOffsets = (uint64_t*)v.dDocValueOffsets[ f].ptr; F.valueOffsets = (uint64_t*)v.dValueOffsets[ f].ptr;
			F.total = (uint64_t*)v.dTotals.ptr + f; F.cursor = (uint32_t*)v.dCursor.ptr + 2*f;
		}
		HIP_CHECK( hipEventRecord( v.run.ev[ 0], stream));
		HIP_CHECK( launchL2ValuesCount( P, c->numCUs, stream));
		// the value buffers are sized from what the passes counted: this read waits for them, the placement below is not waited for
		HIP_CHECK( hipStreamSynchronize( stream));
		uint64_t totals[ 2];
		copySync( c->own, totals, v.dTotals.ptr, sizeof(totals), hipMemcpyDeviceToHost);
		for (int f=0; f<2; ++f) if (flags & (1u << f))
		{
			reserveOrNoMem( v.dValues[ f], totals[ f] + 16);
			P.family[ f].outValues = (uint8_t*)v.dValues[ f].ptr; P.family[ f].outCapacity = totals[ f];
		}
		HIP_CHECK( launchL2ValuesPlace( P, c->numCUs, stream));
		HIP_CHECK( hipEventRecord( v.run.ev[ 1], stream));
		v.run.completed( stream); v.flags = flags; v.ndocs = ndocs;
		for (int f=0; f<2; ++f) { v.nrecords[ f] = records[ f]; v.totals[ f] = (flags & (1u << f)) ? totals[ f] : 0; }
		if (out)
		{
			out->ndocs = ndocs;
			if (flags & SP_VALUE_RESULTS) { out->d_result_values = v.dValues[ 0].ptr; out->d_result_value_offsets = v.dValueOffsets[ 0].ptr; }
			if (flags & SP_VALUE_ITEMS) { out->d_item_values = v.dValues[ 1].ptr; out->d_item_value_offsets = v.dValueOffsets[ 1].ptr; }
			out->d_doc_value_status = v.dStatus.ptr; out->d_totals = v.dTotals.ptr;
		}
	});
}

// plain copy of the value buffers
int sp_matcher_ctx_finished_values_fetch( sp_matcher_ctx_t* c, sp_match_values_t* out)
{
	std::memset( out, 0, sizeof(*out));
	const int rc = guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		const sp_matcher_ctx::Values& v = c->val;
		if (!v.run.done) throw std::runtime_error( "no values of the last batch of this context (sp_matcher_ctx_finished_values_device)");
		HIP_CHECK( hipSetDevice( c->device));
		HIP_CHECK( hipStreamSynchronize( v.run.stream));
		allocMatchValues( out, v.ndocs, v.nrecords[ 0], v.nrecords[ 1], v.flags);
		out->totals[ 0] = v.totals[ 0]; out->totals[ 1] = v.totals[ 1];
		allocMatchValuesBytes( out, v.flags);
		if (v.ndocs) copySync( c->own, out->doc_value_status, v.dStatus.ptr, v.ndocs*sizeof(int32_t), hipMemcpyDeviceToHost);
		char* const bytes[ 2] = {out->result_values, out->item_values};
		uint64_t* const offsets[ 2] = {out->result_value_offsets, out->item_value_offsets};
		for (int f=0; f<2; ++f) if (v.flags & (1u << f))
		{
			copySync( c->own, offsets[ f], v.dValueOffsets[ f].ptr, (v.nrecords[ f]+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
			if (v.totals[ f]) copySync( c->own, bytes[ f], v.dValues[ f].ptr, v.totals[ f], hipMemcpyDeviceToHost);
		}
	});
	if (rc != SP_OK) sp_match_values_free( out);
	return rc;
}

// duration of the passes of the last values call in milliseconds (HIP events on its stream)
int sp_matcher_ctx_last_values_ms( sp_matcher_ctx_t* c, double* ms) { return c->val.run.ms( 0, 1, ms); }

uint32_t sp_matcher_value_max_depth(void) { return VALUE_MAX_DEPTH; }

// the same rule over host arrays (result_values.hpp)
int sp_match_batch_values( const sp_matcher_t* m, const sp_match_batch_t* mb, const char* text, uint64_t nbytes, const uint64_t* seg_offsets,
			   size_t nseg, const uint64_t* doc_seg_offsets, uint32_t flags, sp_match_values_t* out, char* err, size_t errsize)
{
	std::memset( out, 0, sizeof(*out));
	copyText( err, errsize, "");
	try
	{
		if (!m) throw std::runtime_error( "no matcher");
		if (!mb) throw std::runtime_error( "no batch");
		const TextSource S = { text, nbytes, seg_offsets, nseg, doc_seg_offsets };
		matchBatchValues( m->formats(), *mb, S, flags, out);
		return SP_OK;
	}
	catch (const std::bad_alloc&) { sp_match_values_free( out); return SP_ERR_NOMEM; }
	catch (const std::exception& e)
	{
		sp_match_values_free( out);
		copyText( err, errsize, e.what());
		return SP_ERR_INVALID;
	}
}

// ---- the pattern frequencies of the finished batch, summed on the device (l2_freq.h)
int sp_matcher_ctx_finished_pattern_freq_device( sp_matcher_ctx_t* c, void* stream_, sp_pattern_freq_device_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		if (!c->fin.run.done) throw std::runtime_error( "the last batch of this context has not been finished (sp_matcher_ctx_batch_finish_device)");
		const size_t ndocs = c->lastNdocs;
		const uint32_t bound = sp_matcher_handle_bound( c->inst);
		sp_matcher_ctx::Freq& q = c->frq;
		hipStream_t stream = (hipStream_t)stream_;
		HIP_CHECK( hipSetDevice( c->device));
		q.run.done = q.run.evValid = false;
		// every result index is checked against the total of the finish: this read waits for it
		HIP_CHECK( hipStreamSynchronize( c->fin.run.stream));
		uint64_t finished[ 2];
		copySync( c->own, finished, c->fin.dTotals.ptr, sizeof(finished), hipMemcpyDeviceToHost);
		reserveOrNoMem( q.dDocCount, (ndocs+1)*sizeof(uint32_t));
		reserveOrNoMem( q.dDocMeta, (ndocs+1)*4*sizeof(uint32_t));
		reserveOrNoMem( q.dStatus, (ndocs+1)*sizeof(int32_t));
		reserveOrNoMem( q.dDocOffsets, (ndocs+1)*sizeof(uint64_t));
		reserveOrNoMem( q.dHandleResults, (size_t)bound*sizeof(uint64_t));
		reserveOrNoMem( q.dHandleDocs, (size_t)bound*sizeof(uint32_t));
		reserveOrNoMem( q.dTotals, sizeof(uint64_t));
		reserveOrNoMem( q.dCursor, 2*sizeof(uint32_t));

		// another stream than the finish's runs behind the finish
		q.run.begin( stream, c->fin.run.stream, c->fin.run.ev[ 3]);
		HIP_CHECK( hipMemsetAsync( q.dCursor.ptr, 0, 2*sizeof(uint32_t), stream));
		HIP_CHECK( hipMemsetAsync( q.dTotals.ptr, 0, sizeof(uint64_t), stream));
		HIP_CHECK( hipMemsetAsync( q.dStatus.ptr, 0, (ndocs+1)*sizeof(int32_t), stream));
		HIP_CHECK( hipMemsetAsync( q.dHandleResults.ptr, 0, (size_t)bound*sizeof(uint64_t), stream));
		HIP_CHECK( hipMemsetAsync( q.dHandleDocs.ptr, 0, (size_t)bound*sizeof(uint32_t), stream));
		FreqParams P;
		std::memset( &P, 0, sizeof(P));
		P.results = (const uint32_t*)c->fin.dResults.ptr; P.docOffsets = (const uint64_t*)c->fin.dDocResultOffsets.ptr;
		P.nresults = finished[ 0]; P.ndocs = (uint32_t)ndocs; P.handleBound = bound;
		P.docCount = (uint32_t*)q.dDocCount.ptr; P.docMeta = (uint32_t*)q.dDocMeta.ptr; P.cursor = (uint32_t*)q.dCursor.ptr;
		P.docStatus = (int32_t*)q.dStatus.ptr; P.docFreqOffsets = (uint64_t*)q.dDocOffsets.ptr; P.total = (uint64_t*)q.dTotals.ptr;
		P.handleResults = (uint64_t*)q.dHandleResults.ptr; P.handleDocs = (uint32_t*)q.dHandleDocs.ptr;
		HIP_CHECK( hipEventRecord( q.run.ev[ 0], stream));
		HIP_CHECK( launchL2FreqCount( P, c->numCUs, stream));
		// the records are sized from what the passes counted: this read waits for them, the passes below are not waited for
		HIP_CHECK( hipStreamSynchronize( stream));
		uint64_t total = 0;
		copySync( c->own, &total, q.dTotals.ptr, sizeof(total), hipMemcpyDeviceToHost);
		reserveOrNoMem( q.dRecords, (total+1)*sizeof(sp_pattern_freq_t));
		P.records = (uint32_t*)q.dRecords.ptr; P.capacity = total;
		if (total) HIP_CHECK( hipMemsetAsync( q.dRecords.ptr, 0, total*sizeof(sp_pattern_freq_t), stream));
		HIP_CHECK( launchL2FreqPlace( P, c->numCUs, stream));
		HIP_CHECK( hipEventRecord( q.run.ev[ 1], stream));
		q.run.completed( stream); q.ndocs = ndocs; q.handleBound = bound; q.total = total;
		if (out)
		{
			out->ndocs = ndocs; out->handle_bound = bound;
			out->d_records = q.dRecords.ptr; out->d_doc_offsets = q.dDocOffsets.ptr; out->d_doc_freq_status = q.dStatus.ptr;
			out->d_handle_results = q.dHandleResults.ptr; out->d_handle_docs = q.dHandleDocs.ptr; out->d_totals = q.dTotals.ptr;
		}
	});
}

// plain copy of the frequency buffers
int sp_matcher_ctx_finished_pattern_freq_fetch( sp_matcher_ctx_t* c, sp_pattern_freq_batch_t* out)
{
	std::memset( out, 0, sizeof(*out));
	const int rc = guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		const sp_matcher_ctx::Freq& q = c->frq;
		if (!q.run.done) throw std::runtime_error( "no pattern frequencies of the last batch of this context (sp_matcher_ctx_finished_pattern_freq_device)");
		HIP_CHECK( hipSetDevice( c->device));
		HIP_CHECK( hipStreamSynchronize( q.run.stream));
		allocPatternFreq( out, q.ndocs, q.handleBound);
		allocPatternFreqRecords( out, q.total);
		if (q.total) copySync( c->own, out->records, q.dRecords.ptr, q.total*sizeof(sp_pattern_freq_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->doc_offsets, q.dDocOffsets.ptr, (q.ndocs+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (q.ndocs) copySync( c->own, out->doc_freq_status, q.dStatus.ptr, q.ndocs*sizeof(int32_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->handle_results, q.dHandleResults.ptr, (size_t)q.handleBound*sizeof(uint64_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->handle_docs, q.dHandleDocs.ptr, (size_t)q.handleBound*sizeof(uint32_t), hipMemcpyDeviceToHost);
	});
	if (rc != SP_OK) sp_pattern_freq_batch_free( out);
	return rc;
}

// duration of the passes of the last frequency call in milliseconds (HIP events on its stream)
int sp_matcher_ctx_last_pattern_freq_ms( sp_matcher_ctx_t* c, double* ms) { return c->frq.run.ms( 0, 1, ms); }

uint32_t sp_matcher_pattern_freq_window(void) { return FREQ_WINDOW; }

// ---- the index terms of the finished batch, grouped on the device (l2_terms.h)
namespace {
// test hook: the bits of a term's hash that the device keeps (32 and more = all)
std::atomic<unsigned>& termHashBits() { static std::atomic<unsigned> bits( 32); return bits; }
}

void sp_test_term_hash_bits( unsigned bits) { termHashBits().store( bits, std::memory_order_relaxed); }

int sp_matcher_ctx_finished_terms_device( sp_matcher_ctx_t* c, uint32_t flags, void* stream_, sp_match_terms_device_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		if (!flags || (flags & ~(uint32_t)(SP_TERM_VALUES | SP_TERM_TEXT))) throw std::runtime_error( "unknown or no term flags");
		if (!c->fin.run.done) throw std::runtime_error( "the last batch of this context has not been finished (sp_matcher_ctx_batch_finish_device)");
		const sp_matcher_ctx::Values& v = c->val;
		const sp_matcher_ctx::Text& x = c->txt;
		if ((flags & SP_TERM_VALUES) && !(v.run.done && (v.flags & SP_VALUE_RESULTS)))
			throw std::runtime_error( "no values of the results of the last finished batch (sp_matcher_ctx_finished_values_device with SP_VALUE_RESULTS)");
		if ((flags & SP_TERM_TEXT) && !(x.run.done && (x.flags & SP_TEXT_RESULTS)))
			throw std::runtime_error( "no text of the results of the last finished batch (sp_matcher_ctx_finished_text_device with SP_TEXT_RESULTS)");
		const size_t ndocs = c->lastNdocs;
		const uint32_t bound = sp_matcher_handle_bound( c->inst);
		sp_matcher_ctx::Terms& t = c->trm;
		hipStream_t stream = (hipStream_t)stream_;
		HIP_CHECK( hipSetDevice( c->device));
		t.run.done = t.run.evValid = false;
		// every result index is checked against the total of the finish: this read waits for it
		HIP_CHECK( hipStreamSynchronize( c->fin.run.stream));
		uint64_t finished[ 2];
		copySync( c->own, finished, c->fin.dTotals.ptr, sizeof(finished), hipMemcpyDeviceToHost);
		const uint64_t nresults = finished[ 0];
		if ((flags & SP_TERM_VALUES) && v.nrecords[ 0] != nresults) throw std::runtime_error( "the values are not those of the finished batch");
		if ((flags & SP_TERM_TEXT) && x.nrecords[ 0] != nresults) throw std::runtime_error( "the text is not that of the finished batch");
		const unsigned waves = l2TermsWaves( ndocs, c->numCUs);
		reserveOrNoMem( t.dLeader, (nresults+1)*sizeof(uint32_t));
		reserveOrNoMem( t.dTable, (nresults+1)*2*sizeof(uint32_t));
		reserveOrNoMem( t.dResultTerm, (nresults+1)*sizeof(uint32_t));
		reserveOrNoMem( t.dHistogram, (size_t)waves*bound*sizeof(uint32_t));
		reserveOrNoMem( t.dDocCount, (ndocs+1)*sizeof(uint32_t));
		reserveOrNoMem( t.dStatus, (ndocs+1)*sizeof(int32_t));
		reserveOrNoMem( t.dDocOffsets, (ndocs+1)*sizeof(uint64_t));
		reserveOrNoMem( t.dTotals, sizeof(uint64_t));
		reserveOrNoMem( t.dCursor, 2*sizeof(uint32_t));

		// another stream than the finish's runs behind the finish, and behind the values and the text call, whose placements
		// nobody has waited for yet
		t.run.begin( stream, c->fin.run.stream, c->fin.run.ev[ 3]);
		if ((flags & SP_TERM_VALUES) && stream != v.run.stream) HIP_CHECK( hipStreamWaitEvent( stream, v.run.ev[ 1], 0));
		if ((flags & SP_TERM_TEXT) && stream != x.run.stream) HIP_CHECK( hipStreamWaitEvent( stream, x.run.ev[ 1], 0));
		HIP_CHECK( hipMemsetAsync( t.dCursor.ptr, 0, 2*sizeof(uint32_t), stream));
		HIP_CHECK( hipMemsetAsync( t.dTotals.ptr, 0, sizeof(uint64_t), stream));
		HIP_CHECK( hipMemsetAsync( t.dStatus.ptr, 0, (ndocs+1)*sizeof(int32_t), stream));
		TermsParams P;
		std::memset( &P, 0, sizeof(P));
		P.results = (const uint32_t*)c->fin.dResults.ptr; P.docOffsets = (const uint64_t*)c->fin.dDocResultOffsets.ptr;
		P.resultFormat = c->io.withFormats ? (const uint32_t*)c->fin.dResultFormat.ptr : 0;
		P.nresults = nresults; P.ndocs = (uint32_t)ndocs; P.handleBound = bound; P.flags = flags;
		const unsigned bits = termHashBits().load( std::memory_order_relaxed);
		P.hashMask = bits >= 32 ? 0xFFFFFFFFu : ((1u << bits) - 1u);
		if (flags & SP_TERM_VALUES)
		{
			const TermSourceDevice S = { (const uint8_t*)v.dValues[ 0].ptr, (const uint64_t*)v.dValueOffsets[ 0].ptr, v.totals[ 0], (const int32_t*)v.dStatus.ptr };
			P.source[ 0] = S;
		}
		if (flags & SP_TERM_TEXT)
		{
			const TermSourceDevice S = { (const uint8_t*)x.dText[ 0].ptr, (const uint64_t*)x.dSpanOffsets[ 0].ptr, x.totals[ 0], (const int32_t*)x.dStatus.ptr };
			P.source[ 1] = S;
		}
		P.leader = (uint32_t*)t.dLeader.ptr; P.table = (uint32_t*)t.dTable.ptr; P.histogram = (uint32_t*)t.dHistogram.ptr;
		P.docCount = (uint32_t*)t.dDocCount.ptr; P.cursor = (uint32_t*)t.dCursor.ptr;
		P.docStatus = (int32_t*)t.dStatus.ptr; P.docTermOffsets = (uint64_t*)t.dDocOffsets.ptr; P.total = (uint64_t*)t.dTotals.ptr;
		P.resultTerm = (uint32_t*)t.dResultTerm.ptr;
		HIP_CHECK( hipEventRecord( t.run.ev[ 0], stream));
		HIP_CHECK( launchL2TermsCount( P, c->numCUs, stream));
		// the records are sized from what the passes counted: this read waits for them, the placement below is not waited for
		HIP_CHECK( hipStreamSynchronize( stream));
		uint64_t total = 0;
		copySync( c->own, &total, t.dTotals.ptr, sizeof(total), hipMemcpyDeviceToHost);
		reserveOrNoMem( t.dRecords, (total+1)*sizeof(sp_match_term_t));
		P.records = (uint32_t*)t.dRecords.ptr; P.capacity = total;
		HIP_CHECK( launchL2TermsPlace( P, c->numCUs, stream));
		HIP_CHECK( hipEventRecord( t.run.ev[ 1], stream));
		t.run.completed( stream); t.ndocs = ndocs; t.handleBound = bound; t.flags = flags; t.nresults = nresults; t.total = total;
		if (out)
		{
			out->ndocs = ndocs; out->handle_bound = bound; out->flags = flags;
			out->d_records = t.dRecords.ptr; out->d_doc_term_offsets = t.dDocOffsets.ptr; out->d_result_term = t.dResultTerm.ptr;
			out->d_doc_term_status = t.dStatus.ptr; out->d_totals = t.dTotals.ptr;
		}
	});
}

// plain copy of the term buffers
int sp_matcher_ctx_finished_terms_fetch( sp_matcher_ctx_t* c, sp_match_terms_t* out)
{
	std::memset( out, 0, sizeof(*out));
	const int rc = guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		const sp_matcher_ctx::Terms& t = c->trm;
		if (!t.run.done) throw std::runtime_error( "no terms of the last batch of this context (sp_matcher_ctx_finished_terms_device)");
		HIP_CHECK( hipSetDevice( c->device));
		HIP_CHECK( hipStreamSynchronize( t.run.stream));
		allocMatchTerms( out, t.ndocs, t.nresults, t.handleBound, t.flags);
		allocMatchTermRecords( out, t.total);
		if (t.total) copySync( c->own, out->records, t.dRecords.ptr, t.total*sizeof(sp_match_term_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->doc_term_offsets, t.dDocOffsets.ptr, (t.ndocs+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (t.nresults) copySync( c->own, out->result_term, t.dResultTerm.ptr, t.nresults*sizeof(uint32_t), hipMemcpyDeviceToHost);
		if (t.ndocs) copySync( c->own, out->doc_term_status, t.dStatus.ptr, t.ndocs*sizeof(int32_t), hipMemcpyDeviceToHost);
	});
	if (rc != SP_OK) sp_match_terms_free( out);
	return rc;
}

// duration of the passes of the last terms call in milliseconds (HIP events on its stream)
int sp_matcher_ctx_last_terms_ms( sp_matcher_ctx_t* c, double* ms) { return c->trm.run.ms( 0, 1, ms); }

uint32_t sp_matcher_term_tile(void) { return TERM_TILE; }

double sp_matcher_ctx_last_kernel_ms( sp_matcher_ctx_t* c) { return lastKernelMs( c); }

int sp_matcher_ctx_match_docs( sp_matcher_ctx_t* c, const sp_lexem_t* lexems, const uint32_t* origseg,
			       const uint64_t* doc_offsets, size_t ndocs, sp_match_batch_t* out)
{
	std::memset( out, 0, sizeof(*out));
	const int rc = guardedCall( c->lasterror, SP_ERR_DEVICE, [&]{
		if (ndocs >= 0xFFFFFFFFull) throw std::runtime_error( "too many documents in one batch");
		HIP_CHECK( hipSetDevice( c->device));
		size_t nlex = ndocs ? (size_t)doc_offsets[ ndocs] : 0;
		c->io.dLexems.reserve( (nlex+1)*sizeof(sp_lexem_t));
		c->io.dDocOffsets.reserve( (ndocs+1)*sizeof(uint64_t));
		if (nlex) copySync( c->own, c->io.dLexems.ptr, lexems, nlex*sizeof(sp_lexem_t), hipMemcpyHostToDevice);
		copySync( c->own, c->io.dDocOffsets.ptr, doc_offsets, (ndocs+1)*sizeof(uint64_t), hipMemcpyHostToDevice);
		const void* dseg = 0;
		if (origseg)
		{
			c->io.dOrigseg.reserve( (nlex+1)*sizeof(uint32_t));
			if (nlex) copySync( c->own, c->io.dOrigseg.ptr, origseg, nlex*sizeof(uint32_t), hipMemcpyHostToDevice);
			dseg = c->io.dOrigseg.ptr;
		}
		BatchCounts counts;
		uint64_t* counters = counts.counters;
		std::vector<uint32_t> again;		// documents whose working set exceeded the per-wave arena: only they run again
		std::vector<int32_t> st( ndocs+1);
		for (int attempt=0;; ++attempt)
		{
			launchBatch( c, c->io.dLexems.ptr, dseg, c->io.dDocOffsets.ptr, ndocs, nlex, c->own, 0, again.empty() ? 0 : &again);
			HIP_CHECK( hipStreamSynchronize( c->own));
			counts = readCounts( c);
			if (ndocs) copySync( c->own, st.data(), c->io.dDocStatus.ptr, ndocs*sizeof(int32_t), hipMemcpyDeviceToHost);
			// the output counters keep counting past the capacity: if the buffers were too small,
			// grow them to what this batch needs and run it again (the kernel is deterministic)
			bool grow = false;
			again.clear();
			if (counters[ SPC_RESULTS] > c->io.results.count) { c->io.minResults = counters[ SPC_RESULTS] + counters[ SPC_RESULTS]/8 + 1024; grow = true; }
			if (counters[ SPC_ITEMS] > c->io.items.count) { c->io.minItems = counters[ SPC_ITEMS] + counters[ SPC_ITEMS]/8 + 1024; grow = true; }
			if (counters[ SPC_FAILED])
			{
				// documents whose working set exceeded the per-wave arena: double the arena and run THEM again
				// (the whole batch only when the output buffers have to be reallocated as well)
				std::vector<uint32_t> arenaDocs;
				for (size_t di=0; di<ndocs; ++di) if (st[ di] == SPD_ERR_ARENA) arenaDocs.push_back( (uint32_t)di);
				if (!arenaDocs.empty() && sp_matcher_ctx_grow_arena( c) == SP_OK)
				{
					if (!grow) again.swap( arenaDocs);
					grow = true;
				}
			}
			if (!grow || attempt >= 12) break;
		}
		{
			// a partial rerun counts failures among the documents it ran again only: the batch's count is what the statuses say
			uint64_t failed = 0;
			for (size_t di=0; di<ndocs; ++di) if (st[ di] != 0) ++failed;
			if (failed != counters[ SPC_FAILED])
			{
				counters[ SPC_FAILED] = failed;
				copySync( c->own, (uint64_t*)c->io.dCounters.ptr + SPC_FAILED, &failed, sizeof(failed), hipMemcpyHostToDevice);
			}
		}
		copyOutBatch( c, 0, ndocs, counts, out);
		if (counters[ SPC_FAILED])
		{
			size_t bad = 0;
			while (bad < ndocs && out->doc_status[ bad] == 0) ++bad;
			char msg[ 128];
			snprintf( msg, sizeof(msg), "at least one document failed: document %zu has status %d (see doc_status)", bad, bad < ndocs ? out->doc_status[ bad] : -1);
			throw DocumentFailed( msg);
		}
	});
	// (every failure but a failed document is SP_ERR_DEVICE here, out of memory too; sp_lexer_ctx_match_docs passes the code on)
	return (rc == SP_OK || rc == SP_ERR_MATCH) ? rc : SP_ERR_DEVICE;
}

void sp_match_batch_free( sp_match_batch_t* b)
{
	std::free( b->results); std::free( b->items); std::free( b->doc_result_offsets);
	std::free( b->doc_stats); std::free( b->doc_status); std::free( b->result_format); std::free( b->item_format);
	std::memset( b, 0, sizeof(*b));
}

// ---- single-document mode: PatternMatcherContextInterface ----
int sp_matcher_ctx_put_input( sp_matcher_ctx_t* c, const sp_lexem_t* lexems, const uint32_t* origseg, size_t n)
{
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		// ascending-order contract checked up front like the reference does per call (src/patternMatcher.cpp:136-139)
		uint32_t cur = c->cur.lexems.empty() ? 0 : c->cur.lexems.back().ordpos;
		for (size_t i=0; i<n; ++i)
		{
			if (lexems[i].ordpos < cur) throw std::runtime_error( "term events not fed in ascending order");
			cur = lexems[i].ordpos;
		}
		if (origseg && !c->cur.hasSeg) { c->cur.origseg.assign( c->cur.lexems.size(), 0); c->cur.hasSeg = true; }
		c->cur.lexems.insert( c->cur.lexems.end(), lexems, lexems+n);
		if (c->cur.hasSeg)
		{
			if (origseg) c->cur.origseg.insert( c->cur.origseg.end(), origseg, origseg+n);
			else c->cur.origseg.insert( c->cur.origseg.end(), n, 0u);
		}
	});
}

int sp_matcher_ctx_fetch_results( sp_matcher_ctx_t* c, sp_result_t** results, size_t* nresults,
				  sp_result_item_t** items, size_t* nitems)
{
	uint64_t offs[2] = {0, (uint64_t)c->cur.lexems.size()};
	sp_match_batch_t b;
	sp_lexem_t dummy = {0,0,0,0};
	int rc = sp_matcher_ctx_match_docs( c, c->cur.lexems.empty() ? &dummy : c->cur.lexems.data(),
					c->cur.hasSeg ? c->cur.origseg.data() : 0, offs, 1, &b);
	if (rc != SP_OK && rc != SP_ERR_MATCH) { sp_match_batch_free( &b); return rc; }
	if (rc == SP_ERR_MATCH)
	{
		static const char* msg[] = {"ok", "term events not fed in ascending order", "working set of the document exceeds the arena",
			"pattern with too many identical key events defined", "internal: encountered past trigger with follow",
			"term event out of range", "illegal free of event data reference"};
		int st = b.doc_status ? b.doc_status[0] : 0;
		c->lasterror = std::string("failed to feed input to pattern matcher: ") + ((st >= 0 && st <= 6) ? msg[ st] : "unknown");
		sp_match_batch_free( &b);
		return SP_ERR_MATCH;
	}
	c->cur.stats.nofProgramsInstalled = (double)b.doc_stats[0];
	c->cur.stats.nofAltKeyProgramsInstalled = (double)b.doc_stats[1];
	c->cur.stats.nofSignalsFired = (double)b.doc_stats[2];
	c->cur.stats.nofTriggersAvgActive = c->cur.lexems.empty() ? 0.0 : (double)b.doc_stats[3] / (double)c->cur.lexems.size();
	c->cur.resultFormat.clear(); c->cur.itemFormat.clear();
	if (b.result_format) c->cur.resultFormat.assign( b.result_format, b.result_format + b.nresults);
	if (b.item_format) c->cur.itemFormat.assign( b.item_format, b.item_format + 2*b.nitems);
	*results = b.results; *nresults = b.nresults; b.results = 0;
	if (items) { *items = b.items; b.items = 0; }
	if (nitems) *nitems = b.nitems;
	sp_match_batch_free( &b);
	return SP_OK;
}

int sp_matcher_ctx_fetch_formats( sp_matcher_ctx_t* c, const uint32_t** result_format, const uint32_t** item_format)
{
	*result_format = c->io.withFormats ? c->cur.resultFormat.data() : 0;
	*item_format = c->io.withFormats ? c->cur.itemFormat.data() : 0;
	return SP_OK;
}

int sp_matcher_ctx_statistics( sp_matcher_ctx_t* c, sp_matcher_stats_t* out)
{
	if (c->join.on)
	{
		// result-set mode installs nothing: no numbers that would look real
		std::memset( out, 0, sizeof(*out));
		c->lasterror = "no statistics in result-set mode (nothing is installed)";
		return SP_ERR_UNAVAILABLE;
	}
	*out = c->cur.stats;
	return SP_OK;
}

int sp_matcher_ctx_reset( sp_matcher_ctx_t* c)
{
	c->cur.lexems.clear(); c->cur.origseg.clear(); c->cur.hasSeg = false;
	c->cur.resultFormat.clear(); c->cur.itemFormat.clear();
	c->cur.stats = sp_matcher_stats_t();
	return SP_OK;
}

} // extern "C"
