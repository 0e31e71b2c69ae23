// C-ABI of level 2 (include/strus_pattern_amd.h): rule compiler handle + GPU match context (capi_l2_ctx.hpp), the batch launch,
// the host entry points, single-document mode.  What is made of a finished batch: capi_l2_finished.cpp.
// No CPU fallback: a context cannot be created without a usable HIP device.
#include "capi_l2_ctx.hpp"
#include <cstdio>

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
	c->prod.drop();		// (a new batch: what was finished is of the one before)
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
