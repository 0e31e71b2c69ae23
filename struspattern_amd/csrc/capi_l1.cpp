// C-ABI of level 1 (include/strus_pattern_amd.h): lexer compiler handle + GPU lexer context.
// No CPU fallback: a context cannot be created without a usable HIP device.
#include "l1_compile.hpp"
#include "l1_image.hpp"
#include "l1_launch.h"
#include "l1_stitch.h"
#include "l2_plan.hpp"		// arenaWaves: the policy of a per-wave arena
#include "capi_util.hpp"
#include <cstdio>

using namespace spa;

struct sp_lexer
{
	LexCompiler compiler;
	mutable std::string lasterror;
};

struct sp_lexer_ctx
{
	const sp_lexer* inst = 0;
	int device = 0;
	std::string lasterror;
	DeviceBuffer dByteClass, dClassCtx, dExCount,
		dPatterns, dSymbols, dSymbolText, dLiterals, dLiteralText, dLitPats, dTableImage, dWordsImage, dPatOfBit, dApprox, dCharCp, dCharPos, dCpBlocks, dCpPages, dUnitStart, dDocSequential, dNullable,
		dScanImage, dShapePats;
	L1Images images;		// the table images behind dTableImage, dScanImage and dWordsImage (l1_image.hpp)
	DeviceBuffer dCounters, dText, dDocOffsets, dDocRange, dDocStatus, dQueue, dReportCount, dWordQueue, dWordCount;
	CountedBuffer arena;		// count: waves of arenaWords words each
	CountedBuffer lexems;		// count: sp_lexem_t
	uint32_t queueMul = 8;		// report queue between the two kernels: queueMul/16 reports per text byte (+64 per document)
	uint32_t eventCap = 32768;
	uint64_t arenaWords = 0;
	uint64_t minLexemCapacity = 0;
	unsigned numCUs = 256;
	Event evStart, evMid, evWords, evStop; bool evValid = false;
	L1LaunchPlan plan;		// of the last launch
	hipStream_t lastStream = 0; size_t lastNdocs = 0;
	// the segments of the last batch stitched to documents on the device (l1_stitch.h); nothing is allocated before the first
	// sp_lexer_ctx_stitch_segments_device
	struct Stitched
	{
		PassRun<2> run;
		DeviceBuffer dLexems, dOrigseg, dSegWork, dDocCount, dDocOffsets, dDocStatus, dTotals, dCursor;
		size_t ndocs = 0;
		uint64_t capacity = 0;		// records in dLexems and dOrigseg: the lexer's lexem capacity at the stitch
	} stitched;
	Stream own;			// the context's own stream (non-blocking): the host-buffer entry points of different contexts -- one per host thread,
				// the reference's threading model -- copy and launch side by side instead of queueing on the null stream
};

extern "C" {

sp_lexer_t* sp_lexer_create(void) { try { return new sp_lexer(); } catch (...) { return 0; } }
void sp_lexer_free( sp_lexer_t* l) { delete l; }
const char* sp_lexer_last_error( const sp_lexer_t* l) { return l->lasterror.c_str(); }

#define LGUARD( CODE, BODY) return guardedCall( l->lasterror, CODE, [&]{ BODY; })

// the compiled lexer as a blob (automaton tables, literal and symbol tables, names) and back: SURVEY.md 8(f).4
int sp_lexer_serialize( const sp_lexer_t* l, void** blob, size_t* size)
{ return exportBlob( l->lasterror, blob, size, [&]( std::vector<uint8_t>& buf){ l->compiler.save( buf); }); }
sp_lexer_t* sp_lexer_deserialize( const void* blob, size_t size, char* err, size_t errsize)
{ return importBlob<sp_lexer>( err, errsize, [&]( sp_lexer& l){ l.compiler.load( blob, size); }); }


int sp_lexer_define_lexem_name( sp_lexer_t* l, uint32_t id, const char* name)
{ LGUARD( SP_ERR_INVALID, l->compiler.defineLexemName( id, name ? name : "")); }
const char* sp_lexer_get_lexem_name( const sp_lexer_t* l, uint32_t id) { return l->compiler.getLexemName( id); }
int sp_lexer_define_lexem( sp_lexer_t* l, uint32_t id, const char* expression, uint32_t resultIndex, uint32_t level, int posbind)
{ LGUARD( SP_ERR_INVALID, l->compiler.defineLexem( id, expression ? expression : "", resultIndex, level, posbind)); }
int sp_lexer_define_symbol( sp_lexer_t* l, uint32_t symbolid, uint32_t patternid, const char* name)
{ LGUARD( SP_ERR_INVALID, l->compiler.defineSymbol( symbolid, patternid, name ? name : "")); }
uint32_t sp_lexer_get_symbol( const sp_lexer_t* l, uint32_t patternid, const char* name) { return l->compiler.getSymbol( patternid, name ? name : ""); }
int sp_lexer_define_option( sp_lexer_t* l, const char* name, double value)
{ LGUARD( SP_ERR_INVALID, l->compiler.defineOption( name ? name : "", value)); }
int sp_lexer_compile( sp_lexer_t* l)
{ LGUARD( SP_ERR_COMPILE, l->compiler.compile()); }

// Flat dump for tests: header of 8 words {nofPasses, nofClasses, maxExceptions, nofPatterns, nofPositions, nofLiterals, reportsOrdered, 0},
// byteClass[256], classCtx[nofClasses], charMask, startMask, acceptMask, shiftDst, selfLoop,
// exCount[nofPasses], exSrc, exDst, then per pattern {id, word, levelBind, prefixLen, suffixLen, mask}
size_t sp_lexer_dump_tables( const sp_lexer_t* l, uint64_t** out)
{
	const LexTables& T = l->compiler.tables();
	std::vector<uint64_t> b;
	b.push_back( T.nofPasses); b.push_back( T.nofClasses); b.push_back( T.maxExceptions); b.push_back( T.patterns.size());
	b.push_back( T.nofPositions); b.push_back( 0); b.push_back( 0); b.push_back( T.ucp ? 1 : 0);
	for (size_t i=0; i<T.byteClass.size(); ++i) b.push_back( T.byteClass[i]);
	for (size_t i=0; i<T.classCtx.size(); ++i) b.push_back( T.classCtx[i]);
	b.insert( b.end(), T.charMask.begin(), T.charMask.end());
	b.insert( b.end(), T.startMask.begin(), T.startMask.end());
	b.insert( b.end(), T.acceptMask.begin(), T.acceptMask.end());
	b.insert( b.end(), T.shiftDst.begin(), T.shiftDst.end());
	b.insert( b.end(), T.selfLoop.begin(), T.selfLoop.end());
	for (size_t i=0; i<T.exCount.size(); ++i) b.push_back( T.exCount[i]);
	b.insert( b.end(), T.exSrc.begin(), T.exSrc.end());
	b.insert( b.end(), T.exDst.begin(), T.exDst.end());
	for (size_t i=0; i<T.patterns.size(); ++i)
	{
		const DevLexPattern& p = T.patterns[i];
		b.push_back( p.id); b.push_back( p.word); b.push_back( p.levelBind); b.push_back( p.prefixLen); b.push_back( p.suffixLen);
		b.push_back( ((uint64_t)p.maskHi << 32) | p.maskLo); b.push_back( p.defIndex);
	}
	// whole-word literals: count, then per literal {len, patCount, bytes..., pattern indices...}
	b[5] = T.nofLiterals;
	b[6] = T.reportsOrdered ? 1 : 0;
	for (size_t i=0; i<T.literals.size(); ++i)
	{
		const DevLiteral& e = T.literals[i];
		if (!e.hash) continue;
		b.push_back( e.len); b.push_back( e.patCount);
		for (uint32_t k=0; k<e.len; ++k) b.push_back( T.literalText[ e.textOffset+k]);
		for (uint32_t k=0; k<e.patCount; ++k) b.push_back( T.litPats[ e.patBegin+k]);
	}
	// ALLOWEMPTY: {patterns entry, emptyOk bits} per expression that matches the empty string
	b.push_back( T.nullable.size());
	for (size_t i=0; i<T.nullable.size(); ++i) { b.push_back( T.nullable[ i].pattern); b.push_back( T.nullable[ i].emptyOk); }
	// classes by code point: block table and pages (both may be empty)
	b.push_back( T.cpBlocks.size());
	for (size_t i=0; i<T.cpBlocks.size(); ++i) b.push_back( T.cpBlocks[ i]);
	b.push_back( T.cpPages.size());
	for (size_t i=0; i<T.cpPages.size(); ++i) b.push_back( T.cpPages[ i]);
	// word shapes: passes the scan kernel runs, expressions taken as shapes, then per table entry {tag, key, patCount, pattern indices...}
	b.push_back( T.scanPasses); b.push_back( T.nofShapes);
	for (size_t i=0; i<T.shapes.size(); ++i)
	{
		const DevShape& e = T.shapes[ i];
		if (!e.tag) continue;
		b.push_back( e.tag); b.push_back( e.key); b.push_back( e.patCount);
		for (uint32_t k=0; k<e.patCount; ++k) b.push_back( T.shapePats[ e.patBegin+k]);
	}
	*out = (uint64_t*)std::malloc( (b.size()+1)*sizeof(uint64_t));
	if (!*out) return 0;
	std::memcpy( *out, b.data(), b.size()*sizeof(uint64_t));
	return b.size();
}

// Test dump of a table image (l1_image.hpp): `which` 0 = all passes, 1 = the scanned passes, 2 = the words kernel's; the eight
// offsets {oChar, oAccept, oStart, oShift, oSelf, oExSrc, oExDst, oShapeFp}, then the words (none: a table without a words kernel has no image 2)
size_t sp_lexer_dump_image( const sp_lexer_t* l, int which, uint64_t** out)
{
	*out = 0;
	try
	{
		if (!l->compiler.compiled() || which < 0 || which > 2) return 0;
		const L1Images images = buildL1Images( l->compiler.tables(), L1Switches::fromEnv());
		if (which == 2 && !images.wordsKernel) return 0;
		const L1Image& img = which == 0 ? images.all : which == 1 ? images.scan : images.words;
		const uint64_t offsets[ 8] = {img.oChar, img.oAccept, img.oStart, img.oShift, img.oSelf, img.oExSrc, img.oExDst, img.oShapeFp};
		*out = (uint64_t*)std::malloc( (8 + img.words.size() + 1)*sizeof(uint64_t));
		if (!*out) return 0;
		std::memcpy( *out, offsets, sizeof(offsets));
		if (!img.words.empty()) std::memcpy( *out + 8, img.words.data(), img.words.size()*sizeof(uint64_t));
		return 8 + img.words.size();
	}
	catch (const std::exception& e) { l->lasterror = e.what(); return 0; }
}

// What a context on a device of `num_cus` compute units would launch for a batch of `ndocs` documents and `nbytes` bytes, without a
// device: one line of key=value fields (include/strus_pattern_amd.h)
int sp_lexer_launch_plan( const sp_lexer_t* l, unsigned num_cus, size_t ndocs, size_t nbytes, char* buf, size_t bufsize)
{
	if (buf && bufsize) buf[ 0] = 0;
	return guardedCall( l->lasterror, SP_ERR_INVALID, [&]{
		if (!l->compiler.compiled()) throw std::runtime_error( "called launch plan without calling 'compile'");
		if (ndocs >= 0xFFFFFFFFull) throw std::runtime_error( "too many documents in one batch");
		const LexTables& T = l->compiler.tables();
		const L1Switches sw = L1Switches::fromEnv();
		const L1Images images = buildL1Images( T, sw);
		const L1LaunchPlan p = planL1Launch( T, images, num_cus ? num_cus : 256u, ndocs, nbytes, sw);
		char route[ 24];
		if (p.route == L1_ROUTE_PASSES) std::snprintf( route, sizeof(route), "passes(%u)", p.scanPasses);
		else std::snprintf( route, sizeof(route), "%s", p.route == L1_ROUTE_APPROX ? "approx" : p.route == L1_ROUTE_LANES ? "lanes" : "none");
		int n = std::snprintf( buf, bufsize, "route=%s cp=%d scan_kernel=%s words_kernel=%s scan_grid=%u scan_threads=%u scan_lds=%zu lane_grid=%u "
			"word_grid=%u word_waves=%u word_lds_words=%u post_grid=%u post_waves=%u chunk_bytes=%u max_units=%llu scan_words=%u post_clusters=%u "
			"image_words=%zu scan_image_words=%zu words_image_words=%zu",
			route, p.cp ? 1 : 0, p.scanKernelName, p.wordsKernelName, p.scanGrid, p.scanThreads, p.scanLdsBytes(), p.laneGrid,
			p.wordGrid, p.wordWaves, p.wordLdsWords, p.postGrid(), p.postWaves, p.chunkBytes, (unsigned long long)p.maxUnits, p.scanWords, p.postClusters,
			images.all.words.size(), images.scan.words.size(), images.wordsKernel ? images.words.words.size() : (size_t)0);
		if (n < 0 || !buf || (size_t)n >= bufsize) throw std::runtime_error( "buffer too small for the launch plan");
	});
}

sp_lexer_ctx_t* sp_lexer_ctx_create( const sp_lexer_t* l, int device)
{
	sp_lexer_ctx* c = 0;
	try
	{
		if (!l->compiler.compiled())
		{
			l->lasterror = "called create context without calling 'compile'";	// src/patternLexer.cpp:1124-1127
			return 0;
		}
		int ndev = 0;
		hipError_t e = hipGetDeviceCount( &ndev);
		if (e != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
		{
			l->lasterror = "no usable HIP device: the pattern lexer runs on the GPU only (no CPU fallback)";
			return 0;
		}
		c = new sp_lexer_ctx();
		c->inst = l; c->device = device;
		HIP_CHECK( hipSetDevice( device));
		hipDeviceProp_t prop;
		HIP_CHECK( hipGetDeviceProperties( &prop, device));
		c->numCUs = prop.multiProcessorCount > 0 ? (unsigned)prop.multiProcessorCount : 256u;
		const LexTables& T = l->compiler.tables();
		c->images = buildL1Images( T, L1Switches::fromEnv());	// (SPA_L1_NO_WORDS_KERNEL is read here; the launch switches at every launch)
		c->dByteClass.upload( T.byteClass.data(), T.byteClass.size());
		c->dClassCtx.upload( T.classCtx.data(), T.classCtx.size());
		c->dExCount.upload( T.exCount.data(), T.exCount.size()*4);
		c->dPatOfBit.upload( T.patOfBit.data(), T.patOfBit.size()*4);
		c->dPatterns.upload( T.patterns.data(), T.patterns.size()*sizeof(DevLexPattern));
		c->dSymbols.upload( T.symbols.data(), T.symbols.size()*sizeof(DevSymbol));
		c->dSymbolText.upload( T.symbolText.data(), T.symbolText.size());
		c->dLiterals.upload( T.literals.data(), T.literals.size()*sizeof(DevLiteral));
		c->dLiteralText.upload( T.literalText.data(), T.literalText.size());
		c->dLitPats.upload( T.litPats.data(), T.litPats.size()*4);
		if (!T.cpBlocks.empty()) { c->dCpBlocks.upload( T.cpBlocks.data(), T.cpBlocks.size()*2); c->dCpPages.upload( T.cpPages.data(), T.cpPages.size()); }
		if (!T.nullable.empty()) c->dNullable.upload( T.nullable.data(), T.nullable.size()*sizeof(DevNullable));
		if (!T.approx.empty()) c->dApprox.upload( T.approx.data(), T.approx.size()*sizeof(DevApproxPattern));
		c->dShapePats.upload( T.shapePats.data(), T.shapePats.size()*4);
		c->dTableImage.upload( c->images.all.words.data(), c->images.all.words.size()*8);
		c->dScanImage.upload( c->images.scan.words.data(), c->images.scan.words.size()*8);
		if (c->images.wordsKernel) c->dWordsImage.upload( c->images.words.words.data(), c->images.words.words.size()*8);
		c->dCounters.alloc( L1C_ALLOC*sizeof(uint64_t));
		c->own.create( device);
		c->evStart.create(); c->evMid.create(); c->evWords.create(); c->evStop.create();
		return c;
	}
	catch (const std::exception& e)
	{
		l->lasterror = e.what();
		delete c;
		return 0;
	}
}

void sp_lexer_ctx_free( sp_lexer_ctx_t* c) { delete c; }	// (`own` waits for its work before it goes: Stream)
const char* sp_lexer_ctx_last_error( const sp_lexer_ctx_t* c) { return c->lasterror.c_str(); }
int sp_lexer_ctx_reset( sp_lexer_ctx_t*) { return SP_OK; }	// the context keeps no per-document state between calls

int sp_lexer_ctx_reserve_output( sp_lexer_ctx_t* c, uint64_t lexems)
{
	if (lexems > c->minLexemCapacity) c->minLexemCapacity = lexems;
	return SP_OK;
}
int sp_lexer_ctx_grow_arena( sp_lexer_ctx_t* c)
{
	// SP_DOC_ERR_ARENA has two sources: the slice of a report queue of some scan unit (queueMul), or the event array of some
	// document (eventCap).  The last batch counted them apart; only what overflowed doubles (both when nothing is known).
	bool queue = true, events = true;
	if (c->evValid && hipSetDevice( c->device) == hipSuccess && hipStreamSynchronize( c->lastStream) == hipSuccess)
	{
		uint64_t over[ 2] = {0, 0};
		if (hipMemcpyAsync( over, (const uint64_t*)c->dCounters.ptr + L1C_OVER_QUEUE, sizeof(over), hipMemcpyDeviceToHost, c->own) == hipSuccess
		&&  hipStreamSynchronize( c->own) == hipSuccess && (over[ 0] || over[ 1])) { queue = over[ 0] != 0; events = over[ 1] != 0; }
	}
	if (events)
	{
		if (c->eventCap >= (1u<<26)) { c->lasterror = "arena at its maximum size"; return SP_ERR_INVALID; }
		c->eventCap *= 2; c->arena.count = 0;
	}
	if (queue)
	{
		if (c->queueMul >= 4096) { c->lasterror = "report queue at its maximum size (4096 x 1/16 reports per text byte)"; return SP_ERR_INVALID; }
		c->queueMul *= 2;
	}
	return SP_OK;
}

} // extern "C"

namespace {
// Host copy of the lexems of the documents [firstDoc, firstDoc+ndocs) of the last launch, grouped by document (batch_fetch.hpp);
// `counters`: of that launch; bulk: the whole batch in one copy, else a copy per document
void copyOutLexBatch( sp_lexer_ctx* c, size_t firstDoc, size_t ndocs, const uint64_t* counters, bool bulk, sp_lex_batch_t* out)
{
	LexBatchSource src;
	src.lexems = (const sp_lexem_t*)c->lexems.ptr(); src.nlexems = clampCount( counters[ L1C_LEXEMS], c->lexems.count);
	src.docRange = (const uint64_t*)c->dDocRange.ptr; src.docStatus = (const int32_t*)c->dDocStatus.ptr;
	src.ndocs = c->lastNdocs;
	fetchLexBatch( src, firstDoc, ndocs, bulk, deviceToHost( c->own), out);
}
void launchLex( sp_lexer_ctx* c, const void* d_text, const void* d_doc_offsets, size_t ndocs, size_t nbytes, hipStream_t stream)
{
	HIP_CHECK( hipSetDevice( c->device));
	c->stitched.run.done = false;		// (a new batch: what was stitched is of the one before)
	const LexTables& T = c->inst->compiler.tables();
	const bool wordsKernel = c->images.wordsKernel;
	L1LaunchPlan plan = planL1Launch( T, c->images, c->numCUs, ndocs, nbytes, L1Switches::fromEnv());
	const uint64_t maxUnits = plan.maxUnits;
	uint64_t perWaveWords = 4ull*c->eventCap;		// the handler's event array (the report queue is per document: dQueue)
	const ArenaWaves aw = arenaWaves( perWaveWords*4, plan.postWaves, plan.postSlots, 4);
	plan.postWaves = aw.run;
	if (c->arena.count < plan.postWaves || c->arenaWords != perWaveWords)
	{
		c->arena.realloc( aw.alloc, perWaveWords*4);
		c->arenaWords = perWaveWords;
	}
	uint64_t want = (uint64_t)nbytes/3 + 4096;
	if (want < c->minLexemCapacity) want = c->minLexemCapacity;
	c->lexems.ensure( want, sizeof(sp_lexem_t));
	c->dDocRange.reserve( (ndocs+1)*2*sizeof(uint64_t));
	c->dDocStatus.reserve( (ndocs+1)*sizeof(int32_t));
	c->dReportCount.reserve( (maxUnits+1)*sizeof(uint32_t));
	c->dUnitStart.reserve( (ndocs+2)*sizeof(uint32_t));
	c->dDocSequential.reserve( (ndocs+1)*sizeof(uint32_t));
	{
		// the report queues follow the text size: refuse a batch whose queues would not fit beside it instead of running into hipMalloc
		const uint64_t qbytes = ((((uint64_t)nbytes * c->queueMul) >> 4) + 64ull*(maxUnits+2)) * 16;
		size_t freeB = 0, totalB = 0;
		if (hipMemGetInfo( &freeB, &totalB) == hipSuccess)
		{
			const uint64_t have = (uint64_t)c->dQueue.bytes + (wordsKernel ? (uint64_t)c->dWordQueue.bytes : 0);
			const uint64_t want = qbytes * (wordsKernel ? 2 : 1);
			if (want > have && want - have > (uint64_t)(0.8 * (double)freeB))
			{
				char msg[ 200];
				snprintf( msg, sizeof(msg), "the report queues of this batch (%llu MB at %u/16 reports per text byte) do not fit the free device memory (%llu MB): pass fewer bytes per batch",
					(unsigned long long)(want >> 20), c->queueMul, (unsigned long long)(freeB >> 20));
				throw std::runtime_error( msg);
			}
		}
	}
	c->dQueue.reserve( ((((uint64_t)nbytes * c->queueMul) >> 4) + 64ull*(maxUnits+2)) * 16);
	if (wordsKernel)
	{
		c->dWordQueue.reserve( ((((uint64_t)nbytes * c->queueMul) >> 4) + 64ull*(maxUnits+2)) * 16);
		c->dWordCount.reserve( (maxUnits+1)*sizeof(uint32_t));
	}
	if (!T.approx.empty())
	{
		// approximate literal table: the decoded characters of every document (code point, byte offset)
		c->dCharCp.reserve( ((uint64_t)nbytes + ndocs + 64) * 4);
		c->dCharPos.reserve( ((uint64_t)nbytes + ndocs + 64) * 4);
	}
	HIP_CHECK( hipMemsetAsync( c->dCounters.ptr, 0, L1C_ALLOC*sizeof(uint64_t), stream));

	L1Params P;
	std::memset( &P, 0, sizeof(P));
	P.byteClass = (const uint8_t*)c->dByteClass.ptr; P.classCtx = (const uint8_t*)c->dClassCtx.ptr;
	P.exCount = (const uint32_t*)c->dExCount.ptr;
	P.patOfBit = (const uint32_t*)c->dPatOfBit.ptr; P.patterns = (const DevLexPattern*)c->dPatterns.ptr;
	P.symbols = (const DevSymbol*)c->dSymbols.ptr; P.symbolText = (const uint8_t*)c->dSymbolText.ptr;
	P.symbolMask = (uint32_t)T.symbols.size()-1;
	P.literals = (const DevLiteral*)c->dLiterals.ptr; P.literalText = (const uint8_t*)c->dLiteralText.ptr;
	P.litPats = (const uint32_t*)c->dLitPats.ptr; P.literalMask = (uint32_t)T.literals.size()-1; P.nofLiterals = T.nofLiterals;
	P.reportsOrdered = T.reportsOrdered ? 1u : 0u;
	P.nofPasses = T.nofPasses; P.nofClasses = T.nofClasses; P.maxExceptions = T.maxExceptions ? T.maxExceptions : 1;
	P.nofPatterns = (uint32_t)T.patterns.size();
	P.text = (const uint8_t*)d_text; P.docOffsets = (const uint64_t*)d_doc_offsets; P.ndocs = (uint32_t)ndocs;
	P.arenaBase = (uint32_t*)c->arena.ptr(); P.arenaWords = perWaveWords; P.eventCap = c->eventCap;
	P.counters = (uint64_t*)c->dCounters.ptr; P.lexems = (uint32_t*)c->lexems.ptr(); P.lexemCapacity = c->lexems.count;
	P.docRange = (uint64_t*)c->dDocRange.ptr; P.docStatus = (int32_t*)c->dDocStatus.ptr;
	P.reportQueue = (uint32_t*)c->dQueue.ptr; P.reportCount = (uint32_t*)c->dReportCount.ptr; P.queueMul = c->queueMul;
	P.approx = T.approx.empty() ? 0 : (const DevApproxPattern*)c->dApprox.ptr; P.nofApprox = (uint32_t)T.approx.size();
	P.charCp = (uint32_t*)c->dCharCp.ptr; P.charPos = (uint32_t*)c->dCharPos.ptr;
	P.cpBlocks = T.cpBlocks.empty() ? 0 : (const uint16_t*)c->dCpBlocks.ptr; P.cpPages = (const uint8_t*)c->dCpPages.ptr;
	P.ucp = T.ucp ? 1u : 0u;
	P.nullable = T.nullable.empty() ? 0 : (const DevNullable*)c->dNullable.ptr; P.nofNullable = (uint32_t)T.nullable.size();
	P.unitStart = (uint32_t*)c->dUnitStart.ptr; P.chunkBytes = plan.chunkBytes; P.docSequential = (uint32_t*)c->dDocSequential.ptr; P.sequentialPass = 0;
	P.splitPatterns = (T.patterns.size() != c->inst->compiler.nofDefinitions()) ? 1u : 0u;
	P.shapePats = (const uint32_t*)c->dShapePats.ptr; P.shapeMask = (uint32_t)T.shapes.size()-1;
	P.nofShapeVariants = (uint32_t)T.shapeVariants.size();
	for (size_t i=0; i<T.shapeVariants.size() && i<SHAPE_MAXVARIANTS; ++i) P.shapeVariants[ i] = T.shapeVariants[ i];
	P.shapeSalt = T.shapeSalt;
	P.wordQueue = (uint32_t*)c->dWordQueue.ptr; P.wordCount = (uint32_t*)c->dWordCount.ptr; P.wordsKernel = wordsKernel ? 1u : 0u;
	HIP_CHECK( hipEventRecord( c->evStart, stream));
	// the post-processing kernel, which walks the scanned patterns backwards, reads the image of all passes from global memory ...
	P.tableImage = (const uint64_t*)c->dTableImage.ptr; P.ldsWords = 0;
	c->images.all.apply( P);
	P.scanWords = plan.scanWords;
	// ... the scan kernel stages the image of the passes it runs in LDS
	L1Params PS = P;
	PS.nofPasses = plan.scanPasses;
	PS.tableImage = (const uint64_t*)c->dScanImage.ptr; PS.ldsWords = plan.scanLdsWords;
	c->images.scan.apply( PS);
	PS.shapeFpOffset = P.shapeFpOffset;		// (the scan image holds no shape table and the scan kernels read none: the value they have always been passed)
	if (plan.scanPasses == 0) HIP_CHECK( hipMemsetAsync( c->dReportCount.ptr, 0, (maxUnits+1)*sizeof(uint32_t), stream));
	// ... the words kernel ITS image -- the passes behind the scanned ones + the shape table -- when it fits
	L1Params PW = P;
	if (wordsKernel)
	{
		PW.tableImage = (const uint64_t*)c->dWordsImage.ptr;
		c->images.words.apply( PW);
	}
	PW.ldsWords = plan.wordLdsWords;
	P.postClusters = plan.postClusters;
	HIP_CHECK( launchL1Lex( plan, PS, PW, P, stream, c->evMid, c->evWords));
	c->plan = plan;
	HIP_CHECK( hipEventRecord( c->evStop, stream));
	c->evValid = true; c->lastStream = stream; c->lastNdocs = ndocs;
}
}

extern "C" {

int sp_lexer_ctx_match_docs_device( sp_lexer_ctx_t* c, const void* d_text, const void* d_doc_offsets,
				    size_t ndocs, size_t nbytes, void* stream, sp_lex_device_batch_t* out)
{
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		if (ndocs >= 0xFFFFFFFFull) throw std::runtime_error( "too many documents in one batch");
		launchLex( c, d_text, d_doc_offsets, ndocs, nbytes, (hipStream_t)stream);
		if (out)
		{
			out->ndocs = ndocs; out->d_lexems = c->lexems.ptr(); out->d_doc_ranges = c->dDocRange.ptr;
			out->d_doc_status = c->dDocStatus.ptr; out->d_counters = c->dCounters.ptr;
		}
	});
}

int sp_lexer_ctx_batch_counters( sp_lexer_ctx_t* c, uint64_t counters[8])
{
	return guardedCall( c->lasterror, SP_ERR_DEVICE, [&]{
		HIP_CHECK( hipSetDevice( c->device));
		HIP_CHECK( hipStreamSynchronize( c->lastStream));
		uint64_t all[ L1C_ALLOC];
		copySync( c->own, all, c->dCounters.ptr, L1C_ALLOC*sizeof(uint64_t), hipMemcpyDeviceToHost);
		for (int i=0; i<L1C_COUNT; ++i) counters[ i] = all[ i];
#ifndef SPA_PROF
		// (the phase profile of a PROF build lives in 4..7) scan units of the batch and documents scanned again in one piece
		counters[ 4] = (uint32_t)all[ L1C_UNITS]; counters[ 5] = all[ L1C_SEQDOCS]; counters[ 6] = all[ L1C_WORDREPORTS];
#endif
	});
}

int sp_lexer_ctx_batch_status( sp_lexer_ctx_t* c, int32_t* status, size_t ndocs) { return batchStatus( c, c->dDocStatus, status, ndocs); }

double sp_lexer_ctx_last_kernel_ms( sp_lexer_ctx_t* c) { return lastKernelMs( c); }

int sp_lexer_ctx_last_kernel_ms_split( sp_lexer_ctx_t* c, double* scan_ms, double* post_ms)
{
	*scan_ms = -1.0; *post_ms = -1.0;
	if (!c->evValid) return SP_ERR_INVALID;
	double a = 0.0, b = 0.0;
	if (hipEventSynchronize( c->evStop) != hipSuccess) return SP_ERR_INVALID;
	if (!elapsedMs( c->evStart, c->evMid, a) || !elapsedMs( c->evMid, c->evStop, b)) return SP_ERR_INVALID;
	*scan_ms = a; *post_ms = b;
	return SP_OK;
}

// the scan kernel the last launch went through (bench.py prices and names the kernel that ran)
const char* sp_lexer_ctx_scan_kernel_name( const sp_lexer_ctx_t* c)
{
	return c->plan.scanKernelName;
}

const char* sp_lexer_ctx_words_kernel_name( const sp_lexer_ctx_t* c)
{
	return c->plan.wordsKernelName;
}

// the same with the words kernel on its own (round 3: automaton scan | literals + word shapes | start of match + handler + ordinal positions)
int sp_lexer_ctx_last_kernel_ms_split3( sp_lexer_ctx_t* c, double* scan_ms, double* words_ms, double* post_ms)
{
	*scan_ms = -1.0; *words_ms = -1.0; *post_ms = -1.0;
	if (!c->evValid) return SP_ERR_INVALID;
	double a = 0.0, b = 0.0, d = 0.0;
	if (hipEventSynchronize( c->evStop) != hipSuccess) return SP_ERR_INVALID;
	if (!elapsedMs( c->evStart, c->evMid, a) || !elapsedMs( c->evMid, c->evWords, b) || !elapsedMs( c->evWords, c->evStop, d)) return SP_ERR_INVALID;
	*scan_ms = a; *words_ms = b; *post_ms = d;
	return SP_OK;
}

int sp_lexer_ctx_match_docs( sp_lexer_ctx_t* c, const char* text, const uint64_t* doc_offsets, size_t ndocs, sp_lex_batch_t* out)
{
	std::memset( out, 0, sizeof(*out));
	// (the code of guardedCall as it is: an invalid batch is SP_ERR_INVALID here, SP_ERR_DEVICE from sp_matcher_ctx_match_docs)
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		if (ndocs >= 0xFFFFFFFFull) throw std::runtime_error( "too many documents in one batch");
		HIP_CHECK( hipSetDevice( c->device));
		size_t nbytes = ndocs ? (size_t)doc_offsets[ ndocs] : 0;
		for (size_t di=0; di<ndocs; ++di)
		{
			if (doc_offsets[ di+1] - doc_offsets[ di] >= 0xFFFFFFFFull) throw std::runtime_error( "size of string to scan out of range");	// :866-869
		}
		c->dText.reserve( nbytes+16);
		c->dDocOffsets.reserve( (ndocs+1)*sizeof(uint64_t));
		if (nbytes) copySync( c->own, c->dText.ptr, text, nbytes, hipMemcpyHostToDevice);
		copySync( c->own, c->dDocOffsets.ptr, doc_offsets, (ndocs+1)*sizeof(uint64_t), hipMemcpyHostToDevice);
		uint64_t counters[ L1C_COUNT];
		std::vector<int32_t> st( ndocs+1);
		for (int attempt=0;; ++attempt)
		{
			launchLex( c, c->dText.ptr, c->dDocOffsets.ptr, ndocs, nbytes, c->own);
			HIP_CHECK( hipStreamSynchronize( c->own));
			copySync( c->own, counters, c->dCounters.ptr, sizeof(counters), hipMemcpyDeviceToHost);
			if (ndocs) copySync( c->own, st.data(), c->dDocStatus.ptr, ndocs*sizeof(int32_t), hipMemcpyDeviceToHost);
			bool grow = false;
			if (counters[ L1C_LEXEMS] > c->lexems.count) { c->minLexemCapacity = counters[ L1C_LEXEMS] + counters[ L1C_LEXEMS]/8 + 1024; grow = true; }
			if (counters[ L1C_FAILED])
			{
				bool arena = false;
				for (size_t di=0; di<ndocs && !arena; ++di) arena = (st[ di] == SP_DOC_ERR_ARENA);
				if (arena && sp_lexer_ctx_grow_arena( c) == SP_OK) grow = true;
			}
			if (!grow || attempt >= 12) break;
		}
		copyOutLexBatch( c, 0, ndocs, counters, true, out);
		if (counters[ L1C_FAILED])
		{
			size_t bad = 0;
			while (bad < ndocs && st[ bad] == 0) ++bad;
			char msg[ 160];
			snprintf( msg, sizeof(msg), "at least one document failed: document %zu has status %d%s", bad, bad < ndocs ? st[ bad] : -1,
				(bad < ndocs && st[ bad] == SP_DOC_ERR_LEXEMSIZE) ? " (size of matched term out of range)" : "");
			throw DocumentFailed( msg);
		}
	});
}

// host copy of the lexems of the documents [first_doc, first_doc+ndocs) of the last device batch
int sp_lexer_ctx_batch_fetch_docs( sp_lexer_ctx_t* c, size_t first_doc, size_t ndocs, sp_lex_batch_t* out)
{
	std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_DEVICE, [&]{
		HIP_CHECK( hipSetDevice( c->device));
		HIP_CHECK( hipStreamSynchronize( c->lastStream));
		uint64_t counters[ L1C_COUNT];
		copySync( c->own, counters, c->dCounters.ptr, sizeof(counters), hipMemcpyDeviceToHost);
		copyOutLexBatch( c, first_doc, ndocs, counters, false, out);
	});
}

// ---- the segments of the last device batch stitched to documents on the device (l1_stitch.h)
int sp_lexer_ctx_stitch_segments_device( sp_lexer_ctx_t* c, const void* d_doc_seg_offsets, size_t ndocs, void* stream_, sp_lex_stitched_batch_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		if (!c->evValid) throw std::runtime_error( "no batch to stitch: no batch has run on this context");
		if (ndocs >= 0xFFFFFFFFull) throw std::runtime_error( "too many documents in one batch");
		if (!d_doc_seg_offsets) throw std::runtime_error( "no segment offsets");
		hipStream_t stream = (hipStream_t)stream_;
		HIP_CHECK( hipSetDevice( c->device));
		sp_lexer_ctx::Stitched& S = c->stitched;
		S.run.done = false;
		// the stitched lexems are a rearrangement of the batch's: the lexer's capacity holds them, nothing is read back to size them
		const uint64_t capacity = c->lexems.count;
		const size_t nseg = c->lastNdocs;
		S.dLexems.reserve( (capacity+1)*sizeof(sp_lexem_t));
		S.dOrigseg.reserve( (capacity+1)*sizeof(uint32_t));
		S.dSegWork.reserve( (nseg+1)*2*sizeof(uint32_t));
		S.dDocCount.reserve( (ndocs+1)*sizeof(uint32_t));
		S.dDocOffsets.reserve( (ndocs+1)*sizeof(uint64_t));
		S.dDocStatus.reserve( (ndocs+1)*sizeof(int32_t));
		if (!S.dTotals.ptr) S.dTotals.alloc( 2*sizeof(uint64_t));
		if (!S.dCursor.ptr) S.dCursor.alloc( 2*sizeof(uint32_t));
		// another stream than the batch's runs behind the batch (evStop closes the launch sequence)
		S.run.begin( stream, c->lastStream, c->evStop);
		hipEvent_t ev[ 2];
		S.run.events( ev);
		HIP_CHECK( hipMemsetAsync( S.dCursor.ptr, 0, 2*sizeof(uint32_t), stream));
		StitchParams P;
		std::memset( &P, 0, sizeof(P));
		P.lexems = (const uint32_t*)c->lexems.ptr(); P.segRange = (const uint64_t*)c->dDocRange.ptr; P.segStatus = (const int32_t*)c->dDocStatus.ptr;
		P.lexemCounter = (const uint64_t*)c->dCounters.ptr + L1C_LEXEMS; P.lexemCapacity = capacity; P.nseg = (uint32_t)nseg;
		P.docSegOffsets = (const uint64_t*)d_doc_seg_offsets; P.ndocs = (uint32_t)ndocs;
		P.segWork = (uint32_t*)S.dSegWork.ptr; P.docCount = (uint32_t*)S.dDocCount.ptr; P.cursor = (uint32_t*)S.dCursor.ptr;
		P.outLexems = (uint32_t*)S.dLexems.ptr; P.outOrigseg = (uint32_t*)S.dOrigseg.ptr;
		P.docOffsets = (uint64_t*)S.dDocOffsets.ptr; P.docStatus = (int32_t*)S.dDocStatus.ptr; P.totals = (uint64_t*)S.dTotals.ptr;
		HIP_CHECK( launchL1Stitch( P, c->numCUs, stream, ev));
		S.run.completed( stream); S.ndocs = ndocs; S.capacity = capacity;
		if (out)
		{
			out->ndocs = ndocs; out->d_lexems = S.dLexems.ptr; out->d_origseg = S.dOrigseg.ptr;
			out->d_doc_offsets = S.dDocOffsets.ptr; out->d_doc_status = S.dDocStatus.ptr; out->d_totals = S.dTotals.ptr;
		}
	});
}

// plain copy of the stitched buffers: nothing is renumbered or regrouped on the host
int sp_lexer_ctx_stitched_fetch( sp_lexer_ctx_t* c, sp_lex_batch_t* out, uint32_t** origseg)
{
	std::memset( out, 0, sizeof(*out));
	if (origseg) *origseg = 0;
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		const sp_lexer_ctx::Stitched& S = c->stitched;
		if (!S.run.done) throw std::runtime_error( "the last batch of this context has not been stitched (sp_lexer_ctx_stitch_segments_device)");
		HIP_CHECK( hipSetDevice( c->device));
		HIP_CHECK( hipStreamSynchronize( S.run.stream));
		uint64_t totals[ 2];
		copySync( c->own, totals, S.dTotals.ptr, sizeof(totals), hipMemcpyDeviceToHost);
		const uint64_t nlex = clampCount( totals[ 0], S.capacity);
		allocLexBatch( out, S.ndocs, nlex);
		if (nlex) copySync( c->own, out->lexems, S.dLexems.ptr, nlex*sizeof(sp_lexem_t), hipMemcpyDeviceToHost);
		copySync( c->own, out->doc_lexem_offsets, S.dDocOffsets.ptr, (S.ndocs+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (S.ndocs) copySync( c->own, out->doc_status, S.dDocStatus.ptr, S.ndocs*sizeof(int32_t), hipMemcpyDeviceToHost);
		out->nlexems = nlex;
		if (origseg)
		{
			*origseg = hostArray<uint32_t>( nlex+1);
			if (nlex) copySync( c->own, *origseg, S.dOrigseg.ptr, nlex*sizeof(uint32_t), hipMemcpyDeviceToHost);
		}
	});
}

int sp_lexer_ctx_stitched_status( sp_lexer_ctx_t* c, int32_t* status, size_t ndocs, size_t* ndocs_stitched)
{
	if (ndocs_stitched) *ndocs_stitched = 0;
	return guardedCall( c->lasterror, SP_ERR_INVALID, [&]{
		const sp_lexer_ctx::Stitched& S = c->stitched;
		if (!S.run.done) throw std::runtime_error( "the last batch of this context has not been stitched (sp_lexer_ctx_stitch_segments_device)");
		if (ndocs_stitched) *ndocs_stitched = S.ndocs;
		if (ndocs > S.ndocs) ndocs = S.ndocs;
		if (!ndocs || !status) return;
		HIP_CHECK( hipSetDevice( c->device));
		HIP_CHECK( hipStreamSynchronize( S.run.stream));
		copySync( c->own, status, S.dDocStatus.ptr, ndocs*sizeof(int32_t), hipMemcpyDeviceToHost);
	});
}

// duration of the three passes of the last stitch in milliseconds (HIP events on its stream; waits for them)
int sp_lexer_ctx_last_stitch_ms( sp_lexer_ctx_t* c, double* ms) { return c->stitched.run.ms( 0, 1, ms); }

void sp_lex_batch_free( sp_lex_batch_t* b)
{
	std::free( b->lexems); std::free( b->doc_lexem_offsets); std::free( b->doc_status);
	std::memset( b, 0, sizeof(*b));
}

int sp_lexer_ctx_match( sp_lexer_ctx_t* c, const char* src, size_t srclen, sp_lexem_t** lexems, size_t* nlexems)
{
	uint64_t offs[2] = {0, (uint64_t)srclen};
	sp_lex_batch_t b;
	int rc = sp_lexer_ctx_match_docs( c, src, offs, 1, &b);
	if (rc != SP_OK) { sp_lex_batch_free( &b); *lexems = 0; *nlexems = 0; return rc; }
	*lexems = b.lexems; *nlexems = b.nlexems; b.lexems = 0;
	sp_lex_batch_free( &b);
	return SP_OK;
}

} // extern "C"
