// Table images and launch plan of the level-1 lexer (l1_image.hpp): host only, no device needed.
#include "l1_image.hpp"
#include <cstdlib>
#include <stdexcept>

namespace spa {

L1Switches L1Switches::fromEnv()
{
	L1Switches sw;
	sw.noWordsKernel = getenv( "SPA_L1_NO_WORDS_KERNEL") != 0;
	if (const char* e = getenv( "SPA_L1_CHUNK_BYTES")) { long v = atol( e); if (v >= 64 && v <= (1l << 30)) sw.chunkBytes = (uint32_t)v & ~63u; }
	if (const char* e = getenv( "SPA_L1_POST_WAVES_PER_CU")) { int v = atoi( e); if (v >= 1 && v <= 40) sw.postWavesPerCU = (unsigned)v; }
	sw.wordWaves12 = getenv( "SPA_L1_WORD_WAVES") != 0;
	sw.postSequential = getenv( "SPA_L1_POST_SEQ") != 0;
	sw.noLanes = getenv( "SPA_L1_NO_LANES") != 0;
	return sw;
}

void L1Image::apply( L1Params& P) const
{
	P.ldsChar = oChar; P.ldsAccept = oAccept; P.ldsStart = oStart; P.ldsShift = oShift; P.ldsSelf = oSelf;
	P.ldsExSrc = oExSrc; P.ldsExDst = oExDst; P.shapeFpOffset = oShapeFp;
}

L1Image buildL1Image( const LexTables& T, uint32_t first, uint32_t end, bool withShapes)
{
	if (first > end || end > T.nofPasses) throw std::logic_error( "internal: pass range of a table image");
	L1Image img;
	std::vector<uint64_t>& w = img.words;
	// rows [first*cut, end*perPass) of a table of perPass words per pass (every table holds exactly nofPasses*perPass words:
	// l1_compile.cpp, compile and load); returns where row 0 would lie
	auto put = [&]( const std::vector<uint64_t>& v, size_t perPass, size_t cut) -> uint32_t
	{
		if (v.size() != (size_t)T.nofPasses*perPass) throw std::logic_error( "internal: size of a lexer table");
		const uint32_t off = (uint32_t)w.size() - (uint32_t)(first*cut);
		w.insert( w.end(), v.begin() + first*cut, v.begin() + end*perPass);
		return off;
	};
	// The exception tables have max( maxExceptions, 1) rows per pass, but the passes in front are cut by maxExceptions as it is:
	// tables without exceptions keep the (zero) rows of the passes left out, unbiased.  Only the words kernel's image has passes
	// in front, and it has always been built so; cutting them would change its size, and with it the choice between the 16- and
	// the 12-wave instance.
	const size_t exRows = T.maxExceptions ? T.maxExceptions : 1;
	img.oChar = put( T.charMask, (size_t)T.nofClasses*64, (size_t)T.nofClasses*64);
	img.oAccept = put( T.acceptMask, (size_t)CTX_COUNT*64, (size_t)CTX_COUNT*64);
	img.oStart = put( T.startMask, (size_t)CTX_COUNT*64, (size_t)CTX_COUNT*64);
	img.oShift = put( T.shiftDst, 64, 64);
	img.oSelf = put( T.selfLoop, 64, 64);
	img.oExSrc = put( T.exSrc, exRows*64, (size_t)T.maxExceptions*64);
	img.oExDst = put( T.exDst, exRows*64, (size_t)T.maxExceptions*64);
	img.oShapeFp = (uint32_t)w.size();
	if (withShapes) w.insert( w.end(), T.shapeFp.begin(), T.shapeFp.end());	// (the compact shape table rides along: staged in LDS with the rest)
	if (w.empty()) w.push_back( 0);
	return img;
}

L1Images buildL1Images( const LexTables& T, const L1Switches& sw)
{
	if (T.nofPasses > 32) throw std::runtime_error( "too many regular expression positions for this version (more than 32 passes of 4096 positions)");
	L1Images r;
	// literals and word shapes by the words kernel: plain tables (words by ASCII word characters, no classes by code point, no empty matches)
	r.wordsKernel = T.approx.empty() && !T.ucp && T.cpBlocks.empty() && T.nullable.empty() && !sw.noWordsKernel;
	if (!r.wordsKernel && T.nofShapes) throw std::runtime_error( "internal: word shapes in a table the words kernel does not take");
	r.scanPasses = r.wordsKernel ? T.scanPasses : T.nofPasses;
	r.all = buildL1Image( T, 0, T.nofPasses, true);
	r.scan = buildL1Image( T, 0, r.scanPasses, false);
	// image of the words kernel: it walks the patterns of the passes BEHIND the scanned ones only, so those passes and the compact
	// shape table are all it stages in LDS (the 10k set: 101 KB instead of 124: room for 16 waves per workgroup)
	if (r.wordsKernel) r.words = buildL1Image( T, T.scanPasses, T.nofPasses, true);
	return r;
}

namespace {
const char* const g_scanKernelNames[ 10] = {"spa_l1_scan_kernel_p1", "spa_l1_scan_kernel_p2", "spa_l1_scan_kernel_p3", "spa_l1_scan_kernel_p4", "spa_l1_scan_kernel_p5",
	"spa_l1_scan_kernel_p6", "spa_l1_scan_kernel_p7", "spa_l1_scan_kernel_p8", "spa_l1_scan_kernel_p16", "spa_l1_scan_kernel_p32"};
template <typename T> T atMost( T a, T b) { return a < b ? a : b; }
}

L1LaunchPlan planL1Launch( const LexTables& T, const L1Images& img, unsigned numCUs, size_t ndocs, size_t nbytes, const L1Switches& sw)
{
	L1LaunchPlan p;
	const size_t scanBytes = img.scan.words.size()*8;
	const size_t wordsBytes = img.wordsKernel ? img.words.words.size()*8 : 0;
	p.scanPasses = img.scanPasses;
	p.wordsKernel = img.wordsKernel;
	p.cp = !T.cpBlocks.empty() || !T.nullable.empty();

	// LDS image of the scan kernel, when it fits (one copy per workgroup; bigger workgroups when the copy is big)
	if (scanBytes <= L1_SCAN_IMAGE_MAX_BYTES && p.scanPasses <= 8)
	{
		p.scanLdsWords = (uint32_t)img.scan.words.size();
		// as many workgroups per CU as copies of the image fit into the 160 KB of LDS, sharing the waves
		// the register budget allows (5 per SIMD up to 2 passes, 4 beyond; two 10-wave workgroups of the
		// 3-pass instance at 96 registers were measured not to share a CU)
		const unsigned maxWaves = p.scanPasses <= 2 ? 20u : 16u;
		unsigned maxCopies = (unsigned)((L1_CU_LDS_BYTES - 1024) / scanBytes);
		if (maxCopies < 1) maxCopies = 1;
		if (maxCopies > 5) maxCopies = 5;
		// waves per workgroup in multiples of 4 (one per SIMD): workgroups of 6 or 10 waves load the four
		// SIMDs unevenly and the next workgroup does not fit beside them (measured: 3 x 6 waves of the
		// 2-pass instance ran at the speed of 10-12 resident waves)
		unsigned best = 0, wpb = 4;
		for (unsigned cp=maxCopies; cp>=1; --cp)
		{
			unsigned wv = (maxWaves / cp) & ~3u;
			if (wv > 16) wv = 16;
			if (wv * cp > best) { best = wv * cp; wpb = wv; }
		}
		p.scanThreads = 64 * wpb;
	}
	else { p.scanLdsWords = 0; p.scanThreads = 256; }

	// documents longer than a chunk are scanned as several units (SPA_L1_CHUNK_BYTES: tests)
	p.chunkBytes = 32768;		// (12288 x 64 KiB documents: scan 102.4 ms unchunked, 95.9 / 95.5 / 97.0 ms at 32 / 16 / 4 KiB chunks)
	// (an expression that can stay live across blanks -- <[^>]*>, ".*" with DOTALL -- fails the warm-up proof of nearly every chunk:
	//  such tables are scanned document by document, the chunked pass would only be thrown away)
	if (!T.lanesOk) p.chunkBytes = 0xFFFFFFC0u;
	if (sw.chunkBytes) p.chunkBytes = sw.chunkBytes;
	p.maxUnits = (uint64_t)ndocs + (uint64_t)nbytes / p.chunkBytes + 2;
	if (p.maxUnits >= 0xFFFFFFFFull) throw std::runtime_error( "too many scan units in one batch");
	// scan kernel: one wave per unit up to what the device holds (a wave without a unit leaves at once)
	const unsigned wavesWanted = (unsigned)atMost<uint64_t>( p.maxUnits, (uint64_t)numCUs*20);
	const unsigned wpb = p.scanThreads / 64;
	p.scanGrid = (wavesWanted + wpb-1) / wpb;
	if (p.scanGrid == 0) p.scanGrid = 1;
	// lane-per-stream scan kernel (a few automaton words left to scan): a wave per unit, workgroups of four waves
	p.laneGrid = (unsigned)atMost<uint64_t>( (p.maxUnits + 3) / 4, (uint64_t)numCUs*4);
	if (p.laneGrid == 0) p.laneGrid = 1;

	// the post-processing kernel (and the approximate-matching kernel) has its own number of waves: one event array each
	const unsigned postPerCU = sw.postWavesPerCU ? sw.postWavesPerCU : 4u*6u;	// (6 per SIMD: the register budget of the kernel, l1_post_kernel.hip)
	p.postSlots = numCUs*postPerCU;
	p.postWaves = (unsigned)atMost<size_t>( ndocs, (size_t)p.postSlots);
	p.postWaves = (p.postWaves + 3u) & ~3u;
	if (p.postWaves == 0) p.postWaves = 4;
	p.postClusters = sw.postSequential ? 0u : 1u;		// (SPA_L1_POST_SEQ: tests and A/B runs, one report after the other)

	// words kernel: a wave per unit, workgroups of 16 (12) waves that share one LDS copy of ITS image when it fits
	// (16 waves per workgroup while the image leaves room for their rings and run ends, else 12; SPA_L1_WORD_WAVES: A/B runs)
	p.wordWaves = (wordsBytes + (size_t)L1_WORD_WAVES_SMALL*L1_WORDS_LDS_PER_WAVE <= L1_CU_LDS_BYTES && !sw.wordWaves12) ? (unsigned)L1_WORD_WAVES_SMALL : (unsigned)L1_WORD_WAVES;
	p.wordLdsWords = (wordsBytes + (size_t)p.wordWaves*L1_WORDS_LDS_PER_WAVE <= L1_CU_LDS_BYTES && T.nofShapes) ? (uint32_t)(wordsBytes/8) : 0u;
	p.wordGrid = (unsigned)atMost<uint64_t>( (p.maxUnits + p.wordWaves-1) / p.wordWaves, (uint64_t)numCUs);
	if (p.wordGrid == 0) p.wordGrid = 1;
	if (p.wordsKernel) p.wordsKernelName = p.wordWaves == (unsigned)L1_WORD_WAVES_SMALL ? "spa_l1_words_kernel_w16" : "spa_l1_words_kernel";

	// (scanWords = 0 keeps the batch off the lane-per-stream scan kernel: an expression that can stay live across blanks would
	//  fail the warm-up proof of most pieces, SPA_L1_NO_LANES: tests)
	p.scanWords = (p.wordsKernel && T.lanesOk && !sw.noLanes) ? T.scanWords : 0u;
	if (!T.approx.empty())
	{
		p.route = L1_ROUTE_APPROX; p.scanKernelName = "spa_l1_approx_kernel";
	}
	else if (p.scanPasses == 1 && p.scanWords >= 1 && p.scanWords <= 4 && T.reportsOrdered && !p.cp && p.scanLdsWords && p.scanLdsBytes() <= L1_STATIC_LDS_LIMIT)
	{
		// what is left to scan fits four automaton words: a lane per stream
		p.route = L1_ROUTE_LANES; p.scanKernelName = "spa_l1_scan_lanes_kernel";
	}
	else if (p.scanPasses == 0) p.route = L1_ROUTE_NONE;
	else
	{
		p.route = L1_ROUTE_PASSES;
		p.scanKernelName = g_scanKernelNames[ p.scanPasses <= 8 ? p.scanPasses-1 : p.scanPasses <= 16 ? 8 : 9];
	}
	return p;
}

} // namespace
