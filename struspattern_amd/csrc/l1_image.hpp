// Host side of a lexer launch that needs no device: the table images the kernels read and the launch plan of a batch
// (which kernel instances, grids, workgroup sizes, LDS).  No HIP header in here: a plain C++ compiler builds it.
#ifndef SPA_L1_IMAGE_HPP
#define SPA_L1_IMAGE_HPP
#include <stdint.h>
#include <cstddef>
#include <vector>
#include "l1_compile.hpp"
#include "l1_device.h"

namespace spa {

// The SPA_L1_* launch switches (tests and A/B runs).  fromEnv() is the one place that reads them.  noWordsKernel is taken when a
// context is created (its images follow it); the others at every launch.
struct L1Switches
{
	bool noWordsKernel = false;	// SPA_L1_NO_WORDS_KERNEL: the post-processing kernel finds the literals itself
	uint32_t chunkBytes = 0;	// SPA_L1_CHUNK_BYTES (64 .. 2^30, rounded down to a multiple of 64); 0 = default
	unsigned postWavesPerCU = 0;	// SPA_L1_POST_WAVES_PER_CU (1 .. 40); 0 = default
	bool wordWaves12 = false;	// SPA_L1_WORD_WAVES: the 12-wave instance of the words kernel whatever the image leaves room for
	bool postSequential = false;	// SPA_L1_POST_SEQ: the handler takes one report after the other
	bool noLanes = false;		// SPA_L1_NO_LANES: keep the batch off the lane-per-stream scan kernel
	static L1Switches fromEnv();
};

// Tables of the passes [first, end) back to back: [charMask][acceptMask][startMask][shiftDst][selfLoop][exSrc][exDst], then the
// compact shape table when asked for.  A kernel indexes by absolute pass: the offsets carry the bias of the passes left out in
// front (modulo 2^32).
struct L1Image
{
	std::vector<uint64_t> words;	// never empty (an image of nothing is one zero word)
	uint32_t oChar = 0, oAccept = 0, oStart = 0, oShift = 0, oSelf = 0, oExSrc = 0, oExDst = 0, oShapeFp = 0;
	// the offsets into the parameters of a kernel that reads this image (not tableImage / ldsWords: where the words lie is the caller's)
	void apply( L1Params& P) const;
};
L1Image buildL1Image( const LexTables& T, uint32_t first, uint32_t end, bool withShapes);

// The three images of a compiled lexer.
struct L1Images
{
	bool wordsKernel = false;	// plain tables: literals and word shapes are found by the words kernel
	uint32_t scanPasses = 0;	// passes the scan kernel runs: [0, scanPasses)
	L1Image all;			// all passes + shape table: what the kernels that walk an automaton backwards read (global memory)
	L1Image scan;			// the scanned passes (the word shapes' passes behind them are never scanned): staged in LDS when it fits
	L1Image words;			// words kernel: the passes BEHIND the scanned ones + shape table (empty without a words kernel)
};
L1Images buildL1Images( const LexTables& T, const L1Switches& sw);

enum L1Route {L1_ROUTE_NONE /*nothing to scan*/, L1_ROUTE_APPROX, L1_ROUTE_LANES, L1_ROUTE_PASSES};

// Everything a launch decides, decided once.  launchL1Lex (l1_launch.cpp) follows it; the kernel names reported are the plan's.
struct L1LaunchPlan
{
	uint32_t chunkBytes = 0;	// documents longer than a chunk are scanned as several units
	uint64_t maxUnits = 0;		// bound of the scan units of the batch
	L1Route route = L1_ROUTE_NONE;
	uint32_t scanPasses = 0;	// passes the scan kernel runs (L1_ROUTE_PASSES: selects the instance)
	bool cp = false;		// the _cp set of scan and post-processing instances: classes by code point or empty matches
	unsigned scanGrid = 1, scanThreads = 256;
	uint32_t scanLdsWords = 0;	// words of the scan image staged in LDS, 0 = read from global memory
	unsigned laneGrid = 1;		// lane-per-stream scan kernel: workgroups of four waves
	bool wordsKernel = false;
	unsigned wordWaves = L1_WORD_WAVES_SMALL, wordGrid = 1;
	uint32_t wordLdsWords = 0;	// words of the words kernel's image staged in LDS, 0 = read from global memory
	unsigned postSlots = 0;		// post-processing (and approximate-matching) kernel: waves the device holds ...
	unsigned postWaves = 4;		// ... and waves of this batch, one event array each (the caller may lower it to what its arena holds)
	uint32_t postClusters = 1, scanWords = 0;	// L1Params fields of the same name
	const char* scanKernelName = "(none)";
	const char* wordsKernelName = "(none)";

	size_t scanLdsBytes() const	{return (size_t)scanLdsWords * 8;}
	unsigned postGrid() const	{return (postWaves + L1_POST_WAVES-1) / L1_POST_WAVES;}
};
// throws std::runtime_error for a batch of too many scan units
L1LaunchPlan planL1Launch( const LexTables& T, const L1Images& img, unsigned numCUs, size_t ndocs, size_t nbytes, const L1Switches& sw);

} // namespace
#endif
