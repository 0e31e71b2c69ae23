// Stitching the segments of a lexer device batch on the device (l1_stitch_kernel.hip): the mirror image, on the input
// side of the matcher, of what l2_finish.h does on its output side.  The "documents" of the lexer batch are content
// segments (whole segments appended in completion order, found through (first, count) pairs); docSegOffsets says which
// run of segments makes up each document.  The stitched batch is what sp_matcher_ctx_match_docs_device takes: the
// lexems of document 0 first, segment order inside a document, the ordinal positions continued from segment to
// segment, and a parallel origseg word (DESIGN.md 4 "Segmented documents" has the rule).  Three passes on one stream:
//   A  count   a wave per document scans its segments in rounds of 64: per segment {destination offset inside the
//              document, ordpos base}, per document the lexem count and the status
//   B  offsets exclusive prefix sum of the per-document counts, and the totals {lexems, failed documents}
//   C  place   a wave per document, a lane per stitched lexem: 16 bytes in, base added to word 1, 16 + 4 bytes out
#ifndef SPA_L1_STITCH_H
#define SPA_L1_STITCH_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>

namespace spa {

struct StitchParams
{
	// the batch as the lexer kernels left it
	const uint32_t* lexems;		// 4 words each
	const uint64_t* segRange;	// nseg x (first lexem, count)
	const int32_t* segStatus;
	const uint64_t* lexemCounter;	// the batch's lexem counter, still on the device: every index formed from a (first, count)
	uint64_t lexemCapacity;		// pair is checked against min( *lexemCounter, lexemCapacity), and so is every index written
	uint32_t nseg;			// "documents" of the lexer batch
	// the documents
	const uint64_t* docSegOffsets;	// ndocs+1
	uint32_t ndocs;
	// working memory
	uint32_t* segWork;		// nseg x {destination offset inside the document, ordpos base}
	uint32_t* docCount;		// ndocs
	uint32_t* cursor;		// [0] pass A, [1] pass C; zeroed
	// the stitched batch
	uint32_t* outLexems;		// lexemCapacity records
	uint32_t* outOrigseg;
	uint64_t* docOffsets;		// ndocs+1
	int32_t* docStatus;		// ndocs
	uint64_t* totals;		// lexems, failed documents
};

// enqueue the passes; ev[0] before them and ev[1] behind them, if given (timing)
hipError_t launchL1Stitch( const StitchParams& P, unsigned numCUs, hipStream_t stream, hipEvent_t* ev);

} // namespace
#endif
