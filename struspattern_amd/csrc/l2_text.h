// Matched text of a finished device batch (l2_text_kernel.hip): behind l2_finish.h on the output side of the matcher, the
// bytes that the finished results and items cover, gathered from the text the lexer batch ran on without leaving HBM.
// The rule is that of span_text.hpp (its device-free twin; include/strus_pattern_amd.h "matched text" states it): words
// 3..6 of a record are (origseg, origpos, origendseg, origend), the span of document d is
// text[ segOffsets[docSeg[d]+origseg] + origpos, segOffsets[docSeg[d]+origendseg] + origend ), and a document with an
// invalid span is empty with status SP_DOC_ERR_RANGE.  Three passes on one stream, per family (results: 9 words a
// record, items: 7; one templated set of kernels):
//   A  count   a wave per document, its spans in rounds of 64, a lane per span: validity and length; a wave scan gives
//              the span's offset inside the document (spanWork), per document the byte count and the status
//   B  offsets exclusive prefix sum of the per-document byte counts (a failed document counts 0), and the total
//   C  place   a wave per document: the span offsets, and the bytes
// A runs for every requested family before B runs for any: a document that fails in one family is empty in both.
// The copy of C is output-driven: the 64 spans of a round are one contiguous range of the output, every lane owns
// aligned dwords of it, finds the span of each byte among the round's 64 offsets in LDS (6 steps), assembles the dword
// from loads clamped to the text and stores it aligned and coalesced.  A span of TEXT_LONG_SPAN bytes or more is copied
// by the whole wave in a loop of its own, without the search.  A dword that lies only in part inside the range a loop
// copies -- at the edges of a document's block, where the neighbouring bytes belong to another wave, as at the edges of a
// round or a long span -- is written with byte stores: a wave never stores a byte it does not own.
#ifndef SPA_L2_TEXT_H
#define SPA_L2_TEXT_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>

namespace spa {

enum { TEXT_LONG_SPAN = 4096 };

struct TextFamily
{
	const uint32_t* records;	// finished results (9 words) or items (7 words)
	const uint64_t* docOffsets;	// ndocs+1: the finished document offsets of the family
	uint64_t nrecords;		// the finished total, read by the host: every record index is checked against it
	// working memory
	uint32_t* spanWork;		// nrecords: offset of the span inside its document
	uint64_t* docBytes;		// ndocs
	// the text batch
	uint64_t* docTextOffsets;	// ndocs+1
	uint64_t* spanOffsets;		// nrecords+1
	uint8_t* outText;		// pass C only
	uint64_t outCapacity;		// bytes of outText: the total that pass B left, read by the host
	uint64_t* total;
	uint32_t* cursor;		// [0] pass A, [1] pass C; zeroed
};

struct TextParams
{
	const uint8_t* text; uint64_t nbytes;
	const uint64_t* segOffsets; uint64_t nseg;
	const uint64_t* docSegOffsets;	// NULL: document d is segment d (the host has checked nseg == ndocs)
	uint32_t ndocs;
	int32_t* docStatus;		// ndocs, zeroed
	TextFamily family[ 2];		// results, items
	uint32_t families;		// SP_TEXT_RESULTS | SP_TEXT_ITEMS
};

// enqueue the passes A and B of the requested families
hipError_t launchL2TextCount( const TextParams& P, unsigned numCUs, hipStream_t stream);
// enqueue pass C (outText and outCapacity set from the totals)
hipError_t launchL2TextPlace( const TextParams& P, unsigned numCUs, hipStream_t stream);

} // namespace
#endif
