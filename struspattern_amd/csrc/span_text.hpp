// The text that the results and items of a finished batch cover, over host arrays: the definition that the device passes
// (l2_text.h) are measured against, and the entry point for batches already fetched to the host (sp_match_batch_text).
// Host only: no HIP header and no HIP call in here.
//
// The rule (DESIGN.md 4 "Matched text"; the project's own, unpinned by a reference vector).  The text holds all segments of
// the lexer batch back to back, segOffsets[nseg+1] says where; document d is the segments [docSeg[d], docSeg[d+1]), or
// segment d alone without docSegOffsets.  Words 3..6 of a result or item record are (origseg, origpos, origendseg, origend);
// for a span of document d
//	s0 = docSeg[d] + origseg, s1 = docSeg[d] + origendseg
//	bytes = text[ segOffsets[s0] + origpos, segOffsets[s1] + origend )
// one contiguous range also when it crosses segments.  A span is valid when docSeg[d] <= docSeg[d+1] <= nseg,
// origseg <= origendseg < docSeg[d+1] - docSeg[d], origpos <= len(s0), origend <= len(s1), begin <= end <= nbytes and the
// segOffsets used ascend (segOffsets[s0] <= segOffsets[s0+1] (<=) segOffsets[s1] <= segOffsets[s1+1]).  A document with an
// invalid span in a requested family, or whose spans of one family add up to 2^32 bytes or more, has text status
// SP_DOC_ERR_RANGE and all its spans, of both families, are empty.  A document without spans has status 0.
#ifndef SPA_SPAN_TEXT_HPP
#define SPA_SPAN_TEXT_HPP
#include "../../include/strus_pattern_amd.h"
#include <cstddef>
#include <cstdint>

namespace spa {

struct TextSource
{
	const char* text; uint64_t nbytes;
	const uint64_t* segOffsets; uint64_t nseg;
	const uint64_t* docSegOffsets;		// NULL: document d is segment d
};

// the byte range of one span of document `doc` (w: words 3..6 of its record); false for an invalid span
bool spanRange( const TextSource& S, uint64_t doc, const uint32_t* w, uint64_t& begin, uint64_t& length);

// the host arrays of the text of `nresults` / `nitems` spans (a family that `flags` does not ask for has none), the
// offsets and the status zeroed (sp_match_text_free)
void allocMatchText( sp_match_text_t* out, size_t ndocs, uint64_t nresults, uint64_t nitems, uint32_t flags);
// the byte arrays, once the totals are known
void allocMatchTextBytes( sp_match_text_t* out, uint32_t flags);

// the text of a finished batch on the host; throws std::runtime_error for arguments that make no batch
void matchBatchText( const sp_match_batch_t& mb, const TextSource& S, uint32_t flags, sp_match_text_t* out);

} // namespace
#endif
