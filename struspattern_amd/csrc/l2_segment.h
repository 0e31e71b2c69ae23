// Lookups in an index segment on the device (l2_segment_kernel.hip): the read side of the term blocks (l2_termblocks.h) and the
// posting blocks (l2_postingblocks.h).  The rule is that of match_segment.hpp (its device-free twin; include/strus_pattern_amd.h
// "segment lookups" states it); the walks are segment_walk.h, the one copy for both sides.
// All launches go on one stream; kernel boundaries are the only ordering between waves, nobody spins on a flag; no atomic decides
// where a byte goes (the one atomic is a maximum into q_status: the status of a query is the largest of its selected positions).
//   find     a lane per query: segmentFind.  Bisects the block table by (block_handles[j], head value), walks one block from its
//            head comparing against the front-coded codes, under the prefix flag bisects and walks once more for the end of the run.
//   runs     one workgroup: scanDocumentCounts over q_count into q_sel_offsets[nq+1]; totals[0] = nsel.  An exact lookup has
//            nsel <= nq, so the host sizes the per-selection arrays by nq and does not wait; a prefix lookup waits here for nsel.
//   sizes    a lane per selected position s (the lanes at and beyond nsel, which they read from totals[0], leave): bisects
//            q_sel_offsets for its query, walks its term block to its code and its posting block to and through its list
//            (walkSelection with a sink that counts); writes the 24-byte record, the status, and the three counts.
//   offsets  one workgroup: the exclusive prefixes of the three counts in place, one scan of three sums; totals[1..3].
//            The host waits here, once, and sizes `values`, `postings` and `positions`.
//   emit     the lanes and the walk of `sizes` with a sink that writes, cut to what `sizes` counted.
// A list is walked by one lane: a list of a megabyte is serial (the follow-up is a wave-parallel parse).
// Working memory (the segment's, it only grows): 4 bytes a selected position for its status, 8 for where its positions start.
#ifndef SPA_L2_SEGMENT_H
#define SPA_L2_SEGMENT_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>
#include "segment_walk.h"

namespace spa {

struct SegmentLookupParams
{
	SegmentView segment;			// device pointers
	// the queries
	const uint32_t* queryHandles;		// nq
	const uint64_t* queryOffsets;		// nq+1
	const uint8_t* queryBytes;		// queryNbytes
	uint64_t queryNbytes;
	uint32_t nq;
	uint32_t prefix;
	// per query
	uint32_t* qFirst;
	uint32_t* qCount;
	uint32_t* qStatus;
	uint64_t* qSelOffsets;			// nq+1
	// per selected position: room for selCapacity of them (nq before nsel is known)
	uint64_t selCapacity;
	uint32_t* selections;			// 6 words a record (sp_segment_selection_t)
	uint32_t* selStatus;
	uint64_t* selValueOffsets;		// selCapacity+1: the counts, then their exclusive prefix
	uint64_t* selPostingOffsets;
	uint64_t* selPositionOffsets;
	uint64_t* totals;			// 4, zeroed: nsel, npostings, npositions, the bytes of the values
	// what the totals size; set after the host's wait
	uint8_t* values;
	uint32_t* postings;			// 4 words a record (sp_segment_posting_t)
	uint64_t* postingPositionOffsets;	// npostings+1
	uint32_t* positions;
	uint64_t nsel, npostings, npositions, nvalueBytes;	// as the host read them
};

// find and runs
hipError_t launchL2SegmentFind( const SegmentLookupParams& P, hipStream_t stream);
// sizes and offsets: what the host waits for
hipError_t launchL2SegmentCount( const SegmentLookupParams& P, hipStream_t stream);
// emit
hipError_t launchL2SegmentPlace( const SegmentLookupParams& P, hipStream_t stream);

} // namespace
#endif
