// Posting positions of a finished device batch (l2_positions_kernel.hip): behind l2_postings.h on the output side of the
// matcher, for every posting the list of ALL its occurrences -- one 8-byte record {ordpos, result} per participating result,
// the occurrences of posting p at [postingOffsets[p], postingOffsets[p+1]) ascending by (ordpos, result) -- and per posting the
// number of distinct positions.  The rule is that of match_positions.hpp (its device-free twin; include/strus_pattern_amd.h
// "posting positions" states it).
// The core is the stable LSD radix partition of radix_passes.h over the pairs (key, payload = global result index r), applied
// in two groups: first keyed by ordpos, then -- a rekey launch in between replaces every key, keeping the order -- by the
// posting p(r).  The pairs come in ascending r, every pass is stable, so the end is ascending by (posting, ordpos, r).
// NON-PARTICIPANTS (results without a term: those of failed documents) go through the partition with a sentinel: key 0 in the
// first group, key N (one beyond the last posting) in the second, which sorts them behind every occurrence; place looks at
// the first nocc slots only.  The other way, compacting them away in the key launch, needs the participants of every document
// counted and scanned first -- two more launches and a second dependent read of result_term -- to save the pair traffic of
// results that a batch without failed documents does not have.  The sentinel costs one more key value: the second group
// orders keys up to N where a non-participant exists (nocc below the finished total), up to N - 1 otherwise.
//   keys       a wave per document from the device cursor, a lane per result, 64 a trip: docOf[r], and the pair (ordpos, r) as
//              one 8-byte store into pairs[0]; beside it the sum of the participants and the unsigned maximum of their ordpos
//              (wave-reduced, then one atomic sum and one atomic maximum per wave: order-free).
//   offsets    one workgroup: the exclusive prefix sums of the postings' count in 64 bits (scanDocumentCounts).
//   -- the host waits here, once, for nocc and the largest ordpos: they set the passes --
//   group 1    ceil(bitwidth(largest participating ordpos) / digitBits) passes of histogram / scan / scatter.
//   rekey      tiles of slots, a lane per slot: the key of the pair becomes p(r) = recordPosting[docTermOffsets[d] + resultTerm[r]],
//              or N; the pair stays in its slot.
//   group 2    ceil(bitwidth(N or N - 1) / digitBits) passes.
//   place      tiles of slots below nocc: occurrences[q] = {ordpos, r - docOffsets[docOf[r]]} as one 8-byte store; a lane is
//              the first of its position iff its predecessor in the same posting has another ordpos; the firsts of a trip
//              with the same posting are ballot-combined into one atomic sum on postingPositions[p].
// All launches on one stream; the data of the partition sees no atomic in HBM; kernel boundaries are the only ordering.
// Whatever the arrays hold: a result index is compared against the finished total before a result is read, a result_term
// against its document's record count, a term record against N, a posting against N, a document against ndocs, a rank against
// the number of pairs (radix_passes.h) and a slot against nocc; a slot that no valid result reaches gets 0xFFFFFFFF words.
#ifndef SPA_L2_POSITIONS_H
#define SPA_L2_POSITIONS_H
#include "radix_passes.h"

namespace spa {

const uint32_t POSITIONS_TILE = RADIX_TILE;
// keys, rekey, place, and histogram and scatter of at most 32 + 32 passes (1-bit digits: 32-bit positions, 32-bit postings)
const uint32_t POSITIONS_CURSORS = 3 + 2*64;
enum PositionsLaunch { POS_NONE = -1, POS_KEYS, POS_HISTOGRAM, POS_SCAN, POS_SCATTER, POS_REKEY, POS_PLACE, POS_OFFSETS, POS_LAUNCH_KINDS };

// diagnostics (host only): an event behind every launch of a call, with the kind of the launch; an event of kind POS_NONE stands
// in front of the first launch of each of the two halves, so the time of launch i is that from event i-1 to event i
struct PositionsLaunchEvents
{
	hipEvent_t* ev;			// capacity events, created
	int* kind;			// the PositionsLaunch behind which ev[i] was recorded
	size_t n, capacity;
};

struct PositionsParams
{
	// the finished batch, its terms and their postings
	const uint32_t* results;	// 9 words a result (sp_result_t)
	const uint64_t* docOffsets;	// ndocs+1
	const uint32_t* resultTerm;	// nresults
	const uint64_t* docTermOffsets;	// ndocs+1
	const uint32_t* postings;	// 4 words a posting (sp_posting_t)
	const uint32_t* recordPosting;	// N
	uint64_t nresults;		// the finished total, below 2^32 - 1: the pairs of the partition
	uint64_t nterms;		// N
	uint32_t ndocs;
	uint32_t digitBits;		// 1..8
	uint32_t tiles;			// radixTiles( nresults)
	// set by the host after its wait
	uint64_t nocc;
	uint32_t passes[ 2];		// of the two groups
	// working memory
	uint32_t* docOf;		// nresults
	uint64_t* pairs[ 2];		// nresults each
	uint32_t* hist;			// radixHistWords( nresults)
	uint32_t* cursor;		// POSITIONS_CURSORS, zeroed
	// the positions
	uint32_t* occurrences;		// 2 words an occurrence (sp_occurrence_t), 8-byte aligned
	uint64_t* postingOffsets;	// N+1
	uint32_t* postingPositions;	// N, zeroed
	uint64_t* totals;		// zeroed: [0] nocc, [1] the sum of postingPositions, [2] the largest participating ordpos
	PositionsLaunchEvents* events;	// host only, may be 0
};

// enqueue keys and offsets: totals[0] and totals[2] are what the host waits for
hipError_t launchL2PositionsCount( const PositionsParams& P, unsigned numCUs, hipStream_t stream);
// enqueue the two groups of passes, the rekey between them and the placement (P.nocc and P.passes set)
hipError_t launchL2PositionsPlace( const PositionsParams& P, unsigned numCUs, hipStream_t stream);

} // namespace
#endif
