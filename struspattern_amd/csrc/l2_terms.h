// Index terms of a finished device batch (l2_terms_kernel.hip): behind l2_finish.h, l2_values.h and l2_text.h on the output
// side of the matcher, per document one record per distinct term (handle, value bytes) of its results and per result the
// index of its term -- 24 bytes per distinct term and 4 per result in the place of 36 per result plus the value bytes.
// The rule is that of match_terms.hpp (its device-free twin; include/strus_pattern_amd.h "index terms" states it).
// The value of a result is its range in one of up to two sources (values, text): bytes plus nresults+1 offsets.
// Passes on one stream, built on doc_passes.h, a wave per document:
//   A  count   a lane per result, 64 a trip.  A first sweep checks every handle against the bound.  Then every lane hashes
//              (handle, length, bytes) of its result and looks its term up in an open-addressing table of 2n slots for the
//              n results of the document -- in the wave's LDS for n <= TERM_TILE, in HBM working memory beyond.  A slot
//              holds the index of a result.  The lane probes from the slot of its hash: an empty slot it takes with a
//              compare-and-swap; the result in an occupied slot it compares with its own, handle, length and BYTES; if
//              they are equal the slot is its term's and takes the minimum of the two indices, if not the lane goes to the
//              next slot.  Slots never empty again, so all results of a term meet in one slot, whatever the timing, and
//              after the sweep the slot holds the term's smallest index: leader[r].  The hash chooses where the probing
//              starts and decides nothing else (sp_test_term_hash_bits masks it down to any width).  The number of
//              results that lead themselves is the number of terms.
//   B  offsets exclusive prefix sum of the term counts (a failed document counts 0), and the total
//   C  place   the order (handle, first_result) without a sort: the terms per handle are counted into a histogram over the
//              handles (HBM working memory of the wave), its exclusive prefix sums are the first record of every handle,
//              and the leaders, taken in index order 64 a trip, get consecutive records behind it (the leaders of a trip
//              with the same handle are ranked among themselves in registers; one atomic add per handle and trip moves
//              the histogram entry on).  A leader initialises its record and writes its term index to resultTerm; then
//              every result copies the term index of its leader and adds its count, minimum and maximum to the record.
// Whatever the records and the working arrays hold: a result index is compared against the finished total, a handle
// against the bound before it is used, a source range against the source's total, a leader against the document's results,
// a term index against the document's block and the block against the capacity.
#ifndef SPA_L2_TERMS_H
#define SPA_L2_TERMS_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>

namespace spa {

// results of a document whose table (2 slots of 4 bytes per result) lies in LDS: 8 KB per wave, 32 KB per workgroup
enum { TERM_TILE = 1024 };

struct TermSourceDevice
{
	const uint8_t* bytes;
	const uint64_t* offsets;	// nresults+1, parallel to the finished results
	uint64_t total;			// bytes of `bytes`, read by the host
	const int32_t* docStatus;	// ndocs
};

struct TermsParams
{
	const uint32_t* results;	// finished results (9 words a record)
	const uint32_t* resultFormat;	// selector with both sources: != 0 the values, else the text; NULL: the text
	const uint64_t* docOffsets;	// ndocs+1: the finished document offsets
	uint64_t nresults;		// the finished total, read by the host: every result index is checked against it
	uint32_t ndocs;
	uint32_t handleBound;		// valid handles: 1 .. handleBound-1
	uint32_t flags;			// SP_TERM_VALUES | SP_TERM_TEXT
	uint32_t hashMask;		// sp_test_term_hash_bits
	TermSourceDevice source[ 2];	// values, text
	// working memory
	uint32_t* leader;		// nresults: index inside the document of the first result with the same term
	uint32_t* table;		// 2 x nresults: the slots of document d start at 2*docOffsets[d]
	uint32_t* histogram;		// waves x handleBound: terms per handle of the document a wave places
	uint32_t* docCount;		// ndocs: terms of the document
	uint32_t* cursor;		// [0] pass A, [1] pass C; zeroed
	// the terms batch
	int32_t* docStatus;		// ndocs
	uint64_t* docTermOffsets;	// ndocs+1
	uint64_t* total;
	uint32_t* resultTerm;		// nresults
	uint32_t* records;		// pass C only: 6 words a record
	uint64_t capacity;		// records of `records`: the total that pass B left, read by the host
};

// the waves of the passes A and C (histogram is sized by it)
unsigned l2TermsWaves( size_t ndocs, unsigned numCUs);
// enqueue the passes A and B
hipError_t launchL2TermsCount( const TermsParams& P, unsigned numCUs, hipStream_t stream);
// enqueue pass C (records and capacity set from the total)
hipError_t launchL2TermsPlace( const TermsParams& P, unsigned numCUs, hipStream_t stream);

} // namespace
#endif
