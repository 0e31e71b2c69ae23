// Batch postings of a finished device batch (l2_postings_kernel.hip): behind l2_dict.h on the output side of the matcher, for
// every entry of the dictionary the list of its documents -- one 16-byte posting {doc, term, count, first_ordpos} per term
// record, the postings of entry e at [entryOffsets[e], entryOffsets[e+1]) ascending by document -- and per term record the
// index of its posting.  The rule is that of match_postings.hpp (its device-free twin; include/strus_pattern_amd.h "batch
// postings" states it).  No source byte is read: termDict says which records are the same term.
// The core is a stable LSD radix partition of the pairs (key = termDict[i], payload = i) by key: the records come in ascending
// i, so a stable partition by entry leaves every list ascending by record, that is by document.  Digits of digitBits bits (8;
// sp_test_postings_digit_bits), ceil(bitwidth(ndict - 1) / digitBits) passes, none for ndict <= 1.  All launches on one stream,
// built on doc_passes.h; the data of the partition sees no atomic in HBM and nobody spins on a flag: kernel boundaries are the
// only ordering between waves, and what a wave does depends on its tile alone, never on which wave it is.
//   keys       a wave per document from the device cursor, a lane per term record, 64 a trip: docOf[i], and the pair
//              (termDict[i], i) as one 8-byte store into pairs[0].  A key at or beyond ndict becomes ndict - 1.
//   offsets    one workgroup: the exclusive prefix sums of doc_freq over the dictionary records in 64 bits (scanDocumentCounts),
//              and the total.
//   per pass   histogram, scan, scatter over fixed tiles of records (radix_passes.h, shared with l2_positions.h).
//   place      for sorted position p holding record i: postings[p] = {docOf[i], i - docTermOffsets[docOf[i]], count,
//              first_ordpos} as one 16-byte store and recordPosting[i] = p.
// POSTINGS_TILE is RADIX_TILE; radix_passes.h says what bounds it.
// Whatever the working arrays hold: a record index is compared against N before a term record is read, a key against ndict,
// a document against ndocs, a rank against N; a digit is masked to the counters of the wave.
#ifndef SPA_L2_POSTINGS_H
#define SPA_L2_POSTINGS_H
#include "radix_passes.h"

namespace spa {

const uint32_t POSTINGS_TILE = RADIX_TILE;		// records per tile
const uint32_t POSTINGS_MAX_DIGIT_BITS = RADIX_MAX_DIGIT_BITS;
const uint32_t POSTINGS_CURSORS = 2 + 2*32;	// keys, place, and histogram and scatter of at most 32 passes (1-bit digits)

struct PostingsParams
{
	// the terms batch and its dictionary
	const uint32_t* terms;		// 6 words a record (sp_match_term_t)
	const uint64_t* docTermOffsets;	// ndocs+1
	const uint32_t* termDict;	// N
	const uint32_t* dictRecords;	// 8 words an entry (sp_dict_term_t)
	uint64_t nterms;		// N, read by the host at the dictionary call (below 2^32 - 1)
	uint32_t ndict;			// read by the host at the dictionary call
	uint32_t ndocs;
	uint32_t digitBits;		// 1..8
	uint32_t passes;		// l2PostingsPasses
	uint32_t tiles;			// l2PostingsTiles
	// working memory
	uint32_t* docOf;		// N
	uint64_t* pairs[ 2];		// N each: key in the low word, record index in the high one
	uint32_t* hist;			// 2^digitBits x tiles, written whole by every histogram launch
	uint32_t* cursor;		// POSTINGS_CURSORS, zeroed
	// the postings
	uint32_t* postings;		// 4 words a posting (sp_posting_t), 16-byte aligned
	uint64_t* entryOffsets;		// ndict+1
	uint32_t* recordPosting;	// N
	uint64_t* total;
};

inline uint32_t l2PostingsTiles( uint64_t nterms) { return radixTiles( nterms); }
// the radix passes for ndict entries: the digits of the largest key, ndict - 1
inline uint32_t l2PostingsPasses( uint64_t ndict, uint32_t digitBits) { return radixPasses( ndict ? ndict - 1 : 0, digitBits); }
// enqueue every launch
hipError_t launchL2Postings( const PostingsParams& P, unsigned numCUs, hipStream_t stream);

} // namespace
#endif
