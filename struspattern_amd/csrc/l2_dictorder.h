// Dictionary order of a finished device batch (l2_dictorder_kernel.hip): behind l2_dict.h on the output side of the matcher, the
// entries of the dictionary ranked by (handle, value bytes) -- order[k] the entry at sorted position k, rank its inverse,
// prefix_bytes[k] the leading bytes that the values of order[k-1] and order[k] share inside one handle, and handleOffsets, the
// exclusive prefix sums of handle_terms.  The rule is that of match_dictorder.hpp (its device-free twin;
// include/strus_pattern_amd.h "dictionary order" states it).  The value of an entry is that of the term record (first_doc,
// first_term): the range of its first_result in the source that the flags of the terms call select (l2_term_value.h).
// A comparison sort: an LSD radix over values of any length has no bounded number of passes, and a refinement by prefix rounds
// needs a wait of the host per round.  The host knows ndict, so it sizes everything and enqueues every launch on one stream;
// kernel boundaries are the only ordering between waves, nobody spins on a flag and no atomic decides where an entry goes.
//   keys     a lane per entry e: key64 = handle << 32 | the first four value bytes, big-endian, missing bytes as zero; the pair
//            (key64, e) into buffer 0, and where the value lies and how long it is into valueAt[e], valueLen[e].
//   tiles    a workgroup per tile of DICTORDER_TILE entries from the device cursor: a bitonic network in LDS over the next power of
//            two of the tile's entries (at least 64), padded with entries that follow every real one.
//   merge    one launch per level between the two buffers, run width doubling from the tile: a lane per entry finds its rank in
//            the partner run by bisection and writes itself to its own index plus that rank.  The order is strict, so every slot
//            of the pair of runs is written once.  A last partial run is merged by the same code; a run without a partner has
//            the rank 0 everywhere and is copied by it.  l2DictOrderLevels( ndict) levels; the order ends in buffer levels & 1.
//   place    a lane per sorted slot k: order[k], rank[order[k]] and prefix_bytes[k]; the handle and the entry of the slot before
//            come from the lane below, lane 0 loads them.
//   offsets  one workgroup: scanDocumentCounts over handle_terms in 64 bits, and the total.
// The comparator decides on key64.  Only on a tie it reads both values and compares the bytes from the first one (zero padding
// makes "a" and "a\0" tie on the key), then the lengths, and finally the entry indices, so that the order is total whatever the
// input holds.
// The tile: an entry is 12 bytes in LDS (key64 and index), 2048 of them 24 KiB, so that six workgroups of 256 threads share the
// 160 KiB of a CU.
// Whatever the records and the working arrays hold: an entry index is compared against ndict, a document against ndocs, a record
// index against N, a first_result against its document's results and those against the finished total, a source range against
// the source's total -- again when it is read back from valueAt / valueLen --, a destination slot against ndict.
#ifndef SPA_L2_DICTORDER_H
#define SPA_L2_DICTORDER_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>
#include "l2_terms.h"

namespace spa {

const uint32_t DICTORDER_TILE = 2048;		// entries per tile: a power of two, a multiple of the 256 threads of its workgroup
const uint32_t DICTORDER_CURSORS = 1;		// tiles

struct DictOrderParams
{
	// the dictionary, its terms batch and what their records point into
	const uint32_t* dictRecords;	// 8 words an entry (sp_dict_term_t)
	const uint32_t* handleTerms;	// handleBound
	const uint32_t* terms;		// 6 words a record (sp_match_term_t)
	const uint64_t* docTermOffsets;	// ndocs+1
	const uint64_t* docOffsets;	// ndocs+1: the finished document offsets
	const uint32_t* resultFormat;	// as in TermsParams
	uint64_t nterms;		// N, read by the host at the dictionary call
	uint64_t nresults;		// the finished total, read by the host at the terms call
	uint32_t ndict;			// read by the host at the dictionary call
	uint32_t ndocs;
	uint32_t handleBound;
	uint32_t flags;			// those of the terms call
	TermSourceDevice source[ 2];	// values, text
	uint32_t tiles;			// l2DictOrderTiles
	uint32_t levels;		// l2DictOrderLevels
	// working memory
	uint64_t* keys[ 2];		// ndict each
	uint32_t* index[ 2];		// ndict each: the entry of the key
	uint64_t* valueAt;		// ndict: the address of the value's first byte
	uint32_t* valueLen;		// ndict
	uint32_t* cursor;		// DICTORDER_CURSORS, zeroed
	// the order
	uint32_t* order;		// ndict
	uint32_t* rank;			// ndict, all 0xFFFFFFFF
	uint32_t* prefixBytes;		// ndict
	uint64_t* handleOffsets;	// handleBound+1
	uint64_t* total;
};

inline uint32_t l2DictOrderTiles( uint64_t ndict) { return (uint32_t)((ndict + DICTORDER_TILE - 1) / DICTORDER_TILE); }
// the merge levels for ndict entries: the doublings that take a run of one tile to all entries
inline uint32_t l2DictOrderLevels( uint64_t ndict)
{
	uint32_t levels = 0;
	for (uint64_t width=DICTORDER_TILE; width<ndict; width<<=1) ++levels;
	return levels;
}
// enqueue every launch
hipError_t launchL2DictOrder( const DictOrderParams& P, unsigned numCUs, hipStream_t stream);

} // namespace
#endif
