// Batch dictionary of a finished device batch (l2_dict_kernel.hip): behind l2_terms.h on the output side of the matcher, every
// distinct term (handle, value bytes) of the terms batch once, in the order of first occurrence, with its document frequency,
// its collection frequency and the largest per-document count, and per term record the index of its entry -- 32 bytes per
// distinct term of the batch and 4 per term record.  The rule is that of match_dict.hpp (its device-free twin;
// include/strus_pattern_amd.h "batch dictionary" states it).  A term record's value is the range of its first_result in
// the source that the flags of the terms call select (l2_term_value.h: valueOf, hashTerm, sameBytes, shared with the terms).
// Five launches on one stream, built on doc_passes.h, a wave per document and a lane per term record, 64 a trip, so that a
// lane knows the document of its own record without a search:
//   1  insert      every lane hashes (handle, length, bytes) of its record and probes ONE open-addressing table of
//                  tableSlots >= 2N slots in HBM (empty = 0xFFFFFFFF, set by hipMemsetAsync); a slot holds a global record
//                  index.  An empty slot is taken with a compare-and-swap; the occupant of a taken slot is compared with the
//                  lane's record by handle, length and BYTES (the occupant's document is found by a binary search over the
//                  term offsets: they were written by an earlier launch); only on equality the slot takes the minimum of the
//                  two indices, else the lane moves on.  Slots never empty again, so all records of a term meet in one slot
//                  whatever the timing.  The lane keeps the slot it ended in: slot[i].  The table is written from every XCD:
//                  it is touched with agent-scope atomics only.
//   2  resolve     leader[i] = table[slot[i]], the smallest record index of i's term; the records that lead themselves are
//                  the entries first seen in their document: docCount.  A launch of its own because a slot has its final
//                  minimum only when every wave of launch 1 is through; no flag, no fence anybody spins on.
//   3  offsets     exclusive prefix sums of docCount: docDictOffsets and the total.  The host waits here once, for the size
//                  of the records.
//   4  place       per trip a ballot of the leaders; the popcount below a lane ranks it behind the running base of the
//                  document.  The leader writes the entry {handle, value_bytes, doc, local index, 0, 0, 0} and termDict[i],
//                  and the leaders of a trip with the same handle add their number to handleTerms with one atomic.
//   5  accumulate  a launch of its own, so that every entry index and every zeroed entry is there: every record copies
//                  termDict[leader[i]] and adds 1 to doc_freq, its count to count (64 bits) and takes the maximum for
//                  max_count.  Sums and maxima: no output word depends on timing, nor on the hash.
// Whatever the records and the working arrays hold: a record index is compared against N, a first_result against its
// document's results and those against the finished total, a source range against the source's total, a slot against the
// table, a leader against its record's own index, an entry index against the document's range and that against the capacity.
#ifndef SPA_L2_DICT_H
#define SPA_L2_DICT_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>
#include "l2_terms.h"

namespace spa {

struct DictParams
{
	// the terms batch and what its records point into
	const uint32_t* terms;		// 6 words a record (sp_match_term_t)
	const uint64_t* docTermOffsets;	// ndocs+1
	uint64_t nterms;		// N, read by the host: every record index is checked against it (below 2^32 - 1)
	const uint64_t* docOffsets;	// ndocs+1: the finished document offsets
	const uint32_t* resultFormat;	// as in TermsParams
	uint64_t nresults;		// the finished total, read by the host
	uint32_t ndocs;
	uint32_t handleBound;
	uint32_t flags;			// those of the terms call
	uint32_t hashMask;		// sp_test_term_hash_bits
	TermSourceDevice source[ 2];	// values, text
	// working memory
	uint32_t* table;		// tableSlots, all 0xFFFFFFFF
	uint32_t tableSlots;		// min( 2N, 2^32 - 1), at least 2
	uint32_t* slot;			// N
	uint32_t* leader;		// N
	uint32_t* docCount;		// ndocs, zeroed: entries first seen in the document
	uint32_t* cursor;		// one per wave-per-document launch (4), zeroed
	// the dictionary
	uint64_t* docDictOffsets;	// ndocs+1
	uint64_t* total;
	uint32_t* termDict;		// N
	uint32_t* handleTerms;		// handleBound, zeroed
	uint32_t* records;		// launches 4 and 5 only: 8 words an entry (sp_dict_term_t)
	uint64_t capacity;		// entries of `records`: the total that launch 3 left, read by the host
};

// the slots of the table for N term records
inline uint32_t l2DictTableSlots( uint64_t nterms)
{
	const uint64_t m = 2*nterms;
	return m < 2 ? 2u : (m > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)m);
}
// enqueue the launches 1 to 3
hipError_t launchL2DictCount( const DictParams& P, unsigned numCUs, hipStream_t stream);
// enqueue the launches 4 and 5 (records and capacity set from the total)
hipError_t launchL2DictPlace( const DictParams& P, unsigned numCUs, hipStream_t stream);

} // namespace
#endif
