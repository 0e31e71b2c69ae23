// Lookups in an index segment -- term blocks and posting blocks -- over host arrays: the definition that the device passes
// (l2_segment.h) are measured against and the entry point for products already fetched or read back from a file
// (sp_match_segment_lookup).  Host only: no HIP header and no HIP call in here.
//
// The rule (include/strus_pattern_amd.h "segment lookups"; the project's own, unpinned by a reference vector).  The walks are
// segment_walk.h, the one copy for this file and for the device; this file runs them in the order of the launches: the run of
// every query, where the runs start in the selection, the sizes of every selected position, their offsets, the bytes.
#ifndef SPA_MATCH_SEGMENT_HPP
#define SPA_MATCH_SEGMENT_HPP
#include "match_postingblocks.hpp"
#include "segment_walk.h"

namespace spa {

// The tables of the two products of one segment, which sp_segment_open and the twin check alike.  Throws std::runtime_error for
// products that are not one segment; the bytes are not decoded.
void checkSegmentTables( const sp_match_term_blocks_t* tb, const sp_match_posting_blocks_t* pb);

// the queries of a lookup call: throws std::runtime_error for unknown flags, arrays that are missing and offsets that descend
void checkSegmentQueries( const uint32_t* queryHandles, const uint64_t* queryOffsets, const uint8_t* queryBytes, uint64_t nq, uint32_t flags);

// the host arrays of a lookup of nq queries and nsel selected positions, zeroed (sp_segment_lookup_free) ...
void allocSegmentLookup( sp_segment_lookup_t* out, uint64_t nq, uint64_t nsel, uint32_t flags);
// ... and those that the totals size: values, postings, positions
void allocSegmentLookupLists( sp_segment_lookup_t* out, uint64_t npostings, uint64_t npositions, uint64_t nvalueBytes);

// throws std::runtime_error when a count of a lookup reaches 2^32 - 1
void checkSegmentLookupLimits( uint64_t nq, uint64_t nsel, uint64_t npostings, uint64_t npositions);

} // namespace
#endif
