// Finishing a device batch on the device (l2_finish_kernel.hip): the output of the rule kernels (L2BatchIO: whole
// documents appended in completion order, found through (first, count) pairs) becomes what fetchResults returns per
// document -- document order, the `exclusive` elimination (src/patternMatcher.cpp:192-246, :278-289) applied, failed
// documents empty, item indices rebased to an item array without gaps.  Three passes on one stream:
//   A  count   kept results and items of every document (with `exclusive`: the covered flags first)
//   B  offsets exclusive prefix sums of the two per-document arrays, and the totals
//   C  place   the survivors and their items (and format words) move to their final place
// With P.canonical a sorting pass between B and C orders the survivors of every document by the tuple T of
// include/strus_pattern_amd.h (SP_FINISH_CANONICAL), and C places through the sorted indices.
// What the passes rely on, as copyOutBatch (capi_l2.cpp) does: the items of one document are ONE block in result order,
// and every result's item_begin is that block's start plus the item counts of the results before it (all three rule
// kernels write it so, for results without items too).
#ifndef SPA_L2_FINISH_H
#define SPA_L2_FINISH_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>

namespace spa {

struct FinishParams
{
	// the batch as the rule kernels left it (L2BatchIO output)
	const uint32_t* results;	// 9 words each
	const uint32_t* items;		// 7 words each
	const uint64_t* docRange;	// ndocs x (first result, count)
	const int32_t* docStatus;
	const uint32_t* resultFormat;	// if withFormats
	const uint32_t* itemFormat;	// 2 words per item, if withFormats
	uint64_t nofResults, nofItems;	// what of the batch's output lies inside its buffers: min( counter, capacity), read by the host after
					// the batch -- every index the passes form is checked against these two, and they size all buffers below
	uint32_t ndocs;
	uint32_t withFormats;
	uint32_t exclusive;
	uint32_t maxResultSize;
	// working memory
	uint8_t* covered;		// [results of the batch], zeroed; `exclusive` only
	uint32_t* kept;			// ndocs x {kept results, kept items}
	uint32_t* cursor;		// [0] pass A, [1] pass C; zeroed
	// the finished batch
	uint32_t* outResults;
	uint32_t* outItems;
	uint64_t* docResultOffsets;	// ndocs+1
	uint64_t* docItemOffsets;	// ndocs+1
	uint32_t* outResultFormat;
	uint32_t* outItemFormat;
	uint64_t* totals;		// results, items
	// canonical order (SP_FINISH_CANONICAL): working memory of the sort, two buffers of entries parallel to outResults
	uint32_t canonical;
	uint64_t* sortKeys[ 2];		// ordpos << 32 | ordend
	uint32_t* sortIdx[ 2];		// index of the result in its document's raw block
	uint32_t* sortCursor;		// zeroed
};

// the most results of one document that the sort orders in one workgroup's LDS without a merge pass: 12 bytes an entry,
// 48 KiB a tile, three workgroups on the 160 KiB of a CU
enum { FINISH_SORT_TILE = 4096 };

// enqueue the passes; between them the events ev[0..3], if given (timing of the passes); with P.canonical ev[4] between
// the sort and the placement
hipError_t launchL2Finish( const FinishParams& P, unsigned numCUs, hipStream_t stream, hipEvent_t* ev);

} // namespace
#endif
