// Pattern frequencies of a finished device batch (l2_freq_kernel.hip): behind l2_finish.h on the output side of the matcher,
// per document one record (handle, count, first ordpos, last ordend) per distinct handle, ascending by handle, and per
// handle the sums over the batch -- 16 bytes per distinct handle of a document in the place of 36 per result.
// The rule is that of pattern_freq.hpp (its device-free twin; include/strus_pattern_amd.h "pattern frequencies" states it).
// Passes on one stream, built on doc_passes.h:
//   A  count   a wave per document, the handle word of its finished records 64 a trip.  A first sweep checks every handle
//              against the bound (before it indexes anything), takes the minimum and maximum handle and marks the windows
//              of FREQ_WINDOW handles that the document touches; then one sweep per occupied window marks the distinct
//              handles of that window in the wave's LDS bitmap, whose popcount is their number.  Per document the record
//              count, the status and what the place pass needs again (minimum, maximum, occupied windows) go to HBM
//   B  offsets exclusive prefix sum of the record counts (a document with a range status counts 0), and the total
//   C  place   a wave per document and occupied window: the bitmap again, a running popcount per bitmap word (the rank of
//              a handle is the number of set bits below it: its record index in the document's block), the records of the
//              window initialised to {handle, 0, 0xFFFFFFFF, 0}, then per result an atomic add, minimum and maximum on its
//              record in HBM
//   D  totals  a thread per record of the batch: its count to handleResults, one to handleDocs.  A launch of its own, so
//              that the records it reads are complete without any ordering inside pass C
// The outputs are sums, minima and maxima: they do not depend on the order of the results nor on timing.  Whatever the
// records hold, a handle indexes the bitmap only inside the window it was compared against, a record index is compared
// against the document's block, the block against the capacity, and a result index against the finished total.
#ifndef SPA_L2_FREQ_H
#define SPA_L2_FREQ_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>

namespace spa {

// handles per sweep: a bitmap of 2 KB and 512 running popcounts of 16 bits, 3 KB of LDS per wave; the 10 000 patterns of
// the headline rule set are one window
enum { FREQ_WINDOW = 16384 };

struct FreqParams
{
	const uint32_t* results;	// finished results (9 words a record)
	const uint64_t* docOffsets;	// ndocs+1: the finished document offsets
	uint64_t nresults;		// the finished total, read by the host: every result index is checked against it
	uint32_t ndocs;
	uint32_t handleBound;		// valid handles: 1 .. handleBound-1
	// working memory
	uint32_t* docCount;		// ndocs: records of the document
	uint32_t* docMeta;		// ndocs x 4: minimum handle, maximum handle, occupied windows (64 bits, window index modulo 64)
	uint32_t* cursor;		// [0] pass A, [1] pass C; zeroed
	// the frequency batch
	int32_t* docStatus;		// ndocs
	uint64_t* docFreqOffsets;	// ndocs+1
	uint64_t* total;
	uint32_t* records;		// pass C and D only: 4 words a record
	uint64_t capacity;		// records of `records`: the total that pass B left, read by the host
	uint64_t* handleResults;	// handleBound, zeroed
	uint32_t* handleDocs;		// handleBound, zeroed
};

// enqueue the passes A and B
hipError_t launchL2FreqCount( const FreqParams& P, unsigned numCUs, hipStream_t stream);
// enqueue the passes C and D (records and capacity set from the total)
hipError_t launchL2FreqPlace( const FreqParams& P, unsigned numCUs, hipStream_t stream);

} // namespace
#endif
