// Result values of a finished device batch (l2_values_kernel.hip): behind l2_finish.h on the output side of the matcher,
// the values of the format strings of the finished results and items, built from the format table, the finished records
// and the text the lexer batch ran on without leaving HBM.  The rule is that of result_values.hpp (its device-free twin;
// include/strus_pattern_amd.h "result values" states it), the walk that evaluates a value is the one copy in value_walk.h.
// Three passes on one stream, per family (results, item records; one templated set of kernels):
//   A  count   a wave per document, its records in rounds of 64, a lane per record: the lane walks its value with the
//              explicit stack of value_walk.h (in LDS, 5 words per level and lane) and adds up the lengths of its pieces;
//              a wave scan gives the value's offset inside the document (valueWork), per document the byte count and status
//   B  offsets exclusive prefix sum of the per-document byte counts (a failed document counts 0), and the total
//   C  place   a wave per document: the value offsets, and the bytes
// A runs for every requested family before B runs for any: a document that fails in one family is empty in both.
// The copy of C goes piece by piece over all lanes at once: every lane repeats its walk and hands out one piece (pool or
// text, source offset, length, destination) per step; the up to 64 pieces of a step are laid end to end in LDS and the
// wave copies their bytes together, a lane per byte, finding the piece of a byte among the step's 64 offsets (6 steps of
// a search).  Every byte is stored on its own, so a wave never stores a byte it does not own, and no lane copies more
// than its share of a long piece.
#ifndef SPA_L2_VALUES_H
#define SPA_L2_VALUES_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>

namespace spa {

struct ValuesFamily
{
	const uint32_t* records;	// finished results (9 words; item_begin, item_count in words 7, 8) or items (7 words)
	const uint32_t* format;		// result_format (1 word a record) or item_format (2 words)
	const uint64_t* docOffsets;	// ndocs+1: the finished document offsets of the family
	uint64_t nrecords;		// the finished total, read by the host: every record index is checked against it
	// working memory
	uint32_t* valueWork;		// nrecords: offset of the value inside its document
	uint64_t* docBytes;		// ndocs
	// the values batch
	uint64_t* docValueOffsets;	// ndocs+1
	uint64_t* valueOffsets;		// nrecords+1
	uint8_t* outValues;		// pass C only
	uint64_t outCapacity;		// bytes of outValues: the total that pass B left, read by the host
	uint64_t* total;
	uint32_t* cursor;		// [0] pass A, [1] pass C; zeroed
};

struct ValuesParams
{
	// the text source (l2_span.h)
	const uint8_t* text; uint64_t nbytes;
	const uint64_t* segOffsets; uint64_t nseg;
	const uint64_t* docSegOffsets;	// NULL: document d is segment d (the host has checked nseg == ndocs)
	// the format table (value_walk.h), uploaded once per context
	const uint32_t* fmtParts; const uint32_t* parts; const uint8_t* pool;
	uint32_t formatCount; uint32_t poolBytes;
	// the finished items: the arguments of every value
	const uint32_t* items; const uint32_t* itemFormat;
	const uint64_t* docItemOffsets; uint64_t nitems;
	uint32_t ndocs;
	int32_t* docStatus;		// ndocs, zeroed
	ValuesFamily family[ 2];	// results, items
	uint32_t families;		// SP_VALUE_RESULTS | SP_VALUE_ITEMS
};

// enqueue the passes A and B of the requested families
hipError_t launchL2ValuesCount( const ValuesParams& P, unsigned numCUs, hipStream_t stream);
// enqueue pass C (outValues and outCapacity set from the totals)
hipError_t launchL2ValuesPlace( const ValuesParams& P, unsigned numCUs, hipStream_t stream);

} // namespace
#endif
