// What the device-free twins of the products of a finished batch share (span_text, result_values, pattern_freq, match_terms,
// match_dict): their zero-filled arrays, the check that a batch is a finished one, the shell of their C entry points and the
// host skeleton of a product of bytes per record.  A new product's twin starts from here.
// Host only and header only: no HIP header and no HIP call in here, and no source file to add to a compile command.  Everything
// has internal linkage (the unnamed namespace): the library exports its entry points and the twins, nothing of this.
#ifndef SPA_FINISHED_HOST_HPP
#define SPA_FINISHED_HOST_HPP
#include "batch_fetch.hpp"

namespace spa {
namespace {

// malloc'ed array of n elements, at least one, every byte of it `byte`
template <class T>
T* filledArray( uint64_t n, int byte = 0)
{
	if (!n) n = 1;
	T* p = hostArray<T>( n);
	std::memset( p, byte, (size_t)n * sizeof(T));
	return p;
}

// the ndocs+1 document offsets of a finished batch: they start at 0, ascend inside its results and cover them
void checkDocOffsets( const uint64_t* docOffsets, size_t ndocs, uint64_t nresults)
{
	if (docOffsets[ 0] != 0) throw std::runtime_error( "document offsets of the batch do not start at its first result");
	for (size_t d=0; d<ndocs; ++d)
	{
		if (docOffsets[ d] > docOffsets[ d+1] || docOffsets[ d+1] > nresults) throw std::runtime_error( "document offsets of the batch do not ascend inside its results");
	}
	if (docOffsets[ ndocs] != nresults) throw std::runtime_error( "document offsets of the batch do not cover its results");
}

// The same check for a product that reads the items too; returns where the records of every document lie, ndocs+1 offsets
// each.  (The items of a finished batch have no gaps and are in result order.  A batch of no documents need not have offsets.)
struct DocRecords { std::vector<uint64_t> results, items; };
DocRecords finishedDocRecords( const sp_match_batch_t& mb)
{
	const size_t ndocs = mb.ndocs;
	if (ndocs && !mb.doc_result_offsets) throw std::runtime_error( "batch without document offsets");
	DocRecords docs = { std::vector<uint64_t>( ndocs + 1, 0), std::vector<uint64_t>( ndocs + 1, 0) };
	if (ndocs) std::memcpy( docs.results.data(), mb.doc_result_offsets, (ndocs + 1) * sizeof(uint64_t));
	checkDocOffsets( docs.results.data(), ndocs, mb.nresults);
	for (size_t d=0; d<ndocs; ++d)
	{
		uint64_t n = 0;
		for (uint64_t i=docs.results[ d]; i<docs.results[ d+1]; ++i) n += mb.results[ i].item_count;
		docs.items[ d+1] = docs.items[ d] + n;
	}
	if (docs.items[ ndocs] != mb.nitems) throw std::runtime_error( "not a finished batch: results or items outside the documents");
	return docs;
}

// The shell of a C entry point sp_match_batch_*: `out` and `err` cleared, then `fn`; after an exception `out` is released and
// empty again, and a failure other than of memory leaves its message in `err`, cut to the buffer.
template <class OUT, class FN>
int hostProduct( OUT* out, void (*release)( OUT*), char* err, size_t errsize, FN fn)
{
	std::memset( out, 0, sizeof(*out));
	if (err && errsize) err[ 0] = 0;
	try { fn(); return SP_OK; }
	catch (const std::bad_alloc&) { release( out); return SP_ERR_NOMEM; }
	catch (const std::exception& e)
	{
		release( out);
		if (err && errsize) { std::strncpy( err, e.what(), errsize-1); err[ errsize-1] = 0; }
		return SP_ERR_INVALID;
	}
}

// ---- One family (results or items) of a product of bytes per record (text, values): the records of document d are
// [docOffsets[d], docOffsets[d+1]).  RECORDS says what a record's bytes are:
//	bool length( size_t d, uint64_t i, uint64_t& n)		the bytes of record i of document d; false: the document fails
//	void write( size_t d, uint64_t i, char* dst)		those bytes to dst (documents without a status only)
// Every requested family is counted before one is placed: the status is that of the document, in both families.
struct ByteFamily
{
	const uint64_t* docOffsets; size_t ndocs;
	char** bytes; uint64_t* offsets; uint64_t* total;	// of the caller's struct: ndocs' records + 1 offsets
	std::vector<uint32_t> work;				// per record: its offset inside the document
	std::vector<uint64_t> docBytes;

	// pass A of the device: offsets inside the document, its byte count, its status (a record that fails, or 2^32 bytes and more)
	template <class RECORDS>
	void count( const RECORDS& records, int32_t* status)
	{
		const uint64_t MAX32 = 0xFFFFFFFFull;
		work.assign( (size_t)docOffsets[ ndocs] + 1, 0);
		docBytes.assign( ndocs + 1, 0);
		for (size_t d=0; d<ndocs; ++d)
		{
			uint64_t sum = 0;
			bool ok = true;
			for (uint64_t i=docOffsets[ d]; ok && i<docOffsets[ d+1]; ++i)
			{
				uint64_t n = 0;
				work[ i] = (uint32_t)sum;
				ok = records.length( d, i, n) && n <= MAX32;
				if (ok) sum += n;
				if (sum > MAX32) ok = false;
			}
			if (ok) docBytes[ d] = sum; else status[ d] = SP_DOC_ERR_RANGE;
		}
	}

	// passes B and C of the device: where the bytes of every document and record start, the bytes (one more than the total)
	template <class RECORDS>
	void place( const RECORDS& records, const int32_t* status)
	{
		std::vector<uint64_t> docAt( ndocs + 1, 0);
		for (size_t d=0; d<ndocs; ++d) docAt[ d+1] = docAt[ d] + (status[ d] ? 0 : docBytes[ d]);
		*total = docAt[ ndocs];
		*bytes = hostArray<char>( docAt[ ndocs] + 1);
		for (size_t d=0; d<ndocs; ++d)
		{
			for (uint64_t i=docOffsets[ d]; i<docOffsets[ d+1]; ++i)
			{
				offsets[ i] = docAt[ d] + (status[ d] ? 0 : work[ i]);
				if (!status[ d]) records.write( d, i, *bytes + offsets[ i]);
			}
		}
		offsets[ docOffsets[ ndocs]] = docAt[ ndocs];
	}
};

} // namespace
} // namespace
#endif
