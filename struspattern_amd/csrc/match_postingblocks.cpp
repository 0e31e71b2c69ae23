// Posting blocks of a dictionary, its order, postings and positions over host arrays, and their reader (match_postingblocks.hpp):
// host only, no device needed.
#include "match_postingblocks.hpp"
#include "posting_block_code.h"
#include "finished_host.hpp"

namespace spa {

void allocMatchPostingBlocks( sp_match_posting_blocks_t* out, uint64_t ndict, uint64_t nblocks, uint32_t blockEntries)
{
	out->ndict = (size_t)ndict; out->nblocks = (size_t)nblocks; out->block_entries = blockEntries;
	out->totals[ 0] = nblocks; out->totals[ 2] = blockEntries;
	out->block_offsets = filledArray<uint64_t>( nblocks + 1, 0);
}

void allocMatchPostingBlockBytes( sp_match_posting_blocks_t* out, uint64_t nbytes)
{
	out->nbytes = (size_t)nbytes; out->totals[ 1] = nbytes;
	out->bytes = filledArray<uint8_t>( nbytes + 1, 0);
}

namespace {

// The occurrences of the list of one sorted position, one behind the other, as the device walks them: fn( firstOfList,
// firstOfPosting, header, ordpos, ordposBefore) per occurrence.
template <class FN>
void walkList( const sp_posting_t* postings, uint64_t p0, uint64_t p1, const sp_occurrence_t* occurrences, const uint64_t* postingOffsets,
	       const uint32_t* postingPositions, FN fn)
{
	for (uint64_t p=p0; p<p1; ++p)
	{
		const PostingBlockHeader h = postingBlockHeader( p == p0, postings[ p].doc, p == p0 ? 0 : postings[ p-1].doc, postings[ p].count, postingPositions[ p]);
		for (uint64_t o=postingOffsets[ p]; o<postingOffsets[ p+1]; ++o)
		{
			const bool first = o == postingOffsets[ p];
			fn( p == p0 && first, first, h, occurrences[ o].ordpos, first ? 0 : occurrences[ o-1].ordpos);
		}
	}
}

} // namespace

void matchPostingBlocks( const sp_dict_term_t* entries, uint64_t ndict, const uint32_t* order, const sp_posting_t* postings,
			 const uint64_t* entryOffsets, uint64_t nterms, const sp_occurrence_t* occurrences, const uint64_t* postingOffsets,
			 const uint32_t* postingPositions, uint64_t nocc, uint32_t blockEntries, sp_match_posting_blocks_t* out)
{
	if (!termBlockEntriesValid( blockEntries)) throw std::runtime_error( "a block size that is not 1, 2, 4, 8, 16, 32 or 64");
	if (ndict && (!entries || !order)) throw std::runtime_error( "a dictionary or an order without its arrays");
	if (!entryOffsets || !postingOffsets || (nterms && (!postings || !postingPositions)) || (nocc && !occurrences))
		throw std::runtime_error( "postings or positions without their arrays");
	// the order, the postings and the positions are those of one dictionary
	std::vector<bool> seen( (size_t)ndict, false);
	for (uint64_t k=0; k<ndict; ++k)
	{
		if (order[ k] >= ndict || seen[ order[ k]]) throw std::runtime_error( "an order that is not a permutation of the entries");
		seen[ order[ k]] = true;
	}
	if (entryOffsets[ 0] != 0 || entryOffsets[ ndict] != nterms) throw std::runtime_error( "entry offsets that do not cover the postings");
	for (uint64_t e=0; e<ndict; ++e)
	{
		if (entryOffsets[ e] > entryOffsets[ e+1] || entryOffsets[ e+1] > nterms) throw std::runtime_error( "entry offsets that do not ascend inside the postings");
		if (entries[ e].doc_freq != entryOffsets[ e+1] - entryOffsets[ e]) throw std::runtime_error( "a doc_freq that is not the length of its list");
	}
	if (postingOffsets[ 0] != 0 || postingOffsets[ nterms] != nocc) throw std::runtime_error( "posting offsets that do not cover the occurrences");
	for (uint64_t p=0; p<nterms; ++p)
	{
		if (postingOffsets[ p] > postingOffsets[ p+1] || postingOffsets[ p+1] > nocc) throw std::runtime_error( "posting offsets that do not ascend inside the occurrences");
		if (!postings[ p].count) throw std::runtime_error( "a posting with a count of 0");
		// (the count is coded as the word says: that it is the number of occurrences is the positions twin's to check)
		if (postingOffsets[ p] == postingOffsets[ p+1]) throw std::runtime_error( "a posting without an occurrence");
		uint64_t distinct = 1;
		for (uint64_t o=postingOffsets[ p]+1; o<postingOffsets[ p+1]; ++o)
		{
			if (occurrences[ o].ordpos < occurrences[ o-1].ordpos) throw std::runtime_error( "positions that do not ascend inside a posting");
			if (occurrences[ o].ordpos != occurrences[ o-1].ordpos) ++distinct;
		}
		if (!postingPositions[ p] || postingPositions[ p] > postings[ p].count) throw std::runtime_error( "a posting_positions that is 0 or above the count");
		if (postingPositions[ p] != distinct) throw std::runtime_error( "a posting_positions that is not the number of distinct positions");
	}
	for (uint64_t e=0; e<ndict; ++e)
	{
		for (uint64_t p=entryOffsets[ e]+1; p<entryOffsets[ e+1]; ++p)
		{
			if (postings[ p].doc <= postings[ p-1].doc) throw std::runtime_error( "documents that do not ascend inside a list");
		}
	}

	const uint64_t nblocks = (ndict + blockEntries - 1) / blockEntries;
	allocMatchPostingBlocks( out, ndict, nblocks, blockEntries);
	// the sizes, the offsets, the codes
	std::vector<uint64_t> body( (size_t)ndict, 0);
	uint64_t nbytes = 0, gaps = 0;
	for (uint64_t k=0; k<ndict; ++k)
	{
		if (k % blockEntries == 0) out->block_offsets[ k / blockEntries] = nbytes;
		walkList( postings, entryOffsets[ order[ k]], entryOffsets[ order[ k]+1], occurrences, postingOffsets, postingPositions,
			[&]( bool, bool firstOfPosting, const PostingBlockHeader& h, uint32_t ordpos, uint32_t before) {
				body[ k] += postingOccurrenceBytes( firstOfPosting, h, ordpos, before);
				if (positionGapBytes( firstOfPosting, ordpos, before)) ++gaps;
			});
		nbytes += postingListBytes( body[ k]);
	}
	out->block_offsets[ nblocks] = nbytes;
	out->totals[ 3] = gaps;
	allocMatchPostingBlockBytes( out, nbytes);
	uint64_t at = 0;
	for (uint64_t k=0; k<ndict; ++k)
	{
		uint8_t piece[ POSTING_BLOCK_OCCURRENCE_MAX];
		walkList( postings, entryOffsets[ order[ k]], entryOffsets[ order[ k]+1], occurrences, postingOffsets, postingPositions,
			[&]( bool firstOfList, bool firstOfPosting, const PostingBlockHeader& h, uint32_t ordpos, uint32_t before) {
				const uint32_t n = writePostingOccurrence( piece, firstOfList, body[ k], firstOfPosting, h, ordpos, before);
				if (n > nbytes - at) throw std::logic_error( "the codes are longer than they were counted");
				std::memcpy( out->bytes + at, piece, n);
				at += n;
			});
	}
	if (at != nbytes) throw std::logic_error( "the codes are not as long as they were counted");
}

} // namespace

extern "C" void sp_match_posting_blocks_free( sp_match_posting_blocks_t* pb)
{
	std::free( pb->bytes); std::free( pb->block_offsets);
	std::memset( pb, 0, sizeof(*pb));
}

extern "C" int sp_match_batch_posting_blocks( const sp_match_dictionary_t* dict, const sp_match_dictionary_order_t* order,
					      const sp_match_postings_t* postings, const sp_match_positions_t* positions,
					      sp_match_posting_blocks_t* out, char* err, size_t errsize)
{
	return spa::hostProduct( out, sp_match_posting_blocks_free, err, errsize, [&]{
		if (!dict) throw std::runtime_error( "no dictionary");
		if (!order) throw std::runtime_error( "no order");
		if (!postings) throw std::runtime_error( "no postings");
		if (!positions) throw std::runtime_error( "no positions");
		if (order->ndict != dict->ndict) throw std::runtime_error( "the order is not that of the dictionary: another number of entries");
		if (postings->ndict != dict->ndict) throw std::runtime_error( "the postings are not those of the dictionary: another number of entries");
		if (positions->nterms != postings->nterms) throw std::runtime_error( "the positions are not those of the postings: another number of postings");
		if (dict->ndict >= 0xFFFFFFFFull || postings->nterms >= 0xFFFFFFFFull || positions->nocc >= 0xFFFFFFFFull)
			throw std::runtime_error( "2^32 - 1 entries, postings or occurrences, or more");
		spa::matchPostingBlocks( dict->records, dict->ndict, order->order, postings->postings, postings->entry_offsets, postings->nterms,
					 positions->occurrences, positions->posting_offsets, positions->posting_positions, positions->nocc,
					 spa::termBlockEntries(), out);
	});
}

extern "C" int sp_match_posting_blocks_decode_block( const sp_match_posting_blocks_t* pb, size_t j, uint32_t* list_postings, size_t nlists_cap,
						     sp_block_posting_t* postings, size_t npostings_cap, uint32_t* positions, size_t npositions_cap,
						     size_t* nlists, size_t* npostings, size_t* npositions, char* err, size_t errsize)
{
	using namespace spa;
	if (nlists) *nlists = 0;
	if (npostings) *npostings = 0;
	if (npositions) *npositions = 0;
	if (err && errsize) err[ 0] = 0;
	try
	{
		if (!pb || !nlists || !npostings || !npositions) throw std::runtime_error( "no posting blocks, or nowhere to count to");
		if (j >= pb->nblocks || !pb->block_offsets) throw std::runtime_error( "no such block");
		if (!termBlockEntriesValid( pb->block_entries)) throw std::runtime_error( "a block size that is not 1, 2, 4, 8, 16, 32 or 64");
		uint64_t at = pb->block_offsets[ j];
		const uint64_t end = pb->block_offsets[ j+1];
		if (at > end || end > pb->nbytes || (end && !pb->bytes)) throw std::runtime_error( "block offsets that descend or leave the bytes");
		if (at == end) throw std::runtime_error( "an empty block");
		const bool count = !list_postings && !postings && !positions;
		const char* const past = "a varint that runs past the block or is longer than ten bytes";
		uint64_t nl = 0, np = 0, nq = 0;
		bool room = true;
		for (; at < end; ++nl)
		{
			if (nl >= pb->block_entries) throw std::runtime_error( "a block of more lists than a block holds");
			uint64_t body = 0;
			if (!readVarint( pb->bytes, at, end, body)) throw std::runtime_error( past);
			if (body > end - at) throw std::runtime_error( "a body that runs past the block");
			if (!body) throw std::runtime_error( "a body of 0: a list without a posting");
			const uint64_t listEnd = at + body;
			uint64_t doc = 0, inList = 0;
			const char* const beyond = "a posting that ends beyond its body";
			for (; at < listEnd; ++inList, ++np)
			{
				uint64_t field[ 3];
				for (int i=0; i<3; ++i)
				{
					if (!readVarint( pb->bytes, at, end, field[ i])) throw std::runtime_error( past);
					if (at > listEnd) throw std::runtime_error( beyond);
				}
				if (inList && !field[ 0]) throw std::runtime_error( "a ddelta of 0 behind the first posting of a list");
				if (field[ 0] > 0xFFFFFFFFull || (doc += field[ 0]) > 0xFFFFFFFFull || field[ 1] > 0xFFFFFFFFull) throw std::runtime_error( "a document or a count that leaves 32 bits");
				if (!field[ 2] || field[ 2] > field[ 1]) throw std::runtime_error( "an npos of 0 or above the count");
				const bool fits = room && !count && postings && np < npostings_cap;
				if (!count && !fits) room = false;
				if (fits)
				{
					const sp_block_posting_t posting = { (uint32_t)doc, (uint32_t)field[ 1], (uint32_t)field[ 2], 0, nq };
					postings[ np] = posting;
				}
				uint64_t pos = 0;
				for (uint64_t i=0; i<field[ 2]; ++i, ++nq)
				{
					uint64_t gap = 0;
					if (at >= listEnd) throw std::runtime_error( beyond);
					if (!readVarint( pb->bytes, at, end, gap)) throw std::runtime_error( past);
					if (at > listEnd) throw std::runtime_error( beyond);
					if (i && !gap) throw std::runtime_error( "a position gap of 0 behind the first position of a posting");
					if (gap > 0xFFFFFFFFull || (pos += gap) > 0xFFFFFFFFull) throw std::runtime_error( "a position that leaves 32 bits");
					if (!count && room && positions && nq < npositions_cap) positions[ nq] = (uint32_t)pos;
					else if (!count) room = false;
				}
			}
			if (inList > 0xFFFFFFFFull) throw std::runtime_error( "a list of 2^32 postings or more");
			if (!count && room && list_postings && nl < nlists_cap) list_postings[ nl] = (uint32_t)inList;
			else if (!count) room = false;
		}
		*nlists = (size_t)nl; *npostings = (size_t)np; *npositions = (size_t)nq;
		if (!room) throw std::runtime_error( "room that does not suffice for the lists, the postings or the positions of the block");
		return SP_OK;
	}
	catch (const std::bad_alloc&) { return SP_ERR_NOMEM; }
	catch (const std::exception& e)
	{
		if (err && errsize) { std::strncpy( err, e.what(), errsize-1); err[ errsize-1] = 0; }
		return SP_ERR_INVALID;
	}
}
