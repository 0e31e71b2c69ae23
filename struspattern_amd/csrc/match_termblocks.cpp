// Term blocks of a dictionary and its order over host arrays, and their reader (match_termblocks.hpp): host only, no device needed.
#include "match_termblocks.hpp"
#include "term_block_code.h"
#include "finished_host.hpp"
#include <atomic>
#include <functional>
#include <unordered_set>

namespace spa {

namespace {
std::atomic<uint32_t>& blockEntriesSwitch() { static std::atomic<uint32_t> n( TERM_BLOCK_ENTRIES); return n; }
}

uint32_t termBlockEntries() { return blockEntriesSwitch().load( std::memory_order_relaxed); }

void allocMatchTermBlocks( sp_match_term_blocks_t* out, uint64_t ndict, uint64_t nblocks, uint32_t blockEntries)
{
	out->ndict = (size_t)ndict; out->nblocks = (size_t)nblocks; out->block_entries = blockEntries;
	out->totals[ 0] = nblocks; out->totals[ 2] = blockEntries;
	out->block_offsets = filledArray<uint64_t>( nblocks + 1, 0);
	out->block_handles = filledArray<uint32_t>( nblocks, 0xFF);
}

void allocMatchTermBlockBytes( sp_match_term_blocks_t* out, uint64_t nbytes)
{
	out->nbytes = (size_t)nbytes; out->totals[ 1] = nbytes;
	out->bytes = filledArray<uint8_t>( nbytes + 1, 0);
}

void matchTermBlocks( const sp_dict_term_t* entries, uint64_t ndict, const std::vector<std::string_view>& value, const uint32_t* order,
		      const uint32_t* prefixBytes, uint32_t blockEntries, sp_match_term_blocks_t* out)
{
	if (!termBlockEntriesValid( blockEntries)) throw std::runtime_error( "a block size that is not 1, 2, 4, 8, 16, 32 or 64");
	if (ndict && (!order || !prefixBytes)) throw std::runtime_error( "order without its arrays");
	// the order is one of this dictionary
	std::vector<bool> seen( (size_t)ndict, false);
	std::unordered_set<std::string_view> ofHandle;		// (the values of the handle that the walk is in)
	for (uint64_t k=0; k<ndict; ++k)
	{
		const uint32_t e = order[ k];
		if (e >= ndict || seen[ e]) throw std::runtime_error( "an order that is not a permutation of the entries");
		seen[ e] = true;
		const bool first = !k || entries[ order[ k-1]].handle != entries[ e].handle;
		if (k && entries[ order[ k-1]].handle > entries[ e].handle) throw std::runtime_error( "an order along which the handles descend");
		if (first) ofHandle.clear();
		if (!ofHandle.insert( value[ e]).second) throw std::runtime_error( "two dictionary entries with the same handle and bytes");
		const std::string_view& b = value[ e];
		uint32_t same = 0;
		if (!first)
		{
			const std::string_view& a = value[ order[ k-1]];
			if (prefixBytes[ k] > a.size() || prefixBytes[ k] > b.size()) throw std::runtime_error( "a prefix_bytes above the length of a neighbour's value");
			while (same < a.size() && same < b.size() && a[ same] == b[ same]) ++same;
		}
		if (prefixBytes[ k] != same) throw std::runtime_error( "a prefix_bytes that is not what the two values share");
	}

	const uint64_t nblocks = (ndict + blockEntries - 1) / blockEntries;
	allocMatchTermBlocks( out, ndict, nblocks, blockEntries);
	// the sizes, the offsets, the codes
	std::vector<TermBlockEntry> code( (size_t)ndict);
	uint64_t nbytes = 0, valueBytes = 0;
	for (uint64_t k=0; k<ndict; ++k)
	{
		const sp_dict_term_t& entry = entries[ order[ k]];
		const bool head = k % blockEntries == 0;
		if (head) { out->block_offsets[ k / blockEntries] = nbytes; out->block_handles[ k / blockEntries] = entry.handle; }
		code[ k] = termBlockEntry( head, entry.handle, k ? entries[ order[ k-1]].handle : 0, prefixBytes[ k], (uint32_t)value[ order[ k]].size(),
					   entry.doc_freq, entry.count);
		nbytes += termBlockCodeBytes( code[ k]);
		valueBytes += value[ order[ k]].size();
	}
	out->block_offsets[ nblocks] = nbytes;
	out->totals[ 3] = valueBytes;
	allocMatchTermBlockBytes( out, nbytes);
	uint64_t at = 0;
	for (uint64_t k=0; k<ndict; ++k)
	{
		const std::string_view& v = value[ order[ k]];
		at += writeTermBlockHeader( out->bytes + at, code[ k]);
		if (code[ k].suffix) std::memcpy( out->bytes + at, v.data() + code[ k].shared, code[ k].suffix);
		at += code[ k].suffix;
	}
	if (at != nbytes) throw std::logic_error( "the codes are not as long as they were counted");
}

} // namespace

extern "C" uint32_t sp_matcher_term_block_entries(void) { return spa::termBlockEntries(); }

extern "C" void sp_test_term_block_entries( unsigned n)
{
	spa::blockEntriesSwitch().store( spa::termBlockEntriesValid( n) ? n : (uint32_t)spa::TERM_BLOCK_ENTRIES, std::memory_order_relaxed);
}

extern "C" void sp_match_term_blocks_free( sp_match_term_blocks_t* tb)
{
	std::free( tb->bytes); std::free( tb->block_offsets); std::free( tb->block_handles);
	std::memset( tb, 0, sizeof(*tb));
}

extern "C" int sp_match_batch_term_blocks( const sp_match_batch_t* mb, const sp_match_values_t* values, const sp_match_text_t* text,
					   const sp_match_terms_t* terms, const sp_match_dictionary_t* dict, const sp_match_dictionary_order_t* order,
					   sp_match_term_blocks_t* out, char* err, size_t errsize)
{
	return spa::hostProduct( out, sp_match_term_blocks_free, err, errsize, [&]{
		if (!mb) throw std::runtime_error( "no batch");
		if (!terms) throw std::runtime_error( "no terms");
		if (!dict) throw std::runtime_error( "no dictionary");
		if (!order) throw std::runtime_error( "no order");
		if (terms->ndocs != mb->ndocs || terms->nresults != mb->nresults) throw std::runtime_error( "the terms are not those of the batch: other counts of documents or results");
		if (dict->ndocs != terms->ndocs || dict->nterms != terms->nrecords) throw std::runtime_error( "the dictionary is not that of the terms: other counts of documents or term records");
		if (dict->handle_bound != terms->handle_bound || dict->flags != terms->flags) throw std::runtime_error( "the dictionary is not that of the terms: another handle bound or other flags");
		if (order->ndict != dict->ndict || order->handle_bound != dict->handle_bound) throw std::runtime_error( "the order is not that of the dictionary: another number of entries or another handle bound");
		spa::TermSource source[ 2] = {};
		spa::termSources( *mb, values, text, terms->flags, source);
		const std::vector<std::string_view> value = spa::dictionaryValues( terms->records, terms->nrecords, terms->doc_term_offsets, mb->doc_result_offsets,
			mb->nresults, mb->result_format, mb->ndocs, source, terms->handle_bound, terms->flags, dict->records, dict->ndict, dict->handle_terms);
		spa::matchTermBlocks( dict->records, dict->ndict, value, order->order, order->prefix_bytes, spa::termBlockEntries(), out);
	});
}

extern "C" int sp_match_term_blocks_decode_block( const sp_match_term_blocks_t* tb, size_t j, sp_term_block_entry_t* entries, size_t nentries_cap,
						  uint8_t* values, size_t values_cap, size_t* nentries, size_t* nvalues, char* err, size_t errsize)
{
	using namespace spa;
	if (nentries) *nentries = 0;
	if (nvalues) *nvalues = 0;
	if (err && errsize) err[ 0] = 0;
	try
	{
		if (!tb || !nentries || !nvalues) throw std::runtime_error( "no term blocks, or nowhere to count to");
		if (j >= tb->nblocks || !tb->block_offsets || !tb->block_handles) throw std::runtime_error( "no such block");
		if (!termBlockEntriesValid( tb->block_entries)) throw std::runtime_error( "a block size that is not 1, 2, 4, 8, 16, 32 or 64");
		uint64_t at = tb->block_offsets[ j];
		const uint64_t end = tb->block_offsets[ j+1];
		if (at > end || end > tb->nbytes || (end && !tb->bytes)) throw std::runtime_error( "block offsets that descend or leave the bytes");
		if (at == end) throw std::runtime_error( "an empty block");
		const bool count = !entries && !values;
		// the value before, as it is rebuilt: only its bytes up to `shared` are read again
		std::string before;
		uint64_t handle = tb->block_handles[ j], n = 0, nv = 0;
		bool room = true;
		for (; at < end; ++n)
		{
			if (n >= tb->block_entries) throw std::runtime_error( "a block of more codes than a block holds");
			uint64_t field[ 5];
			for (int i=0; i<5; ++i)
			{
				if (!readVarint( tb->bytes, at, end, field[ i])) throw std::runtime_error( "a varint that runs past the block or is longer than ten bytes");
			}
			const uint64_t hdelta = field[ 0], shared = field[ 1], suffix = field[ 2];
			if (n == 0 && (hdelta || shared)) throw std::runtime_error( "a head that does not carry its handle and its value in full");
			if (shared > before.size()) throw std::runtime_error( "a shared prefix above the length of the value before");
			if (suffix > end - at) throw std::runtime_error( "a suffix that runs past the block");
			handle += hdelta;
			if (handle > 0xFFFFFFFFull || shared + suffix > 0xFFFFFFFFull || field[ 3] > 0xFFFFFFFFull) throw std::runtime_error( "a handle, a value length or a doc_freq that leaves 32 bits");
			before.resize( (size_t)shared);
			before.append( (const char*)tb->bytes + at, (size_t)suffix);
			at += suffix;
			if (!count && (n >= nentries_cap || !entries || before.size() > values_cap - (nv < values_cap ? nv : values_cap) || (before.size() && !values))) room = false;
			if (!count && room)
			{
				const sp_term_block_entry_t entry = { (uint32_t)handle, (uint32_t)before.size(), nv, (uint32_t)field[ 3], 0, field[ 4] };
				entries[ n] = entry;
				if (!before.empty()) std::memcpy( values + nv, before.data(), before.size());
			}
			nv += before.size();
		}
		*nentries = (size_t)n; *nvalues = (size_t)nv;
		if (!room) throw std::runtime_error( "room that does not suffice for the entries or the values of the block");
		return SP_OK;
	}
	catch (const std::bad_alloc&) { return SP_ERR_NOMEM; }
	catch (const std::exception& e)
	{
		if (err && errsize) { std::strncpy( err, e.what(), errsize-1); err[ errsize-1] = 0; }
		return SP_ERR_INVALID;
	}
}
