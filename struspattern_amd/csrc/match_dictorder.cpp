// Dictionary order of a terms batch and its dictionary over host arrays (match_dictorder.hpp): host only, no device needed.
#include "match_dictorder.hpp"
#include "finished_host.hpp"
#include <algorithm>
#include <string_view>
#include <vector>

namespace spa {

void allocMatchDictionaryOrder( sp_match_dictionary_order_t* out, uint64_t ndict, uint32_t handleBound)
{
	out->ndict = (size_t)ndict; out->handle_bound = handleBound;
	out->totals[ 0] = ndict;
	out->order = filledArray<uint32_t>( ndict, 0xFF);
	out->rank = filledArray<uint32_t>( ndict, 0xFF);
	out->prefix_bytes = filledArray<uint32_t>( ndict, 0xFF);
	out->handle_offsets = filledArray<uint64_t>( (uint64_t)handleBound + 1, 0);
}

std::vector<std::string_view> dictionaryValues( const sp_match_term_t* records, uint64_t nrecords, const uint64_t* docTermOffsets, const uint64_t* docOffsets,
						uint64_t nresults, const uint32_t* resultFormat, size_t ndocs, const TermSource (&source)[ 2], uint32_t handleBound,
						uint32_t flags, const sp_dict_term_t* entries, uint64_t ndict, const uint32_t* handleTerms)
{
	if (!flags || (flags & ~(uint32_t)(SP_TERM_VALUES | SP_TERM_TEXT))) throw std::runtime_error( "unknown or no term flags");
	if (!handleBound) throw std::runtime_error( "a handle bound of 0 leaves no valid handle");
	if (!docOffsets) throw std::runtime_error( "batch without document offsets");
	if (!docTermOffsets) throw std::runtime_error( "terms without document offsets");
	if (nrecords && !records) throw std::runtime_error( "terms without records");
	if (ndict && !entries) throw std::runtime_error( "dictionary without records");
	if (!handleTerms) throw std::runtime_error( "dictionary without handle_terms");
	if (nrecords >= 0xFFFFFFFFull) throw std::runtime_error( "2^32 - 1 term records or more");
	if (ndict > nrecords) throw std::runtime_error( "a dictionary of more entries than term records");
	if (ndocs > 0xFFFFFFFFull) throw std::runtime_error( "2^32 documents or more");
	checkDocOffsets( docOffsets, ndocs, nresults);
	if (docTermOffsets[ 0] != 0) throw std::runtime_error( "term offsets do not start at the first record");
	for (size_t d=0; d<ndocs; ++d)
	{
		if (docTermOffsets[ d] > docTermOffsets[ d+1] || docTermOffsets[ d+1] > nrecords) throw std::runtime_error( "term offsets do not ascend inside the records");
	}
	if (docTermOffsets[ ndocs] != nrecords) throw std::runtime_error( "term offsets do not cover the records");
	if (flags & SP_TERM_VALUES) checkTermSource( source[ 0], "values");
	if (flags & SP_TERM_TEXT) checkTermSource( source[ 1], "text");

	// the value of every entry, and the entries of every handle
	std::vector<std::string_view> value( (size_t)ndict);
	std::vector<uint64_t> perHandle( handleBound, 0);
	for (uint64_t e=0; e<ndict; ++e)
	{
		const sp_dict_term_t& entry = entries[ e];
		if (entry.handle < 1 || entry.handle >= handleBound) throw std::runtime_error( "a dictionary entry with a handle outside the bound");
		if (entry.first_doc >= ndocs) throw std::runtime_error( "a dictionary entry whose first_doc lies outside the documents");
		const uint64_t t0 = docTermOffsets[ entry.first_doc], t1 = docTermOffsets[ (size_t)entry.first_doc+1];
		if (entry.first_term >= t1 - t0) throw std::runtime_error( "a dictionary entry whose first_term lies outside its document's records");
		const sp_match_term_t& rec = records[ t0 + entry.first_term];
		if (rec.handle != entry.handle) throw std::runtime_error( "a dictionary entry whose handle is not that of its term record");
		const uint64_t r0 = docOffsets[ entry.first_doc], r1 = docOffsets[ (size_t)entry.first_doc+1];
		if (rec.first_result >= r1 - r0) throw std::runtime_error( "a term record whose first_result lies outside its document");
		const uint64_t r = r0 + rec.first_result;
		const TermSource& S = source[ termSourceIndex( flags, resultFormat, r)];
		if (S.offsets[ r] > S.offsets[ r+1] || S.offsets[ r+1] > S.total) throw std::runtime_error( "a term value outside the bytes of its source");
		const uint64_t size = S.offsets[ r+1] - S.offsets[ r];
		if (size != rec.value_bytes) throw std::runtime_error( "a term record whose value_bytes is not the length of its value");
		if (size != entry.value_bytes) throw std::runtime_error( "a dictionary entry whose value_bytes is not the length of its value");
		value[ (size_t)e] = std::string_view( size ? S.bytes + S.offsets[ r] : "", (size_t)size);
		perHandle[ entry.handle] += 1;
	}
	for (uint32_t h=0; h<handleBound; ++h)
	{
		if (handleTerms[ h] != perHandle[ h]) throw std::runtime_error( "handle_terms that are not the number of entries of their handle");
	}
	return value;
}

void matchDictionaryOrder( const sp_match_term_t* records, uint64_t nrecords, const uint64_t* docTermOffsets, const uint64_t* docOffsets,
			   uint64_t nresults, const uint32_t* resultFormat, size_t ndocs, const TermSource (&source)[ 2], uint32_t handleBound,
			   uint32_t flags, const sp_dict_term_t* entries, uint64_t ndict, const uint32_t* handleTerms,
			   sp_match_dictionary_order_t* out)
{
	const std::vector<std::string_view> value = dictionaryValues( records, nrecords, docTermOffsets, docOffsets, nresults, resultFormat, ndocs, source,
									 handleBound, flags, entries, ndict, handleTerms);
	// (std::string_view compares as memcmp over the common length does, unsigned, then by length)
	std::vector<uint32_t> order( (size_t)ndict);
	for (uint64_t e=0; e<ndict; ++e) order[ (size_t)e] = (uint32_t)e;
	std::sort( order.begin(), order.end(), [&]( uint32_t a, uint32_t b) {
		if (entries[ a].handle != entries[ b].handle) return entries[ a].handle < entries[ b].handle;
		return value[ a] < value[ b];
	});
	for (uint64_t k=1; k<ndict; ++k)
	{
		const uint32_t a = order[ (size_t)k-1], b = order[ (size_t)k];
		if (entries[ a].handle == entries[ b].handle && value[ a] == value[ b]) throw std::runtime_error( "two dictionary entries with the same handle and bytes");
	}

	allocMatchDictionaryOrder( out, ndict, handleBound);
	for (uint64_t k=0; k<ndict; ++k)
	{
		const uint32_t e = order[ (size_t)k];
		uint32_t prefix = 0;
		if (k && entries[ order[ (size_t)k-1]].handle == entries[ e].handle)
		{
			const std::string_view& a = value[ order[ (size_t)k-1]], & b = value[ e];
			while (prefix < a.size() && prefix < b.size() && a[ prefix] == b[ prefix]) ++prefix;
		}
		out->order[ k] = e; out->rank[ e] = (uint32_t)k; out->prefix_bytes[ k] = prefix;
	}
	uint64_t sum = 0;
	for (uint32_t h=0; h<handleBound; ++h) { out->handle_offsets[ h] = sum; sum += handleTerms[ h]; }
	out->handle_offsets[ handleBound] = sum;
}

} // namespace

extern "C" void sp_match_dictionary_order_free( sp_match_dictionary_order_t* o)
{
	std::free( o->order); std::free( o->rank); std::free( o->prefix_bytes); std::free( o->handle_offsets);
	std::memset( o, 0, sizeof(*o));
}

extern "C" int sp_match_batch_dictionary_order( const sp_match_batch_t* mb, const sp_match_values_t* values, const sp_match_text_t* text,
						const sp_match_terms_t* terms, const sp_match_dictionary_t* dict,
						sp_match_dictionary_order_t* out, char* err, size_t errsize)
{
	return spa::hostProduct( out, sp_match_dictionary_order_free, err, errsize, [&]{
		if (!mb) throw std::runtime_error( "no batch");
		if (!terms) throw std::runtime_error( "no terms");
		if (!dict) throw std::runtime_error( "no dictionary");
		if (terms->ndocs != mb->ndocs || terms->nresults != mb->nresults) throw std::runtime_error( "the terms are not those of the batch: other counts of documents or results");
		if (dict->ndocs != terms->ndocs || dict->nterms != terms->nrecords) throw std::runtime_error( "the dictionary is not that of the terms: other counts of documents or term records");
		if (dict->handle_bound != terms->handle_bound || dict->flags != terms->flags) throw std::runtime_error( "the dictionary is not that of the terms: another handle bound or other flags");
		spa::TermSource source[ 2] = {};
		spa::termSources( *mb, values, text, terms->flags, source);
		spa::matchDictionaryOrder( terms->records, terms->nrecords, terms->doc_term_offsets, mb->doc_result_offsets, mb->nresults,
					   mb->result_format, mb->ndocs, source, terms->handle_bound, terms->flags, dict->records, dict->ndict,
					   dict->handle_terms, out);
	});
}
