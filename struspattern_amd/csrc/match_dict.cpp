// Batch dictionary of a terms batch over host arrays (match_dict.hpp): host only, no device needed.
#include "match_dict.hpp"
#include "finished_host.hpp"
#include <string_view>
#include <unordered_map>
#include <vector>

namespace spa {

namespace {

// a dictionary term: the bytes are those of a source, which outlives the map
struct Key
{
	uint32_t handle;
	std::string_view bytes;
	bool operator==( const Key& o) const { return handle == o.handle && bytes == o.bytes; }
};
struct KeyHash
{
	size_t operator()( const Key& k) const { return std::hash<std::string_view>()( k.bytes) * 31u + k.handle; }
};

} // namespace

void allocMatchDictionary( sp_match_dictionary_t* out, size_t ndocs, uint64_t nterms, uint32_t handleBound, uint32_t flags)
{
	out->ndocs = ndocs; out->nterms = (size_t)nterms; out->ndict = 0; out->handle_bound = handleBound; out->flags = flags;
	out->totals[ 0] = 0;
	out->doc_dict_offsets = filledArray<uint64_t>( ndocs + 1, 0);
	out->handle_terms = filledArray<uint32_t>( handleBound, 0);
	out->term_dict = filledArray<uint32_t>( nterms, 0xFF);
}

void allocMatchDictionaryRecords( sp_match_dictionary_t* out, uint64_t ndict)
{
	out->records = filledArray<sp_dict_term_t>( ndict, 0);
	out->ndict = (size_t)ndict; out->totals[ 0] = ndict;
}

void matchDictionary( const sp_match_term_t* records, uint64_t nrecords, const uint64_t* docTermOffsets, const uint64_t* docOffsets,
		      uint64_t nresults, const uint32_t* resultFormat, size_t ndocs, const TermSource (&source)[ 2], uint32_t handleBound,
		      uint32_t flags, sp_match_dictionary_t* out)
{
	if (!flags || (flags & ~(uint32_t)(SP_TERM_VALUES | SP_TERM_TEXT))) throw std::runtime_error( "unknown or no term flags");
	if (!handleBound) throw std::runtime_error( "a handle bound of 0 leaves no valid handle");
	if (!docOffsets) throw std::runtime_error( "batch without document offsets");
	if (!docTermOffsets) throw std::runtime_error( "terms without document offsets");
	if (nrecords && !records) throw std::runtime_error( "terms without records");
	if (nrecords >= 0xFFFFFFFFull) throw std::runtime_error( "2^32 - 1 term records or more");
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

	allocMatchDictionary( out, ndocs, nrecords, handleBound, flags);
	std::vector<sp_dict_term_t> entries;
	std::unordered_map<Key, uint32_t, KeyHash> index;
	for (size_t d=0; d<ndocs; ++d)
	{
		out->doc_dict_offsets[ d] = entries.size();
		const uint64_t r0 = docOffsets[ d], r1 = docOffsets[ d+1];
		for (uint64_t i=docTermOffsets[ d]; i<docTermOffsets[ d+1]; ++i)
		{
			const sp_match_term_t& rec = records[ i];
			if (rec.handle < 1 || rec.handle >= handleBound) throw std::runtime_error( "a term record with a handle outside the bound");
			if (rec.first_result >= r1 - r0) throw std::runtime_error( "a term record whose first_result lies outside its document");
			const uint64_t r = r0 + rec.first_result;
			const TermSource& S = source[ termSourceIndex( flags, resultFormat, r)];
			if (S.offsets[ r] > S.offsets[ r+1] || S.offsets[ r+1] > S.total) throw std::runtime_error( "a term value outside the bytes of its source");
			const uint64_t size = S.offsets[ r+1] - S.offsets[ r];
			if (size != rec.value_bytes) throw std::runtime_error( "a term record whose value_bytes is not the length of its value");
			const Key key = { rec.handle, std::string_view( size ? S.bytes + S.offsets[ r] : "", (size_t)size) };
			const auto ins = index.emplace( key, (uint32_t)entries.size());
			if (ins.second)
			{
				const sp_dict_term_t e = { rec.handle, rec.value_bytes, (uint32_t)d, (uint32_t)(i - docTermOffsets[ d]), 0, 0, 0 };
				entries.push_back( e);
				out->handle_terms[ rec.handle] += 1;
			}
			sp_dict_term_t& e = entries[ ins.first->second];
			e.doc_freq += 1;
			if (rec.count > e.max_count) e.max_count = rec.count;
			e.count += rec.count;
			out->term_dict[ i] = ins.first->second;
		}
	}
	out->doc_dict_offsets[ ndocs] = entries.size();
	allocMatchDictionaryRecords( out, entries.size());
	if (!entries.empty()) std::memcpy( out->records, entries.data(), entries.size() * sizeof(sp_dict_term_t));
}

} // namespace

extern "C" void sp_match_dictionary_free( sp_match_dictionary_t* d)
{
	std::free( d->records); std::free( d->term_dict); std::free( d->doc_dict_offsets); std::free( d->handle_terms);
	std::memset( d, 0, sizeof(*d));
}

extern "C" int sp_match_batch_dictionary( const sp_match_batch_t* mb, const sp_match_values_t* values, const sp_match_text_t* text,
					  const sp_match_terms_t* terms, sp_match_dictionary_t* out, char* err, size_t errsize)
{
	return spa::hostProduct( out, sp_match_dictionary_free, err, errsize, [&]{
		if (!mb) throw std::runtime_error( "no batch");
		if (!terms) throw std::runtime_error( "no terms");
		if (terms->ndocs != mb->ndocs || terms->nresults != mb->nresults) throw std::runtime_error( "the terms are not those of the batch: other counts of documents or results");
		spa::TermSource source[ 2] = {};
		spa::termSources( *mb, values, text, terms->flags, source);
		spa::matchDictionary( terms->records, terms->nrecords, terms->doc_term_offsets, mb->doc_result_offsets, mb->nresults,
				      mb->result_format, mb->ndocs, source, terms->handle_bound, terms->flags, out);
	});
}
