// Batch postings of a terms batch and its dictionary over host arrays (match_postings.hpp): host only, no device needed.
#include "match_postings.hpp"
#include "finished_host.hpp"
#include <vector>

namespace spa {

void allocMatchPostings( sp_match_postings_t* out, size_t ndocs, uint64_t nterms, uint64_t ndict)
{
	out->ndocs = ndocs; out->nterms = (size_t)nterms; out->ndict = (size_t)ndict;
	out->totals[ 0] = nterms;
	out->postings = filledArray<sp_posting_t>( nterms, 0);
	out->entry_offsets = filledArray<uint64_t>( ndict + 1, 0);
	out->record_posting = filledArray<uint32_t>( nterms, 0xFF);
}

void matchPostings( const sp_match_term_t* records, uint64_t nrecords, const uint64_t* docTermOffsets, size_t ndocs,
		    const sp_dict_term_t* entries, uint64_t ndict, const uint32_t* termDict, sp_match_postings_t* out)
{
	if (!docTermOffsets) throw std::runtime_error( "terms without document offsets");
	if (nrecords && !records) throw std::runtime_error( "terms without records");
	if (nrecords && !termDict) throw std::runtime_error( "dictionary without term_dict");
	if (ndict && !entries) throw std::runtime_error( "dictionary without records");
	if (nrecords >= 0xFFFFFFFFull) throw std::runtime_error( "2^32 - 1 term records or more");
	if (ndocs > 0xFFFFFFFFull) throw std::runtime_error( "2^32 documents or more");
	if (docTermOffsets[ 0] != 0) throw std::runtime_error( "term offsets do not start at the first record");
	for (size_t d=0; d<ndocs; ++d)
	{
		if (docTermOffsets[ d] > docTermOffsets[ d+1] || docTermOffsets[ d+1] > nrecords) throw std::runtime_error( "term offsets do not ascend inside the records");
	}
	if (docTermOffsets[ ndocs] != nrecords) throw std::runtime_error( "term offsets do not cover the records");

	// count: the records of every entry are its doc_freq
	std::vector<uint64_t> next( (size_t)ndict + 1, 0);
	for (uint64_t i=0; i<nrecords; ++i)
	{
		if (termDict[ i] >= ndict) throw std::runtime_error( "a term_dict entry outside the dictionary");
		next[ termDict[ i]] += 1;
	}
	for (uint64_t e=0; e<ndict; ++e)
	{
		if (entries[ e].doc_freq != next[ e]) throw std::runtime_error( "a doc_freq that is not the number of records of its entry");
	}
	allocMatchPostings( out, ndocs, nrecords, ndict);
	// offsets, then place in record order: every list ascends by record, that is by document
	uint64_t sum = 0;
	for (uint64_t e=0; e<ndict; ++e) { out->entry_offsets[ e] = sum; sum += next[ e]; next[ e] = out->entry_offsets[ e]; }
	out->entry_offsets[ ndict] = sum;
	for (size_t d=0; d<ndocs; ++d)
	{
		for (uint64_t i=docTermOffsets[ d]; i<docTermOffsets[ d+1]; ++i)
		{
			const uint64_t p = next[ termDict[ i]]++;
			const sp_posting_t posting = { (uint32_t)d, (uint32_t)(i - docTermOffsets[ d]), records[ i].count, records[ i].first_ordpos };
			out->postings[ p] = posting;
			out->record_posting[ i] = (uint32_t)p;
		}
	}
}

} // namespace

extern "C" void sp_match_postings_free( sp_match_postings_t* p)
{
	std::free( p->postings); std::free( p->entry_offsets); std::free( p->record_posting);
	std::memset( p, 0, sizeof(*p));
}

extern "C" int sp_match_batch_postings( const sp_match_terms_t* terms, const sp_match_dictionary_t* dict, sp_match_postings_t* out,
					char* err, size_t errsize)
{
	return spa::hostProduct( out, sp_match_postings_free, err, errsize, [&]{
		if (!terms) throw std::runtime_error( "no terms");
		if (!dict) throw std::runtime_error( "no dictionary");
		if (terms->ndocs != dict->ndocs || terms->nrecords != dict->nterms) throw std::runtime_error( "the dictionary is not that of the terms: other counts of documents or term records");
		spa::matchPostings( terms->records, terms->nrecords, terms->doc_term_offsets, terms->ndocs, dict->records, dict->ndict, dict->term_dict, out);
	});
}
