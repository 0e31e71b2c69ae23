// Index terms of a finished batch over host arrays: the definition that the device passes (l2_terms.h) are measured
// against, and the entry point for batches already fetched to the host (sp_match_batch_terms).
// Host only: no HIP header and no HIP call in here.
//
// The rule (include/strus_pattern_amd.h "index terms"; the project's own, unpinned by a reference vector).  A term of a
// document is a pair (handle, value bytes); the value of result r is its range in one of up to two sources (bytes plus
// nresults+1 offsets parallel to the results), chosen per result.  A document gives one 24-byte record per distinct term,
// ascending by (handle, first_result), and every result the index of its term inside the document's block.  A document
// with a source status or with a handle outside 1 .. handleBound-1 has term status SP_DOC_ERR_RANGE, no records and
// result_term 0xFFFFFFFF throughout.
#ifndef SPA_MATCH_TERMS_HPP
#define SPA_MATCH_TERMS_HPP
#include "../../include/strus_pattern_amd.h"
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

namespace spa {

// one source of term values: NULL offsets = not given
struct TermSource
{
	const char* bytes;
	const uint64_t* offsets;	// nresults+1
	uint64_t total;			// bytes of `bytes`
	const int32_t* docStatus;	// ndocs, may be NULL
};

// ---- what matchTerms, matchDictionary (match_dict.hpp) and their entry points share, with internal linkage as in
// finished_host.hpp: the library exports nothing of it
namespace {

// The sources that `flags` selects, from the values and the text of the results of `mb`: source[0] the values, source[1] the
// text.  Throws std::runtime_error for a selected one that is absent, has no results family or other counts than the batch.
void termSources( const sp_match_batch_t& mb, const sp_match_values_t* values, const sp_match_text_t* text, uint32_t flags, TermSource (&source)[ 2])
{
	if (flags & SP_TERM_VALUES)
	{
		if (!values || !values->result_value_offsets) throw std::runtime_error( "no values of the results of the batch");
		if (values->ndocs != mb.ndocs || values->nresults != mb.nresults) throw std::runtime_error( "the values are not those of the batch: other counts of documents or results");
		const TermSource S = { values->result_values, values->result_value_offsets, values->totals[ 0], values->doc_value_status };
		source[ 0] = S;
	}
	if (flags & SP_TERM_TEXT)
	{
		if (!text || !text->result_text_offsets) throw std::runtime_error( "no text of the results of the batch");
		if (text->ndocs != mb.ndocs || text->nresults != mb.nresults) throw std::runtime_error( "the text is not that of the batch: other counts of documents or results");
		const TermSource S = { text->result_text, text->result_text_offsets, text->totals[ 0], text->doc_text_status };
		source[ 1] = S;
	}
}

// which source holds the value of result r: the values unless the flags say text; with both flags the text of a result
// without a format (resultFormat may be NULL: no result has one)
inline int termSourceIndex( uint32_t flags, const uint32_t* resultFormat, uint64_t r)
{
	if (flags == (SP_TERM_VALUES | SP_TERM_TEXT)) return (resultFormat && resultFormat[ r] != 0) ? 0 : 1;
	return (flags & SP_TERM_VALUES) ? 0 : 1;
}

// a selected source is there (matchDictionary, which reads the ranges of the first results only and checks each of them) ...
void checkTermSource( const TermSource& S, const char* name)
{
	if (!S.offsets) throw std::runtime_error( std::string( "no ") + name + " of the results of the batch");
	if (S.total && !S.bytes) throw std::runtime_error( std::string( name) + " without bytes");
}

// ... and its offsets start at 0, ascend inside its bytes and cover them (matchTerms, which reads every range)
void checkTermSource( const TermSource& S, uint64_t nresults, const char* name)
{
	checkTermSource( S, name);
	if (S.offsets[ 0] != 0) throw std::runtime_error( std::string( "offsets of the ") + name + " do not start at the first byte");
	for (uint64_t r=0; r<nresults; ++r)
	{
		if (S.offsets[ r] > S.offsets[ r+1] || S.offsets[ r+1] > S.total) throw std::runtime_error( std::string( "offsets of the ") + name + " do not ascend inside its bytes");
	}
	if (S.offsets[ nresults] != S.total) throw std::runtime_error( std::string( "offsets of the ") + name + " do not cover its bytes");
}

} // namespace

// the host arrays of the terms of `ndocs` documents and `nresults` results, everything but the records: offsets and status
// zeroed, result_term all 0xFFFFFFFF (sp_match_terms_free)
void allocMatchTerms( sp_match_terms_t* out, size_t ndocs, uint64_t nresults, uint32_t handleBound, uint32_t flags);
// the records, once their number is known
void allocMatchTermRecords( sp_match_terms_t* out, uint64_t nrecords);

// the terms of a batch on the host: source[0] the values, source[1] the text; resultFormat may be NULL; throws
// std::runtime_error for arguments that make no batch
void matchTerms( const sp_result_t* results, uint64_t nresults, const uint64_t* docOffsets, const int32_t* docStatus,
		 const uint32_t* resultFormat, size_t ndocs, const TermSource (&source)[ 2], uint32_t handleBound, uint32_t flags,
		 sp_match_terms_t* out);

} // namespace
#endif
