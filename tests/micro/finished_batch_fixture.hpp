// The fixture of the stand-alone sanitizer programs over the twins that read a finished batch together with the text and the
// values of its results (match_terms_san.cpp, match_dict_san.cpp).
#ifndef SPA_FINISHED_BATCH_FIXTURE_HPP
#define SPA_FINISHED_BATCH_FIXTURE_HPP
#include "match_terms.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK( COND) do { if (!(COND)) { std::fprintf( stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #COND); std::exit( 1); } } while (0)

// A finished batch with the text and the values of its results.  Every array is exactly as long as what it holds (the bytes
// live in heap blocks of their exact size), so a read past it is the sanitizer's to report.
struct Batch
{
	std::vector<sp_result_t> results;
	std::vector<uint64_t> offsets = {0};
	std::vector<int32_t> status, textStatus, valueStatus;
	std::vector<uint32_t> format;
	std::vector<uint64_t> textOffsets = {0}, valueOffsets = {0};
	std::string text, values;
	std::vector<char> exactText, exactValues;

	void document() { offsets.push_back( results.size()); status.push_back( 0); textStatus.push_back( 0); valueStatus.push_back( 0); }
	// a result at a position of its own ...
	void result( uint32_t handle, const std::string& txt, const std::string& value = "", uint32_t fmt = 0)
	{
		sp_result_t r = {};
		r.handle = handle; r.ordpos = (uint32_t)results.size(); r.ordend = r.ordpos + 1;
		results.push_back( r); format.push_back( fmt);
		text += txt; textOffsets.push_back( text.size());
		values += value; valueOffsets.push_back( values.size());
	}
	// ... or at a given one, with the same bytes as its text and as its value
	void result( uint32_t handle, uint32_t ordpos, uint32_t ordend, const std::string& value, uint32_t fmt = 0)
	{
		result( handle, value, value, fmt);
		results.back().ordpos = ordpos; results.back().ordend = ordend;
	}
	sp_match_batch_t view()
	{
		sp_match_batch_t mb = {};
		mb.ndocs = status.size(); mb.nresults = results.size();
		mb.results = results.empty() ? 0 : results.data(); mb.doc_result_offsets = offsets.data(); mb.doc_status = status.empty() ? 0 : status.data();
		mb.result_format = format.empty() ? 0 : format.data();
		return mb;
	}
	sp_match_text_t textView()
	{
		exactText.assign( text.begin(), text.end());
		sp_match_text_t t = {};
		t.ndocs = status.size(); t.nresults = results.size();
		t.result_text = exactText.empty() ? 0 : exactText.data(); t.result_text_offsets = textOffsets.data();
		t.doc_text_status = textStatus.empty() ? 0 : textStatus.data(); t.totals[ 0] = exactText.size();
		return t;
	}
	sp_match_values_t valuesView()
	{
		exactValues.assign( values.begin(), values.end());
		sp_match_values_t v = {};
		v.ndocs = status.size(); v.nresults = results.size();
		v.result_values = exactValues.empty() ? 0 : exactValues.data(); v.result_value_offsets = valueOffsets.data();
		v.doc_value_status = valueStatus.empty() ? 0 : valueStatus.data(); v.totals[ 0] = exactValues.size();
		return v;
	}
};

#endif
