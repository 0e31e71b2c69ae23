// Stand-alone host program for a sanitizer run of the device-free twin of the value passes (csrc/result_values.hpp) over the
// malformed batches of tests/test_result_values_abi.py: an nsub beyond its list, a format handle beyond the table, nesting at
// and beyond the limit, invalid spans used and unused, a result whose items lie outside its document.  No HIP code is linked:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Istruspattern_amd/csrc \
//       tests/micro/result_values_host_check.cpp struspattern_amd/csrc/result_values.cpp struspattern_amd/csrc/span_text.cpp \
//       -o result_values_host_check && ./result_values_host_check
#include "result_values.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#define CHECK( COND) do { if (!(COND)) { std::fprintf( stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #COND); std::exit( 1); } } while (0)

using namespace spa;

// A finished batch.  Every array is exactly as long as what it holds, so a read past it is the sanitizer's to report.
struct Batch
{
	std::vector<sp_result_t> results;
	std::vector<sp_result_item_t> items;
	std::vector<uint32_t> resultFormat, itemFormat;
	std::vector<uint64_t> offsets = {0};

	void document() { offsets.push_back( results.size()); }
	// a result over the `count` items that follow
	void result( uint32_t fmt, uint32_t count)
	{
		sp_result_t r = {};
		r.handle = 1; r.item_begin = (uint32_t)items.size(); r.item_count = count;
		results.push_back( r); resultFormat.push_back( fmt);
	}
	void item( uint32_t variable, uint32_t fmt, uint32_t nsub, uint32_t origpos, uint32_t origend)
	{
		sp_result_item_t it = {};
		it.variable = variable; it.origpos = origpos; it.origend = origend;
		items.push_back( it); itemFormat.push_back( fmt); itemFormat.push_back( nsub);
	}
	sp_match_batch_t view()
	{
		sp_match_batch_t mb = {};
		mb.ndocs = offsets.size() - 1; mb.nresults = results.size(); mb.nitems = items.size();
		mb.results = results.empty() ? 0 : results.data(); mb.items = items.empty() ? 0 : items.data();
		mb.doc_result_offsets = offsets.data();
		mb.result_format = resultFormat.empty() ? 0 : resultFormat.data(); mb.item_format = itemFormat.empty() ? 0 : itemFormat.data();
		return mb;
	}
};

static const char TEXT[] = "0123456789abcdefghijABCDEFGHIJ";		// every document is one segment of 10 bytes
static const uint64_t SEGS[] = {0, 10, 20, 30};

struct Values
{
	sp_match_values_t v;
	Values( const FormatTable& table, Batch& b, uint32_t flags)
	{
		std::memset( &v, 0, sizeof(v));
		const sp_match_batch_t mb = b.view();
		CHECK( mb.ndocs <= 3);
		const TextSource S = { TEXT, SEGS[ mb.ndocs], SEGS, mb.ndocs, 0 };
		matchBatchValues( table, mb, S, flags, &v);
	}
	~Values() { sp_match_values_free( &v); }
	std::string result( size_t i) const { return std::string( v.result_values + v.result_value_offsets[ i], v.result_values + v.result_value_offsets[ i+1]); }
	std::string item( size_t i) const { return std::string( v.item_values + v.item_value_offsets[ i], v.item_values + v.item_value_offsets[ i+1]); }
};

int main()
{
	// formats: 1 "<{a}>"  2 "{a|,}+{b}"  3 "x"  4 "{v}"  5 "[{nosuch}]"
	const std::vector<std::string> formats = { "<{a}>", "{a|,}+{b}", "x", "{v}", "[{nosuch}]" };
	const std::map<std::string, uint32_t> variables = { {"a", 1}, {"b", 2}, {"v", 3} };
	const FormatTable table = buildFormatTable( (uint32_t)formats.size(),
		[&]( uint32_t f) { return formats[ f-1].c_str(); },
		[&]( const std::string& name) { auto it = variables.find( name); return it == variables.end() ? 0u : it->second; });
	CHECK( table.error.empty() && table.count == 5);
	const uint32_t BOTH = SP_VALUE_RESULTS | SP_VALUE_ITEMS;

	// the good neighbours around the document under test
	auto good = []( Batch& b) { b.result( 2, 3); b.item( 1, 0, 0, 0, 2); b.item( 2, 0, 0, 2, 3); b.item( 1, 0, 0, 4, 6); b.document(); };
	{
		Batch b; good( b);
		Values V( table, b, BOTH);
		CHECK( V.v.doc_value_status[ 0] == 0 && V.result( 0) == "01,45+2" && V.v.totals[ 1] == 0);
	}
	// an nsub that runs beyond its list, a format handle of count + 1: the document fails, its neighbours are intact
	for (int what=0; what<2; ++what)
	{
		Batch b; good( b);
		b.result( 1, 2); b.item( 1, what ? 6 : 3, what ? 1 : 2, 0, 1); b.item( 1, 0, 0, 1, 2); b.document();
		good( b);
		Values V( table, b, BOTH);
		CHECK( V.v.doc_value_status[ 0] == 0 && V.v.doc_value_status[ 1] == SP_DOC_ERR_RANGE && V.v.doc_value_status[ 2] == 0);
		CHECK( V.result( 0) == "01,45+2" && V.result( 1) == "" && V.result( 2) == "AB,EF+C");
		for (size_t i=3; i<5; ++i) CHECK( V.item( i) == "");
	}
	// nesting: a chain of "{v}" formats around one "x"; `depth` formats inside each other
	for (uint32_t depth=VALUE_MAX_DEPTH-1; depth<=VALUE_MAX_DEPTH+1; ++depth)
	{
		Batch b; good( b);
		b.result( 4, depth - 1);
		for (uint32_t k=1; k<depth; ++k) b.item( 3, k + 1 < depth ? 4 : 3, depth - 1 - k, 0, 1);
		b.document();
		good( b);
		Values V( table, b, BOTH);
		const bool ok = depth <= VALUE_MAX_DEPTH;
		CHECK( V.v.doc_value_status[ 1] == (ok ? 0 : SP_DOC_ERR_RANGE) && V.v.doc_value_status[ 0] == 0 && V.v.doc_value_status[ 2] == 0);
		CHECK( V.result( 1) == (ok ? "x" : "") && V.result( 0) == "01,45+2" && V.result( 2) == "AB,EF+C");
		CHECK( V.item( 3) == (ok ? "x" : ""));
		// the results alone fail at the same depth; the items alone start one level further in
		Values R( table, b, SP_VALUE_RESULTS);
		CHECK( R.v.doc_value_status[ 1] == (ok ? 0 : SP_DOC_ERR_RANGE) && !R.v.item_value_offsets);
		Values I( table, b, SP_VALUE_ITEMS);
		CHECK( I.v.doc_value_status[ 1] == 0 && I.item( 3) == "x" && !I.v.result_value_offsets);
	}
	// an invalid span that no format part uses does not fail the document; one that a part uses does
	for (int used=0; used<2; ++used)
	{
		Batch b; good( b);
		b.result( 1, 2); b.item( used ? 1 : 2, 0, 0, 5, 11); b.item( 1, 0, 0, 1, 3); b.document();
		Values V( table, b, BOTH);
		CHECK( V.v.doc_value_status[ 0] == 0 && V.v.doc_value_status[ 1] == (used ? SP_DOC_ERR_RANGE : 0));
		CHECK( V.result( 1) == (used ? "" : "<bc>"));
	}
	// a variable that the rule set does not have matches nothing; a result whose items lie outside its document fails
	{
		Batch b;
		b.result( 5, 1); b.item( 1, 0, 0, 0, 1); b.document();
		b.result( 1, 1); b.item( 1, 0, 0, 0, 1); b.results.back().item_begin = 0; b.document();
		Values V( table, b, BOTH);
		CHECK( V.result( 0) == "[]" && V.v.doc_value_status[ 0] == 0 && V.v.doc_value_status[ 1] == SP_DOC_ERR_RANGE);
	}
	// a format string that does not parse: the values call is refused, the table says why
	{
		const std::vector<std::string> bad = { "ok", "{open" };
		const FormatTable t2 = buildFormatTable( 2, [&]( uint32_t f) { return bad[ f-1].c_str(); }, []( const std::string&) { return 0u; });
		CHECK( !t2.error.empty() && t2.error.find( "{open") != std::string::npos);
		Batch b; good( b);
		bool thrown = false;
		sp_match_values_t v;
		std::memset( &v, 0, sizeof(v));
		const sp_match_batch_t mb = b.view();
		const TextSource S = { TEXT, 10, SEGS, 1, 0 };
		try { matchBatchValues( t2, mb, S, BOTH, &v); } catch (const std::runtime_error&) { thrown = true; }
		sp_match_values_free( &v);
		CHECK( thrown);
	}
	std::printf( "result_values_host_check: ok\n");
	return 0;
}
