// Stand-alone host program for a sanitizer run of the device-free twin of the dictionary order (csrc/match_dictorder.hpp) over
// the edge batches of tests/test_dictorder_abi.py and the refused arguments.  The terms and the dictionary come from their twins.
// No HIP code is linked:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Istruspattern_amd/csrc \
//       tests/micro/match_dictorder_san.cpp struspattern_amd/csrc/match_dictorder.cpp struspattern_amd/csrc/match_dict.cpp \
//       struspattern_amd/csrc/match_terms.cpp -o match_dictorder_san && ./match_dictorder_san
#include "match_dictorder.hpp"
#include "finished_batch_fixture.hpp"

// the terms of a batch and their dictionary by the twins, and the order of that
struct Order
{
	sp_match_batch_t mb;
	sp_match_text_t x;
	sp_match_values_t v;
	sp_match_terms_t t;
	sp_match_dictionary_t d;
	sp_match_dictionary_order_t o;
	char err[ 160];
	int rc;
	Order( Batch& b, uint32_t bound, uint32_t flags = SP_TERM_TEXT, void (*damage)( Order&) = 0)
	{
		mb = b.view(); x = b.textView(); v = b.valuesView();
		const sp_match_values_t* values = (flags & SP_TERM_VALUES) ? &v : 0;
		const sp_match_text_t* text = (flags & SP_TERM_TEXT) ? &x : 0;
		CHECK( sp_match_batch_terms( &mb, values, text, bound, flags, &t, err, sizeof(err)) == SP_OK);
		CHECK( sp_match_batch_dictionary( &mb, values, text, &t, &d, err, sizeof(err)) == SP_OK);
		if (damage) damage( *this);
		rc = sp_match_batch_dictionary_order( &mb, values, text, &t, &d, &o, err, sizeof(err));
	}
	~Order() { sp_match_dictionary_order_free( &o); sp_match_dictionary_free( &d); sp_match_terms_free( &t); }
	// the value of the entry at sorted position k
	std::string at( uint64_t k) const
	{
		const sp_dict_term_t& e = d.records[ o.order[ k]];
		const uint64_t r = mb.doc_result_offsets[ e.first_doc] + t.records[ t.doc_term_offsets[ e.first_doc] + e.first_term].first_result;
		const bool fromValues = t.flags == SP_TERM_VALUES || (t.flags == (SP_TERM_VALUES | SP_TERM_TEXT) && mb.result_format && mb.result_format[ r]);
		const uint64_t* offsets = fromValues ? v.result_value_offsets : x.result_text_offsets;
		const char* bytes = (const char*)(fromValues ? v.result_values : x.result_text);
		return offsets[ r+1] == offsets[ r] ? std::string() : std::string( bytes + offsets[ r], bytes + offsets[ r+1]);
	}
	uint32_t handleAt( uint64_t k) const { return d.records[ o.order[ k]].handle; }
	bool empty() const { return !o.order && !o.rank && !o.prefix_bytes && !o.handle_offsets && o.ndict == 0 && o.totals[ 0] == 0; }
	// the invariants of the header
	void invariants() const
	{
		CHECK( rc == SP_OK && o.ndict == d.ndict && o.totals[ 0] == d.ndict && o.handle_bound == d.handle_bound);
		CHECK( o.handle_offsets[ 0] == 0 && o.handle_offsets[ o.handle_bound] == o.ndict);
		for (uint64_t k=0; k<o.ndict; ++k)
		{
			CHECK( o.order[ k] < o.ndict && o.rank[ o.order[ k]] == k);
			CHECK( o.handle_offsets[ handleAt( k)] <= k && k < o.handle_offsets[ handleAt( k) + 1]);
			if (!k || handleAt( k-1) != handleAt( k)) { CHECK( o.prefix_bytes[ k] == 0); CHECK( !k || handleAt( k-1) < handleAt( k)); continue; }
			const std::string a = at( k-1), b = at( k);
			const uint32_t p = o.prefix_bytes[ k];
			CHECK( p <= a.size() && p <= b.size() && a.compare( 0, p, b, 0, p) == 0);
			CHECK( a.size() == p || (b.size() > p && (unsigned char)a[ p] < (unsigned char)b[ p]));
		}
	}
};

static void shapes()
{
	// no documents; documents without results; one entry
	{ Batch b; Order q( b, 3); q.invariants(); CHECK( q.o.ndict == 0 && q.o.handle_offsets[ 3] == 0); }
	{ Batch b; b.document(); b.document(); Order q( b, 3); q.invariants(); CHECK( q.o.ndict == 0); }
	Batch b;
	b.result( 2, "only"); b.document(); b.result( 2, "only"); b.document();
	Order q( b, 3);
	q.invariants();
	CHECK( q.o.ndict == 1 && q.o.order[ 0] == 0 && q.o.rank[ 0] == 0 && q.o.prefix_bytes[ 0] == 0 && q.o.handle_offsets[ 2] == 0 && q.o.handle_offsets[ 3] == 1);
}

static void comparatorEdges()
{
	// the empty value, prefixes, the zero paddings, unsigned bytes, the same bytes under two handles, handles without an entry,
	// values equal in their first 4, 15, 16 and 17 bytes
	const std::string zero( 1, '\0'), longer = "0123456789abcdefghij";
	Batch b;
	b.result( 2, "abc"); b.result( 2, "ab"); b.result( 2, std::string( "a") + zero + zero + zero + zero); b.result( 2, std::string( "a") + zero);
	b.result( 2, "a"); b.result( 2, std::string( "a") + zero + zero + zero); b.document();
	b.result( 2, "\x80"); b.result( 2, "\x7f"); b.result( 2, ""); b.result( 5, "abc"); b.result( 5, ""); b.result( 1, "abc"); b.document();
	for (size_t n : { 4u, 15u, 16u, 17u}) { b.result( 2, longer.substr( 0, n) + "b"); b.result( 2, longer.substr( 0, n) + "a"); b.result( 2, longer.substr( 0, n)); }
	b.document();
	Order q( b, 8);
	q.invariants();
	CHECK( q.o.ndict == 24 && q.handleAt( 0) == 1 && q.handleAt( 1) == 2 && q.at( 1).empty() && q.handleAt( 22) == 5 && q.at( 22).empty() && q.at( 23) == "abc");
	const uint64_t a = q.o.rank[ 4];		// (2, "a"): entry 4, the terms of a document ascend by handle, then by first result
	CHECK( q.at( a) == "a" && q.at( a+1).size() == 2 && q.at( a+2).size() == 4 && q.at( a+3).size() == 5 && q.at( a+4) == "ab" && q.at( a+5) == "abc");
	CHECK( q.o.prefix_bytes[ a+1] == 1 && q.o.prefix_bytes[ a+2] == 2 && q.o.prefix_bytes[ a+3] == 4 && q.o.prefix_bytes[ a+4] == 1 && q.o.prefix_bytes[ a+5] == 2);
	CHECK( q.at( 20) == "\x7f" && q.at( 21) == "\x80");
	CHECK( q.o.handle_offsets[ 3] == 22 && q.o.handle_offsets[ 4] == 22 && q.o.handle_offsets[ 5] == 22 && q.o.handle_offsets[ 6] == 24 && q.o.handle_offsets[ 8] == 24);
}

static void bothSourcesAndOrders()
{
	// values for the formatted results and text for the others in one batch
	Batch b;
	b.result( 1, "?", "usd", 1); b.result( 1, "eur", "", 0); b.result( 2, "c", "", 0); b.document();
	b.result( 2, "?", "b", 1); b.result( 2, "a", "", 0); b.result( 2, "?", "", 1); b.document();
	Order q( b, 3, SP_TERM_VALUES | SP_TERM_TEXT);
	q.invariants();
	CHECK( q.o.ndict == 6 && q.at( 0) == "eur" && q.at( 1) == "usd" && q.at( 2).empty() && q.at( 3) == "a" && q.at( 4) == "b" && q.at( 5) == "c");
	// input already ascending, and descending
	for (int descending=0; descending<2; ++descending)
	{
		Batch c;
		for (int k=0; k<300; ++k)
		{
			char value[ 16];
			std::snprintf( value, sizeof(value), "t%06d", descending ? 299 - k : k);
			c.result( 1, value); c.document();
		}
		Order r( c, 2);
		r.invariants();
		for (uint32_t k=0; k<300; ++k) CHECK( r.o.order[ k] == (descending ? 299 - k : k));
	}
}

static void refusedArguments()
{
	Batch b;
	b.result( 1, "bb"); b.result( 1, "a"); b.result( 2, "a"); b.document();
	b.result( 1, "c"); b.result( 1, "a"); b.result( 2, "d"); b.document();
	{ Order good( b, 3); good.invariants(); CHECK( good.o.ndict == 5); }
	void (*damages[])( Order&) = {
		[]( Order& q) { q.d.ndocs += 1; },
		[]( Order& q) { q.d.nterms -= 1; },
		[]( Order& q) { q.d.handle_bound += 1; },
		[]( Order& q) { q.d.flags = SP_TERM_VALUES; },
		[]( Order& q) { q.t.doc_term_offsets[ 1] = 99; },
		[]( Order& q) { q.d.records[ 1].handle = 0; },
		[]( Order& q) { q.d.records[ 1].handle = 3; },
		[]( Order& q) { q.d.records[ 1].handle = 2; },
		[]( Order& q) { q.d.records[ 0].first_doc = 2; },
		[]( Order& q) { q.d.records[ 0].first_doc = 0xFFFFFFFFu; },
		[]( Order& q) { q.d.records[ 0].first_term = 3; },
		[]( Order& q) { q.t.records[ 0].first_result = 3; },
		[]( Order& q) { q.t.records[ 0].value_bytes = 9; },
		[]( Order& q) { q.d.records[ 0].value_bytes = 9; },
		[]( Order& q) { q.d.handle_terms[ 2] = 1; },
		[]( Order& q) { q.d.records[ 4].first_doc = 0; q.d.records[ 4].first_term = 2; },
		[]( Order& q) { q.x.totals[ 0] -= 1; },
	};
	for (auto damage : damages)
	{
		Order bad( b, 3, SP_TERM_TEXT, damage);
		CHECK( bad.rc == SP_ERR_INVALID && bad.err[ 0] && bad.empty());
	}
	Order good( b, 3);
	sp_match_dictionary_order_t o;
	char err[ 8];
	CHECK( sp_match_batch_dictionary_order( &good.mb, 0, 0, &good.t, &good.d, &o, err, sizeof(err)) == SP_ERR_INVALID && std::strlen( err) == 7);	// (the message is cut to the buffer)
	CHECK( sp_match_batch_dictionary_order( 0, 0, &good.x, &good.t, &good.d, &o, 0, 0) == SP_ERR_INVALID);
	CHECK( sp_match_batch_dictionary_order( &good.mb, 0, &good.x, 0, &good.d, &o, 0, 0) == SP_ERR_INVALID);
	CHECK( sp_match_batch_dictionary_order( &good.mb, 0, &good.x, &good.t, 0, &o, 0, 0) == SP_ERR_INVALID);
}

int main()
{
	shapes();
	comparatorEdges();
	bothSourcesAndOrders();
	refusedArguments();
	std::printf( "match_dictorder_san: ok\n");
	return 0;
}
