// Stand-alone host program for a sanitizer run of the device-free twin of the term passes (csrc/match_terms.hpp) over the edge
// batches of tests/test_terms_abi.py, the invalid handles and the refused arguments included.  No HIP code is linked:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Istruspattern_amd/csrc \
//       tests/micro/match_terms_san.cpp struspattern_amd/csrc/match_terms.cpp -o match_terms_san && ./match_terms_san
// (the batch is that of finished_batch_fixture.hpp: one string per result serves as its text and as its value)
#include "finished_batch_fixture.hpp"

struct Terms
{
	sp_match_terms_t t;
	char err[ 128];
	int rc;
	Terms( Batch& b, uint32_t bound, uint32_t flags = SP_TERM_TEXT)
	{
		sp_match_batch_t mb = b.view();
		sp_match_text_t x = b.textView();
		sp_match_values_t v = b.valuesView();
		rc = sp_match_batch_terms( &mb, (flags & SP_TERM_VALUES) ? &v : 0, (flags & SP_TERM_TEXT) ? &x : 0, bound, flags, &t, err, sizeof(err));
	}
	~Terms() { sp_match_terms_free( &t); }
	bool record( uint64_t i, uint32_t h, uint32_t n, uint32_t lo, uint32_t hi, uint32_t first, uint32_t size) const
	{
		const sp_match_term_t& r = t.records[ i];
		return r.handle == h && r.count == n && r.first_ordpos == lo && r.last_ordend == hi && r.first_result == first && r.value_bytes == size;
	}
};

static void documentSizes()
{
	// documents of 0, 1, 2 and 65 results: one term, then all values distinct under one handle
	Batch b;
	const uint32_t sizes[ 4] = {0, 1, 2, 65};
	for (uint32_t n : sizes)
	{
		for (uint32_t k=0; k<n; ++k) b.result( 7, 3*k, 3*k+2, "same");
		b.document();
		for (uint32_t k=0; k<n; ++k) b.result( 7, 5+k, 9+k, std::string( 1 + k%3, (char)('a' + k/3)));
		b.document();
	}
	Terms q( b, 8);
	CHECK( q.rc == SP_OK && q.t.ndocs == 8 && q.t.nrecords == 1+1+1+2+1+65 && q.t.totals[ 0] == q.t.nrecords);
	CHECK( q.record( 5, 7, 65, 0, 3*64+2, 0, 4));
	for (uint32_t k=0; k<65; ++k) CHECK( q.record( 6+k, 7, 1, 5+k, 9+k, k, 1 + k%3) && q.t.result_term[ 71+k] == k);
	for (int d=0; d<8; ++d) CHECK( q.t.doc_term_status[ d] == 0);
}

static void valuesAndOrder()
{
	Batch b;
	// a prefix, the last and the first byte, the empty value, the same bytes under two handles; first_result is not the least ordpos
	b.result( 2, 50, 51, "abc"); b.result( 1, 40, 41, "abc"); b.result( 2, 10, 90, "ab"); b.result( 2, 30, 31, "abd"); b.result( 2, 6, 7, "");
	b.result( 2, 5, 9, "abc"); b.result( 2, 1, 2, "bbc"); b.result( 2, 3, 4, "");
	b.document();
	Terms q( b, 3);
	CHECK( q.rc == SP_OK && q.t.nrecords == 6);
	CHECK( q.record( 0, 1, 1, 40, 41, 1, 3) && q.record( 1, 2, 2, 5, 51, 0, 3) && q.record( 2, 2, 1, 10, 90, 2, 2));
	CHECK( q.record( 3, 2, 1, 30, 31, 3, 3) && q.record( 4, 2, 2, 3, 7, 4, 0) && q.record( 5, 2, 1, 1, 2, 6, 3));
	const uint32_t want[ 8] = {1, 0, 2, 3, 4, 1, 5, 4};
	for (int r=0; r<8; ++r) CHECK( q.t.result_term[ r] == want[ r]);
	// the selector: a formatted result takes the value, another one the text (here the same bytes serve as both sources)
	Batch s;
	s.result( 1, 0, 1, "v", 1); s.result( 1, 2, 3, "v", 0); s.document();
	Terms both( s, 2, SP_TERM_VALUES | SP_TERM_TEXT);
	CHECK( both.rc == SP_OK && both.t.nrecords == 1 && both.record( 0, 1, 2, 0, 3, 0, 1));
	Terms values( s, 2, SP_TERM_VALUES);
	CHECK( values.rc == SP_OK && values.t.nrecords == 1);
}

static void rangeRule()
{
	const uint32_t bad[ 4] = {0, 6, 7, 0xFFFFFFFFu};
	for (uint32_t h : bad)
	{
		Batch b;
		b.result( 5, 1, 2, "x"); b.result( 1, 0, 9, "x"); b.document();
		b.result( 2, 0, 1, "y"); b.result( h, 3, 4, "y"); b.result( 2, 5, 6, "y"); b.document();
		b.result( 5, 7, 8, ""); b.document();
		Terms q( b, 6);
		CHECK( q.rc == SP_OK && q.t.nrecords == 3);
		CHECK( q.t.doc_term_status[ 0] == 0 && q.t.doc_term_status[ 1] == SP_DOC_ERR_RANGE && q.t.doc_term_status[ 2] == 0);
		CHECK( q.t.doc_term_offsets[ 1] == 2 && q.t.doc_term_offsets[ 2] == 2 && q.t.doc_term_offsets[ 3] == 3);
		CHECK( q.t.result_term[ 0] == 1 && q.t.result_term[ 1] == 0 && q.t.result_term[ 5] == 0);
		for (int r=2; r<5; ++r) CHECK( q.t.result_term[ r] == 0xFFFFFFFFu);
	}
	// a source status between two good documents; a document the matcher failed
	Batch b;
	b.result( 1, 0, 1, "x"); b.document();
	b.result( 1, 0, 1, "x"); b.document(); b.textStatus[ 1] = SP_DOC_ERR_RANGE;
	b.result( 1, 0, 1, "x"); b.document();
	b.result( 1, 0, 1, "x"); b.document(); b.status[ 3] = 1;
	Terms q( b, 2);
	CHECK( q.rc == SP_OK && q.t.nrecords == 2 && q.t.doc_term_status[ 1] == SP_DOC_ERR_RANGE && q.t.doc_term_status[ 3] == 0);
	CHECK( q.t.result_term[ 0] == 0 && q.t.result_term[ 1] == 0xFFFFFFFFu && q.t.result_term[ 2] == 0 && q.t.result_term[ 3] == 0xFFFFFFFFu);
}

static void refusedArguments()
{
	Batch b;
	b.result( 1, 0, 1, "ab"); b.result( 1, 2, 3, "c"); b.document(); b.result( 1, 4, 5, ""); b.document();
	{ Terms q( b, 0); CHECK( q.rc == SP_ERR_INVALID && q.err[ 0] && !q.t.records && !q.t.doc_term_offsets && !q.t.result_term); }
	{ Terms q( b, 2, 0); CHECK( q.rc == SP_ERR_INVALID); }
	{ Terms q( b, 2, 4); CHECK( q.rc == SP_ERR_INVALID); }
	sp_match_batch_t mb = b.view();
	sp_match_text_t x = b.textView();
	sp_match_terms_t t;
	char err[ 8];
	CHECK( sp_match_batch_terms( &mb, 0, &x, 2, SP_TERM_VALUES, &t, err, sizeof(err)) == SP_ERR_INVALID && std::strlen( err) == 7);	// (the message is cut to the buffer)
	CHECK( sp_match_batch_terms( &mb, 0, 0, 2, SP_TERM_TEXT, &t, 0, 0) == SP_ERR_INVALID);
	CHECK( sp_match_batch_terms( 0, 0, &x, 2, SP_TERM_TEXT, &t, 0, 0) == SP_ERR_INVALID);
	x.nresults -= 1;
	CHECK( sp_match_batch_terms( &mb, 0, &x, 2, SP_TERM_TEXT, &t, 0, 0) == SP_ERR_INVALID);
	x = b.textView(); x.result_text_offsets = 0;
	CHECK( sp_match_batch_terms( &mb, 0, &x, 2, SP_TERM_TEXT, &t, 0, 0) == SP_ERR_INVALID);
	const uint64_t sourceOffsets[ 3][ 4] = {{0, 3, 2, 3}, {0, 2, 3, 4}, {1, 2, 3, 3}};
	for (const uint64_t* o : sourceOffsets)
	{
		Batch c = b;
		c.textOffsets.assign( o, o+4);
		Terms q( c, 2);
		CHECK( q.rc == SP_ERR_INVALID && std::strstr( q.err, "offsets"));
	}
	const uint64_t offsets[ 4][ 3] = {{0, 4, 3}, {0, 1, 2}, {0, 2, 4}, {1, 2, 3}};
	for (const uint64_t* o : offsets)
	{
		Batch c = b;
		c.offsets.assign( o, o+3);
		Terms q( c, 2);
		CHECK( q.rc == SP_ERR_INVALID && std::strstr( q.err, "offsets"));
	}
	Batch none;
	Terms q( none, 2);
	CHECK( q.rc == SP_OK && q.t.ndocs == 0 && q.t.nrecords == 0 && q.t.doc_term_offsets[ 0] == 0);
}

int main()
{
	documentSizes();
	valuesAndOrder();
	rangeRule();
	refusedArguments();
	std::printf( "match_terms_san: ok\n");
	return 0;
}
