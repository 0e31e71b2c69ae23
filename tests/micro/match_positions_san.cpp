// Stand-alone host program for a sanitizer run of the device-free twin of the position passes (csrc/match_positions.hpp) over
// the edge batches of tests/test_positions_abi.py and the refused arguments.  The terms, the dictionary and the postings come
// from their twins.  No HIP code is linked:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Istruspattern_amd/csrc \
//       tests/micro/match_positions_san.cpp struspattern_amd/csrc/match_positions.cpp struspattern_amd/csrc/match_postings.cpp \
//       struspattern_amd/csrc/match_dict.cpp struspattern_amd/csrc/match_terms.cpp -o match_positions_san && ./match_positions_san
#include "match_positions.hpp"
#include "finished_batch_fixture.hpp"

// the terms, dictionary and postings of a batch by their twins, and the positions
struct Positions
{
	sp_match_batch_t mb;
	sp_match_text_t x;
	sp_match_terms_t t;
	sp_match_dictionary_t d;
	sp_match_postings_t p;
	sp_match_positions_t q;
	struct { sp_match_terms_t t; sp_match_postings_t p; } owned;
	char err[ 160];
	int rc;
	Positions( Batch& b, uint32_t bound, void (*damage)( Positions&) = 0)
	{
		mb = b.view(); x = b.textView();
		CHECK( sp_match_batch_terms( &mb, 0, &x, bound, SP_TERM_TEXT, &t, err, sizeof(err)) == SP_OK);
		CHECK( sp_match_batch_dictionary( &mb, 0, &x, &t, &d, err, sizeof(err)) == SP_OK);
		CHECK( sp_match_batch_postings( &t, &d, &p, err, sizeof(err)) == SP_OK);
		owned.t = t; owned.p = p;		// (a damage may clear a pointer: what is released is what was allocated)
		if (damage) damage( *this);
		rc = sp_match_batch_positions( &mb, &t, &p, &q, err, sizeof(err));
	}
	~Positions() { sp_match_positions_free( &q); sp_match_postings_free( &owned.p); sp_match_dictionary_free( &d); sp_match_terms_free( &owned.t); }
	bool occurrence( uint64_t i, uint32_t ordpos, uint32_t result) const { return q.occurrences[ i].ordpos == ordpos && q.occurrences[ i].result == result; }
	bool empty() const { return !q.occurrences && !q.posting_offsets && !q.posting_positions && q.nocc == 0 && q.nterms == 0 && q.totals[ 0] == 0 && q.totals[ 1] == 0; }
};

static void shapes()
{
	// no documents; documents without results; one document with one result
	{ Batch b; Positions q( b, 3); CHECK( q.rc == SP_OK && q.q.ndocs == 0 && q.q.nocc == 0 && q.q.nterms == 0 && q.q.posting_offsets[ 0] == 0); }
	{ Batch b; b.document(); b.document(); Positions q( b, 3); CHECK( q.rc == SP_OK && q.q.nocc == 0 && q.q.posting_offsets[ 0] == 0 && q.q.totals[ 1] == 0); }
	Batch b;
	b.result( 2, 7, 8, "abc"); b.document();
	Positions q( b, 3);
	CHECK( q.rc == SP_OK && q.q.nocc == 1 && q.q.nterms == 1 && q.occurrence( 0, 7, 0) && q.q.posting_positions[ 0] == 1 && q.q.posting_offsets[ 1] == 1);
}

static void orderAndTies()
{
	// lists out of position order, a tie at one position with two ends, a failed document in the middle, position 0, and a
	// list of 300 occurrences that descend
	Batch b;
	b.result( 1, 9, 10, "eur"); b.result( 2, 4, 5, "x"); b.result( 1, 3, 4, "eur"); b.result( 1, 3, 6, "eur"); b.result( 1, 0, 1, "eur"); b.document();
	b.result( 1, 5, 6, "usd"); b.document(); b.textStatus[ 1] = SP_DOC_ERR_RANGE;
	b.result( 2, 2, 3, "x"); b.result( 1, 7, 8, "eur"); b.result( 1, 1, 2, "eur"); b.result( 2, 2, 9, "x"); b.document();
	for (uint32_t k=0; k<300; ++k) b.result( 3, 1000 - 3*(k/2), 2000, "q");
	b.document();
	Positions q( b, 4);
	CHECK( q.rc == SP_OK && q.q.nterms == 5 && q.q.nocc == 309 && q.q.totals[ 0] == 309 && q.t.doc_term_status[ 1] == SP_DOC_ERR_RANGE);
	CHECK( q.occurrence( 0, 0, 4) && q.occurrence( 1, 3, 2) && q.occurrence( 2, 3, 3) && q.occurrence( 3, 9, 0));
	CHECK( q.occurrence( 4, 1, 2) && q.occurrence( 5, 7, 1) && q.occurrence( 6, 4, 1) && q.occurrence( 7, 2, 0) && q.occurrence( 8, 2, 3));
	CHECK( q.q.posting_positions[ 0] == 3 && q.q.posting_positions[ 1] == 2 && q.q.posting_positions[ 2] == 1 && q.q.posting_positions[ 3] == 1);
	CHECK( q.q.posting_positions[ 4] == 150 && q.q.totals[ 1] == 157 && q.q.posting_offsets[ 4] == 9 && q.q.posting_offsets[ 5] == 309);
	CHECK( q.occurrence( 9, 1000 - 3*149, 298) && q.occurrence( 10, 1000 - 3*149, 299) && q.occurrence( 308, 1000, 1));
	for (uint64_t i=10; i<309; ++i) CHECK( q.q.occurrences[ i-1].ordpos <= q.q.occurrences[ i].ordpos);
}

static void refusedArguments()
{
	Batch b;
	b.result( 1, 2, 3, "ab"); b.result( 1, 1, 2, "ab"); b.result( 2, 5, 6, "c"); b.document(); b.result( 1, 4, 5, "ab"); b.document();
	{ Positions q( b, 3); CHECK( q.rc == SP_OK && q.q.nocc == 4 && q.q.nterms == 3); }
	void (*damages[])( Positions&) = {
		[]( Positions& q) { q.mb.ndocs += 1; },
		[]( Positions& q) { q.t.ndocs -= 1; },
		[]( Positions& q) { q.p.ndocs += 1; },
		[]( Positions& q) { q.t.nresults -= 1; },
		[]( Positions& q) { q.mb.nresults += 1; },
		[]( Positions& q) { q.p.nterms -= 1; },
		[]( Positions& q) { q.t.nrecords += 1; },
		[]( Positions& q) { q.mb.doc_result_offsets = 0; },
		[]( Positions& q) { q.t.doc_term_offsets = 0; },
		[]( Positions& q) { q.t.result_term = 0; },
		[]( Positions& q) { q.p.record_posting = 0; },
		[]( Positions& q) { q.p.postings = 0; },
		[]( Positions& q) { q.mb.results = 0; },
		[]( Positions& q) { q.t.doc_term_offsets[ 0] = 1; },
		[]( Positions& q) { q.t.doc_term_offsets[ 1] = 3; q.t.doc_term_offsets[ 2] = 2; },
		[]( Positions& q) { q.t.doc_term_offsets[ 2] = 2; },
		[]( Positions& q) { q.mb.nresults -= 1; q.t.nresults -= 1; },
		[]( Positions& q) { q.t.nrecords -= 1; q.p.nterms -= 1; },
		[]( Positions& q) { q.t.result_term[ 3] = 1; },
		[]( Positions& q) { q.t.result_term[ 0] = 0xFFFFFFFEu; },
		[]( Positions& q) { q.p.record_posting[ 1] = 3; },
		[]( Positions& q) { q.p.record_posting[ 0] = 0xFFFFFFFFu; },
		[]( Positions& q) { q.p.postings[ 0].count += 1; },
		[]( Positions& q) { q.t.result_term[ 0] = 1; },
		[]( Positions& q) { q.t.result_term[ 3] = 0xFFFFFFFFu; },
	};
	for (auto damage : damages)
	{
		Positions q( b, 3, damage);
		CHECK( q.rc == SP_ERR_INVALID && q.err[ 0] && q.empty());
	}
	Positions good( b, 3);
	sp_match_positions_t out;
	char err[ 8];
	CHECK( sp_match_batch_positions( 0, &good.t, &good.p, &out, err, sizeof(err)) == SP_ERR_INVALID && std::strlen( err) == 7);	// (the message is cut to the buffer)
	CHECK( sp_match_batch_positions( &good.mb, 0, &good.p, &out, 0, 0) == SP_ERR_INVALID);
	CHECK( sp_match_batch_positions( &good.mb, &good.t, 0, &out, 0, 0) == SP_ERR_INVALID);
}

int main()
{
	shapes();
	orderAndTies();
	refusedArguments();
	std::printf( "match_positions_san: ok\n");
	return 0;
}
