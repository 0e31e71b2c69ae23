// Stand-alone host program for a sanitizer run of the device-free twin of the dictionary passes (csrc/match_dict.hpp) over the
// edge batches of tests/test_dictionary_abi.py and the refused arguments.  The terms come from the twin of the term passes.
// No HIP code is linked:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Istruspattern_amd/csrc \
//       tests/micro/match_dict_san.cpp struspattern_amd/csrc/match_dict.cpp struspattern_amd/csrc/match_terms.cpp \
//       -o match_dict_san && ./match_dict_san
#include "match_dict.hpp"
#include "finished_batch_fixture.hpp"

// the terms of a batch by the twin of the term passes, and their dictionary
struct Dictionary
{
	sp_match_batch_t mb;
	sp_match_text_t x;
	sp_match_values_t v;
	sp_match_terms_t t;
	sp_match_dictionary_t d;
	char err[ 160];
	int rc;
	Dictionary( Batch& b, uint32_t bound, uint32_t flags = SP_TERM_TEXT, void (*damage)( Dictionary&) = 0)
	{
		mb = b.view(); x = b.textView(); v = b.valuesView();
		CHECK( sp_match_batch_terms( &mb, (flags & SP_TERM_VALUES) ? &v : 0, (flags & SP_TERM_TEXT) ? &x : 0, bound, flags, &t, err, sizeof(err)) == SP_OK);
		if (damage) damage( *this);
		rc = sp_match_batch_dictionary( &mb, (flags & SP_TERM_VALUES) ? &v : 0, (flags & SP_TERM_TEXT) ? &x : 0, &t, &d, err, sizeof(err));
	}
	~Dictionary() { sp_match_dictionary_free( &d); sp_match_terms_free( &t); }
	bool entry( uint64_t i, uint32_t h, uint32_t size, uint32_t doc, uint32_t term, uint32_t df, uint32_t mx, uint64_t n) const
	{
		const sp_dict_term_t& e = d.records[ i];
		return e.handle == h && e.value_bytes == size && e.first_doc == doc && e.first_term == term && e.doc_freq == df && e.max_count == mx && e.count == n;
	}
	bool empty() const { return !d.records && !d.term_dict && !d.doc_dict_offsets && !d.handle_terms && d.ndict == 0; }
};

static void shapes()
{
	// no documents; documents without results; one document
	{ Batch b; Dictionary q( b, 3); CHECK( q.rc == SP_OK && q.d.ndocs == 0 && q.d.ndict == 0 && q.d.nterms == 0 && q.d.doc_dict_offsets[ 0] == 0); }
	{ Batch b; b.document(); b.document(); Dictionary q( b, 3); CHECK( q.rc == SP_OK && q.d.ndict == 0 && q.d.doc_dict_offsets[ 2] == 0 && q.d.handle_terms[ 2] == 0); }
	Batch b;
	b.result( 2, "abc"); b.result( 1, "abc"); b.result( 2, "abc"); b.result( 2, ""); b.document();
	Dictionary q( b, 3);
	CHECK( q.rc == SP_OK && q.d.ndict == 3 && q.d.nterms == 3 && q.d.totals[ 0] == 3);
	CHECK( q.entry( 0, 1, 3, 0, 0, 1, 1, 1) && q.entry( 1, 2, 3, 0, 1, 1, 2, 2) && q.entry( 2, 2, 0, 0, 2, 1, 1, 1));
	CHECK( q.d.handle_terms[ 0] == 0 && q.d.handle_terms[ 1] == 1 && q.d.handle_terms[ 2] == 2);
	for (uint32_t i=0; i<3; ++i) CHECK( q.d.term_dict[ i] == i);
}

static void acrossDocuments()
{
	// a term in the documents 0, 2 and 3; the same bytes under two handles; a prefix; the last and the first byte; the empty
	// value in two documents; a document whose terms are all known; 65 documents that repeat one term
	Batch b;
	b.result( 1, "eur"); b.result( 1, "eur"); b.result( 2, "x"); b.result( 1, "ab"); b.result( 3, ""); b.document();
	b.result( 2, "eur"); b.result( 1, "abc"); b.result( 1, "aby"); b.result( 1, "xb"); b.document();
	b.result( 1, "eur"); b.result( 3, ""); b.result( 1, "eur"); b.result( 1, "eur"); b.document();
	b.result( 1, "eur"); b.result( 2, "x"); b.document();
	for (int k=0; k<65; ++k) { b.result( 3, ""); b.result( 3, std::string( 1 + k%17, 'q')); b.document(); }
	Dictionary q( b, 4);
	CHECK( q.rc == SP_OK && q.d.ndict == 4 + 4 + 17 && q.d.nterms == 4 + 4 + 2 + 2 + 130);
	CHECK( q.entry( 0, 1, 3, 0, 0, 3, 3, 6) && q.entry( 1, 1, 2, 0, 1, 1, 1, 1) && q.entry( 2, 2, 1, 0, 2, 2, 1, 2) && q.entry( 3, 3, 0, 0, 3, 67, 1, 67));
	CHECK( q.entry( 4, 1, 3, 1, 0, 1, 1, 1) && q.entry( 5, 1, 3, 1, 1, 1, 1, 1) && q.entry( 6, 1, 2, 1, 2, 1, 1, 1) && q.entry( 7, 2, 3, 1, 3, 1, 1, 1));
	CHECK( q.d.doc_dict_offsets[ 1] == 4 && q.d.doc_dict_offsets[ 2] == 8 && q.d.doc_dict_offsets[ 3] == 8 && q.d.doc_dict_offsets[ 4] == 8);
	CHECK( q.d.doc_dict_offsets[ 4 + 17] == 25 && q.d.doc_dict_offsets[ 4 + 18] == 25 && q.d.doc_dict_offsets[ 4 + 65] == 25);
	CHECK( q.entry( 8, 3, 1, 4, 1, 4, 1, 4) && q.entry( 24, 3, 17, 20, 1, 3, 1, 3));
	uint64_t docFreq = 0, count = 0, terms = 0;
	for (size_t i=0; i<q.d.ndict; ++i) { docFreq += q.d.records[ i].doc_freq; count += q.d.records[ i].count; }
	for (uint32_t h=0; h<4; ++h) terms += q.d.handle_terms[ h];
	CHECK( docFreq == q.d.nterms && count == b.results.size() && terms == q.d.ndict);
	for (size_t i=0; i<q.d.nterms; ++i) CHECK( q.d.term_dict[ i] < q.d.ndict);
}

static void sourcesAndFailedDocuments()
{
	// both flags: a formatted value equal to the text of an unformatted result in another document is one entry
	Batch b;
	b.result( 1, "zzz", "eur", 7); b.document();
	b.result( 1, "eur"); b.result( 1, "eur", "", 2); b.document();
	Dictionary both( b, 2, SP_TERM_VALUES | SP_TERM_TEXT);
	CHECK( both.rc == SP_OK && both.d.ndict == 2 && both.entry( 0, 1, 3, 0, 0, 2, 1, 2) && both.entry( 1, 1, 0, 1, 1, 1, 1, 1));
	Dictionary values( b, 2, SP_TERM_VALUES);
	CHECK( values.rc == SP_OK && values.d.ndict == 2 && values.entry( 0, 1, 3, 0, 0, 1, 1, 1) && values.entry( 1, 1, 0, 1, 0, 1, 2, 2));
	Dictionary text( b, 2, SP_TERM_TEXT);
	CHECK( text.rc == SP_OK && text.d.ndict == 2 && text.entry( 1, 1, 3, 1, 0, 1, 2, 2));
	// a document with a term status between two good ones, and one the matcher failed
	Batch f;
	f.result( 1, "a"); f.document();
	f.result( 1, "b"); f.document(); f.textStatus[ 1] = SP_DOC_ERR_RANGE;
	f.result( 1, "c"); f.result( 1, "a"); f.document();
	f.result( 1, "d"); f.document(); f.status[ 3] = 1;
	Dictionary q( f, 2);
	CHECK( q.rc == SP_OK && q.t.doc_term_status[ 1] == SP_DOC_ERR_RANGE && q.d.ndict == 2 && q.d.nterms == 3);
	CHECK( q.entry( 0, 1, 1, 0, 0, 2, 1, 2) && q.entry( 1, 1, 1, 2, 0, 1, 1, 1) && q.d.doc_dict_offsets[ 2] == 1 && q.d.doc_dict_offsets[ 4] == 2);
}

static void refusedArguments()
{
	Batch b;
	b.result( 1, "ab", "v", 1); b.result( 1, "c"); b.document(); b.result( 1, ""); b.document();
	const uint32_t both = SP_TERM_VALUES | SP_TERM_TEXT;
	{ Dictionary q( b, 2, both); CHECK( q.rc == SP_OK && q.d.ndict == 3); }
	void (*damages[])( Dictionary&) = {
		[]( Dictionary& q) { q.t.ndocs += 1; },
		[]( Dictionary& q) { q.t.nresults -= 1; },
		[]( Dictionary& q) { q.x.nresults += 1; },
		[]( Dictionary& q) { q.v.ndocs -= 1; },
		[]( Dictionary& q) { q.x.result_text_offsets = 0; },
		[]( Dictionary& q) { q.v.result_value_offsets = 0; },
		[]( Dictionary& q) { q.t.doc_term_offsets[ 0] = 1; },
		[]( Dictionary& q) { q.t.doc_term_offsets[ 1] = 3; q.t.doc_term_offsets[ 2] = 2; },
		[]( Dictionary& q) { q.t.doc_term_offsets[ 2] = 2; },
		[]( Dictionary& q) { q.t.nrecords -= 1; },
		[]( Dictionary& q) { q.t.records[ 2].first_result = 1; },
		[]( Dictionary& q) { q.t.records[ 0].first_result = 0xFFFFFFFFu; },
		[]( Dictionary& q) { q.t.records[ 1].value_bytes = 2; },
		[]( Dictionary& q) { q.t.records[ 2].value_bytes = 1; },
		[]( Dictionary& q) { q.t.records[ 0].handle = 2; },
		[]( Dictionary& q) { q.t.records[ 0].handle = 0; },
		[]( Dictionary& q) { q.t.flags = 4; },
		[]( Dictionary& q) { q.t.handle_bound = 0; },
	};
	for (auto damage : damages)
	{
		Dictionary q( b, 2, both, damage);
		CHECK( q.rc == SP_ERR_INVALID && q.err[ 0] && q.empty());
	}
	Dictionary good( b, 2, both);
	sp_match_dictionary_t d;
	char err[ 8];
	CHECK( sp_match_batch_dictionary( &good.mb, 0, &good.x, &good.t, &d, err, sizeof(err)) == SP_ERR_INVALID && std::strlen( err) == 7);	// (the message is cut to the buffer)
	CHECK( sp_match_batch_dictionary( &good.mb, &good.v, 0, &good.t, &d, 0, 0) == SP_ERR_INVALID);
	CHECK( sp_match_batch_dictionary( 0, &good.v, &good.x, &good.t, &d, 0, 0) == SP_ERR_INVALID);
	CHECK( sp_match_batch_dictionary( &good.mb, &good.v, &good.x, 0, &d, 0, 0) == SP_ERR_INVALID);
}

int main()
{
	shapes();
	acrossDocuments();
	sourcesAndFailedDocuments();
	refusedArguments();
	std::printf( "match_dict_san: ok\n");
	return 0;
}
