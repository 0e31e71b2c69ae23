// Stand-alone host program for a sanitizer run of the device-free twin of the frequency passes (csrc/pattern_freq.hpp) over the
// edge batches of tests/test_pattern_freq_abi.py, the invalid handles and the refused arguments included.  No HIP code is linked:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Istruspattern_amd/csrc \
//       tests/micro/pattern_freq_san.cpp struspattern_amd/csrc/pattern_freq.cpp -o pattern_freq_san && ./pattern_freq_san
#include "pattern_freq.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK( COND) do { if (!(COND)) { std::fprintf( stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #COND); std::exit( 1); } } while (0)

// A finished batch.  Every array is exactly as long as what it holds, so a read past it is the sanitizer's to report.
struct Batch
{
	std::vector<sp_result_t> results;
	std::vector<uint64_t> offsets = {0};
	std::vector<int32_t> status;

	void document() { offsets.push_back( results.size()); status.push_back( 0); }
	void result( uint32_t handle, uint32_t ordpos, uint32_t ordend)
	{
		sp_result_t r = {};
		r.handle = handle; r.ordpos = ordpos; r.ordend = ordend;
		results.push_back( r);
	}
	sp_match_batch_t view()
	{
		sp_match_batch_t mb = {};
		mb.ndocs = status.size(); mb.nresults = results.size();
		mb.results = results.empty() ? 0 : results.data(); mb.doc_result_offsets = offsets.data(); mb.doc_status = status.empty() ? 0 : status.data();
		return mb;
	}
};

struct Freq
{
	sp_pattern_freq_batch_t f;
	char err[ 128];
	int rc;
	Freq( Batch& b, uint32_t bound) { sp_match_batch_t mb = b.view(); rc = sp_match_batch_pattern_freq( &mb, bound, &f, err, sizeof(err)); }
	~Freq() { sp_pattern_freq_batch_free( &f); }
	bool record( uint64_t i, uint32_t h, uint32_t n, uint32_t lo, uint32_t hi) const
	{
		const sp_pattern_freq_t& r = f.records[ i];
		return r.handle == h && r.count == n && r.first_ordpos == lo && r.last_ordend == hi;
	}
};

static void documentSizes()
{
	// documents of 0, 1, 2 and 65 results: one handle, then all handles distinct (descending)
	Batch b;
	const uint32_t sizes[ 4] = {0, 1, 2, 65};
	for (uint32_t n : sizes)
	{
		for (uint32_t k=0; k<n; ++k) b.result( 250, 3*k, 3*k+2);
		b.document();
		for (uint32_t k=0; k<n; ++k) b.result( 200-k, 5+k, 9+k);
		b.document();
	}
	Freq q( b, 251);
	CHECK( q.rc == SP_OK && q.f.ndocs == 8 && q.f.nrecords == 1+1+1+2+1+65 && q.f.totals[ 0] == q.f.nrecords);
	const uint64_t want[ 9] = {0, 0, 0, 1, 2, 3, 5, 6, 71};
	for (int d=0; d<=8; ++d) CHECK( q.f.doc_offsets[ d] == want[ d]);
	CHECK( q.record( 5, 250, 65, 0, 3*64+2));
	for (uint32_t k=0; k<65; ++k) CHECK( q.record( 6+k, 136+k, 1, 5+(64-k), 9+(64-k)));
	CHECK( q.f.handle_results[ 250] == 68 && q.f.handle_docs[ 250] == 3 && q.f.handle_results[ 0] == 0 && q.f.handle_docs[ 200] == 3);
	for (int d=0; d<8; ++d) CHECK( q.f.doc_freq_status[ d] == 0);
}

static void minimumAndMaximum()
{
	Batch b;
	b.result( 4, 50, 51); b.result( 9, 7, 8); b.result( 4, 10, 90); b.result( 4, 30, 31); b.result( 9, 6, 7); b.result( 9, 8, 9);
	b.document();
	b.result( 2, 0xFFFFFFF0u, 0xFFFFFFFEu); b.result( 2, 0x80000000u, 0x80000001u); b.result( 2, 5, 6);
	b.document();
	Freq q( b, 10);
	CHECK( q.rc == SP_OK && q.f.nrecords == 3);
	CHECK( q.record( 0, 4, 3, 10, 90) && q.record( 1, 9, 3, 6, 9) && q.record( 2, 2, 3, 5, 0xFFFFFFFEu));
}

static void failedDocument()
{
	Batch b;
	b.result( 1, 0, 1); b.document();
	b.document(); b.status[ 1] = 2;
	b.result( 2, 4, 5); b.result( 1, 1, 2); b.document();
	b.result( 2, 0, 1); b.document(); b.status[ 3] = 1;		// a status and a range that is not empty: no records
	Freq q( b, 3);
	CHECK( q.rc == SP_OK && q.f.nrecords == 3 && q.f.doc_offsets[ 2] == 1 && q.f.doc_offsets[ 3] == 3 && q.f.doc_offsets[ 4] == 3);
	for (int d=0; d<4; ++d) CHECK( q.f.doc_freq_status[ d] == 0);
	CHECK( q.f.handle_docs[ 1] == 2 && q.f.handle_docs[ 2] == 1 && q.f.handle_results[ 1] == 2);
}

static void rangeRule()
{
	const uint32_t bad[ 4] = {0, 6, 7, 0xFFFFFFFFu};
	for (uint32_t h : bad)
	{
		Batch b;
		b.result( 5, 1, 2); b.result( 1, 0, 9); b.document();
		b.result( 2, 0, 1); b.result( h, 3, 4); b.result( 2, 5, 6); b.document();
		b.result( 5, 7, 8); b.document();
		Freq q( b, 6);
		CHECK( q.rc == SP_OK && q.f.nrecords == 3);
		CHECK( q.f.doc_freq_status[ 0] == 0 && q.f.doc_freq_status[ 1] == SP_DOC_ERR_RANGE && q.f.doc_freq_status[ 2] == 0);
		CHECK( q.f.doc_offsets[ 1] == 2 && q.f.doc_offsets[ 2] == 2 && q.f.doc_offsets[ 3] == 3);
		CHECK( q.record( 0, 1, 1, 0, 9) && q.record( 1, 5, 1, 1, 2) && q.record( 2, 5, 1, 7, 8));
		CHECK( q.f.handle_docs[ 2] == 0 && q.f.handle_results[ 2] == 0 && q.f.handle_docs[ 5] == 2);
	}
	// a bound of 1 leaves no valid handle: every document with results fails
	Batch b;
	b.result( 1, 0, 1); b.document(); b.document();
	Freq q( b, 1);
	CHECK( q.rc == SP_OK && q.f.nrecords == 0 && q.f.doc_freq_status[ 0] == SP_DOC_ERR_RANGE && q.f.doc_freq_status[ 1] == 0);
}

static void refusedArguments()
{
	Batch b;
	b.result( 1, 0, 1); b.result( 1, 2, 3); b.document(); b.result( 1, 4, 5); b.document();
	{ Freq q( b, 0); CHECK( q.rc == SP_ERR_INVALID && q.err[ 0] && !q.f.records && !q.f.doc_offsets); }
	const uint64_t offsets[ 4][ 3] = {{0, 3, 2}, {0, 1, 2}, {0, 2, 4}, {1, 2, 3}};
	for (const uint64_t* o : offsets)
	{
		b.offsets.assign( o, o+3);
		Freq q( b, 4);
		CHECK( q.rc == SP_ERR_INVALID && std::strstr( q.err, "offsets"));
	}
	sp_pattern_freq_batch_t f;
	char err[ 8];
	CHECK( sp_match_batch_pattern_freq( 0, 4, &f, err, sizeof(err)) == SP_ERR_INVALID && std::strlen( err) == 7);	// (the message is cut to the buffer)
	CHECK( sp_match_batch_pattern_freq( 0, 4, &f, 0, 0) == SP_ERR_INVALID);
	Batch none;
	Freq q( none, 2);
	CHECK( q.rc == SP_OK && q.f.ndocs == 0 && q.f.nrecords == 0 && q.f.doc_offsets[ 0] == 0 && q.f.handle_docs[ 1] == 0);
}

int main()
{
	documentSizes();
	minimumAndMaximum();
	failedDocument();
	rangeRule();
	refusedArguments();
	std::printf( "pattern_freq_san: ok\n");
	return 0;
}
