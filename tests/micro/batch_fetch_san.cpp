// Stand-alone host program for a sanitizer run of the device-free host fetch layer (csrc/batch_fetch.hpp): block planning, item
// planning, eliminateCovered and both regroups over a synthetic batch in the device layout (documents in completion order), with
// memcpy in the place of the device copies.  No HIP code is linked:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Istruspattern_amd/csrc \
//       tests/micro/batch_fetch_san.cpp struspattern_amd/csrc/batch_fetch.cpp -o batch_fetch_san && ./batch_fetch_san
#include "batch_fetch.hpp"
#include <cstdio>
#include <string>

using namespace spa;

#define CHECK( COND) do { if (!(COND)) { std::fprintf( stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #COND); std::exit( 1); } } while (0)

static void hostCopy( void* dst, const void* src, size_t n) { std::memcpy( dst, src, n); }

// A batch as the kernels leave it.  Every array is exactly as long as what lies "inside the buffer", so a read past it is the
// sanitizer's to report.
struct Batch
{
	std::vector<sp_result_t> results;
	std::vector<sp_result_item_t> items;
	std::vector<uint32_t> rf, itf;
	std::vector<sp_lexem_t> lexems;
	std::vector<uint64_t> range, lexRange;
	std::vector<int32_t> status;
	std::vector<uint64_t> stats;

	size_t ndocs() const { return status.size(); }
	MatchBatchSource matchSource( bool formats) const
	{
		MatchBatchSource s;
		s.results = results.data(); s.nresults = results.size(); s.items = items.data(); s.nitems = items.size();
		s.resultFormat = formats ? rf.data() : 0; s.itemFormat = formats ? itf.data() : 0;
		s.docRange = range.data(); s.docStatus = status.data(); s.docStats = stats.data(); s.ndocs = ndocs();
		return s;
	}
	LexBatchSource lexSource() const
	{
		LexBatchSource s;
		s.lexems = lexems.data(); s.nlexems = lexems.size(); s.docRange = lexRange.data(); s.docStatus = status.data(); s.ndocs = ndocs();
		return s;
	}
};

// document d has d % 5 results at positions that nest (for `exclusive`), every second result without items, and 3*d % 7 lexems;
// the documents complete in the order d*7 mod ndocs
static Batch makeBatch( size_t ndocs)
{
	Batch b;
	b.range.resize( 2*ndocs); b.lexRange.resize( 2*ndocs); b.status.assign( ndocs, 0); b.stats.resize( 4*ndocs);
	for (size_t k=0; k<ndocs; ++k)
	{
		const uint32_t d = (uint32_t)((k*7) % ndocs);		// (ndocs is no multiple of 7)
		const uint32_t n = d % 5;
		b.range[ 2*d] = b.results.size(); b.range[ 2*d+1] = n;
		for (uint32_t ri=0; ri<n; ++ri)
		{
			sp_result_t r = {};
			r.handle = 100*d + ri; r.ordpos = ri; r.ordend = ri+1;
			r.origpos = 10*(ri/2); r.origend = r.origpos + 4 - (ri%2);	// (an odd result lies inside the even one before it)
			r.item_count = (ri % 2) ? 0 : 1 + d % 3;
			r.item_begin = (uint32_t)b.items.size();
			for (uint32_t ii=0; ii<r.item_count; ++ii)
			{
				sp_result_item_t it = {};
				it.variable = 1000*d + 10*ri + ii;
				b.items.push_back( it);
				b.itf.push_back( it.variable + 1); b.itf.push_back( ii);
			}
			b.results.push_back( r);
			b.rf.push_back( r.handle + 7);
		}
		b.lexRange[ 2*d] = b.lexems.size(); b.lexRange[ 2*d+1] = (3*d) % 7;
		for (uint32_t li=0; li<(3*d) % 7; ++li) { sp_lexem_t l = {d, li, li, 1}; b.lexems.push_back( l); }
		for (int i=0; i<4; ++i) b.stats[ 4*d+i] = 4*d+i;
	}
	return b;
}

// what document d must come out as
static void checkMatchDoc( const Batch& b, const sp_match_batch_t& out, size_t od, uint32_t d, bool formats, bool exclusive, bool empty)
{
	const uint64_t lo = out.doc_result_offsets[ od], hi = out.doc_result_offsets[ od+1];
	CHECK( out.doc_status[ od] == b.status[ d]);
	for (int i=0; i<4; ++i) CHECK( out.doc_stats[ 4*od+i] == 4*d+i);
	if (empty) { CHECK( lo == hi); return; }
	uint64_t ri = lo;
	for (uint32_t k=0; k<d % 5; ++k)
	{
		if (exclusive && (k % 2)) continue;			// covered by the result before it
		CHECK( ri < hi);
		const sp_result_t& r = out.results[ ri];
		CHECK( r.handle == 100*d + k && r.item_count == ((k % 2) ? 0 : 1 + d % 3));
		if (formats) CHECK( out.result_format[ ri] == r.handle + 7);
		for (uint32_t ii=0; ii<r.item_count; ++ii)
		{
			CHECK( r.item_begin + ii < out.nitems);
			CHECK( out.items[ r.item_begin+ii].variable == 1000*d + 10*k + ii);
			if (formats) CHECK( out.item_format[ 2*(r.item_begin+ii)] == 1000*d + 10*k + ii + 1 && out.item_format[ 2*(r.item_begin+ii)+1] == ii);
		}
		++ri;
	}
	CHECK( ri == hi);
}

static void checkMatchFetch( const Batch& b, size_t first, size_t n, bool formats, bool exclusive, int emptyA=-1, int emptyB=-1)
{
	sp_match_batch_t out;
	std::memset( &out, 0, sizeof(out));
	fetchMatchBatch( b.matchSource( formats), first, n, exclusive, 30, hostCopy, &out);
	CHECK( out.ndocs == n && out.doc_result_offsets[ 0] == 0 && out.doc_result_offsets[ n] == out.nresults);
	CHECK( (out.result_format != 0) == formats && (out.item_format != 0) == formats);
	uint64_t ip = 0;
	for (uint64_t ri=0; ri<out.nresults; ++ri) { CHECK( out.results[ ri].item_begin == ip); ip += out.results[ ri].item_count; }
	CHECK( ip == out.nitems);
	for (size_t od=0; od<n; ++od) checkMatchDoc( b, out, od, (uint32_t)(first+od), formats, exclusive, (int)(first+od) == emptyA || (int)(first+od) == emptyB);
	std::free( out.results); std::free( out.items); std::free( out.doc_result_offsets); std::free( out.doc_stats); std::free( out.doc_status);
	std::free( out.result_format); std::free( out.item_format);
}

static void checkLexFetch( const Batch& b, size_t first, size_t n, bool bulk, int emptyA=-1, int emptyB=-1)
{
	sp_lex_batch_t out;
	std::memset( &out, 0, sizeof(out));
	fetchLexBatch( b.lexSource(), first, n, bulk, hostCopy, &out);
	CHECK( out.ndocs == n && out.doc_lexem_offsets[ 0] == 0 && out.doc_lexem_offsets[ n] == out.nlexems);
	for (size_t od=0; od<n; ++od)
	{
		const uint32_t d = (uint32_t)(first+od);
		const uint64_t lo = out.doc_lexem_offsets[ od], hi = out.doc_lexem_offsets[ od+1];
		CHECK( out.doc_status[ od] == b.status[ d]);
		if ((int)d == emptyA || (int)d == emptyB) { CHECK( lo == hi); continue; }
		CHECK( hi - lo == (3*d) % 7);
		for (uint64_t li=lo; li<hi; ++li) CHECK( out.lexems[ li].id == d && out.lexems[ li].ordpos == li-lo);
	}
	std::free( out.lexems); std::free( out.doc_lexem_offsets); std::free( out.doc_status);
}

template <class FN>
static bool throwsWith( const char* msg, FN fn)
{
	try { fn(); }
	catch (const std::runtime_error& e) { return std::string( e.what()) == msg; }
	return false;
}

int main()
{
	const size_t NDOCS = 24;
	const Batch b = makeBatch( NDOCS);
	const size_t ranges[][ 2] = {{0,NDOCS}, {0,0}, {0,1}, {5,3}, {NDOCS-1,1}, {NDOCS,0}, {1,NDOCS-1}, {0,NDOCS-1}};

	// the plans: the whole batch is one bulk segment with the ranges as they are, a sub-range one segment per non-empty document
	{
		const DocBlocks whole = planDocBlocks( b.range, b.status.data(), b.results.size(), true);
		CHECK( whole.segments.size() == 1 && whole.segments[ 0].src == 0 && whole.segments[ 0].count == b.results.size() && whole.segments[ 0].dst == 0);
		CHECK( whole.packed == b.results.size() && whole.range == b.range);
		std::vector<sp_result_t> raw = b.results;
		const ItemBlocks wi = planItemBlocks( whole, raw.data(), b.items.size(), true);
		CHECK( wi.segments.size() == 1 && wi.segments[ 0].count == b.items.size() && wi.packed == b.items.size() && wi.kept == b.items.size());
		CHECK( std::memcmp( raw.data(), b.results.data(), raw.size()*sizeof(sp_result_t)) == 0);
		const std::vector<uint64_t> sub( b.range.begin() + 2*5, b.range.begin() + 2*8);		// documents 5 (no results), 6, 7
		const DocBlocks part = planDocBlocks( sub, b.status.data() + 5, b.results.size(), false);
		CHECK( part.segments.size() == 2 && part.packed == 1 + 2 && part.first( 1) == 0 && part.count( 1) == 1 && part.first( 2) == 1 && part.count( 2) == 2);
		CHECK( part.segments[ 0].src == b.range[ 2*6] && part.segments[ 1].src == b.range[ 2*7] && part.segments[ 1].dst == 1);
		CHECK( planDocBlocks( std::vector<uint64_t>(), 0, 0, true).segments.empty() && planDocBlocks( std::vector<uint64_t>(), 0, 5, false).packed == 0);
	}
	// eliminateCovered: equal results stay, the inner of two goes, nothing beyond maxResultSize is looked at
	{
		sp_result_t r[ 4] = {};
		r[ 0].origpos = 0; r[ 0].origend = 10; r[ 1].origpos = 0; r[ 1].origend = 10; r[ 2].origpos = 2; r[ 2].origend = 5; r[ 3].origpos = 50; r[ 3].origend = 51;
		std::vector<char> covered;
		eliminateCovered( r, 4, 30, covered);
		CHECK( covered.size() == 4 && !covered[ 0] && !covered[ 1] && covered[ 2] && !covered[ 3]);
		eliminateCovered( r, 0, 30, covered);
		CHECK( covered.empty());
	}
	// both regroups, every range, with and without format handles and `exclusive`
	for (const auto& r : ranges)
	{
		for (int formats=0; formats<2; ++formats) for (int exclusive=0; exclusive<2; ++exclusive) checkMatchFetch( b, r[ 0], r[ 1], formats != 0, exclusive != 0);
		checkLexFetch( b, r[ 0], r[ 1], false); checkLexFetch( b, r[ 0], r[ 1], true);
	}
	// one failed document, and the one at the end of the buffers with its range one record past the count: empty in both modes
	{
		Batch bad = b;
		const int failed = 6;
		int last = 0, lastLex = 0;
		for (size_t d=0; d<NDOCS; ++d)
		{
			if (bad.range[ 2*d] + bad.range[ 2*d+1] == bad.results.size() && bad.range[ 2*d+1]) last = (int)d;
			if (bad.lexRange[ 2*d] + bad.lexRange[ 2*d+1] == bad.lexems.size() && bad.lexRange[ 2*d+1]) lastLex = (int)d;
		}
		CHECK( last != failed && lastLex != failed && bad.results.back().item_count == 0);
		bad.status[ failed] = 1;
		bad.results.pop_back(); bad.rf.pop_back();
		bad.lexems.pop_back();
		for (const auto& r : ranges)
		{
			for (int formats=0; formats<2; ++formats) for (int exclusive=0; exclusive<2; ++exclusive) checkMatchFetch( bad, r[ 0], r[ 1], formats != 0, exclusive != 0, failed, last);
			checkLexFetch( bad, r[ 0], r[ 1], false, failed, lastLex); checkLexFetch( bad, r[ 0], r[ 1], true, failed, lastLex);
		}
		checkMatchFetch( bad, last, 1, true, true, failed, last);
		checkLexFetch( bad, lastLex, 1, false, failed, lastLex);
		// only failed documents
		Batch none = b;
		none.status.assign( NDOCS, 3);
		for (const auto& r : ranges)
		{
			sp_match_batch_t out;
			std::memset( &out, 0, sizeof(out));
			CHECK( sp_match_batch_regroup( none.results.data(), none.results.size(), none.items.data(), none.items.size(), none.rf.data(), none.itf.data(),
							none.range.data(), none.status.data(), NDOCS, r[ 0], r[ 1], 1, 30, &out, 0, 0) == SP_OK);
			CHECK( out.ndocs == r[ 1] && out.nresults == 0 && out.nitems == 0 && out.doc_result_offsets[ r[ 1]] == 0 && (r[ 1] == 0 || out.doc_status[ 0] == 3));
			std::free( out.results); std::free( out.items); std::free( out.doc_result_offsets); std::free( out.doc_stats); std::free( out.doc_status);
			std::free( out.result_format); std::free( out.item_format);
			sp_lex_batch_t lout;
			std::memset( &lout, 0, sizeof(lout));
			fetchLexBatch( none.lexSource(), r[ 0], r[ 1], true, hostCopy, &lout);
			CHECK( lout.nlexems == 0 && lout.doc_lexem_offsets[ r[ 1]] == 0);
			std::free( lout.lexems); std::free( lout.doc_lexem_offsets); std::free( lout.doc_status);
		}
	}
	// an item block that ends outside the buffer is an error in both modes; a range outside the batch too
	{
		Batch bad = b;
		int last = -1;
		for (size_t d=0; d<NDOCS; ++d) for (uint64_t ri=0; ri<bad.range[ 2*d+1]; ++ri)
		{
			const sp_result_t& r = bad.results[ bad.range[ 2*d]+ri];
			if (r.item_count && r.item_begin + r.item_count == bad.items.size()) last = (int)d;
		}
		CHECK( last >= 0);
		bad.items.pop_back(); bad.itf.pop_back(); bad.itf.pop_back();
		sp_match_batch_t out;
		const char* msg = "item block of a document lies outside the device buffer";
		CHECK( throwsWith( msg, [&]{ fetchMatchBatch( bad.matchSource( true), 0, NDOCS, false, 30, hostCopy, &out); }));
		CHECK( throwsWith( msg, [&]{ fetchMatchBatch( bad.matchSource( true), last, 1, false, 30, hostCopy, &out); }));
		checkMatchFetch( bad, (last+1) % NDOCS, 1, true, false);
		const char* outside = "document range outside the last batch";
		CHECK( throwsWith( outside, [&]{ fetchMatchBatch( b.matchSource( false), NDOCS+1, 0, false, 30, hostCopy, &out); }));
		CHECK( throwsWith( outside, [&]{ fetchMatchBatch( b.matchSource( false), NDOCS-1, 2, false, 30, hostCopy, &out); }));
		sp_lex_batch_t lout;
		CHECK( throwsWith( outside, [&]{ fetchLexBatch( b.lexSource(), 1, NDOCS, false, hostCopy, &lout); }));
		char err[ 64];
		CHECK( sp_match_batch_regroup( b.results.data(), b.results.size(), b.items.data(), b.items.size(), 0, 0, b.range.data(), b.status.data(),
						NDOCS, NDOCS+1, 0, 0, 30, &out, err, sizeof(err)) == SP_ERR_INVALID && std::string( err) == outside);
	}
	// an empty batch
	{
		const Batch none = makeBatch( 0);
		checkMatchFetch( none, 0, 0, false, true);
		checkLexFetch( none, 0, 0, false); checkLexFetch( none, 0, 0, true);
	}
	std::printf( "batch fetch: ok\n");
	return 0;
}
