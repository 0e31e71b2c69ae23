// Stand-alone host program for a sanitizer run of the device-free twin of the segment lookups (csrc/match_segment.hpp) and,
// through it, of the walks that the device passes share (csrc/segment_walk.h): segments coded by hand, every answer compared with
// a pass over all entries, the refused tables, and hand-corrupted segments.  Every array is exactly as long as its content: a read
// behind one is the sanitizer's.  No HIP code is linked:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Istruspattern_amd/csrc \
//       tests/micro/match_segment_san.cpp struspattern_amd/csrc/match_segment.cpp struspattern_amd/csrc/match_postingblocks.cpp \
//       struspattern_amd/csrc/match_termblocks.cpp struspattern_amd/csrc/match_dictorder.cpp struspattern_amd/csrc/match_dict.cpp \
//       struspattern_amd/csrc/match_terms.cpp -o match_segment_san && ./match_segment_san
#include "match_segment.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK( cond) do { if (!(cond)) { std::fprintf( stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); std::exit( 1); } } while (0)

struct Posting { uint32_t doc, count; std::vector<uint32_t> positions; };
struct Entry { uint32_t handle; std::string value; uint64_t count; std::vector<Posting> list; };
struct Query { uint32_t handle; std::string value; };

static void put( std::string& out, uint64_t v)
{
	uint8_t buf[ 10];
	out.append( (const char*)buf, spa::writeVarint( buf, v));
}

// a segment over exactly sized arrays
struct Segment
{
	std::vector<uint8_t> termBytes, postingBytes;
	std::vector<uint64_t> termOffsets, postingOffsets;
	std::vector<uint32_t> handles;
	sp_match_term_blocks_t tb;
	sp_match_posting_blocks_t pb;

	Segment( const std::vector<std::string>& termBlocks, const std::vector<std::string>& postingBlocks, const std::vector<uint32_t>& handles_, size_t ndict, uint32_t B)
		:handles(handles_)
	{
		termOffsets.push_back( 0); postingOffsets.push_back( 0);
		for (const std::string& b : termBlocks) { termBytes.insert( termBytes.end(), b.begin(), b.end()); termOffsets.push_back( termBytes.size()); }
		for (const std::string& b : postingBlocks) { postingBytes.insert( postingBytes.end(), b.begin(), b.end()); postingOffsets.push_back( postingBytes.size()); }
		std::memset( &tb, 0, sizeof(tb)); std::memset( &pb, 0, sizeof(pb));
		tb.ndict = pb.ndict = ndict; tb.nblocks = pb.nblocks = handles.size(); tb.block_entries = pb.block_entries = B;
		tb.nbytes = termBytes.size(); tb.bytes = termBytes.data(); tb.block_offsets = termOffsets.data(); tb.block_handles = handles.data();
		pb.nbytes = postingBytes.size(); pb.bytes = postingBytes.data(); pb.block_offsets = postingOffsets.data();
	}
};

// the sorted entries coded as the two headers say
static Segment coded( const std::vector<Entry>& entries, uint32_t B)
{
	std::vector<std::string> termBlocks, postingBlocks;
	std::vector<uint32_t> handles;
	for (size_t k=0; k<entries.size(); ++k)
	{
		const Entry& e = entries[ k];
		const bool head = k % B == 0;
		if (head) { termBlocks.push_back( ""); postingBlocks.push_back( ""); handles.push_back( e.handle); }
		size_t shared = 0;
		if (!head && entries[ k-1].handle == e.handle)
		{
			const std::string& a = entries[ k-1].value;
			while (shared < a.size() && shared < e.value.size() && a[ shared] == e.value[ shared]) ++shared;
		}
		std::string& t = termBlocks.back();
		put( t, head ? 0 : e.handle - entries[ k-1].handle); put( t, shared); put( t, e.value.size() - shared); put( t, e.list.size()); put( t, e.count);
		t += e.value.substr( shared);
		std::string body;
		uint32_t doc = 0;
		for (size_t i=0; i<e.list.size(); ++i)
		{
			const Posting& x = e.list[ i];
			put( body, i ? x.doc - doc : x.doc); put( body, x.count); put( body, x.positions.size());
			doc = x.doc;
			for (size_t j=0; j<x.positions.size(); ++j) put( body, j ? x.positions[ j] - x.positions[ j-1] : x.positions[ j]);
		}
		put( postingBlocks.back(), body.size());
		postingBlocks.back() += body;
	}
	return Segment( termBlocks, postingBlocks, handles, entries.size(), B);
}

struct Lookup
{
	sp_segment_lookup_t out;
	char err[ 160];
	int rc;
	Lookup( const Segment& s, const std::vector<Query>& queries, uint32_t flags)
	{
		// exactly sized query arrays
		std::vector<uint32_t> handles;
		std::vector<uint64_t> offsets( 1, 0);
		std::vector<uint8_t> bytes;
		for (const Query& q : queries) { handles.push_back( q.handle); bytes.insert( bytes.end(), q.value.begin(), q.value.end()); offsets.push_back( bytes.size()); }
		rc = sp_match_segment_lookup( &s.tb, &s.pb, handles.data(), offsets.data(), bytes.data(), queries.size(), flags, &out, err, sizeof(err));
	}
	~Lookup() { sp_segment_lookup_free( &out); }
	bool empty() const { return !out.q_first && !out.selections && !out.values && out.nq == 0 && out.nsel == 0; }
};

static bool matches( const Entry& e, const Query& q, bool prefix)
{
	if (e.handle != q.handle) return false;
	return prefix ? e.value.compare( 0, q.value.size(), q.value) == 0 && e.value.size() >= q.value.size() : e.value == q.value;
}

static bool below( const Entry& e, const Query& q)
{
	if (e.handle != q.handle) return e.handle < q.handle;
	const size_t n = e.value.size() < q.value.size() ? e.value.size() : q.value.size();
	const int c = std::memcmp( e.value.data(), q.value.data(), n);
	return c < 0 || (c == 0 && e.value.size() < q.value.size());
}

// the answers are what going through all entries gives
static void answers( const std::vector<Entry>& entries, uint32_t B, const std::vector<Query>& queries, bool prefix)
{
	const Segment s = coded( entries, B);
	Lookup x( s, queries, prefix ? SP_LOOKUP_PREFIX : 0);
	CHECK( x.rc == SP_OK && x.out.nq == queries.size());
	uint64_t sel = 0, np = 0, nq = 0, nv = 0;
	for (size_t i=0; i<queries.size(); ++i)
	{
		size_t first = 0;
		while (first < entries.size() && below( entries[ first], queries[ i])) ++first;
		size_t end = first;
		while (end < entries.size() && matches( entries[ end], queries[ i], prefix)) ++end;
		CHECK( x.out.q_status[ i] == 0 && x.out.q_first[ i] == first && x.out.q_count[ i] == end - first && x.out.q_sel_offsets[ i] == sel);
		for (size_t k=first; k<end; ++k, ++sel)
		{
			const Entry& e = entries[ k];
			const sp_segment_selection_t& r = x.out.selections[ sel];
			CHECK( r.position == k && r.handle == e.handle && r.doc_freq == e.list.size() && r.value_bytes == e.value.size() && r.count == e.count);
			CHECK( x.out.sel_value_offsets[ sel] == nv && x.out.sel_posting_offsets[ sel] == np);
			CHECK( std::memcmp( x.out.values + nv, e.value.data(), e.value.size()) == 0);
			nv += e.value.size();
			for (const Posting& p : e.list)
			{
				const sp_segment_posting_t& g = x.out.postings[ np];
				CHECK( g.doc == p.doc && g.count == p.count && g.npos == p.positions.size() && g.reserved == 0 && x.out.posting_position_offsets[ np] == nq);
				for (uint32_t pos : p.positions) CHECK( x.out.positions[ nq++] == pos);
				++np;
			}
		}
	}
	CHECK( x.out.q_sel_offsets[ queries.size()] == sel && x.out.nsel == sel && x.out.npostings == np && x.out.npositions == nq && x.out.nvalue_bytes == nv);
	CHECK( x.out.sel_value_offsets[ sel] == nv && x.out.sel_posting_offsets[ sel] == np && x.out.posting_position_offsets[ np] == nq);
	CHECK( x.out.totals[ 0] == sel && x.out.totals[ 1] == np && x.out.totals[ 2] == nq && x.out.totals[ 3] == nv);
}

static std::vector<Entry> numbered( int n)
{
	std::vector<Entry> entries;
	const uint32_t handles[] = { 1, 2, 5};
	for (uint32_t h : handles)
	{
		for (int k=0; k<n; ++k)
		{
			char name[ 32];
			std::snprintf( name, sizeof(name), "t%02d%s%c", k / 5, k % 3 ? "xy" : "", 'a' + k % 5);
			Entry e = { h, name, (uint64_t)k + 1, {}};
			if (k == 7) e.value += std::string( 200, '\xff');
			for (int d=0; d<1+k%3; ++d)
			{
				Posting p = { (uint32_t)(130 * d + k % 4), (uint32_t)(k % 3 + 1) + (k == 9 ? 200u : 0u), {}};
				for (int i=0; i<k%3+1; ++i) p.positions.push_back( (uint32_t)(k + i * (k == 9 ? 20000 : 3)));
				e.list.push_back( p);
			}
			entries.push_back( e);
		}
	}
	// sorted by (handle, value)
	for (size_t i=0; i<entries.size(); ++i) for (size_t j=i+1; j<entries.size(); ++j)
	{
		const Query q = { entries[ i].handle, entries[ i].value };
		if (below( entries[ j], q)) std::swap( entries[ i], entries[ j]);
	}
	return entries;
}

static void shapes()
{
	for (uint32_t B : { 1u, 2u, 16u, 64u})
	{
		for (int n : { 0, 1, 5, 23})
		{
			const std::vector<Entry> entries = numbered( n);
			std::vector<Query> queries = { { 0, ""}, { 0, "t"}, { 1, ""}, { 3, ""}, { 5, "zz"}, { 9, ""}, { 2, "t0"}, { 2, "t00"}, { 5, std::string( 1, '\xff')}, { 1, std::string( 1, '\0')} };
			for (const Entry& e : entries)
			{
				queries.push_back( Query{ e.handle, e.value});
				queries.push_back( Query{ e.handle, e.value.substr( 0, e.value.size() - 1)});
				queries.push_back( Query{ e.handle, e.value + std::string( 1, '\0')});
				queries.push_back( Query{ e.handle + 1, e.value});
			}
			answers( entries, B, queries, false);
			answers( entries, B, queries, true);
			answers( entries, B, {}, true);
		}
	}
}

static void refusedTables()
{
	const std::vector<Entry> entries = numbered( 12);
	void (*damages[])( Segment&) = {
		[]( Segment& s) { s.pb.ndict -= 1; },
		[]( Segment& s) { s.pb.nblocks -= 1; },
		[]( Segment& s) { s.pb.block_entries = 8; },
		[]( Segment& s) { s.tb.block_entries = s.pb.block_entries = 3; },
		[]( Segment& s) { s.tb.block_entries = s.pb.block_entries = 128; },
		[]( Segment& s) { s.tb.ndict = s.pb.ndict = 16; },
		[]( Segment& s) { s.termOffsets[ 1] = s.termOffsets[ 2] + 1; },
		[]( Segment& s) { s.postingOffsets[ 1] = s.postingOffsets[ 2]; },
		[]( Segment& s) { s.termOffsets[ 0] = 1; },
		[]( Segment& s) { s.tb.nbytes -= 1; },
		[]( Segment& s) { s.pb.nbytes += 1; },
		[]( Segment& s) { s.handles[ 1] = s.handles[ 2] + 1; },
		[]( Segment& s) { s.tb.block_offsets = 0; },
		[]( Segment& s) { s.pb.bytes = 0; },
	};
	for (auto damage : damages)
	{
		Segment bad = coded( entries, 16);
		damage( bad);
		Lookup x( bad, { { 1, "t00a"}}, 0);
		CHECK( x.rc == SP_ERR_INVALID && x.err[ 0] && x.empty());
	}
	const Segment good = coded( entries, 16);
	sp_segment_lookup_t out;
	char err[ 8];
	const uint32_t handle = 1;
	const uint64_t descending[] = { 2, 1}, flat[] = { 0, 0};
	CHECK( sp_match_segment_lookup( &good.tb, 0, &handle, flat, 0, 1, 0, &out, err, sizeof(err)) == SP_ERR_INVALID && std::strlen( err) == 7);	// (the message is cut to the buffer)
	CHECK( sp_match_segment_lookup( &good.tb, &good.pb, &handle, descending, (const uint8_t*)"ab", 1, 0, &out, 0, 0) == SP_ERR_INVALID);
	CHECK( sp_match_segment_lookup( &good.tb, &good.pb, &handle, flat, 0, 1, 2, &out, 0, 0) == SP_ERR_INVALID);
	CHECK( sp_match_segment_lookup( &good.tb, &good.pb, &handle, flat, 0, 1, SP_LOOKUP_PREFIX, &out, 0, 0) == SP_OK && out.q_count[ 0] == 12);
	sp_segment_lookup_free( &out);
}

// the arrays are as long as the totals say
static void consistent( const sp_segment_lookup_t& o)
{
	CHECK( o.totals[ 0] == o.nsel && o.totals[ 1] == o.npostings && o.totals[ 2] == o.npositions && o.totals[ 3] == o.nvalue_bytes);
	CHECK( o.q_sel_offsets[ o.nq] == o.nsel && o.sel_value_offsets[ o.nsel] == o.nvalue_bytes && o.sel_posting_offsets[ o.nsel] == o.npostings);
	CHECK( o.posting_position_offsets[ o.npostings] == o.npositions);
}

static void corruptedSegments()
{
	const std::string goodTerms = std::string( "\0\0\2\1\1ab", 7) + std::string( "\0\1\1\1\1c", 6), goodLists = std::string( "\4\0\1\1\1", 5) + std::string( "\x09\2\3\2\5\4\2\1\1\1", 10);
	const std::vector<Query> queries = { { 1, "b"}, { 1, "ac"}, { 1, "ab"}, { 1, ""}, { 0, "x"}, { 2, ""} };
	{
		const Segment s( { goodTerms, std::string( "\0\0\1\1\1b", 6)}, { goodLists, std::string( "\4\7\2\1\3", 5)}, { 1, 1}, 3, 2);
		for (uint32_t flags : { 0u, SP_LOOKUP_PREFIX})
		{
			Lookup x( s, queries, flags);
			CHECK( x.rc == SP_OK && x.out.nsel == (flags ? 6u : 3u) && x.out.npostings == (flags ? 8u : 4u));
			for (size_t i=0; i<queries.size(); ++i) CHECK( x.out.q_status[ i] == 0);
			consistent( x.out);
		}
	}
	const std::string badTerms[] = {
		std::string( "\0\0\2\1\1ab", 7) + std::string( "\0\1\1\1\x80", 5), std::string( "\0\0\2\1", 4), std::string( ""), std::string( "\0\0\2\1\1a", 6),
		std::string( "\0\0\2\1", 4) + std::string( 10, '\x80') + std::string( "\1ab", 3), std::string( "\0\0\2\1", 4) + std::string( 9, '\xff') + std::string( "\2ab", 3),
		std::string( "\0\1\1\1\1b", 6), std::string( "\1\0\1\1\1b", 6),
		std::string( "\0\0\2\1\1ab", 7) + std::string( "\0\3\1\1\1c", 6),
		std::string( "\0\0\2\1\1ab", 7) + std::string( "\0\1\5\1\1c", 6), std::string( "\0\0\7\1\1ab", 7),
		std::string( "\0\0\2\1\1ab", 7) + std::string( 9, '\xff') + std::string( "\1\1\1\1\1c", 6),
		std::string( "\0\0\2\1\1ab", 7) + std::string( "\xff\xff\xff\xff\x0f\1\1\1\1c", 10),
		std::string( "\0\0\2\xff\xff\xff\xff\x1f\1ab", 11) + std::string( "\0\1\1\1\1c", 6),
	};
	for (const std::string& terms : badTerms)
	{
		// (an empty block is what the tables refuse: the twin reads it only where a later block makes the offsets ascend)
		if (terms.empty()) continue;
		const Segment s( { terms}, { goodLists}, { 1}, 2, 16);
		for (uint32_t flags : { 0u, SP_LOOKUP_PREFIX})
		{
			Lookup x( s, queries, flags);
			CHECK( x.rc == SP_OK && x.out.nsel <= 1 && x.out.npostings <= 1 && x.out.nvalue_bytes <= 2);
			// ("b" and "ac" walk the whole block; an exact "ab" ends at the head, a prefix run looks for its end behind it)
			for (size_t i=0; i<(flags ? 4u : 2u); ++i) CHECK( x.out.q_status[ i] != 0 && x.out.q_count[ i] == 0 && x.out.q_first[ i] == 0);
			consistent( x.out);
		}
	}
	const std::string badLists[] = {
		std::string( "\4\0\1\1\x80", 5), std::string( "\x80", 1), std::string( 10, '\x80') + std::string( "\1\0\1\1\1", 5), std::string( 9, '\xff') + std::string( "\2\0\1\1\1", 5),
		std::string( "\5\0\1\1\1", 5), std::string( 9, '\xff') + std::string( "\1\0\1\1\1", 5), std::string( "\0", 1),
		std::string( "\3\0\1\1\1", 5), std::string( "\4\0\2\2\1\4\0\1\1\1", 10), std::string( "\2\0\1\1\1", 5),
		std::string( "\x08\2\1\1\5\0\1\1\1", 9), std::string( "\5\0\2\2\5\0", 6),
		std::string( "\3\0\1\0", 4), std::string( "\5\0\1\2\5\1", 6),
		std::string( "\x08\xff\xff\xff\xff\x1f\1\1\1", 9), std::string( "\x08\0\xff\xff\xff\xff\x1f\1\1", 9),
		std::string( "\x08\0\1\1\xff\xff\xff\xff\x1f", 9), std::string( "\x09\0\2\2\xff\xff\xff\xff\x0f\1", 10),
	};
	for (const std::string& bad : badLists) for (bool badFirst : { false, true})
	{
		const std::string lists0 = badFirst ? bad + std::string( "\4\0\1\1\1", 5) : std::string( "\4\0\1\1\1", 5) + bad;
		const Segment s( { goodTerms, std::string( "\0\0\1\1\1b", 6)}, { lists0, std::string( "\4\7\2\1\3", 5)}, { 1, 1}, 3, 2);
		for (uint32_t flags : { 0u, SP_LOOKUP_PREFIX})
		{
			Lookup x( s, queries, flags);
			CHECK( x.rc == SP_OK && x.out.q_status[ 0] == 0 && x.out.q_count[ 0] == 1 && x.out.q_count[ 1] == 1 && x.out.q_count[ 2] == 1);
			CHECK( x.out.q_status[ badFirst ? 2 : 1] != 0);
			if (!badFirst) CHECK( x.out.q_status[ 2] == 0);
			const sp_segment_selection_t& r = x.out.selections[ badFirst ? 2 : 1];
			CHECK( r.position == (badFirst ? 0u : 1u) && r.handle == 0 && r.doc_freq == 0 && r.value_bytes == 0 && r.count == 0);
			CHECK( x.out.sel_posting_offsets[ badFirst ? 2 : 1] == x.out.sel_posting_offsets[ badFirst ? 3 : 2]);
			if (flags) CHECK( x.out.q_status[ 3] != 0 && x.out.q_count[ 3] == 3);
			consistent( x.out);
		}
	}
	// block offsets inside the tables' rules that cut a code in two: the walk ends at the end of its block
	{
		Segment s( { goodTerms.substr( 0, 9), goodTerms.substr( 9) + std::string( "\0\0\1\1\1b", 6)}, { goodLists.substr( 0, 7), goodLists.substr( 7) + std::string( "\4\7\2\1\3", 5)}, { 1, 1}, 3, 2);
		for (uint32_t flags : { 0u, SP_LOOKUP_PREFIX})
		{
			Lookup x( s, queries, flags);
			CHECK( x.rc == SP_OK);
			consistent( x.out);
		}
	}
}

int main()
{
	shapes();
	refusedTables();
	corruptedSegments();
	std::printf( "match_segment_san: ok\n");
	return 0;
}
