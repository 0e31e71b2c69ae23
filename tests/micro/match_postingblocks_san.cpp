// Stand-alone host program for a sanitizer run of the device-free twin of the posting blocks and of their reader
// (csrc/match_postingblocks.hpp) over hand-made dictionaries, orders, postings and positions, the refused inputs and malformed
// blocks.  Every array is exactly as long as its content: a read behind one is the sanitizer's.  No HIP code is linked:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Istruspattern_amd/csrc \
//       tests/micro/match_postingblocks_san.cpp struspattern_amd/csrc/match_postingblocks.cpp struspattern_amd/csrc/match_termblocks.cpp \
//       struspattern_amd/csrc/match_dictorder.cpp struspattern_amd/csrc/match_dict.cpp struspattern_amd/csrc/match_terms.cpp \
//       -o match_postingblocks_san && ./match_postingblocks_san
#include "match_postingblocks.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#define CHECK( cond) do { if (!(cond)) { std::fprintf( stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); std::exit( 1); } } while (0)

struct Posting { uint32_t doc, count; std::vector<uint32_t> positions; };
typedef std::vector<Posting> List;

// a dictionary, its order (the entries in reverse), its postings and their positions made of the lists of the entries
struct Inputs
{
	std::vector<sp_dict_term_t> records;
	std::vector<uint32_t> order, npos;
	std::vector<sp_posting_t> postings;
	std::vector<uint64_t> entryOffsets, postingOffsets;
	std::vector<sp_occurrence_t> occurrences;
	sp_match_dictionary_t d;
	sp_match_dictionary_order_t o;
	sp_match_postings_t q;
	sp_match_positions_t p;
	sp_match_posting_blocks_t b;
	char err[ 160];

	explicit Inputs( const std::vector<List>& lists)
	{
		entryOffsets.push_back( 0); postingOffsets.push_back( 0);
		for (size_t e=0; e<lists.size(); ++e)
		{
			sp_dict_term_t rec;
			std::memset( &rec, 0, sizeof(rec));
			rec.handle = 1; rec.doc_freq = (uint32_t)lists[ e].size();
			records.push_back( rec);
			order.push_back( (uint32_t)(lists.size() - 1 - e));
			for (const Posting& x : lists[ e])
			{
				const sp_posting_t posting = { x.doc, 0, x.count, x.positions.empty() ? 0 : x.positions[ 0] };
				postings.push_back( posting);
				for (size_t i=0; i<x.positions.size(); ++i) { const sp_occurrence_t occ = { x.positions[ i], (uint32_t)i }; occurrences.push_back( occ); }
				postingOffsets.push_back( occurrences.size());
				npos.push_back( (uint32_t)std::set<uint32_t>( x.positions.begin(), x.positions.end()).size());
			}
			entryOffsets.push_back( postings.size());
		}
		std::memset( &d, 0, sizeof(d)); std::memset( &o, 0, sizeof(o)); std::memset( &q, 0, sizeof(q)); std::memset( &p, 0, sizeof(p)); std::memset( &b, 0, sizeof(b));
		d.ndict = o.ndict = q.ndict = lists.size(); d.records = records.data(); o.order = order.data();
		q.nterms = p.nterms = postings.size(); q.postings = postings.data(); q.entry_offsets = entryOffsets.data();
		p.nocc = occurrences.size(); p.occurrences = occurrences.data(); p.posting_offsets = postingOffsets.data(); p.posting_positions = npos.data();
	}
	~Inputs() { sp_match_posting_blocks_free( &b); }
	int run() { sp_match_posting_blocks_free( &b); return sp_match_batch_posting_blocks( &d, &o, &q, &p, &b, err, sizeof(err)); }
	bool empty() const { return !b.bytes && !b.block_offsets && b.ndict == 0 && b.nblocks == 0 && b.nbytes == 0 && b.totals[ 1] == 0; }
	// every block decodes to the lists of its sorted positions
	void decodes( const std::vector<List>& lists)
	{
		CHECK( run() == SP_OK && b.ndict == lists.size() && b.totals[ 0] == b.nblocks && b.totals[ 1] == b.nbytes && b.block_offsets[ b.nblocks] == b.nbytes);
		size_t k = 0;
		uint64_t gaps = 0;
		for (size_t j=0; j<b.nblocks; ++j)
		{
			size_t nl = 0, np = 0, nq = 0;
			char e[ 100];
			CHECK( sp_match_posting_blocks_decode_block( &b, j, 0, 0, 0, 0, 0, 0, &nl, &np, &nq, e, sizeof(e)) == SP_OK && nl >= 1 && nl <= b.block_entries);
			std::vector<uint32_t> inList( nl), positions( nq);
			std::vector<sp_block_posting_t> found( np);
			CHECK( sp_match_posting_blocks_decode_block( &b, j, inList.data(), nl, found.data(), np, positions.data(), nq, &nl, &np, &nq, e, sizeof(e)) == SP_OK);
			size_t at = 0;
			for (size_t i=0; i<nl; ++i, ++k)
			{
				const List& want = lists[ lists.size() - 1 - k];
				CHECK( inList[ i] == want.size());
				for (const Posting& x : want)
				{
					const std::set<uint32_t> distinct( x.positions.begin(), x.positions.end());
					const sp_block_posting_t& f = found[ at++];
					CHECK( f.doc == x.doc && f.count == x.count && f.npos == distinct.size() && f.position_offset + f.npos <= nq);
					CHECK( std::vector<uint32_t>( distinct.begin(), distinct.end()) == std::vector<uint32_t>( positions.begin() + f.position_offset, positions.begin() + f.position_offset + f.npos));
					gaps += f.npos;
				}
			}
			CHECK( at == np);
			if (np > 1) CHECK( sp_match_posting_blocks_decode_block( &b, j, inList.data(), nl, found.data(), np - 1, positions.data(), nq, &nl, &np, &nq, e, sizeof(e)) == SP_ERR_INVALID);
			if (nq > 1) CHECK( sp_match_posting_blocks_decode_block( &b, j, inList.data(), nl, found.data(), np, positions.data(), nq - 1, &nl, &np, &nq, e, sizeof(e)) == SP_ERR_INVALID);
		}
		CHECK( k == lists.size() && gaps == b.totals[ 3]);
	}
};

static std::vector<List> numbered( int n)
{
	std::vector<List> lists;
	for (int e=0; e<n; ++e)
	{
		List list;
		for (int d=0; d<1+e%3; ++d)
		{
			Posting x = { (uint32_t)(7*d + e%5), (uint32_t)(e%4 + 1), {} };
			for (int i=0; i<e%4+1; ++i) x.positions.push_back( (uint32_t)(3 + e + (i/2) * (e%9 + 1)) * (e % 11 == 10 ? 40000u : 1u));
			list.push_back( x);
		}
		lists.push_back( list);
	}
	return lists;
}

static void shapes()
{
	const uint32_t M = 0xFFFFFFFFu;
	for (unsigned B : { 0u, 1u, 4u, 64u})
	{
		sp_test_term_block_entries( B);
		{ Inputs x( {}); x.decodes( {}); CHECK( x.b.nblocks == 0 && x.b.nbytes == 0 && x.b.block_offsets[ 0] == 0 && x.b.totals[ 2] == (B ? B : 16)); }
		{
			const std::vector<List> one = { { { 0, 1, { 1}}}};
			Inputs x( one); x.decodes( one);
			CHECK( x.b.nblocks == 1 && x.b.nbytes == 5 && std::memcmp( x.b.bytes, "\4\0\1\1\1", 5) == 0);
		}
		for (int n : { 3, 4, 5, 13, 64, 65, 200}) { const std::vector<List> lists = numbered( n); Inputs x( lists); x.decodes( lists); }
		// wide varints: a count of 2^32 - 1, documents and positions at 2^32 - 1, a body of two and of three bytes
		std::vector<List> wide = { { { M - 1, M, { M - 1, M - 1, M}}, { M, 2, { M}}}, { { 3, 3, { 5, 132, 133 + (1u << 28)}}}, {}, {}};
		for (uint32_t d=1; d<=40; ++d) wide[ 2].push_back( Posting{ d, 1, { 9}});
		for (uint32_t d=1; d<=5000; ++d) wide[ 3].push_back( Posting{ 3*d, 1, { d}});
		Inputs x( wide); x.decodes( wide);
	}
	sp_test_term_block_entries( 0);
}

static void refusedInputs()
{
	const std::vector<List> lists = { { { 2, 3, { 5, 5, 9}}, { 4, 1, { 1}}}, { { 0, 2, { 7, 7}}}};
	{ Inputs good( lists); good.decodes( lists); }
	void (*damages[])( Inputs&) = {
		[]( Inputs& x) { x.o.ndict = 1; },
		[]( Inputs& x) { x.q.ndict = 1; },
		[]( Inputs& x) { x.p.nterms = 2; },
		[]( Inputs& x) { x.order[ 0] = 0; },
		[]( Inputs& x) { x.order[ 0] = 2; },
		[]( Inputs& x) { x.order[ 1] = 0xFFFFFFFFu; },
		[]( Inputs& x) { x.entryOffsets[ 2] = 2; },
		[]( Inputs& x) { x.entryOffsets[ 1] = 4; },
		[]( Inputs& x) { x.entryOffsets[ 0] = 1; },
		[]( Inputs& x) { x.records[ 0].doc_freq = 1; },
		[]( Inputs& x) { x.postingOffsets[ 3] = 5; },
		[]( Inputs& x) { x.postingOffsets[ 1] = 7; },
		[]( Inputs& x) { x.postings[ 1].count = 0; },
		[]( Inputs& x) { x.postingOffsets[ 2] = 3; },
		[]( Inputs& x) { x.postings[ 1].doc = 2; },
		[]( Inputs& x) { x.occurrences[ 2].ordpos = 4; },
		[]( Inputs& x) { x.npos[ 0] = 0; },
		[]( Inputs& x) { x.npos[ 0] = 4; },
		[]( Inputs& x) { x.npos[ 0] = 3; },
	};
	for (auto damage : damages)
	{
		Inputs bad( lists);
		damage( bad);
		CHECK( bad.run() == SP_ERR_INVALID && bad.err[ 0] && bad.empty());
	}
	Inputs good( lists);
	sp_match_posting_blocks_t out;
	char err[ 8];
	CHECK( sp_match_batch_posting_blocks( &good.d, &good.o, &good.q, 0, &out, err, sizeof(err)) == SP_ERR_INVALID && std::strlen( err) == 7);	// (the message is cut to the buffer)
	CHECK( sp_match_batch_posting_blocks( 0, &good.o, &good.q, &good.p, &out, 0, 0) == SP_ERR_INVALID);
}

// a block made by hand (exactly as long as its bytes)
static int decodeBytes( const std::string& data, size_t* nl, size_t* np, size_t* nq)
{
	std::vector<uint8_t> bytes( data.begin(), data.end());
	uint64_t offsets[ 2] = { 0, bytes.size()};
	sp_match_posting_blocks_t pb;
	std::memset( &pb, 0, sizeof(pb));
	pb.nblocks = 1; pb.nbytes = bytes.size(); pb.block_entries = 16; pb.bytes = bytes.data(); pb.block_offsets = offsets;
	uint32_t lists[ 16], positions[ 64];
	sp_block_posting_t postings[ 32];
	char err[ 100];
	return sp_match_posting_blocks_decode_block( &pb, 0, lists, 16, postings, 32, positions, 64, nl, np, nq, err, sizeof(err));
}

static void malformedBlocks()
{
	size_t nl = 0, np = 0, nq = 0;
	CHECK( decodeBytes( std::string( "\x09\2\3\2\5\4\2\1\1\1", 10), &nl, &np, &nq) == SP_OK && nl == 1 && np == 2 && nq == 3);
	const std::string bad[] = {
		std::string( "\4\0\1\1\x80", 5), std::string( "\x80", 1),				// a varint that runs past the block
		std::string( 10, '\x80') + std::string( "\1\0\1\1\1", 5),				// a varint longer than ten bytes
		std::string( 9, '\xff') + std::string( "\2\0\1\1\1", 5),
		std::string( "\5\0\1\1\1", 5), std::string( 9, '\xff') + std::string( "\1\0\1\1\1", 5),	// a body past the block
		std::string( "\0", 1),
		std::string( "\3\0\1\1\1", 5), std::string( "\4\0\2\2\1\4\0\1\1\1", 10), std::string( "\2\0\1\1\1", 5),	// a posting beyond its body
		std::string( "\x08\2\1\1\5\0\1\1\1", 9),						// a ddelta of 0
		std::string( "\5\0\2\2\5\0", 6),							// a gap of 0
		std::string( "\3\0\1\0", 4), std::string( "\5\0\1\2\5\1", 6),				// npos 0, npos above count
		std::string( "\x08\xff\xff\xff\xff\x1f\1\1\1", 9), std::string( "\x08\0\xff\xff\xff\xff\x1f\1\1", 9),	// 32 bits
		std::string( "\x08\0\1\1\xff\xff\xff\xff\x1f", 9), std::string( "\x09\0\2\2\xff\xff\xff\xff\x0f\1", 10),
		std::string( ""),
	};
	for (const std::string& data : bad) CHECK( decodeBytes( data, &nl, &np, &nq) == SP_ERR_INVALID);
	std::string many;
	for (int k=0; k<17; ++k) many += std::string( "\4\0\1\1\1", 5);
	CHECK( decodeBytes( many, &nl, &np, &nq) == SP_ERR_INVALID);
}

int main()
{
	shapes();
	refusedInputs();
	malformedBlocks();
	std::printf( "match_postingblocks_san: ok\n");
	return 0;
}
