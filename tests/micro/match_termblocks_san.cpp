// Stand-alone host program for a sanitizer run of the device-free twin of the term blocks and of their reader
// (csrc/match_termblocks.hpp) over edge batches of tests/test_termblocks_abi.py, the refused orders and malformed blocks.  The
// terms, the dictionary and the order come from their twins.  No HIP code is linked:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Istruspattern_amd/csrc \
//       tests/micro/match_termblocks_san.cpp struspattern_amd/csrc/match_termblocks.cpp struspattern_amd/csrc/match_dictorder.cpp \
//       struspattern_amd/csrc/match_dict.cpp struspattern_amd/csrc/match_terms.cpp -o match_termblocks_san && ./match_termblocks_san
#include "match_termblocks.hpp"
#include "finished_batch_fixture.hpp"
#include <string>
#include <vector>

// the terms of a batch, their dictionary and its order by the twins, and the blocks of that
struct Blocks
{
	sp_match_batch_t mb;
	sp_match_text_t x;
	sp_match_values_t v;
	sp_match_terms_t t;
	sp_match_dictionary_t d;
	sp_match_dictionary_order_t o;
	sp_match_term_blocks_t b;
	char err[ 160];
	int rc;
	Blocks( Batch& batch, uint32_t bound, uint32_t flags = SP_TERM_TEXT, void (*damage)( Blocks&) = 0)
	{
		mb = batch.view(); x = batch.textView(); v = batch.valuesView();
		const sp_match_values_t* values = (flags & SP_TERM_VALUES) ? &v : 0;
		const sp_match_text_t* text = (flags & SP_TERM_TEXT) ? &x : 0;
		CHECK( sp_match_batch_terms( &mb, values, text, bound, flags, &t, err, sizeof(err)) == SP_OK);
		CHECK( sp_match_batch_dictionary( &mb, values, text, &t, &d, err, sizeof(err)) == SP_OK);
		CHECK( sp_match_batch_dictionary_order( &mb, values, text, &t, &d, &o, err, sizeof(err)) == SP_OK);
		if (damage) damage( *this);
		rc = sp_match_batch_term_blocks( &mb, values, text, &t, &d, &o, &b, err, sizeof(err));
	}
	~Blocks() { sp_match_term_blocks_free( &b); sp_match_dictionary_order_free( &o); sp_match_dictionary_free( &d); sp_match_terms_free( &t); }
	bool empty() const { return !b.bytes && !b.block_offsets && !b.block_handles && b.ndict == 0 && b.nblocks == 0 && b.nbytes == 0 && b.totals[ 1] == 0; }
	// every block decodes, to as many entries as the dictionary has, handles ascending, doc_freq and count those of the entry
	void decodes() const
	{
		CHECK( rc == SP_OK && b.ndict == d.ndict && b.totals[ 0] == b.nblocks && b.totals[ 1] == b.nbytes && b.block_offsets[ b.nblocks] == b.nbytes);
		uint64_t k = 0, valueBytes = 0;
		for (size_t j=0; j<b.nblocks; ++j)
		{
			size_t n = 0, nv = 0;
			char e[ 80];
			CHECK( sp_match_term_blocks_decode_block( &b, j, 0, 0, 0, 0, &n, &nv, e, sizeof(e)) == SP_OK && n >= 1 && n <= b.block_entries);
			std::vector<sp_term_block_entry_t> entries( n);
			std::vector<uint8_t> values( nv + 1);
			CHECK( sp_match_term_blocks_decode_block( &b, j, entries.data(), n, values.data(), nv, &n, &nv, e, sizeof(e)) == SP_OK);
			CHECK( entries[ 0].handle == b.block_handles[ j] && b.block_offsets[ j] < b.block_offsets[ j+1]);
			for (size_t i=0; i<n; ++i, ++k)
			{
				const sp_dict_term_t& entry = d.records[ o.order[ k]];
				CHECK( entries[ i].handle == entry.handle && entries[ i].value_bytes == entry.value_bytes && entries[ i].doc_freq == entry.doc_freq && entries[ i].count == entry.count);
				CHECK( entries[ i].value_offset + entries[ i].value_bytes <= nv);
				valueBytes += entry.value_bytes;
			}
			if (n > 1) CHECK( sp_match_term_blocks_decode_block( &b, j, entries.data(), n - 1, values.data(), nv, &n, &nv, e, sizeof(e)) == SP_ERR_INVALID);
		}
		CHECK( k == d.ndict && valueBytes == b.totals[ 3]);
	}
};

static void shapes()
{
	for (unsigned B : { 0u, 1u, 4u, 64u})
	{
		sp_test_term_block_entries( B);
		{ Batch b; Blocks q( b, 3); q.decodes(); CHECK( q.b.nblocks == 0 && q.b.nbytes == 0 && q.b.block_offsets[ 0] == 0 && q.b.totals[ 2] == (B ? B : 16)); }
		{ Batch b; b.document(); b.document(); Blocks q( b, 3); q.decodes(); CHECK( q.b.ndict == 0); }
		Batch b;
		b.result( 2, "only"); b.document(); b.result( 2, "only"); b.document();
		Blocks q( b, 3);
		q.decodes();
		CHECK( q.b.nblocks == 1 && q.b.nbytes == 9 && std::memcmp( q.b.bytes, "\0\0\4\2\2only", 9) == 0 && q.b.block_handles[ 0] == 2);
		// ndict at the block edges, prefixes and long values
		for (int n : { 3, 4, 5, 13, 64, 65, 200})
		{
			Batch c;
			for (int k=0; k<n; ++k)
			{
				char value[ 16];
				std::snprintf( value, sizeof(value), "t%06d", (k * 37) % n);
				c.result( 1 + k % 3, std::string( value) + std::string( (size_t)(k % 5) * 40, 'x'));
				if (k % 7 == 6) c.document();
			}
			c.result( 2, std::string( 20000, 'y')); c.result( 2, std::string( 16384, 'y') + "z"); c.result( 2, ""); c.document();
			Blocks r( c, 4);
			r.decodes();
			CHECK( r.b.nblocks == (r.d.ndict + r.b.block_entries - 1) / r.b.block_entries);
		}
	}
	sp_test_term_block_entries( 0);
}

static void bothSources()
{
	Batch b;
	b.result( 1, "?", "usd", 1); b.result( 1, "eur", "", 0); b.result( 2, "c", "", 0); b.document();
	b.result( 2, "?", "b", 1); b.result( 2, "a", "", 0); b.result( 2, "?", "", 1); b.document();
	Blocks q( b, 3, SP_TERM_VALUES | SP_TERM_TEXT);
	q.decodes();
	CHECK( q.b.ndict == 6 && q.b.nblocks == 1);
}

static void refusedArguments()
{
	Batch b;
	b.result( 1, "c"); b.result( 1, "ab"); b.result( 2, "a"); b.document();
	b.result( 1, "abc"); b.result( 1, "a"); b.result( 1, "ab"); b.result( 2, "d"); b.document();
	{ Blocks good( b, 3); good.decodes(); CHECK( good.b.ndict == 6 && good.o.prefix_bytes[ 1] == 1 && good.o.prefix_bytes[ 2] == 2); }
	void (*damages[])( Blocks&) = {
		[]( Blocks& q) { q.d.nterms -= 1; },
		[]( Blocks& q) { q.d.records[ 1].handle = 0; },
		[]( Blocks& q) { q.d.records[ 0].first_doc = 0xFFFFFFFFu; },
		[]( Blocks& q) { q.d.handle_terms[ 2] = 1; },
		[]( Blocks& q) { q.x.totals[ 0] -= 1; },
		[]( Blocks& q) { q.o.ndict -= 1; },
		[]( Blocks& q) { q.o.handle_bound += 1; },
		[]( Blocks& q) { q.o.order[ 2] = q.o.order[ 1]; },
		[]( Blocks& q) { q.o.order[ 0] = 6; },
		[]( Blocks& q) { q.o.order[ 0] = 0xFFFFFFFFu; },
		[]( Blocks& q) { const uint32_t e = q.o.order[ 3]; q.o.order[ 3] = q.o.order[ 4]; q.o.order[ 4] = e; },
		[]( Blocks& q) { q.o.prefix_bytes[ 1] = 2; },
		[]( Blocks& q) { q.o.prefix_bytes[ 2] = 0xFFFFFFFFu; },
		[]( Blocks& q) { q.o.prefix_bytes[ 2] = 1; },
		[]( Blocks& q) { q.o.prefix_bytes[ 4] = 1; },
	};
	for (auto damage : damages)
	{
		Blocks bad( b, 3, SP_TERM_TEXT, damage);
		CHECK( bad.rc == SP_ERR_INVALID && bad.err[ 0] && bad.empty());
	}
	Blocks good( b, 3);
	sp_match_term_blocks_t out;
	char err[ 8];
	CHECK( sp_match_batch_term_blocks( &good.mb, 0, 0, &good.t, &good.d, &good.o, &out, err, sizeof(err)) == SP_ERR_INVALID && std::strlen( err) == 7);	// (the message is cut to the buffer)
	CHECK( sp_match_batch_term_blocks( 0, 0, &good.x, &good.t, &good.d, &good.o, &out, 0, 0) == SP_ERR_INVALID);
	CHECK( sp_match_batch_term_blocks( &good.mb, 0, &good.x, &good.t, &good.d, 0, &out, 0, 0) == SP_ERR_INVALID);
}

// a block made by hand (exactly as long as its bytes: a read behind them is the sanitizer's)
static int decodeBytes( const std::string& data, size_t* n, size_t* nv)
{
	std::vector<uint8_t> bytes( data.begin(), data.end());
	uint64_t offsets[ 2] = { 0, bytes.size()};
	uint32_t handles[ 1] = { 1};
	sp_match_term_blocks_t tb;
	std::memset( &tb, 0, sizeof(tb));
	tb.nblocks = 1; tb.nbytes = bytes.size(); tb.block_entries = 16; tb.bytes = bytes.data(); tb.block_offsets = offsets; tb.block_handles = handles;
	sp_term_block_entry_t entries[ 16];
	uint8_t values[ 64];
	char err[ 80];
	return sp_match_term_blocks_decode_block( &tb, 0, entries, 16, values, sizeof(values), n, nv, err, sizeof(err));
}

static void malformedBlocks()
{
	size_t n = 0, nv = 0;
	CHECK( decodeBytes( std::string( "\0\0\2\1\1ab", 7), &n, &nv) == SP_OK && n == 1 && nv == 2);
	CHECK( decodeBytes( std::string( "\0\0\2\1\1ab\0\2\1\1\1c", 13), &n, &nv) == SP_OK && n == 2 && nv == 5);
	const std::string bad[] = {
		std::string( "\0\0\2\1\1ab\0\1\1\1\x80", 12),				// a varint that runs past the block
		std::string( "\0\0\2\1", 4),
		std::string( "\0\0\2\1", 4) + std::string( 10, '\x80') + "\1ab",		// a varint longer than ten bytes
		std::string( "\0\0\2\1", 4) + std::string( 9, '\xff') + "\2ab",
		std::string( "\0\0\2\1\1ab\0\3\1\1\1c", 13),				// a shared prefix above the value before
		std::string( "\0\1\1\1\1b", 6),
		std::string( "\0\0\2\1\1ab\0\1\3\1\1cd", 14),				// a suffix that runs past the block
		std::string( "\0\0", 2) + std::string( 9, '\xff') + "\1\1\1ab",
		std::string( "\0\0\1\1\1a", 6) + std::string( "\xff\xff\xff\xff\x0f\0\1\1\1b", 10),	// a handle that leaves 32 bits
		std::string( ""),
	};
	for (const std::string& data : bad) CHECK( decodeBytes( data, &n, &nv) == SP_ERR_INVALID);
	std::string many;
	for (int k=0; k<17; ++k) many += std::string( "\0\0\0\1\1", 5);
	CHECK( decodeBytes( many, &n, &nv) == SP_ERR_INVALID);
}

int main()
{
	shapes();
	bothSources();
	refusedArguments();
	malformedBlocks();
	std::printf( "match_termblocks_san: ok\n");
	return 0;
}
