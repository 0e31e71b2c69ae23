// Lookups in an index segment over host arrays (match_segment.hpp): host only, no device needed.
#include "match_segment.hpp"
#include "finished_host.hpp"

namespace spa {

namespace {

// block_offsets of one product: they start at 0, ascend without an empty block and end at nbytes
void checkBlockOffsets( const uint64_t* offsets, uint64_t nblocks, uint64_t nbytes, const uint8_t* bytes, const char* what)
{
	if (!offsets) throw std::runtime_error( std::string( what) + " without block offsets");
	if (offsets[ 0] != 0) throw std::runtime_error( std::string( what) + ": block offsets that do not start at 0");
	for (uint64_t j=0; j<nblocks; ++j)
	{
		if (offsets[ j] > offsets[ j+1]) throw std::runtime_error( std::string( what) + ": block offsets that descend");
		if (offsets[ j] == offsets[ j+1]) throw std::runtime_error( std::string( what) + ": an empty block");
	}
	if (offsets[ nblocks] != nbytes) throw std::runtime_error( std::string( what) + ": block offsets that do not end at nbytes");
	if (nbytes && !bytes) throw std::runtime_error( std::string( what) + " without bytes");
}

SegmentView hostView( const sp_match_term_blocks_t* tb, const sp_match_posting_blocks_t* pb)
{
	const SegmentView S = { tb->bytes, tb->block_offsets, tb->block_handles, tb->nbytes, pb->bytes, pb->block_offsets, pb->nbytes,
				(uint32_t)tb->ndict, (uint32_t)tb->nblocks, tb->block_entries };
	return S;
}

} // namespace

void checkSegmentTables( const sp_match_term_blocks_t* tb, const sp_match_posting_blocks_t* pb)
{
	if (!tb) throw std::runtime_error( "no term blocks");
	if (!pb) throw std::runtime_error( "no posting blocks");
	if (tb->ndict != pb->ndict || tb->nblocks != pb->nblocks || tb->block_entries != pb->block_entries)
		throw std::runtime_error( "the posting blocks are not those of the term blocks: another ndict, nblocks or block size");
	const uint32_t B = tb->block_entries;
	if (!termBlockEntriesValid( B)) throw std::runtime_error( "a block size that is not 1, 2, 4, 8, 16, 32 or 64");
	if (tb->ndict >= SEG_MAX32) throw std::runtime_error( "2^32 - 1 entries or more");
	if (tb->nblocks != (tb->ndict + B - 1) / B) throw std::runtime_error( "a number of blocks that is not ceil( ndict / B)");
	checkBlockOffsets( tb->block_offsets, tb->nblocks, tb->nbytes, tb->bytes, "term blocks");
	checkBlockOffsets( pb->block_offsets, pb->nblocks, pb->nbytes, pb->bytes, "posting blocks");
	if (tb->nblocks && !tb->block_handles) throw std::runtime_error( "term blocks without block handles");
	for (uint64_t j=1; j<tb->nblocks; ++j)
	{
		if (tb->block_handles[ j-1] > tb->block_handles[ j]) throw std::runtime_error( "block handles that descend");
	}
}

void checkSegmentQueries( const uint32_t* queryHandles, const uint64_t* queryOffsets, const uint8_t* queryBytes, uint64_t nq, uint32_t flags)
{
	if (flags & ~(uint32_t)SP_LOOKUP_PREFIX) throw std::runtime_error( "unknown lookup flags");
	if (!nq) return;
	if (!queryHandles || !queryOffsets) throw std::runtime_error( "queries without their handles or offsets");
	for (uint64_t i=0; i<nq; ++i)
	{
		if (queryOffsets[ i] > queryOffsets[ i+1]) throw std::runtime_error( "query offsets that descend");
	}
	if (queryOffsets[ nq] > queryOffsets[ 0] && !queryBytes) throw std::runtime_error( "queries without their bytes");
}

void checkSegmentLookupLimits( uint64_t nq, uint64_t nsel, uint64_t npostings, uint64_t npositions)
{
	if (nq >= SEG_MAX32 || nsel >= SEG_MAX32 || npostings >= SEG_MAX32 || npositions >= SEG_MAX32)
		throw std::runtime_error( "2^32 - 1 queries, selected positions, postings or positions, or more");
}

void allocSegmentLookup( sp_segment_lookup_t* out, uint64_t nq, uint64_t nsel, uint32_t flags)
{
	out->nq = (size_t)nq; out->nsel = (size_t)nsel; out->flags = flags;
	out->totals[ 0] = nsel;
	out->q_first = filledArray<uint32_t>( nq); out->q_count = filledArray<uint32_t>( nq); out->q_status = filledArray<uint32_t>( nq);
	out->q_sel_offsets = filledArray<uint64_t>( nq + 1);
	out->selections = filledArray<sp_segment_selection_t>( nsel);
	out->sel_value_offsets = filledArray<uint64_t>( nsel + 1);
	out->sel_posting_offsets = filledArray<uint64_t>( nsel + 1);
}

void allocSegmentLookupLists( sp_segment_lookup_t* out, uint64_t npostings, uint64_t npositions, uint64_t nvalueBytes)
{
	out->npostings = (size_t)npostings; out->npositions = (size_t)npositions; out->nvalue_bytes = (size_t)nvalueBytes;
	out->totals[ 1] = npostings; out->totals[ 2] = npositions; out->totals[ 3] = nvalueBytes;
	out->values = filledArray<uint8_t>( nvalueBytes);
	out->postings = filledArray<sp_segment_posting_t>( npostings);
	out->posting_position_offsets = filledArray<uint64_t>( npostings + 1);
	out->positions = filledArray<uint32_t>( npositions);
}

} // namespace

extern "C" void sp_segment_lookup_free( sp_segment_lookup_t* lk)
{
	std::free( lk->q_first); std::free( lk->q_count); std::free( lk->q_status); std::free( lk->q_sel_offsets);
	std::free( lk->selections); std::free( lk->sel_value_offsets); std::free( lk->sel_posting_offsets);
	std::free( lk->values); std::free( lk->postings); std::free( lk->posting_position_offsets); std::free( lk->positions);
	std::memset( lk, 0, sizeof(*lk));
}

extern "C" int sp_match_segment_lookup( const sp_match_term_blocks_t* tb, const sp_match_posting_blocks_t* pb, const uint32_t* query_handles,
					const uint64_t* query_offsets, const uint8_t* query_bytes, size_t nq, uint32_t flags,
					sp_segment_lookup_t* out, char* err, size_t errsize)
{
	using namespace spa;
	return hostProduct( out, sp_segment_lookup_free, err, errsize, [&]{
		checkSegmentTables( tb, pb);
		checkSegmentQueries( query_handles, query_offsets, query_bytes, nq, flags);
		checkSegmentLookupLimits( nq, 0, 0, 0);
		const SegmentView S = hostView( tb, pb);
		const bool prefix = (flags & SP_LOOKUP_PREFIX) != 0;
		// find: the run of every query; runs: where they start in the selection
		std::vector<SegmentRun> run( nq);
		uint64_t nsel = 0;
		for (size_t i=0; i<nq; ++i)
		{
			const uint64_t qlen = query_offsets[ i+1] - query_offsets[ i];
			run[ i] = segmentFind( S, query_handles[ i], qlen ? query_bytes + query_offsets[ i] : (const uint8_t*)"", qlen, prefix);
			nsel += run[ i].count;
		}
		checkSegmentLookupLimits( nq, nsel, 0, 0);
		allocSegmentLookup( out, nq, nsel, flags);
		for (size_t i=0; i<nq; ++i)
		{
			out->q_first[ i] = run[ i].first; out->q_count[ i] = run[ i].count; out->q_status[ i] = run[ i].status;
			out->q_sel_offsets[ i+1] = out->q_sel_offsets[ i] + run[ i].count;
		}
		// sizes: every selected position; offsets: where its value, its postings and its positions start
		std::vector<uint32_t> selStatus( (size_t)nsel, 0);
		std::vector<uint64_t> selPositionOffsets( (size_t)nsel + 1, 0);
		for (uint64_t s=0; s<nsel; ++s)
		{
			const uint32_t qi = selectionQuery( out->q_sel_offsets, (uint32_t)nq, s);
			const uint32_t k = out->q_first[ qi] + (uint32_t)(s - out->q_sel_offsets[ qi]);
			CountingSink counting;
			const SelectionSizes z = walkSelection( S, k, counting);
			const sp_segment_selection_t record = { k, z.handle, z.docFreq, z.valueBytes, z.count };
			out->selections[ s] = record;
			selStatus[ s] = z.status;
			if (z.status > out->q_status[ qi]) out->q_status[ qi] = z.status;
			out->sel_value_offsets[ s+1] = out->sel_value_offsets[ s] + z.valueBytes;
			out->sel_posting_offsets[ s+1] = out->sel_posting_offsets[ s] + z.npostings;
			selPositionOffsets[ s+1] = selPositionOffsets[ s] + z.npositions;
		}
		const uint64_t npostings = out->sel_posting_offsets[ nsel], npositions = selPositionOffsets[ nsel];
		checkSegmentLookupLimits( nq, nsel, npostings, npositions);
		allocSegmentLookupLists( out, npostings, npositions, out->sel_value_offsets[ nsel]);
		// emit: the same walks, writing what was counted
		for (uint64_t s=0; s<nsel; ++s)
		{
			if (selStatus[ s]) continue;
			const uint64_t p0 = out->sel_posting_offsets[ s];
			WritingSink writing = { out->values + out->sel_value_offsets[ s], out->selections[ s].value_bytes,
						(uint32_t*)(out->postings + p0), out->posting_position_offsets + p0, out->sel_posting_offsets[ s+1] - p0,
						out->positions + selPositionOffsets[ s], selPositionOffsets[ s+1] - selPositionOffsets[ s], selPositionOffsets[ s] };
			walkSelection( S, out->selections[ s].position, writing);
		}
		out->posting_position_offsets[ npostings] = npositions;
	});
}
