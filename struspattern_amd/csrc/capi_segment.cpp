// C-ABI of the segment lookups: a segment on the device -- copies of the term blocks and the posting blocks that no context is
// needed for --, the lookup call with its fetch and timing calls (l2_segment.h).  The twin is match_segment.cpp.
#include "capi_l2_ctx.hpp"
#include "l2_segment.h"
#include "match_segment.hpp"
#include "finished_host.hpp"

struct sp_segment
{
	int device = 0;
	std::string lasterror;
	// the two products
	DeviceBuffer dTermBytes, dTermOffsets, dTermHandles, dPostingBytes, dPostingOffsets;
	uint64_t ndict = 0, nblocks = 0, termNbytes = 0, postingNbytes = 0;
	uint32_t blockEntries = 0;
	// the last lookup and its buffers; nothing is allocated before the first sp_segment_lookup_device
	PassRun<2> run;
	DeviceBuffer dQueryHandles, dQueryOffsets, dQueryBytes;
	DeviceBuffer dQFirst, dQCount, dQStatus, dQSelOffsets;
	DeviceBuffer dSelections, dSelStatus, dSelValueOffsets, dSelPostingOffsets, dSelPositionOffsets, dTotals;
	DeviceBuffer dValues, dPostings, dPostingPositionOffsets, dPositions;
	uint64_t nq = 0, nsel = 0, npostings = 0, npositions = 0, nvalueBytes = 0;
	uint32_t flags = 0;
	Stream own;		// (last member: it waits for its work before anything else goes)

	void allocTables()
	{
		dTermBytes.alloc( termNbytes + 16); dTermOffsets.alloc( (nblocks+1)*sizeof(uint64_t)); dTermHandles.alloc( (nblocks+1)*sizeof(uint32_t));
		dPostingBytes.alloc( postingNbytes + 16); dPostingOffsets.alloc( (nblocks+1)*sizeof(uint64_t));
	}
	SegmentView view() const
	{
		const SegmentView S = { (const uint8_t*)dTermBytes.ptr, (const uint64_t*)dTermOffsets.ptr, (const uint32_t*)dTermHandles.ptr, termNbytes,
					(const uint8_t*)dPostingBytes.ptr, (const uint64_t*)dPostingOffsets.ptr, postingNbytes,
					(uint32_t)ndict, (uint32_t)nblocks, blockEntries };
		return S;
	}
};

namespace {

// a new segment that `fill` has filled, or NULL with the message in `err`
template <class FN>
int newSegment( sp_segment_t** out, std::string& err, FN fill)
{
	*out = 0;
	sp_segment* s = 0;
	const int rc = guardedCall( err, SP_ERR_INVALID, [&]{ s = new sp_segment(); fill( *s); });
	if (rc != SP_OK) { (void)hipGetLastError(); delete s; return rc; }
	*out = s;
	return SP_OK;
}

// the per-selection arrays for `rows` selected positions
void reserveSelections( sp_segment* s, uint64_t rows)
{
	reserveOrNoMem( s->dSelections, (rows+1)*sizeof(sp_segment_selection_t));
	reserveOrNoMem( s->dSelStatus, (rows+1)*sizeof(uint32_t));
	reserveOrNoMem( s->dSelValueOffsets, (rows+1)*sizeof(uint64_t));
	reserveOrNoMem( s->dSelPostingOffsets, (rows+1)*sizeof(uint64_t));
	reserveOrNoMem( s->dSelPositionOffsets, (rows+1)*sizeof(uint64_t));
}

} // namespace

extern "C" {

int sp_segment_open( const sp_match_term_blocks_t* tb, const sp_match_posting_blocks_t* pb, sp_segment_t** out, char* err, size_t errsize)
{
	std::string message;
	if (err && errsize) err[ 0] = 0;
	const int rc = newSegment( out, message, [&]( sp_segment& s){
		checkSegmentTables( tb, pb);
		HIP_CHECK( hipGetDevice( &s.device));
		s.own.create( s.device);
		s.ndict = tb->ndict; s.nblocks = tb->nblocks; s.termNbytes = tb->nbytes; s.postingNbytes = pb->nbytes; s.blockEntries = tb->block_entries;
		try { s.allocTables(); }
		catch (const HipError&) { (void)hipGetLastError(); throw std::bad_alloc(); }
		if (s.termNbytes) copySync( s.own, s.dTermBytes.ptr, tb->bytes, s.termNbytes, hipMemcpyHostToDevice);
		if (s.postingNbytes) copySync( s.own, s.dPostingBytes.ptr, pb->bytes, s.postingNbytes, hipMemcpyHostToDevice);
		copySync( s.own, s.dTermOffsets.ptr, tb->block_offsets, (s.nblocks+1)*sizeof(uint64_t), hipMemcpyHostToDevice);
		copySync( s.own, s.dPostingOffsets.ptr, pb->block_offsets, (s.nblocks+1)*sizeof(uint64_t), hipMemcpyHostToDevice);
		if (s.nblocks) copySync( s.own, s.dTermHandles.ptr, tb->block_handles, s.nblocks*sizeof(uint32_t), hipMemcpyHostToDevice);
	});
	if (rc != SP_OK) copyText( err, errsize, message.c_str());
	return rc;
}

int sp_segment_from_ctx( sp_matcher_ctx_t* c, void* stream_, sp_segment_t** out)
{
	return newSegment( out, c->lasterror, [&]( sp_segment& s){
		const sp_matcher_ctx::TermBlocks& t = c->prod.blk;
		const sp_matcher_ctx::PostingBlocks& p = c->prod.pbk;
		if (!t.run.done || !p.run.done)
			throw std::runtime_error( "no term blocks and posting blocks of the last finished batch (sp_matcher_ctx_finished_term_blocks_device, sp_matcher_ctx_finished_posting_blocks_device)");
		if (t.ndict != p.ndict || t.nblocks != p.nblocks || t.blockEntries != p.blockEntries)
			throw std::runtime_error( "the posting blocks are not those of the term blocks: another ndict, nblocks or block size");
		hipStream_t stream = (hipStream_t)stream_;
		HIP_CHECK( hipSetDevice( c->device));
		s.device = c->device;
		s.own.create( s.device);
		s.ndict = t.ndict; s.nblocks = t.nblocks; s.termNbytes = t.nbytes; s.postingNbytes = p.nbytes; s.blockEntries = t.blockEntries;
		try { s.allocTables(); }
		catch (const HipError&) { (void)hipGetLastError(); throw std::bad_alloc(); }
		// behind the emitting launches of the two calls, which nobody has waited for yet
		if (stream != t.run.stream) HIP_CHECK( hipStreamWaitEvent( stream, t.run.ev[ 1], 0));
		if (stream != p.run.stream) HIP_CHECK( hipStreamWaitEvent( stream, p.run.ev[ 1], 0));
		if (s.termNbytes) HIP_CHECK( hipMemcpyAsync( s.dTermBytes.ptr, t.dBytes.ptr, s.termNbytes, hipMemcpyDeviceToDevice, stream));
		if (s.postingNbytes) HIP_CHECK( hipMemcpyAsync( s.dPostingBytes.ptr, p.dBytes.ptr, s.postingNbytes, hipMemcpyDeviceToDevice, stream));
		HIP_CHECK( hipMemcpyAsync( s.dTermOffsets.ptr, t.dBlockOffsets.ptr, (s.nblocks+1)*sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
		HIP_CHECK( hipMemcpyAsync( s.dPostingOffsets.ptr, p.dBlockOffsets.ptr, (s.nblocks+1)*sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
		if (s.nblocks) HIP_CHECK( hipMemcpyAsync( s.dTermHandles.ptr, t.dBlockHandles.ptr, s.nblocks*sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
		// the context's next call may write the buffers again
		HIP_CHECK( hipStreamSynchronize( stream));
	});
}

void sp_segment_free( sp_segment_t* s)
{
	if (!s) return;
	(void)hipSetDevice( s->device);
	delete s;
}

const char* sp_segment_last_error( sp_segment_t* s) { return s->lasterror.c_str(); }

int sp_segment_lookup_device( sp_segment_t* s, const uint32_t* query_handles, const uint64_t* query_offsets, const uint8_t* query_bytes,
			      size_t nq, uint32_t flags, void* stream_, sp_segment_lookup_device_t* out)
{
	if (out) std::memset( out, 0, sizeof(*out));
	hipStream_t stream = (hipStream_t)stream_;
	const int rc = guardedCall( s->lasterror, SP_ERR_INVALID, [&]{
		checkSegmentQueries( query_handles, query_offsets, query_bytes, nq, flags);
		HIP_CHECK( hipSetDevice( s->device));
		s->run.done = s->run.evValid = false;
		const bool prefix = (flags & SP_LOOKUP_PREFIX) != 0;
		const uint64_t q0 = nq ? query_offsets[ 0] : 0, queryNbytes = nq ? query_offsets[ nq] - q0 : 0;
		reserveOrNoMem( s->dQueryHandles, (nq+1)*sizeof(uint32_t));
		reserveOrNoMem( s->dQueryOffsets, (nq+1)*sizeof(uint64_t));
		reserveOrNoMem( s->dQueryBytes, queryNbytes + 16);
		reserveOrNoMem( s->dQFirst, (nq+1)*sizeof(uint32_t));
		reserveOrNoMem( s->dQCount, (nq+1)*sizeof(uint32_t));
		reserveOrNoMem( s->dQStatus, (nq+1)*sizeof(uint32_t));
		reserveOrNoMem( s->dQSelOffsets, (nq+1)*sizeof(uint64_t));
		reserveOrNoMem( s->dTotals, 4*sizeof(uint64_t));
		if (!prefix) reserveSelections( s, nq);
		s->run.begin( stream, stream, 0);
		HIP_CHECK( hipEventRecord( s->run.ev[ 0], stream));
		HIP_CHECK( hipMemsetAsync( s->dTotals.ptr, 0, 4*sizeof(uint64_t), stream));
		HIP_CHECK( hipMemsetAsync( s->dQSelOffsets.ptr, 0, (nq+1)*sizeof(uint64_t), stream));
		SegmentLookupParams P;
		std::memset( &P, 0, sizeof(P));
		uint64_t totals[ 4] = { 0, 0, 0, 0};
		if (nq >= SEG_MAX32) throw std::runtime_error( "2^32 - 1 queries or more");
		if (nq && s->ndict)
		{
			// (the offsets go up relative to the first: the bytes uploaded are those of the queries alone)
			std::vector<uint64_t> relative( nq + 1);
			for (size_t i=0; i<=nq; ++i) relative[ i] = query_offsets[ i] - q0;
			HIP_CHECK( hipMemcpyAsync( s->dQueryHandles.ptr, query_handles, nq*sizeof(uint32_t), hipMemcpyHostToDevice, stream));
			copySync( stream, s->dQueryOffsets.ptr, relative.data(), (nq+1)*sizeof(uint64_t), hipMemcpyHostToDevice);
			if (queryNbytes) HIP_CHECK( hipMemcpyAsync( s->dQueryBytes.ptr, query_bytes + q0, queryNbytes, hipMemcpyHostToDevice, stream));
			P.segment = s->view();
			P.queryHandles = (const uint32_t*)s->dQueryHandles.ptr; P.queryOffsets = (const uint64_t*)s->dQueryOffsets.ptr;
			P.queryBytes = (const uint8_t*)s->dQueryBytes.ptr; P.queryNbytes = queryNbytes; P.nq = (uint32_t)nq; P.prefix = prefix ? 1u : 0u;
			P.qFirst = (uint32_t*)s->dQFirst.ptr; P.qCount = (uint32_t*)s->dQCount.ptr; P.qStatus = (uint32_t*)s->dQStatus.ptr;
			P.qSelOffsets = (uint64_t*)s->dQSelOffsets.ptr; P.totals = (uint64_t*)s->dTotals.ptr;
			HIP_CHECK( launchL2SegmentFind( P, stream));
			P.selCapacity = nq;
			if (prefix)
			{
				// a prefix run is as long as the segment says: the host waits for nsel
				HIP_CHECK( hipStreamSynchronize( stream));
				copySync( s->own, totals, s->dTotals.ptr, sizeof(uint64_t), hipMemcpyDeviceToHost);
				if (totals[ 0] >= SEG_MAX32) throw std::runtime_error( "2^32 - 1 selected positions or more");
				P.selCapacity = totals[ 0];
				reserveSelections( s, P.selCapacity);
			}
			P.selections = (uint32_t*)s->dSelections.ptr; P.selStatus = (uint32_t*)s->dSelStatus.ptr;
			P.selValueOffsets = (uint64_t*)s->dSelValueOffsets.ptr; P.selPostingOffsets = (uint64_t*)s->dSelPostingOffsets.ptr;
			P.selPositionOffsets = (uint64_t*)s->dSelPositionOffsets.ptr;
			if (P.selCapacity)
			{
				// the one wait of an exact lookup: for what sizes `values`, `postings` and `positions`
				HIP_CHECK( launchL2SegmentCount( P, stream));
				HIP_CHECK( hipStreamSynchronize( stream));
				copySync( s->own, totals, s->dTotals.ptr, sizeof(totals), hipMemcpyDeviceToHost);
				checkSegmentLookupLimits( nq, totals[ 0], totals[ 1], totals[ 2]);
				if (totals[ 0] > P.selCapacity) throw std::logic_error( "more selected positions than were counted");
			}
		}
		else if (nq)
		{
			// the empty segment: every run is empty, nothing to launch
			HIP_CHECK( hipMemsetAsync( s->dQFirst.ptr, 0, nq*sizeof(uint32_t), stream));
			HIP_CHECK( hipMemsetAsync( s->dQCount.ptr, 0, nq*sizeof(uint32_t), stream));
			HIP_CHECK( hipMemsetAsync( s->dQStatus.ptr, 0, nq*sizeof(uint32_t), stream));
		}
		reserveSelections( s, totals[ 0]);
		if (!totals[ 0])
		{
			HIP_CHECK( hipMemsetAsync( s->dSelValueOffsets.ptr, 0, sizeof(uint64_t), stream));
			HIP_CHECK( hipMemsetAsync( s->dSelPostingOffsets.ptr, 0, sizeof(uint64_t), stream));
		}
		reserveOrNoMem( s->dValues, totals[ 3] + 16);
		reserveOrNoMem( s->dPostings, (totals[ 1]+1)*sizeof(sp_segment_posting_t));
		reserveOrNoMem( s->dPostingPositionOffsets, (totals[ 1]+1)*sizeof(uint64_t));
		reserveOrNoMem( s->dPositions, (totals[ 2]+1)*sizeof(uint32_t));
		if (!totals[ 0]) HIP_CHECK( hipMemsetAsync( s->dPostingPositionOffsets.ptr, 0, sizeof(uint64_t), stream));
		if (totals[ 0])
		{
			P.values = (uint8_t*)s->dValues.ptr; P.postings = (uint32_t*)s->dPostings.ptr;
			P.postingPositionOffsets = (uint64_t*)s->dPostingPositionOffsets.ptr; P.positions = (uint32_t*)s->dPositions.ptr;
			P.nsel = totals[ 0]; P.npostings = totals[ 1]; P.npositions = totals[ 2]; P.nvalueBytes = totals[ 3];
			HIP_CHECK( launchL2SegmentPlace( P, stream));
		}
		HIP_CHECK( hipEventRecord( s->run.ev[ 1], stream));
		s->run.completed( stream);
		s->nq = nq; s->nsel = totals[ 0]; s->npostings = totals[ 1]; s->npositions = totals[ 2]; s->nvalueBytes = totals[ 3]; s->flags = flags;
		if (out)
		{
			out->nq = nq; out->nsel = (size_t)totals[ 0]; out->npostings = (size_t)totals[ 1]; out->npositions = (size_t)totals[ 2];
			out->nvalue_bytes = (size_t)totals[ 3]; out->flags = flags;
			out->d_q_first = s->dQFirst.ptr; out->d_q_count = s->dQCount.ptr; out->d_q_status = s->dQStatus.ptr; out->d_q_sel_offsets = s->dQSelOffsets.ptr;
			out->d_selections = s->dSelections.ptr; out->d_sel_value_offsets = s->dSelValueOffsets.ptr; out->d_sel_posting_offsets = s->dSelPostingOffsets.ptr;
			out->d_values = s->dValues.ptr; out->d_postings = s->dPostings.ptr; out->d_posting_position_offsets = s->dPostingPositionOffsets.ptr;
			out->d_positions = s->dPositions.ptr; out->d_totals = s->dTotals.ptr;
		}
	});
	// after a failure nothing of the caller's arrays is still being read
	if (rc != SP_OK) { (void)hipStreamSynchronize( stream); (void)hipGetLastError(); }
	return rc;
}

int sp_segment_lookup_fetch( sp_segment_t* s, sp_segment_lookup_t* out)
{
	std::memset( out, 0, sizeof(*out));
	const int rc = guardedCall( s->lasterror, SP_ERR_INVALID, [&]{
		if (!s->run.done) throw std::runtime_error( "no lookup on this segment (sp_segment_lookup_device)");
		HIP_CHECK( hipSetDevice( s->device));
		HIP_CHECK( hipStreamSynchronize( s->run.stream));
		const uint64_t nq = s->nq, nsel = s->nsel;
		allocSegmentLookup( out, nq, nsel, s->flags);
		allocSegmentLookupLists( out, s->npostings, s->npositions, s->nvalueBytes);
		if (nq)
		{
			copySync( s->own, out->q_first, s->dQFirst.ptr, nq*sizeof(uint32_t), hipMemcpyDeviceToHost);
			copySync( s->own, out->q_count, s->dQCount.ptr, nq*sizeof(uint32_t), hipMemcpyDeviceToHost);
			copySync( s->own, out->q_status, s->dQStatus.ptr, nq*sizeof(uint32_t), hipMemcpyDeviceToHost);
		}
		copySync( s->own, out->q_sel_offsets, s->dQSelOffsets.ptr, (nq+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (nsel) copySync( s->own, out->selections, s->dSelections.ptr, nsel*sizeof(sp_segment_selection_t), hipMemcpyDeviceToHost);
		copySync( s->own, out->sel_value_offsets, s->dSelValueOffsets.ptr, (nsel+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		copySync( s->own, out->sel_posting_offsets, s->dSelPostingOffsets.ptr, (nsel+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (s->nvalueBytes) copySync( s->own, out->values, s->dValues.ptr, s->nvalueBytes, hipMemcpyDeviceToHost);
		if (s->npostings) copySync( s->own, out->postings, s->dPostings.ptr, s->npostings*sizeof(sp_segment_posting_t), hipMemcpyDeviceToHost);
		copySync( s->own, out->posting_position_offsets, s->dPostingPositionOffsets.ptr, (s->npostings+1)*sizeof(uint64_t), hipMemcpyDeviceToHost);
		if (s->npositions) copySync( s->own, out->positions, s->dPositions.ptr, s->npositions*sizeof(uint32_t), hipMemcpyDeviceToHost);
		copySync( s->own, out->totals, s->dTotals.ptr, 4*sizeof(uint64_t), hipMemcpyDeviceToHost);
	});
	if (rc != SP_OK) sp_segment_lookup_free( out);
	return rc;
}

int sp_segment_last_lookup_ms( sp_segment_t* s, double* ms) { return s->run.ms( 0, 1, ms); }

} // extern "C"
