// The reader's side of an index segment -- term blocks (term_block_code.h) and posting blocks (posting_block_code.h), which
// state the writer's side --: one copy of the walks for the device-free twin of the segment lookups (match_segment.cpp) and the
// device passes (l2_segment_kernel.hip).  include/strus_pattern_amd.h "segment lookups" states the rule.  No HIP header in
// here: SPA_TB_HD is empty for a host compiler.
//   nextTermCode, skipPostingList, walkPostingList	the steps: the next code of a term block, a list skipped by its `body`,
//							a list walked posting by posting
//   TermMatch						a query compared against the front-coded codes without a value being
//							materialised: the leading query bytes known to equal the current entry
//							are carried, and `shared` cuts them
//   segmentFind					what a lane of `find` does for its query
//   walkSelection					what a lane of `sizes` and of `emit` does for its selected position; the
//							sink says whether it counts or writes
// Every read of `bytes` is bounded by the range of its block and that range by nbytes; a code that does not parse ends the walk
// with one of the SP_LOOKUP_ERR_* of the header.
#ifndef SPA_SEGMENT_WALK_H
#define SPA_SEGMENT_WALK_H
#include "posting_block_code.h"

namespace spa {

// (the values of SP_LOOKUP_ERR_* in include/strus_pattern_amd.h, which this header does not include: the kernels do not see it)
enum SegmentWalkStatus
{
	SEG_OK = 0,
	SEG_ERR_VARINT = 1,	// a varint past its block (or its list) or longer than ten bytes
	SEG_ERR_HEAD = 2,	// a head that does not carry its handle and its value in full
	SEG_ERR_SHARED = 3,	// a `shared` above the length of the value before
	SEG_ERR_SUFFIX = 4,	// a suffix past the block
	SEG_ERR_BODY = 5,	// a `body` of 0 or past the block, or a posting that ends beyond its `body`
	SEG_ERR_DELTA = 6,	// a ddelta of 0 behind the first posting of a list, a position gap of 0 behind the first position
	SEG_ERR_NPOS = 7,	// an npos of 0 or above the count
	SEG_ERR_RANGE = 8	// a handle, a value length, a doc_freq, a document, a count or a position that leaves 32 bits
};

const uint64_t SEG_MAX32 = 0xFFFFFFFFull;

// the two products of a segment, on the host or on the device
struct SegmentView
{
	const uint8_t* termBytes; const uint64_t* termOffsets; const uint32_t* termHandles; uint64_t termNbytes;
	const uint8_t* postingBytes; const uint64_t* postingOffsets; uint64_t postingNbytes;
	uint32_t ndict, nblocks, blockEntries;
};

// the range of block j of a product, cut to its bytes: an empty range fails at the first varint
SPA_TB_HD void segmentBlockRange( const uint64_t* offsets, uint64_t nbytes, uint32_t j, uint64_t& at, uint64_t& end)
{
	at = offsets[ j]; end = offsets[ (uint64_t)j+1];
	if (end > nbytes) end = nbytes;
	if (at > end) at = end;
}

// ---- the term side
struct TermCursor
{
	uint64_t at, end;	// the next code, the end of the block
	uint64_t suffixAt;	// where the stored bytes of the current code lie
	uint32_t handle, shared, suffix, docFreq;
	uint64_t count;
	uint32_t length;	// of the current value: shared + suffix; 0 in front of the head
};

SPA_TB_HD void openTermBlock( const SegmentView& S, uint32_t j, TermCursor& c)
{
	segmentBlockRange( S.termOffsets, S.termNbytes, j, c.at, c.end);
	c.suffixAt = c.at; c.handle = S.termHandles[ j]; c.shared = c.suffix = c.docFreq = c.length = 0; c.count = 0;
}

// the next code of the block: the head for a cursor just opened
SPA_TB_HD uint32_t nextTermCode( const SegmentView& S, TermCursor& c, bool head)
{
	uint64_t field[ 5];
	for (int i=0; i<5; ++i) if (!readVarint( S.termBytes, c.at, c.end, field[ i])) return SEG_ERR_VARINT;
	if (head && (field[ 0] || field[ 1])) return SEG_ERR_HEAD;
	if (field[ 1] > c.length) return SEG_ERR_SHARED;
	if (field[ 2] > c.end - c.at) return SEG_ERR_SUFFIX;
	const uint64_t handle = (uint64_t)c.handle + (field[ 0] <= SEG_MAX32 ? field[ 0] : SEG_MAX32);
	if (field[ 0] > SEG_MAX32 || handle > SEG_MAX32 || field[ 1] + field[ 2] > SEG_MAX32 || field[ 3] > SEG_MAX32) return SEG_ERR_RANGE;
	c.handle = (uint32_t)handle; c.shared = (uint32_t)field[ 1]; c.suffix = (uint32_t)field[ 2]; c.docFreq = (uint32_t)field[ 3];
	c.count = field[ 4]; c.length = c.shared + c.suffix;
	c.suffixAt = c.at; c.at += c.suffix;
	return SEG_OK;
}

// A query against the codes of a block, one behind the other: m is the number of leading query bytes that equal the current
// value, cmp says how the value stands to the query (-1 below, 0 equal, +1 above; bytes as memcmp, a prefix before what it is a
// prefix of).  A code that shares more than m bytes with the value before stands as that one does; any other is compared from
// byte `shared` on, against its stored bytes alone.
struct TermMatch
{
	uint64_t m;
	int cmp;
};

SPA_TB_HD void matchTermCode( const SegmentView& S, const TermCursor& c, const uint8_t* q, uint64_t qlen, bool head, TermMatch& t)
{
	if (!head && c.shared > t.m) return;
	uint64_t m = head ? 0 : c.shared;
	const uint64_t length = c.length;
	while (m < qlen && m < length && S.termBytes[ c.suffixAt + (m - c.shared)] == q[ m]) ++m;
	t.m = m;
	if (m == length) t.cmp = m == qlen ? 0 : -1;
	else if (m == qlen) t.cmp = 1;
	else t.cmp = S.termBytes[ c.suffixAt + (m - c.shared)] < q[ m] ? -1 : 1;
}

// whether (handle, value) as `t` compares it lies at or behind a bound of the run of the query (h, q):
//   the start	the first position that is not below (h, q)
//   the end	(prefix mode) the first position behind every value of h that starts with q
SPA_TB_HD bool behindBound( uint32_t handle, const TermMatch& t, uint32_t h, uint64_t qlen, bool endOfPrefixRun)
{
	if (handle != h) return handle > h;
	return endOfPrefixRun ? (t.cmp > 0 && t.m < qlen) : t.cmp >= 0;
}

// The first sorted position at or behind the bound, ndict if there is none; `equal` says whether the entry there is (h, q)
// itself.  Bisects the heads of the blocks -- a head carries its value in full --, then walks the one block in front of the
// first head behind the bound, and that head.
SPA_TB_HD uint32_t segmentBound( const SegmentView& S, uint32_t h, const uint8_t* q, uint64_t qlen, bool endOfPrefixRun, uint32_t& position, bool& equal)
{
	const uint32_t B = S.blockEntries;
	uint32_t lo = 0, hi = S.nblocks;	// the first block whose head lies behind the bound
	while (lo < hi)
	{
		const uint32_t mid = lo + ((hi - lo) >> 1);
		bool behind = S.termHandles[ mid] > h;
		if (S.termHandles[ mid] == h)
		{
			TermCursor c;
			TermMatch t = { 0, 0};
			openTermBlock( S, mid, c);
			const uint32_t status = nextTermCode( S, c, true);
			if (status) return status;
			matchTermCode( S, c, q, qlen, true, t);
			behind = behindBound( c.handle, t, h, qlen, endOfPrefixRun);
		}
		if (behind) hi = mid; else lo = mid + 1;
	}
	const uint64_t last = (uint64_t)lo * B + 1 < S.ndict ? (uint64_t)lo * B + 1 : S.ndict;	// (one behind the head found)
	TermCursor c;
	TermMatch t = { 0, 0};
	c.at = c.end = c.suffixAt = 0; c.handle = c.shared = c.suffix = c.docFreq = c.length = 0; c.count = 0;
	position = S.ndict; equal = false;
	for (uint64_t k = lo ? (uint64_t)(lo - 1) * B : 0; k < last; ++k)
	{
		const bool head = (k & (B - 1)) == 0;
		if (head) openTermBlock( S, (uint32_t)(k / B), c);
		const uint32_t status = nextTermCode( S, c, head);
		if (status) return status;
		matchTermCode( S, c, q, qlen, head, t);
		if (behindBound( c.handle, t, h, qlen, endOfPrefixRun))
		{
			position = (uint32_t)k; equal = c.handle == h && t.cmp == 0;
			break;
		}
	}
	return SEG_OK;
}

// ---- find: the run of one query
struct SegmentRun { uint32_t first, count, status; };

SPA_TB_HD SegmentRun segmentFind( const SegmentView& S, uint32_t h, const uint8_t* q, uint64_t qlen, bool prefix)
{
	SegmentRun run = { 0, 0, SEG_OK};
	if (!S.ndict) return run;
	uint32_t first = 0, end = 0;
	bool equal = false, unused = false;
	run.status = segmentBound( S, h, q, qlen, false, first, equal);
	if (run.status) return run;
	run.first = first;
	if (!prefix) { run.count = equal ? 1u : 0u; return run; }
	run.status = segmentBound( S, h, q, qlen, true, end, unused);
	if (run.status) { run.first = 0; return run; }
	run.count = end > first ? end - first : 0u;
	return run;
}

// ---- the posting side
// skips the list at `at` by its `body`
SPA_TB_HD uint32_t skipPostingList( const uint8_t* bytes, uint64_t& at, uint64_t end)
{
	uint64_t body = 0;
	if (!readVarint( bytes, at, end, body)) return SEG_ERR_VARINT;
	if (!body || body > end - at) return SEG_ERR_BODY;
	at += body;
	return SEG_OK;
}

// Walks the list at `at`: sink.posting( i, doc, count, npos, firstPosition) for posting i of the list, whose positions are
// [firstPosition, firstPosition + npos) of the list; sink.position( i, pos) for position i of the list.
template <class SINK>
SPA_TB_HD uint32_t walkPostingList( const uint8_t* bytes, uint64_t& at, uint64_t end, SINK& sink, uint64_t& npostings, uint64_t& npositions)
{
	uint64_t body = 0;
	npostings = npositions = 0;
	if (!readVarint( bytes, at, end, body)) return SEG_ERR_VARINT;
	if (!body || body > end - at) return SEG_ERR_BODY;
	const uint64_t listEnd = at + body;
	uint64_t doc = 0;
	while (at < listEnd)
	{
		uint64_t field[ 3];
		for (int i=0; i<3; ++i) if (!readVarint( bytes, at, listEnd, field[ i])) return SEG_ERR_VARINT;
		if (npostings && !field[ 0]) return SEG_ERR_DELTA;
		if (field[ 0] > SEG_MAX32 || (doc += field[ 0]) > SEG_MAX32 || field[ 1] > SEG_MAX32) return SEG_ERR_RANGE;
		if (!field[ 2] || field[ 2] > field[ 1]) return SEG_ERR_NPOS;
		sink.posting( npostings, (uint32_t)doc, (uint32_t)field[ 1], (uint32_t)field[ 2], npositions);
		uint64_t pos = 0;
		for (uint64_t i=0; i<field[ 2]; ++i, ++npositions)
		{
			uint64_t gap = 0;
			if (at >= listEnd) return SEG_ERR_BODY;
			if (!readVarint( bytes, at, listEnd, gap)) return SEG_ERR_VARINT;
			if (i && !gap) return SEG_ERR_DELTA;
			if (gap > SEG_MAX32 || (pos += gap) > SEG_MAX32) return SEG_ERR_RANGE;
			sink.position( npositions, (uint32_t)pos);
		}
		++npostings;
	}
	return SEG_OK;
}

// ---- sizes and emit: one selected position
struct SelectionSizes
{
	uint32_t status, handle, docFreq, valueBytes;
	uint64_t count, npostings, npositions;
};

// a sink that counts
struct CountingSink
{
	SPA_TB_HD void value( uint32_t, const uint8_t*, uint32_t) {}
	SPA_TB_HD void posting( uint64_t, uint32_t, uint32_t, uint32_t, uint64_t) {}
	SPA_TB_HD void position( uint64_t, uint32_t) {}
};

// Walks the term block of sorted position k from its head to its code, then skips `body` by `body` to its list and walks it.
// sink.value( at, src, n): the bytes [at, at+n) of the value are those at src, step by step from the head value on -- a step may
// reach beyond the final length, which the sink cuts.  After a status the sizes are zero: the selection is empty.
template <class SINK>
SPA_TB_HD SelectionSizes walkSelection( const SegmentView& S, uint32_t k, SINK& sink)
{
	SelectionSizes z = { SEG_OK, 0, 0, 0, 0, 0, 0};
	const uint32_t B = S.blockEntries, j = k / B, inBlock = k & (B - 1);
	TermCursor c;
	openTermBlock( S, j, c);
	for (uint32_t i=0; i<=inBlock && !z.status; ++i)
	{
		z.status = nextTermCode( S, c, i == 0);
		if (!z.status) sink.value( c.shared, S.termBytes + c.suffixAt, c.suffix);
	}
	uint64_t at = 0, end = 0;
	segmentBlockRange( S.postingOffsets, S.postingNbytes, j, at, end);
	for (uint32_t i=0; i<inBlock && !z.status; ++i) z.status = skipPostingList( S.postingBytes, at, end);
	uint64_t npostings = 0, npositions = 0;
	if (!z.status) z.status = walkPostingList( S.postingBytes, at, end, sink, npostings, npositions);
	if (!z.status && (npostings > SEG_MAX32 || npositions > SEG_MAX32)) z.status = SEG_ERR_RANGE;
	if (z.status) return z;
	z.handle = c.handle; z.docFreq = c.docFreq; z.valueBytes = c.length; z.count = c.count;
	z.npostings = npostings; z.npositions = npositions;
	return z;
}

// A sink that writes what a CountingSink walk of the same position counted, and not a byte more: the value to value[0, valueBytes),
// the postings to the 4-word records postings[0, npostings), where their positions start to postingPositionOffsets[0, npostings)
// (positionBase added), the positions to positions[0, npositions).
struct WritingSink
{
	uint8_t* valueOut; uint32_t valueBytes;
	uint32_t* postings; uint64_t* postingPositionOffsets; uint64_t npostings;
	uint32_t* positions; uint64_t npositions;
	uint64_t positionBase;

	SPA_TB_HD void value( uint32_t at, const uint8_t* src, uint32_t n)
	{
		for (uint32_t i=0; i<n && (uint64_t)at + i < valueBytes; ++i) valueOut[ at + i] = src[ i];
	}
	SPA_TB_HD void posting( uint64_t i, uint32_t doc, uint32_t count, uint32_t npos, uint64_t firstPosition)
	{
		if (i >= npostings) return;
		postings[ 4*i] = doc; postings[ 4*i+1] = count; postings[ 4*i+2] = npos; postings[ 4*i+3] = 0;
		postingPositionOffsets[ i] = positionBase + firstPosition;
	}
	SPA_TB_HD void position( uint64_t i, uint32_t pos) { if (i < npositions) positions[ i] = pos; }
};

// the query that selection s belongs to: the last query whose run starts at or before s (a query without a run is skipped)
SPA_TB_HD uint32_t selectionQuery( const uint64_t* selOffsets, uint32_t nq, uint64_t s)
{
	uint32_t lo = 0, hi = nq;
	while (hi - lo > 1)
	{
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (selOffsets[ mid] <= s) lo = mid; else hi = mid;
	}
	return lo;
}

} // namespace
#endif
