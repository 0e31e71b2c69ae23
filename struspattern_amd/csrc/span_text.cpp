// The matched text of a finished batch over host arrays (span_text.hpp): host only, no device needed.
#include "span_text.hpp"
#include "finished_host.hpp"

namespace spa {

namespace {

// the records of one family, `stride` words each: the bytes of a record are those of its span
struct Spans
{
	const TextSource& S; const uint32_t* words; size_t stride;
	bool length( size_t d, uint64_t i, uint64_t& n) const { uint64_t begin; return spanRange( S, d, words + stride*i + 3, begin, n); }
	void write( size_t d, uint64_t i, char* dst) const
	{
		uint64_t begin, n;
		if (spanRange( S, d, words + stride*i + 3, begin, n) && n) std::memcpy( dst, S.text + begin, (size_t)n);
	}
};

} // namespace

bool spanRange( const TextSource& S, uint64_t doc, const uint32_t* w, uint64_t& begin, uint64_t& length)
{
	const uint64_t origseg = w[ 0], origpos = w[ 1], origendseg = w[ 2], origend = w[ 3];
	const uint64_t d0 = S.docSegOffsets ? S.docSegOffsets[ doc] : doc, d1 = S.docSegOffsets ? S.docSegOffsets[ doc+1] : doc+1;
	begin = 0; length = 0;
	if (d0 > d1 || d1 > S.nseg) return false;
	if (origseg > origendseg || origendseg >= d1 - d0) return false;
	const uint64_t s0 = d0 + origseg, s1 = d0 + origendseg;
	const uint64_t a = S.segOffsets[ s0], b = S.segOffsets[ s0+1], c = S.segOffsets[ s1], e = S.segOffsets[ s1+1];
	if (a > b || c > e || (s0 != s1 && b > c)) return false;
	if (origpos > b - a || origend > e - c) return false;
	const uint64_t end = c + origend;
	begin = a + origpos;
	if (begin > end || end > S.nbytes) return false;
	length = end - begin;
	return true;
}

void allocMatchText( sp_match_text_t* out, size_t ndocs, uint64_t nresults, uint64_t nitems, uint32_t flags)
{
	out->ndocs = ndocs; out->nresults = (size_t)nresults; out->nitems = (size_t)nitems;
	out->doc_text_status = filledArray<int32_t>( ndocs + 1);
	if (flags & SP_TEXT_RESULTS) out->result_text_offsets = filledArray<uint64_t>( nresults + 1);
	if (flags & SP_TEXT_ITEMS) out->item_text_offsets = filledArray<uint64_t>( nitems + 1);
}

void allocMatchTextBytes( sp_match_text_t* out, uint32_t flags)
{
	if (flags & SP_TEXT_RESULTS) out->result_text = hostArray<char>( out->totals[ 0] + 1);
	if (flags & SP_TEXT_ITEMS) out->item_text = hostArray<char>( out->totals[ 1] + 1);
}

void matchBatchText( const sp_match_batch_t& mb, const TextSource& S, uint32_t flags, sp_match_text_t* out)
{
	if (!flags || (flags & ~(uint32_t)(SP_TEXT_RESULTS | SP_TEXT_ITEMS))) throw std::runtime_error( "unknown or no text flags");
	if (!S.segOffsets || (!S.text && S.nbytes)) throw std::runtime_error( "no text source");
	if (!S.docSegOffsets && S.nseg != mb.ndocs) throw std::runtime_error( "without document segment offsets every document is one segment: nseg must be ndocs");
	const size_t ndocs = mb.ndocs;
	const DocRecords docs = finishedDocRecords( mb);
	allocMatchText( out, ndocs, mb.nresults, mb.nitems, flags);
	const Spans results = { S, (const uint32_t*)mb.results, 9 }, items = { S, (const uint32_t*)mb.items, 7 };
	ByteFamily R = { docs.results.data(), ndocs, &out->result_text, out->result_text_offsets, &out->totals[ 0] };
	ByteFamily I = { docs.items.data(), ndocs, &out->item_text, out->item_text_offsets, &out->totals[ 1] };
	if (flags & SP_TEXT_RESULTS) R.count( results, out->doc_text_status);
	if (flags & SP_TEXT_ITEMS) I.count( items, out->doc_text_status);
	if (flags & SP_TEXT_RESULTS) R.place( results, out->doc_text_status);
	if (flags & SP_TEXT_ITEMS) I.place( items, out->doc_text_status);
}

} // namespace

extern "C" void sp_match_text_free( sp_match_text_t* t)
{
	std::free( t->result_text); std::free( t->result_text_offsets); std::free( t->item_text); std::free( t->item_text_offsets);
	std::free( t->doc_text_status);
	std::memset( t, 0, sizeof(*t));
}

extern "C" int sp_match_batch_text( const sp_match_batch_t* mb, const char* text, uint64_t nbytes, const uint64_t* seg_offsets,
				    size_t nseg, const uint64_t* doc_seg_offsets, uint32_t flags, sp_match_text_t* out, char* err, size_t errsize)
{
	return spa::hostProduct( out, sp_match_text_free, err, errsize, [&]{
		if (!mb) throw std::runtime_error( "no batch");
		const spa::TextSource S = { text, nbytes, seg_offsets, nseg, doc_seg_offsets };
		spa::matchBatchText( *mb, S, flags, out);
	});
}
