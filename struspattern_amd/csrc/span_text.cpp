// The matched text of a finished batch over host arrays (span_text.hpp): host only, no device needed.
#include "span_text.hpp"
#include "batch_fetch.hpp"

namespace spa {

namespace {
const uint64_t MAX32 = 0xFFFFFFFFull;
enum {TEXT_ERR_RANGE = SP_DOC_ERR_RANGE};

template <class T>
T* zeroedArray( uint64_t n)
{
	T* p = hostArray<T>( n);
	std::memset( p, 0, (size_t)n * sizeof(T));
	return p;
}

// one family: the records of document d are [docOffsets[d], docOffsets[d+1]), `stride` words each
struct Family
{
	const uint32_t* records; size_t stride;
	std::vector<uint64_t> docOffsets;
	std::vector<uint32_t> work;		// per span: its offset inside the document
	std::vector<uint64_t> docBytes;
	char** text; uint64_t* offsets; uint64_t* total;
};

// pass A of the device: offsets inside the document, its byte count, its status
void countFamily( Family& F, const TextSource& S, int32_t* status)
{
	const size_t ndocs = F.docOffsets.size() - 1;
	F.work.assign( (size_t)F.docOffsets[ ndocs] + 1, 0);
	F.docBytes.assign( ndocs + 1, 0);
	for (size_t d=0; d<ndocs; ++d)
	{
		uint64_t total = 0;
		bool ok = true;
		for (uint64_t i=F.docOffsets[ d]; ok && i<F.docOffsets[ d+1]; ++i)
		{
			uint64_t begin, length;
			ok = spanRange( S, d, F.records + F.stride*i + 3, begin, length) && length <= MAX32;
			F.work[ i] = (uint32_t)total;
			if (ok) total += length;
			if (total > MAX32) ok = false;
		}
		if (ok) F.docBytes[ d] = total; else status[ d] = TEXT_ERR_RANGE;
	}
}

// passes B and C of the device
void placeFamily( Family& F, const TextSource& S, const int32_t* status)
{
	const size_t ndocs = F.docOffsets.size() - 1;
	std::vector<uint64_t> docAt( ndocs + 1, 0);
	for (size_t d=0; d<ndocs; ++d) docAt[ d+1] = docAt[ d] + (status[ d] ? 0 : F.docBytes[ d]);
	*F.total = docAt[ ndocs];
	*F.text = hostArray<char>( docAt[ ndocs] + 1);
	for (size_t d=0; d<ndocs; ++d)
	{
		for (uint64_t i=F.docOffsets[ d]; i<F.docOffsets[ d+1]; ++i)
		{
			F.offsets[ i] = docAt[ d] + (status[ d] ? 0 : F.work[ i]);
			uint64_t begin, length;
			if (status[ d] || !spanRange( S, d, F.records + F.stride*i + 3, begin, length) || !length) continue;
			std::memcpy( *F.text + F.offsets[ i], S.text + begin, (size_t)length);
		}
	}
	F.offsets[ F.docOffsets[ ndocs]] = docAt[ ndocs];
}

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
	out->doc_text_status = zeroedArray<int32_t>( ndocs + 1);
	if (flags & SP_TEXT_RESULTS) out->result_text_offsets = zeroedArray<uint64_t>( nresults + 1);
	if (flags & SP_TEXT_ITEMS) out->item_text_offsets = zeroedArray<uint64_t>( nitems + 1);
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
	if (ndocs && !mb.doc_result_offsets) throw std::runtime_error( "batch without document offsets");
	Family R, I;
	R.records = (const uint32_t*)mb.results; R.stride = 9; R.docOffsets.assign( ndocs + 1, 0);
	I.records = (const uint32_t*)mb.items; I.stride = 7; I.docOffsets.assign( ndocs + 1, 0);
	for (size_t d=0; d<ndocs; ++d)
	{
		const uint64_t r0 = mb.doc_result_offsets[ d], r1 = mb.doc_result_offsets[ d+1];
		if (r0 > r1 || r1 > mb.nresults || (d == 0 && r0 != 0)) throw std::runtime_error( "document offsets of the batch do not ascend inside its results");
		R.docOffsets[ d] = r0; R.docOffsets[ d+1] = r1;
		// the items of a finished batch have no gaps and are in result order
		uint64_t n = 0;
		for (uint64_t i=r0; i<r1; ++i) n += mb.results[ i].item_count;
		I.docOffsets[ d+1] = I.docOffsets[ d] + n;
	}
	if (R.docOffsets[ ndocs] != mb.nresults || I.docOffsets[ ndocs] != mb.nitems) throw std::runtime_error( "not a finished batch: results or items outside the documents");
	allocMatchText( out, ndocs, mb.nresults, mb.nitems, flags);
	R.text = &out->result_text; R.offsets = out->result_text_offsets; R.total = &out->totals[ 0];
	I.text = &out->item_text; I.offsets = out->item_text_offsets; I.total = &out->totals[ 1];
	if (flags & SP_TEXT_RESULTS) countFamily( R, S, out->doc_text_status);
	if (flags & SP_TEXT_ITEMS) countFamily( I, S, out->doc_text_status);
	if (flags & SP_TEXT_RESULTS) placeFamily( R, S, out->doc_text_status);
	if (flags & SP_TEXT_ITEMS) placeFamily( I, S, out->doc_text_status);
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
	std::memset( out, 0, sizeof(*out));
	if (err && errsize) err[ 0] = 0;
	try
	{
		if (!mb) throw std::runtime_error( "no batch");
		const spa::TextSource S = { text, nbytes, seg_offsets, nseg, doc_seg_offsets };
		spa::matchBatchText( *mb, S, flags, out);
		return SP_OK;
	}
	catch (const std::bad_alloc&) { sp_match_text_free( out); return SP_ERR_NOMEM; }
	catch (const std::exception& e)
	{
		sp_match_text_free( out);
		if (err && errsize) { std::strncpy( err, e.what(), errsize-1); err[ errsize-1] = 0; }
		return SP_ERR_INVALID;
	}
}
