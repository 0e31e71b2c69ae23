// The values of the format strings of a finished batch over host arrays (result_values.hpp): host only, no device needed.
#include "result_values.hpp"
#include "batch_fetch.hpp"

namespace spa {

namespace {
const uint64_t MAX32 = 0xFFFFFFFFull;
enum {VALUE_ERR_RANGE = SP_DOC_ERR_RANGE};

template <class T>
T* zeroedArray( uint64_t n)
{
	T* p = hostArray<T>( n);
	std::memset( p, 0, (size_t)n * sizeof(T));
	return p;
}

struct HostStack
{
	uint32_t w[ VALUE_MAX_DEPTH][ VALUE_FRAME_WORDS];
	uint32_t& word( uint32_t level, uint32_t k) { return w[ level][ k]; }
};

// the item records of one document, indices relative to its first item
struct DocItems
{
	const sp_match_batch_t& mb; const TextSource& S; uint64_t doc, first;
	uint32_t variable( uint32_t i) const { return mb.items[ first + i].variable; }
	void format( uint32_t i, uint32_t& fmt, uint32_t& nsub) const { fmt = mb.item_format[ 2*(first + i)]; nsub = mb.item_format[ 2*(first + i) + 1]; }
	bool span( uint32_t i, uint64_t& begin, uint64_t& length) const { return spanRange( S, doc, (const uint32_t*)(mb.items + first + i) + 3, begin, length); }
};

struct Batch
{
	const FormatTable& table; const sp_match_batch_t& mb; const TextSource& S;
	std::vector<uint64_t> docItems;		// ndocs+1: the items of a finished batch have no gaps and are in result order
};

// one family: the records of document d are [docOffsets[d], docOffsets[d+1])
struct Family
{
	int items;				// 0: results, 1: item records
	const uint64_t* docOffsets;
	std::vector<uint32_t> work;		// per record: the offset of its value inside the document
	std::vector<uint64_t> docBytes;
	char** bytes; uint64_t* offsets; uint64_t* total;
};

// Whether record `i` of the family has a value in document d: its format and its list, relative to the document's items.
// ok = false: the record makes the document fail.
bool valueOf( const Batch& B, const Family& F, size_t d, uint64_t i, uint32_t& fmt, uint32_t& b, uint32_t& e, bool& ok)
{
	const uint64_t i0 = B.docItems[ d], i1 = B.docItems[ d+1];
	uint64_t lb, le;
	if (F.items) { fmt = B.mb.item_format[ 2*i]; lb = i + 1; le = lb + B.mb.item_format[ 2*i + 1]; }
	else { fmt = B.mb.result_format[ i]; lb = B.mb.results[ i].item_begin; le = lb + B.mb.results[ i].item_count; }
	ok = true;
	if (!fmt) return false;
	ok = fmt <= B.table.count && lb >= i0 && le <= i1 && i1 - i0 <= MAX32;
	b = (uint32_t)(lb - i0); e = (uint32_t)(le - i0);
	return ok;
}

// pass A of the device: offsets inside the document, its byte count, its status
void countFamily( const Batch& B, Family& F, int32_t* status)
{
	const size_t ndocs = B.mb.ndocs;
	const ValueFormats T = B.table.view();
	F.work.assign( (size_t)F.docOffsets[ ndocs] + 1, 0);
	F.docBytes.assign( ndocs + 1, 0);
	for (size_t d=0; d<ndocs; ++d)
	{
		uint64_t total = 0;
		bool ok = true;
		const DocItems items = { B.mb, B.S, d, B.docItems[ d] };
		for (uint64_t i=F.docOffsets[ d]; ok && i<F.docOffsets[ d+1]; ++i)
		{
			uint32_t fmt, b, e;
			F.work[ i] = (uint32_t)total;
			if (!valueOf( B, F, d, i, fmt, b, e, ok)) continue;
			HostStack stack;
			ValueWalk<HostStack, DocItems> walk( T, stack, items);
			walk.start( fmt, b, e);
			ValuePiece p;
			uint64_t length = 0;
			while (length <= MAX32 && walk.next( p)) length += p.len;
			ok = !walk.failed && length <= MAX32;
			if (ok) total += length;
			if (total > MAX32) ok = false;
		}
		if (ok) F.docBytes[ d] = total; else status[ d] = VALUE_ERR_RANGE;
	}
}

// passes B and C of the device
void placeFamily( const Batch& B, Family& F, const int32_t* status)
{
	const size_t ndocs = B.mb.ndocs;
	const ValueFormats T = B.table.view();
	std::vector<uint64_t> docAt( ndocs + 1, 0);
	for (size_t d=0; d<ndocs; ++d) docAt[ d+1] = docAt[ d] + (status[ d] ? 0 : F.docBytes[ d]);
	*F.total = docAt[ ndocs];
	*F.bytes = hostArray<char>( docAt[ ndocs] + 1);
	for (size_t d=0; d<ndocs; ++d)
	{
		const DocItems items = { B.mb, B.S, d, B.docItems[ d] };
		for (uint64_t i=F.docOffsets[ d]; i<F.docOffsets[ d+1]; ++i)
		{
			F.offsets[ i] = docAt[ d] + (status[ d] ? 0 : F.work[ i]);
			uint32_t fmt, b, e;
			bool ok;
			if (status[ d] || !valueOf( B, F, d, i, fmt, b, e, ok)) continue;
			HostStack stack;
			ValueWalk<HostStack, DocItems> walk( T, stack, items);
			walk.start( fmt, b, e);
			ValuePiece p;
			char* at = *F.bytes + F.offsets[ i];
			while (walk.next( p))
			{
				std::memcpy( at, (p.kind == VALUE_PIECE_TEXT ? B.S.text : B.table.pool.data()) + p.src, p.len);
				at += p.len;
			}
		}
	}
	F.offsets[ F.docOffsets[ ndocs]] = docAt[ ndocs];
}

void appendLiteral( FormatTable& T, std::string& lit)
{
	if (lit.empty()) return;
	const uint32_t part[ VALUE_PART_WORDS] = { VALUE_PART_LITERAL, 0, (uint32_t)T.pool.size(), (uint32_t)lit.size() };
	T.parts.insert( T.parts.end(), part, part + VALUE_PART_WORDS);
	T.pool += lit;
	lit.clear();
}

// the parts of one format string (resultformat.parse, pattern_resultformat.hpp); false when it does not parse
bool parseFormat( FormatTable& T, const std::string& fmt, const std::function<uint32_t(const std::string&)>& variableId, std::string& why)
{
	std::string lit;
	for (size_t i=0; i<fmt.size();)
	{
		const char c = fmt[ i];
		if (c == '\\' && i + 1 < fmt.size()) { lit.push_back( fmt[ i+1]); i += 2; }
		else if (c == '{')
		{
			const size_t j = fmt.find( '}', i + 1);
			if (j == std::string::npos) { why = "missing '}'"; return false; }
			appendLiteral( T, lit);
			const std::string body = fmt.substr( i + 1, j - i - 1);
			const size_t bar = body.find( '|');
			std::string var = body.substr( 0, bar), sep = bar == std::string::npos ? std::string( " ") : body.substr( bar + 1);
			size_t v0 = 0, v1 = var.size();
			while (v0 < v1 && (unsigned char)var[ v0] <= 32) ++v0;
			while (v1 > v0 && (unsigned char)var[ v1-1] <= 32) --v1;
			var = var.substr( v0, v1 - v0);
			if (var.empty()) { why = "empty variable reference"; return false; }
			const uint32_t part[ VALUE_PART_WORDS] = { VALUE_PART_VARIABLE, variableId( var), (uint32_t)T.pool.size(), (uint32_t)sep.size() };
			T.parts.insert( T.parts.end(), part, part + VALUE_PART_WORDS);
			T.pool += sep;
			i = j + 1;
		}
		else { lit.push_back( c); ++i; }
	}
	appendLiteral( T, lit);
	return true;
}

} // namespace

FormatTable buildFormatTable( uint32_t count, const std::function<const char*(uint32_t)>& formatString,
			      const std::function<uint32_t(const std::string&)>& variableId)
{
	FormatTable T;
	T.count = count;
	T.fmtParts.assign( 2, 0);
	for (uint32_t f=1; f<=count; ++f)
	{
		const char* s = formatString( f);
		const std::string fmt = s ? s : "";
		std::string why;
		const size_t nparts = T.parts.size(), npool = T.pool.size();
		if (!parseFormat( T, fmt, variableId, why))
		{
			// (such a format has no parts; the values calls fail before they look at it)
			T.parts.resize( nparts); T.pool.resize( npool);
			if (T.error.empty()) T.error = why + " in result format string " + std::to_string( f) + ": \"" + fmt + "\"";
		}
		T.fmtParts.push_back( (uint32_t)(T.parts.size() / VALUE_PART_WORDS));
	}
	return T;
}

void allocMatchValues( sp_match_values_t* out, size_t ndocs, uint64_t nresults, uint64_t nitems, uint32_t flags)
{
	out->ndocs = ndocs; out->nresults = (size_t)nresults; out->nitems = (size_t)nitems;
	out->doc_value_status = zeroedArray<int32_t>( ndocs + 1);
	if (flags & SP_VALUE_RESULTS) out->result_value_offsets = zeroedArray<uint64_t>( nresults + 1);
	if (flags & SP_VALUE_ITEMS) out->item_value_offsets = zeroedArray<uint64_t>( nitems + 1);
}

void allocMatchValuesBytes( sp_match_values_t* out, uint32_t flags)
{
	if (flags & SP_VALUE_RESULTS) out->result_values = hostArray<char>( out->totals[ 0] + 1);
	if (flags & SP_VALUE_ITEMS) out->item_values = hostArray<char>( out->totals[ 1] + 1);
}

void matchBatchValues( const FormatTable& table, const sp_match_batch_t& mb, const TextSource& S, uint32_t flags, sp_match_values_t* out)
{
	if (!flags || (flags & ~(uint32_t)(SP_VALUE_RESULTS | SP_VALUE_ITEMS))) throw std::runtime_error( "unknown or no value flags");
	if (!S.segOffsets || (!S.text && S.nbytes)) throw std::runtime_error( "no text source");
	if (!S.docSegOffsets && S.nseg != mb.ndocs) throw std::runtime_error( "without document segment offsets every document is one segment: nseg must be ndocs");
	if (!table.error.empty()) throw std::runtime_error( table.error);
	const size_t ndocs = mb.ndocs;
	if (ndocs && !mb.doc_result_offsets) throw std::runtime_error( "batch without document offsets");
	Batch B = { table, mb, S, std::vector<uint64_t>( ndocs + 1, 0) };
	for (size_t d=0; d<ndocs; ++d)
	{
		const uint64_t r0 = mb.doc_result_offsets[ d], r1 = mb.doc_result_offsets[ d+1];
		if (r0 > r1 || r1 > mb.nresults || (d == 0 && r0 != 0)) throw std::runtime_error( "document offsets of the batch do not ascend inside its results");
		uint64_t n = 0;
		for (uint64_t i=r0; i<r1; ++i) n += mb.results[ i].item_count;
		B.docItems[ d+1] = B.docItems[ d] + n;
	}
	if ((ndocs ? mb.doc_result_offsets[ ndocs] : 0) != mb.nresults || B.docItems[ ndocs] != mb.nitems) throw std::runtime_error( "not a finished batch: results or items outside the documents");
	allocMatchValues( out, ndocs, mb.nresults, mb.nitems, flags);
	// a batch without formats: all values empty
	if (!table.count || !mb.result_format || !mb.item_format) { allocMatchValuesBytes( out, flags); return; }
	std::vector<uint64_t> docResults( ndocs + 1, 0);
	if (ndocs) docResults.assign( mb.doc_result_offsets, mb.doc_result_offsets + ndocs + 1);
	Family R, I;
	R.items = 0; R.docOffsets = docResults.data();
	I.items = 1; I.docOffsets = B.docItems.data();
	R.bytes = &out->result_values; R.offsets = out->result_value_offsets; R.total = &out->totals[ 0];
	I.bytes = &out->item_values; I.offsets = out->item_value_offsets; I.total = &out->totals[ 1];
	if (flags & SP_VALUE_RESULTS) countFamily( B, R, out->doc_value_status);
	if (flags & SP_VALUE_ITEMS) countFamily( B, I, out->doc_value_status);
	if (flags & SP_VALUE_RESULTS) placeFamily( B, R, out->doc_value_status);
	if (flags & SP_VALUE_ITEMS) placeFamily( B, I, out->doc_value_status);
}

} // namespace

extern "C" void sp_match_values_free( sp_match_values_t* v)
{
	std::free( v->result_values); std::free( v->result_value_offsets); std::free( v->item_values); std::free( v->item_value_offsets);
	std::free( v->doc_value_status);
	std::memset( v, 0, sizeof(*v));
}
