// The values of the format strings of a finished batch over host arrays (result_values.hpp): host only, no device needed.
#include "result_values.hpp"
#include "finished_host.hpp"

namespace spa {

namespace {
const uint64_t MAX32 = 0xFFFFFFFFull;

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

// the records of one family: the bytes of a record with a format are its value, a record without one has none
struct Values
{
	const FormatTable& table; const ValueFormats T; const sp_match_batch_t& mb; const TextSource& S;
	const uint64_t* docItems;		// ndocs+1
	int items;				// 0: results, 1: item records

	// Whether record `i` has a value in document d: its format and its list, relative to the document's items.
	// ok = false: the record makes the document fail.
	bool valueOf( size_t d, uint64_t i, uint32_t& fmt, uint32_t& b, uint32_t& e, bool& ok) const
	{
		const uint64_t i0 = docItems[ d], i1 = docItems[ d+1];
		uint64_t lb, le;
		if (items) { fmt = mb.item_format[ 2*i]; lb = i + 1; le = lb + mb.item_format[ 2*i + 1]; }
		else { fmt = mb.result_format[ i]; lb = mb.results[ i].item_begin; le = lb + mb.results[ i].item_count; }
		ok = true;
		if (!fmt) return false;
		ok = fmt <= table.count && lb >= i0 && le <= i1 && i1 - i0 <= MAX32;
		b = (uint32_t)(lb - i0); e = (uint32_t)(le - i0);
		return ok;
	}
	// the pieces of the value of record i, one after the other, to `piece`, which says whether to go on; false: the document fails
	template <class FN>
	bool walk( size_t d, uint64_t i, FN piece) const
	{
		uint32_t fmt, b, e;
		bool ok;
		if (!valueOf( d, i, fmt, b, e, ok)) return ok;
		const DocItems list = { mb, S, d, docItems[ d] };
		HostStack stack;
		ValueWalk<HostStack, DocItems> w( T, stack, list);
		w.start( fmt, b, e);
		ValuePiece p;
		while (w.next( p) && piece( p)) {}
		return !w.failed;
	}
	bool length( size_t d, uint64_t i, uint64_t& n) const
	{
		return walk( d, i, [&]( const ValuePiece& p) { n += p.len; return n <= MAX32; });
	}
	void write( size_t d, uint64_t i, char* at) const
	{
		walk( d, i, [&]( const ValuePiece& p) {
			std::memcpy( at, (p.kind == VALUE_PIECE_TEXT ? S.text : table.pool.data()) + p.src, p.len);
			at += p.len;
			return true;
		});
	}
};

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
	out->doc_value_status = filledArray<int32_t>( ndocs + 1);
	if (flags & SP_VALUE_RESULTS) out->result_value_offsets = filledArray<uint64_t>( nresults + 1);
	if (flags & SP_VALUE_ITEMS) out->item_value_offsets = filledArray<uint64_t>( nitems + 1);
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
	const DocRecords docs = finishedDocRecords( mb);
	allocMatchValues( out, ndocs, mb.nresults, mb.nitems, flags);
	// a batch without formats: all values empty
	if (!table.count || !mb.result_format || !mb.item_format) { allocMatchValuesBytes( out, flags); return; }
	const Values results = { table, table.view(), mb, S, docs.items.data(), 0 }, items = { table, table.view(), mb, S, docs.items.data(), 1 };
	ByteFamily R = { docs.results.data(), ndocs, &out->result_values, out->result_value_offsets, &out->totals[ 0] };
	ByteFamily I = { docs.items.data(), ndocs, &out->item_values, out->item_value_offsets, &out->totals[ 1] };
	if (flags & SP_VALUE_RESULTS) R.count( results, out->doc_value_status);
	if (flags & SP_VALUE_ITEMS) I.count( items, out->doc_value_status);
	if (flags & SP_VALUE_RESULTS) R.place( results, out->doc_value_status);
	if (flags & SP_VALUE_ITEMS) I.place( items, out->doc_value_status);
}

} // namespace

extern "C" void sp_match_values_free( sp_match_values_t* v)
{
	std::free( v->result_values); std::free( v->result_value_offsets); std::free( v->item_values); std::free( v->item_value_offsets);
	std::free( v->doc_value_status);
	std::memset( v, 0, sizeof(*v));
}
