// The values of the format strings of a finished batch, over host arrays: the definition that the device passes
// (l2_values.h) are measured against, and the entry point for batches already fetched to the host (sp_match_batch_values).
// Host only: no HIP header and no HIP call in here.
//
// The rule (include/strus_pattern_amd.h "result values"; the project's own restatement of resultformat.Formatter).  The
// format table holds for every format handle the parts of its string: literals, and variables with their separator.  A
// result with a format has the value eval( result_format[r], its items ), an item record with a format the value
// eval( item_format[i][0], the nsub records behind it ); eval is the walk of value_walk.h.  A document in which an
// evaluation meets an invalid span, a format handle beyond the table, an nsub beyond its list, more than VALUE_MAX_DEPTH
// formats inside each other, or whose values of one family add up to 2^32 bytes or more, has value status
// SP_DOC_ERR_RANGE and all its values, of both families, are empty.
#ifndef SPA_RESULT_VALUES_HPP
#define SPA_RESULT_VALUES_HPP
#include "../../include/strus_pattern_amd.h"
#include "span_text.hpp"
#include "value_walk.h"
#include <functional>
#include <string>
#include <vector>

namespace spa {

// the parts of every format string of a rule set, built on the host when the rule set compiles
struct FormatTable
{
	std::vector<uint32_t> fmtParts;		// count+2
	std::vector<uint32_t> parts;		// VALUE_PART_WORDS each
	std::string pool;			// literals and separators
	uint32_t count = 0;
	std::string error;			// the first format string that does not parse: every values call fails with it

	ValueFormats view() const { const ValueFormats v = { fmtParts.data(), parts.data(), count }; return v; }
};

// formatString( f) for f in 1..count; variableId( name) gives the handle of a variable or 0
FormatTable buildFormatTable( uint32_t count, const std::function<const char*(uint32_t)>& formatString,
			      const std::function<uint32_t(const std::string&)>& variableId);

// the host arrays of the values of `nresults` / `nitems` records (a family that `flags` does not ask for has none), the
// offsets and the status zeroed (sp_match_values_free)
void allocMatchValues( sp_match_values_t* out, size_t ndocs, uint64_t nresults, uint64_t nitems, uint32_t flags);
// the byte arrays, once the totals are known
void allocMatchValuesBytes( sp_match_values_t* out, uint32_t flags);

// the values of a finished batch on the host; throws std::runtime_error for arguments that make no batch and for a table
// with a format string that does not parse
void matchBatchValues( const FormatTable& table, const sp_match_batch_t& mb, const TextSource& S, uint32_t flags, sp_match_values_t* out);

} // namespace
#endif
