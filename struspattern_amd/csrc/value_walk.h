// The walk that evaluates one result value (include/strus_pattern_amd.h "result values"): one copy of the rule for the
// device-free twin (result_values.cpp) and the device passes (l2_values_kernel.hip).  No HIP header in here: SPA_WALK_HD is
// empty for a host compiler.
//
// A value is eval( f, [b,e)): the parts of format f in order; a literal part gives its bytes of the pool, a variable part v
// gives, for every top-level record of the list whose word 0 is v, in list order, joined by the part's separator, the
// value of the record's own format over its arguments if it has one, else the bytes of its span.  The walk produces the
// value as a sequence of PIECES (bytes of the pool or of the text), one per call of next(), without recursion: the
// frames of the formats under evaluation live in a stack of VALUE_MAX_DEPTH frames that the caller provides.
// Indices of item records are relative to the first item of the document.
#ifndef SPA_VALUE_WALK_H
#define SPA_VALUE_WALK_H
#include <stdint.h>

#if defined(__HIPCC__)
#define SPA_WALK_HD __host__ __device__ __forceinline__
#else
#define SPA_WALK_HD inline
#endif

namespace spa {

enum { VALUE_MAX_DEPTH = 8 };		// formats under evaluation at once: 5 words of LDS per lane and level on the device
enum { VALUE_FRAME_WORDS = 5 };
enum { VALUE_PART_WORDS = 4 };		// a part of the format table: {kind, variable, pool offset, length}
enum { VALUE_PART_LITERAL = 0, VALUE_PART_VARIABLE = 1 };
enum { VALUE_PIECE_POOL = 0, VALUE_PIECE_TEXT = 1 };

// the format table as the walk reads it
struct ValueFormats
{
	const uint32_t* fmtParts;	// count+2: the parts of format f are [fmtParts[f], fmtParts[f+1]); fmtParts[0] = fmtParts[1] = 0
	const uint32_t* parts;		// VALUE_PART_WORDS each
	uint32_t count;
};

struct ValuePiece
{
	uint32_t kind;			// VALUE_PIECE_*
	uint64_t src;			// offset in the pool or in the text
	uint32_t len;			// > 0
};

// STACK: u32& word( level, k), k < VALUE_FRAME_WORDS -- the frame of a level: {part | flags, end of the parts, b, e, i}
// ITEMS: u32 variable( i), void format( i, fmt, nsub), bool span( i, begin, length) -- record i of the document's items
template <class STACK, class ITEMS>
struct ValueWalk
{
	enum { NOT_FIRST = 0x80000000u, SEP_DONE = 0x40000000u, PART_MASK = 0x3FFFFFFFu, NONE = 0xFFFFFFFFu };
	const ValueFormats& T;
	STACK& stack;
	const ITEMS& items;
	uint32_t depth;			// 0: the value is complete
	bool failed;			// the document fails (SP_DOC_ERR_RANGE)

	SPA_WALK_HD ValueWalk( const ValueFormats& T_, STACK& stack_, const ITEMS& items_) :T(T_), stack(stack_), items(items_), depth(0), failed(false) {}

	SPA_WALK_HD void push( uint32_t fmt, uint32_t b, uint32_t e)
	{
		stack.word( depth, 0) = T.fmtParts[ fmt]; stack.word( depth, 1) = T.fmtParts[ fmt+1];
		stack.word( depth, 2) = b; stack.word( depth, 3) = e; stack.word( depth, 4) = NONE;
		++depth;
	}

	// the value of format `fmt` (the caller has checked 1 <= fmt <= T.count) over the records [b, e) (inside the document)
	SPA_WALK_HD void start( uint32_t fmt, uint32_t b, uint32_t e) { depth = 0; failed = false; push( fmt, b, e); }

	// the next piece of the value; false when the value is complete or the document has failed
	SPA_WALK_HD bool next( ValuePiece& out)
	{
		while (depth && !failed)
		{
			const uint32_t lv = depth - 1;
			const uint32_t pw = stack.word( lv, 0), part = pw & PART_MASK;
			uint32_t i = stack.word( lv, 4);
			if (i == NONE)
			{
				// between two parts
				if (part >= stack.word( lv, 1)) { --depth; continue; }
				const uint32_t* P = T.parts + (uint64_t)VALUE_PART_WORDS * part;
				if (P[ 0] == VALUE_PART_LITERAL)
				{
					stack.word( lv, 0) = part + 1;
					if (!P[ 3]) continue;
					out.kind = VALUE_PIECE_POOL; out.src = P[ 2]; out.len = P[ 3];
					return true;
				}
				stack.word( lv, 0) = part;			// (no item of this part yet)
				stack.word( lv, 4) = i = stack.word( lv, 2);
			}
			// the walk of a variable part over the top-level records of the list
			const uint32_t* P = T.parts + (uint64_t)VALUE_PART_WORDS * part;
			const uint32_t e = stack.word( lv, 3);
			if (i >= e) { stack.word( lv, 0) = part + 1; stack.word( lv, 4) = NONE; continue; }
			uint32_t fmt, nsub;
			items.format( i, fmt, nsub);
			uint32_t follow = i + 1;
			if (fmt)
			{
				if (fmt > T.count || nsub > e - (i + 1)) { failed = true; break; }
				follow = i + 1 + nsub;
			}
			if (!P[ 1] || items.variable( i) != P[ 1]) { stack.word( lv, 4) = follow; continue; }
			const uint32_t flags = stack.word( lv, 0);
			if ((flags & NOT_FIRST) && !(flags & SEP_DONE) && P[ 3])
			{
				// the separator first; the record is met again by the next call
				stack.word( lv, 0) = flags | SEP_DONE;
				out.kind = VALUE_PIECE_POOL; out.src = P[ 2]; out.len = P[ 3];
				return true;
			}
			stack.word( lv, 0) = part | NOT_FIRST;
			stack.word( lv, 4) = follow;
			if (fmt)
			{
				if (depth >= VALUE_MAX_DEPTH) { failed = true; break; }
				push( fmt, i + 1, follow);
				continue;
			}
			uint64_t begin, length;
			if (!items.span( i, begin, length) || length > 0xFFFFFFFFull) { failed = true; break; }
			if (!length) continue;
			out.kind = VALUE_PIECE_TEXT; out.src = begin; out.len = (uint32_t)length;
			return true;
		}
		return false;
	}
};

} // namespace
#endif
