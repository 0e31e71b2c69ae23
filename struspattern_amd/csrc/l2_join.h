// RESULT-SET MODE (sp_matcher_ctx_create_ex( .., SP_CTX_RESULT_SETS), or SPA_L2_JOIN=1): the rule automaton WITHOUT
// materialised rule instances, for rule sets made of two-term programs (sequence, within, their _struct forms, any) that
// nobody listens to ("The ceiling").
// The reference installs an instance at every key event and retires it at the first later completing term or when it expires
// (src/ruleMatcherAutomaton.cpp:589-1334); the result MULTISET of a document follows from the positions alone:
//   (A at lexem i, B at lexem j) matches  iff  ordpos(i) < ordpos(j) <= ordpos(i) + range  and no B lies between them at a
//   position behind i's (that B would have taken the instance).
// Programs that the optimizer moved off a frequent key event A onto their other term B (DevKeyRef::pastEvent,
// ruleMatcherAutomaton.cpp:512-586) follow another predicate: an instance at every B that replays only the LATEST logged A,
// is cancelled by a delimiter logged after it, and lingers until it expires when it does not complete at once -- so a pair
// can match more than once.  JOIN_ALT_* below and tests/result_set_model.py (checked against the oracle) give its terms.
// So every lexem j looks back over the lexems of the last `maxRange` positions and asks a hash table keyed by the PAIR of event
// ids (id(i), id(j)) for the programs it completes -- lane-parallel over the lexems, no per-document state at all (a first
// version that sorted the document's (id, index) pairs in LDS and searched them per rule was 7 x SLOWER than the exact
// engine: it pays per (lexem, rule that ends with it) pair, which is as many as the exact engine's installs).
// What this mode does NOT reproduce: the order of the results inside a document (the reference's depends on the swap history
// of its trigger buckets) and the statistics (nothing is installed); results come in (end lexem, start lexem descending,
// rule) order.  Parity is therefore checked on result multisets (tests/test_l2_join_gpu.py, tests/test_result_sets_gpu.py).
#ifndef SPA_L2_JOIN_H
#define SPA_L2_JOIN_H
#include <stdint.h>
#include <string>
#include <vector>
#include "l2_device.h"

namespace spa {


struct JoinKey			// 16 B, open addressing by joinHash( first, second), first==0 = empty: the programs sequence( first, second | .. )
{
	uint32_t first, second;
	uint32_t begin;		// rules[begin .. begin+count), definition order
	uint32_t count;
};
// THE LIMIT of this mode: the counting pass hands every lexem's count to the writing pass as matches | items << 16
// (JoinParams::counts), so at most JOIN_COUNT_MAX = 32 767 matches may END AT ONE LEXEM (two items per match at most: 65 534
// fit the high half).  The count saturates: a document in which one lexem completes more fails with SP_DOC_ERR_RANGE, reserves
// nothing and writes nothing; the other documents of the batch are not affected.  The exact engine has no such limit.
// The sums of a document are 32 bit as well: a document of 2^32 results or items fails in the same way.
enum {JOIN_COUNT_MAX=0x7FFF};
enum {JOIN_COUNT_OVERFLOW=0xFFFFFFFFu};	// what the counting pass returns for a lexem beyond the limit (no valid count: its low half exceeds JOIN_COUNT_MAX)
enum {JOIN_FILTER_WORDS=4096};		// 16 KB = 131072 bits
enum {JOIN_SELF=0xFFFFFFFFu};		// `first` of the entries for any( .. ): the lexem alone is the match
enum {JOIN_STRUCT=1u};			// JoinRule::flags: no delimiter lexem may lie between the two terms (*_struct);
					// bits 8..15 / 16..23: the variable attached to the first / the completing term (0 = none)
// JoinRule::flags, entries of moved key references (A = id(i), B = id(j) of the pair (i, j), "taken": a B in (i, j) at a
// position behind i's):
enum {
	JOIN_ALT_SEQ=2u,		// sequence( A, B) keyed at B, past A:  [no A in (i, j)]  (the replay of the instance at j)
					//  + [not taken] * #{B in (i, next A) at ordpos(i)}  (instances of Bs beside i that replayed i)
					//  + [not taken] * #{B at k < i: ordpos(k) + range >= ordpos(j), ordpos(k) > ordpos(latest A before i)
					//     + range, no delimiter in (k, i)}  (instances of Bs without a replay that took i as their A)
	JOIN_ALT_REPLAY=4u,		// within( A, B) keyed at B, past A:  [no A in (i, j)]
	JOIN_ALT_LINGER=8u,		// within( .., ..) keyed at A, past B (pair A at i, B at j):  [not taken] *
					//  [no B before i at a position >= ordpos(i) - range]  (no replay: the instance waited for a B)
	JOIN_ALT=14u
};
struct JoinRule			// 16 B
{
	uint32_t range;
	uint32_t resultHandle;
	uint32_t formatHandle;
	uint32_t flags;
};
static inline
#if defined(__HIPCC__)
__host__ __device__
#endif
uint32_t joinHash( uint32_t first, uint32_t second)
{
	uint32_t h = first * 0x9E3779B1u ^ (second + 0x7F4A7C15u) * 0x85EBCA6Bu;
	h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12;
	return h;
}

struct JoinParams
{
	const JoinKey* keytab; uint32_t keymask;
	const JoinRule* rules;
	const uint32_t* filter;		// JOIN_FILTER_WORDS words: bit (joinHash( first, second) >> 8) % bits set for every table key -- copied to LDS,
					// so that most pairs of nearby lexems (which complete nothing) are refused without a memory access
	uint32_t* counts;		// per lexem of the batch: its number of matches | items << 16 (first pass -> second pass)
	uint64_t countsCapacity;	// lexem indices below it have a slot (a document beyond it counts twice instead)
	uint32_t maxRange;		// the largest position range of any program
	uint32_t delimiter;		// the delimiter event of the *_struct programs (0 = none)
	L2BatchIO io;
	uint32_t altRules;		// some rule has a JOIN_ALT_* flag: the look-back goes on behind a taking lexem
};

// enqueue the join kernel (l2_join_kernel.hip): one wave per document
hipError_t launchL2Join( const JoinParams& P, unsigned nwaves, hipStream_t stream);
// the join tables of a rule set (l2_join_tables.cpp), or the reason why it is not eligible
struct FlatTables;
std::string buildJoinTables( const FlatTables& ft, std::vector<JoinKey>& keytab, std::vector<JoinRule>& rules, std::vector<uint32_t>& filter, uint32_t& maxRange, uint32_t& delimiter, uint32_t& altPrograms);

} // namespace
#endif
