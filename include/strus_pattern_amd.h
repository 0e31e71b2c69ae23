/*
 * strus_pattern_amd.h -- C-ABI of the MI355X-native two-level pattern engine.
 *
 * This is the drop-in boundary underneath strus's PatternLexerInterface / PatternMatcherInterface
 * (the C++ shim in struspattern_amd/host/ implements those virtual interfaces on top of these
 * entry points; the module load point stays `modstrus_analyzer_pattern`).
 * Plain C: opaque handles, plain pointers and sizes, no C++ or torch types, no exceptions.
 * Every call returns 0 on success or a negative SP_ERR_* code; the message is retrievable with
 * sp_*_last_error(handle).  Buffers returned through `**out` parameters are owned by the caller
 * and released with sp_free().  Each entry point cites the reference interface it replaces
 * (paths relative to the strusPattern source tree).
 */
#ifndef STRUS_PATTERN_AMD_H
#define STRUS_PATTERN_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_OK                    0
#define SP_ERR_INVALID          -1   /* bad argument / call order (reference: std::runtime_error -> ErrorCodeRuntimeError) */
#define SP_ERR_NOMEM            -2   /* reference: std::bad_alloc -> ErrorCodeOutOfMem */
#define SP_ERR_DEVICE           -3   /* HIP runtime error, or no GPU / HIP extension unusable */
#define SP_ERR_COMPILE          -4   /* rule / regex compilation failed */
#define SP_ERR_MATCH            -5   /* at least one document failed, see per-document status */
#define SP_ERR_UNAVAILABLE      -6   /* the value does not exist for this context (statistics of a result-set context) */

/* per-document status codes written by the kernels (0 = ok) */
#define SP_DOC_OK                0
#define SP_DOC_ERR_ORDER         1   /* lexems not in ascending ordpos   (src/patternMatcher.cpp:136-139) */
#define SP_DOC_ERR_ARENA         2   /* per-document working set exceeded the arena (retry with a larger arena) */
#define SP_DOC_ERR_KEYTRIGGERS   3   /* >32 identical key events in one pattern (src/ruleMatcherAutomaton.cpp:1213-1216) */
#define SP_DOC_ERR_PASTFOLLOW    4   /* "encountered past trigger with follow" (src/ruleMatcherAutomaton.cpp:1328-1332) */
#define SP_DOC_ERR_RANGE         5   /* origsize/origpos out of range    (src/patternMatcher.cpp:144-155); in result-set mode
                                       (SP_CTX_RESULT_SETS on the join kernel) also: more than 32 767 matches end at one lexem */
#define SP_DOC_ERR_DATAREF       6   /* "illegal free of event data reference" (src/ruleMatcherAutomaton.cpp:726-731) */
#define SP_DOC_ERR_LEXEMSIZE     7   /* matched lexem >= 65535 bytes    (src/patternLexer.cpp:727-730) */
#define SP_DOC_ERR_INTERNAL      8   /* a list walk exceeded its bound: corrupted per-document state (bug) */
#define SP_DOC_ERR_OUTPUT        9   /* result/item output buffer too small (host entry points grow it and rerun) */

/* strus::PatternMatcherInstanceInterface::JoinOperation, in the order of the switch at
 * src/patternMatcher.cpp:401-440 */
enum sp_join_op {
	SP_OP_SEQUENCE = 0, SP_OP_SEQUENCE_IMM = 1, SP_OP_SEQUENCE_STRUCT = 2,
	SP_OP_WITHIN = 3, SP_OP_WITHIN_STRUCT = 4, SP_OP_ANY = 5, SP_OP_AND = 6
};

/* strus::analyzer::PositionBind (src/patternLexer.cpp:902-915) */
enum sp_position_bind {
	SP_BIND_CONTENT = 0, SP_BIND_SUCCESSOR = 1, SP_BIND_PREDECESSOR = 2, SP_BIND_UNIQUE = 3
};

/* analyzer::PatternLexem(id, ordpos, Position(seg, ofs), origsize)  (src/patternLexer.cpp:908).
 * 16 bytes; the segment index travels in a parallel optional array: 0 for everything out of the lexer, the index of the
 * segment inside its document after sp_lexer_ctx_stitch_segments_device. */
typedef struct sp_lexem {
	uint32_t id;
	uint32_t ordpos;
	uint32_t origpos;
	uint32_t origsize;
} sp_lexem_t;

/* analyzer::PatternMatcherResult minus strings = strus::Result (src/ruleMatcherAutomaton.hpp:273-289),
 * 36 bytes.  `handle` maps to the pattern name with sp_matcher_pattern_name(). */
typedef struct sp_result {
	uint32_t handle;
	uint32_t ordpos;
	uint32_t ordend;
	uint32_t origseg;
	uint32_t origpos;
	uint32_t origendseg;
	uint32_t origend;
	uint32_t item_begin;   /* index of the first item of this result in the items array */
	uint32_t item_count;
} sp_result_t;

/* analyzer::PatternMatcherResultItem minus strings (src/patternMatcher.cpp:182) */
typedef struct sp_result_item {
	uint32_t variable;     /* maps to the variable name with sp_matcher_variable_name() */
	uint32_t ordpos;
	uint32_t ordend;
	uint32_t origseg;
	uint32_t origpos;
	uint32_t origendseg;
	uint32_t origend;
} sp_result_item_t;

/* analyzer::PatternMatcherStatistics items (src/patternMatcher.cpp:303-318) */
typedef struct sp_matcher_stats {
	double nofProgramsInstalled;
	double nofAltKeyProgramsInstalled;
	double nofSignalsFired;
	double nofTriggersAvgActive;
} sp_matcher_stats_t;

typedef struct sp_matcher sp_matcher_t;          /* PatternMatcherInstanceInterface */
typedef struct sp_matcher_ctx sp_matcher_ctx_t;  /* PatternMatcherContextInterface (+ batch mode) */
typedef struct sp_lexer sp_lexer_t;              /* PatternLexerInstanceInterface */
typedef struct sp_lexer_ctx sp_lexer_ctx_t;      /* PatternLexerContextInterface (+ batch mode) */

/* ---- library ---- */
const char* sp_version(void);
/* number of usable HIP devices (0 when no GPU is visible); never initialises more than the runtime */
int sp_device_count(void);
void sp_free(void* p);
/* test hook (tests only): device allocations of at least `bytes` fail like an out-of-memory hipMalloc; 0 switches it off */
void sp_test_fail_alloc_above(uint64_t bytes);
/* test hook (tests only, needs no device): what sp_matcher_ctx_batch_fetch_docs(first_doc, ndocs) makes of a batch of batch_ndocs
 * documents, run over host arrays in the layout the kernels leave on the device: `results` / `items` with the counts that lie
 * inside the buffers, the optional format handles (both or none), per document a (first, count) range of results in `doc_ranges`
 * and a status; `exclusive`, `max_result_size`: the matcher's options.  Fills `out` (sp_match_batch_free; doc_stats all 0);
 * SP_ERR_INVALID with the message in `err` otherwise. */
struct sp_match_batch;
int sp_match_batch_regroup(const sp_result_t* results, uint64_t nresults, const sp_result_item_t* items, uint64_t nitems,
	const uint32_t* result_format, const uint32_t* item_format, const uint64_t* doc_ranges, const int32_t* doc_status,
	size_t batch_ndocs, size_t first_doc, size_t ndocs, int exclusive, uint32_t max_result_size,
	struct sp_match_batch* out, char* err, size_t errsize);

/* ==== level 2: token pattern matcher ==== */

/* strus::createPatternMatcher_std + PatternMatcherInterface::createInstance
 * (src/libstrus_pattern.cpp:21-33, src/patternMatcher.cpp:718-726) */
sp_matcher_t* sp_matcher_create(void);
void sp_matcher_free(sp_matcher_t* m);
const char* sp_matcher_last_error(const sp_matcher_t* m);

/* PatternMatcherInstanceInterface (src/patternMatcher.cpp:361-671), same argument meaning */
int sp_matcher_define_term_frequency(sp_matcher_t* m, uint32_t termid, double df);                 /* :361 */
int sp_matcher_push_term(sp_matcher_t* m, uint32_t termid);                                         /* :366 */
int sp_matcher_push_expression(sp_matcher_t* m, int joinop, size_t argc, uint32_t range, uint32_t cardinality); /* :377 */
int sp_matcher_push_pattern(sp_matcher_t* m, const char* name);                                     /* :510 */
int sp_matcher_attach_variable(sp_matcher_t* m, const char* name);                                  /* :522 */
int sp_matcher_define_pattern(sp_matcher_t* m, const char* name, const char* formatstring, int visible); /* :545 */
int sp_matcher_define_option(sp_matcher_t* m, const char* name, double value);                      /* :614 */
int sp_matcher_compile(sp_matcher_t* m);                                                            /* :646 */
/* symbol tables behind result handles / item variables (patternMap / variableMap, :82-83) */
uint32_t sp_matcher_pattern_id(const sp_matcher_t* m, const char* name);
const char* sp_matcher_pattern_name(const sp_matcher_t* m, uint32_t handle);
uint32_t sp_matcher_variable_id(const sp_matcher_t* m, const char* name);
const char* sp_matcher_variable_name(const sp_matcher_t* m, uint32_t variable);
/* canonical dump of the compiled ProgramTable (test hook; format in csrc/l2_compile.hpp) */
size_t sp_matcher_dump_table(const sp_matcher_t* m, uint32_t** out);
/* which kernel a context of this matcher runs on (test / diagnostics hook): 1 = the rule set is flat (every program
 * has at most 3 triggers over input terms, position range <= 63, no rule listens to another rule's result) and its
 * documents run with their whole hot state in LDS; 0 = general kernel, `why` says what disqualifies it.
 * Both kernels produce the reference's results (src/ruleMatcherAutomaton.cpp:772-1334); the choice is not observable. */
int sp_matcher_fast_tier(const sp_matcher_t* m, char* why, size_t whysize);
/* whether a context created with SP_CTX_RESULT_SETS runs this compiled matcher on the join kernel (result-set mode,
 * csrc/l2_join.h): 1 = it does, and `alt_programs` (may be NULL) receives the number of programs whose key the optimizer
 * moved off a frequent event (they follow the reference's replay of the latest logged key event); 0 = it runs on the exact
 * engine, `why` says what disqualifies it (programs of more or fewer than two terms, nested programs, `and`, more than one
 * delimiter, the `exclusive` option -- whose outcome depends on the order of the results). */
int sp_matcher_result_set_tier(const sp_matcher_t* m, char* why, size_t whysize, uint32_t* alt_programs);
/* What a context created now with `ctx_flags` (sp_matcher_ctx_create_ex) on a device of num_cus compute units (0 = 256), where
 * fast_blocks_per_cu workgroups of the LDS-resident kernel fit a compute unit, launches for a batch of ndocs documents and nlexems
 * lexems, and why -- the decisions of csrc/l2_plan.hpp without a device.  rerun_docs > 0: the partial rerun of that many documents
 * of the batch; arena_grows: after that many sp_matcher_ctx_grow_arena; min_results, min_items: what sp_matcher_ctx_reserve_output
 * has reserved.  Writes key=value fields, one per line (the reasons are texts with blanks):
 *   engine            general | flat | join, kind = what sp_matcher_ctx_kernel_kind returns, kernel = sp_matcher_ctx_kernel_name
 *   flat_why_not, join_why_not   empty for an engine the rule set can run on; alt_programs as sp_matcher_result_set_tier
 *   route             general | flat+list | join | rerun-list: the kernels of this launch
 *   general_blocks, arena_run, arena_alloc, arena_alloc_waves (the waves allocated when the arena has to grow),
 *   arena_per_wave_bytes, arena_max_rules, arena_scratch_cap, stop_words      the general kernel and its per-wave arena
 *   fast_blocks, spill_alloc_waves, spill_per_wave_bytes, list_blocks         the LDS-resident kernel, the general one behind it
 *   join_blocks, want_results, want_items (capacities of the output buffers, which only grow)
 *   R, T, exp_shift, spill_words, max_rules, max_staged, bucket_caps (16, comma separated)   the LDS-resident kernel's layout
 * The SPA_L2_* switches of the environment count as they do for a context created now.  SP_ERR_INVALID when the arena cannot
 * grow that often, for a batch of too many documents or when the text does not fit bufsize. */
int sp_matcher_launch_plan(const sp_matcher_t* m, uint32_t ctx_flags, unsigned num_cus, unsigned fast_blocks_per_cu,
                           size_t ndocs, size_t nlexems, size_t rerun_docs, uint32_t arena_grows,
                           uint64_t min_results, uint64_t min_items, char* buf, size_t bufsize);

/* Compiled-table serialisation (the reference has none -- every process recompiles, and with
 * Hyperscan that takes seconds for 10k patterns, src/patternLexer.cpp:1068-1118): the rule set with its key
 * index, stop words, names, format strings and options as one self-checking blob (magic, version, FNV-1a 64),
 * so that the ranks of a multi-GPU job or the workers of a service load it instead of compiling.  The blob is
 * malloc'ed (sp_free); a loaded matcher behaves like the one that was saved (same tables word for word).
 * sp_matcher_deserialize returns NULL and the reason in `err` for a blob that is truncated, corrupt or foreign. */
int sp_matcher_serialize(const sp_matcher_t* m, void** blob, size_t* size);
sp_matcher_t* sp_matcher_deserialize(const void* blob, size_t size, char* err, size_t errsize);

/* ---- result format strings (definePattern's formatstring, src/patternMatcher.cpp:561-566, :172-181, :253-262).
 * The matcher kernels do not build strings: they report which format applies and what its arguments are; the device
 * builds the strings on request, from a finished batch (see "result values" below).
 *   - a result with a format handle: its item list holds the ARGUMENTS of the format string; the
 *     reference returns such a result with a value and an empty item list (:253-262).
 *   - an item with a format handle (a variable bound to a sub-pattern that has a format string): the
 *     `nsub` records that follow it are the arguments of ITS format (nested the same way) and are not
 *     items of the enclosing list (:172-181); items without a format are followed by their sub-items
 *     as siblings (:185-188), as in a matcher without format strings.
 * Format strings are numbered 1..sp_matcher_format_count() in definePattern order.  The formatter
 * itself (PatternResultFormat) lives in strusAnalyzer, outside the reference repository; the host
 * mirrors implement "{variable}" / "{variable|separator}" substitution as its documentation describes. */
uint32_t sp_matcher_format_count(const sp_matcher_t* m);
const char* sp_matcher_format_string(const sp_matcher_t* m, uint32_t format_handle);

/* PatternMatcherInstanceInterface::createContext (src/patternMatcher.cpp:586).  `device` is the
 * HIP device ordinal.  Fails with SP_ERR_DEVICE when no GPU is usable: there is no CPU fallback. */
sp_matcher_ctx_t* sp_matcher_ctx_create(const sp_matcher_t* m, int device);
/* sp_matcher_ctx_create with flags.  SP_CTX_RESULT_SETS: the context returns, per document, the right MULTISET of results
 * with their items -- not the reference's order of the results inside a document, and no statistics
 * (sp_matcher_ctx_statistics returns SP_ERR_UNAVAILABLE).  An eligible rule set (sp_matcher_result_set_tier) runs on the
 * join kernel (sp_matcher_ctx_kernel_kind 2), any other on the exact engine, whose results are a correct multiset too.
 * The join kernel has one limit the exact engine has not: a document in which ONE lexem completes more than 32 767 matches
 * fails with SP_DOC_ERR_RANGE and is empty (the other documents of the batch are not affected; csrc/l2_join.h).
 * The environment variable SPA_L2_JOIN=1 at context creation sets this flag on every context (sp_matcher_ctx_create too). */
#define SP_CTX_RESULT_SETS       1u
sp_matcher_ctx_t* sp_matcher_ctx_create_ex(const sp_matcher_t* m, int device, uint32_t flags);
void sp_matcher_ctx_free(sp_matcher_ctx_t* c);
const char* sp_matcher_ctx_last_error(const sp_matcher_ctx_t* c);

/* PatternMatcherContextInterface::putInput (src/patternMatcher.cpp:131): appends lexems of the
 * current document (host side, ascending ordpos); origseg may be NULL (= all 0). */
int sp_matcher_ctx_put_input(sp_matcher_ctx_t* c, const sp_lexem_t* lexems, const uint32_t* origseg, size_t n);
/* PatternMatcherContextInterface::fetchResults (:271): runs the document on the GPU. */
int sp_matcher_ctx_fetch_results(sp_matcher_ctx_t* c, sp_result_t** results, size_t* nresults,
                                 sp_result_item_t** items, size_t* nitems);
/* format handles of the results / items of the last sp_matcher_ctx_fetch_results (borrowed pointers,
 * valid until the next fetch or reset; NULL when the matcher has no format strings) */
int sp_matcher_ctx_fetch_formats(sp_matcher_ctx_t* c, const uint32_t** result_format, const uint32_t** item_format);
/* PatternMatcherContextInterface::getStatistics (:303) of the last fetch; SP_ERR_UNAVAILABLE (and zeros) on a context
 * that runs in result-set mode on the join kernel, which installs nothing */
int sp_matcher_ctx_statistics(sp_matcher_ctx_t* c, sp_matcher_stats_t* out);
/* PatternMatcherContextInterface::reset (:320) */
int sp_matcher_ctx_reset(sp_matcher_ctx_t* c);

/* ---- batch mode: one Context per document, many documents per launch
 *      (the reference runs one Context per document per thread,
 *       tests/randomTokenPatternMatch/src/testRandomTokenPatternMatch.cpp:130-146, :325-345) ---- */
typedef struct sp_match_batch {
	size_t ndocs;
	size_t nresults;
	size_t nitems;
	sp_result_t* results;          /* grouped by document, firing order inside a document */
	sp_result_item_t* items;
	uint64_t* doc_result_offsets;  /* ndocs+1 */
	uint64_t* doc_stats;           /* ndocs x 4: programs installed, alt-key programs installed, signals fired, sum of active triggers */
	int32_t* doc_status;           /* ndocs x SP_DOC_* */
	/* matchers with format strings only (else NULL), see "result format strings" below */
	uint32_t* result_format;       /* nresults: format handle of the result (0 = none) */
	uint32_t* item_format;         /* nitems x {format handle of the item, nsub} */
} sp_match_batch_t;

/* host buffers in, host buffers out (PCIe both ways) */
int sp_matcher_ctx_match_docs(sp_matcher_ctx_t* c, const sp_lexem_t* lexems, const uint32_t* origseg,
                              const uint64_t* doc_offsets, size_t ndocs, sp_match_batch_t* out);
void sp_match_batch_free(sp_match_batch_t* b);

/* device-resident variant: d_lexems / d_origseg (may be NULL) / d_doc_offsets are device pointers,
 * the launch is asynchronous on `stream` (a hipStream_t, NULL = default stream); results stay in HBM. */
typedef struct sp_match_device_batch {
	size_t ndocs;
	void* d_results;             /* sp_result_t[result_capacity]: whole documents in COMPLETION order, not document order;
	                                sp_matcher_ctx_batch_finish_device puts them in document order */
	void* d_items;               /* sp_result_item_t[] */
	void* d_doc_result_offsets;  /* uint64_t[ndocs][2] = (first result, count) of every document */
	void* d_doc_stats;           /* uint64_t[ndocs*4] */
	void* d_doc_status;          /* int32_t[ndocs] */
	void* d_counters;            /* uint64_t[8]: results, items, events, failed docs, ... */
	void* d_result_format;       /* uint32_t[] parallel to d_results, NULL without format strings */
	void* d_item_format;         /* uint32_t[][2] parallel to d_items, NULL without format strings */
} sp_match_device_batch_t;
int sp_matcher_ctx_match_docs_device(sp_matcher_ctx_t* c, const void* d_lexems, const void* d_origseg,
                                     const void* d_doc_offsets, size_t ndocs, size_t nlexems,
                                     void* stream, sp_match_device_batch_t* out);
/* fused pipeline entry: the lexems and per-document (first, count) ranges produced by
 * sp_lexer_ctx_match_docs_device are consumed in place, nothing leaves HBM in between */
int sp_matcher_ctx_match_lexed_device(sp_matcher_ctx_t* c, const void* d_lexems, const void* d_doc_ranges,
                                      size_t ndocs, size_t nlexems_hint, void* stream, sp_match_device_batch_t* out);
/* Finishes the last batch of this context on the device: what sp_matcher_ctx_batch_fetch returns, left in HBM.  The raw
 * batch above is in completion order, with results of failed documents, without the `exclusive` elimination
 * (src/patternMatcher.cpp:192-246, :278-289) and with item indices into a buffer with gaps; the finished one has none of
 * that.  The buffers belong to the context (allocated at the first call, a context that never finishes has none) and
 * are valid until the next finish on it; the raw batch stays as it is. */
typedef struct sp_match_finished_batch {
	size_t ndocs;
	void* d_results;             /* sp_result_t[]: document 0's results first; inside a document the order the
	                                engine produced, or with SP_FINISH_CANONICAL ascending by the tuple T below; `exclusive` applied;
	                                item_begin indexes d_items below */
	void* d_items;               /* sp_result_item_t[], in result order, no gaps */
	void* d_doc_result_offsets;  /* uint64_t[ndocs+1]; a failed document (d_doc_status != 0) has an empty range */
	void* d_doc_item_offsets;    /* uint64_t[ndocs+1] */
	void* d_result_format;       /* parallel to d_results / d_items, NULL without format strings */
	void* d_item_format;
	void* d_totals;              /* uint64_t[2]: results, items */
} sp_match_finished_batch_t;
/* Enqueues the finishing passes (count, offsets, place: csrc/l2_finish.h) on `stream` and returns; the call itself waits
 * for the batch only to read its counters, from which it sizes the buffers.  A `stream` other than the batch's is ordered
 * behind the batch with an event.  SP_ERR_INVALID before any batch has run on the context.  The next batch on the
 * context invalidates the finished state (not the buffers: a consumer still reading them orders itself as with any
 * stream work); it works on whatever the last launch sequence left, the reruns of sp_matcher_ctx_match_docs included. */
int sp_matcher_ctx_batch_finish_device(sp_matcher_ctx_t* c, void* stream, sp_match_finished_batch_t* out);
/* sp_matcher_ctx_batch_finish_device with flags; 0 is exactly that call, unknown bits return SP_ERR_INVALID.
 * SP_FINISH_CANONICAL: inside each document the surviving results are ascending by the tuple
 *   T(r) = ( ordpos, ordend, origseg, origpos, origendseg, origend,    words 1..6 of the record
 *            handle,                                                   word 0
 *            item_count,                                               word 8
 *            result_format[r]                    (matchers with format strings only),
 *            the 7*item_count words of r's items, in item order,
 *            the 2*item_count words of item_format for those items     (with format strings only) )
 * compared lexicographically, every word as an unsigned 32-bit value.  item_begin (word 7) is not part of the key: it is
 * assigned after the sort, the block start plus the item counts of the results before.  Two results with equal T have
 * byte-identical finished records, so the finished bytes are a function of the results alone and not of the engine that
 * produced them: the same from the general, the LDS-resident and the join kernel (result-set mode).  Everything else is
 * as without the flag: document order, failed documents empty, `exclusive` evaluated on the engine's order (the
 * survivors are sorted), items gapless in result order, the same offsets and totals.  The working memory of the sort
 * (24 bytes per result of the batch) belongs to the context and is allocated at the first finish that asks for it. */
#define SP_FINISH_CANONICAL      1u
int sp_matcher_ctx_batch_finish_device_ex(sp_matcher_ctx_t* c, void* stream, uint32_t flags, sp_match_finished_batch_t* out);
/* plain copy of the finished buffers to the host (plus doc_stats and doc_status of the batch): NO regrouping and NO
 * elimination on the host; field for field what sp_matcher_ctx_batch_fetch returns for the same batch.
 * SP_ERR_INVALID when the last batch has not been finished. */
int sp_matcher_ctx_finished_fetch(sp_matcher_ctx_t* c, sp_match_batch_t* out);
/* durations of the three passes of the last finish in milliseconds (HIP events on its stream; waits for them);
 * place_ms is the final placement, also after a canonical finish */
int sp_matcher_ctx_last_finish_ms(sp_matcher_ctx_t* c, double* count_ms, double* offsets_ms, double* place_ms);
/* duration of the sorting pass of the last finish, between offsets and place (HIP events on its stream); 0.0 after a
 * finish without SP_FINISH_CANONICAL */
int sp_matcher_ctx_last_finish_sort_ms(sp_matcher_ctx_t* c, double* sort_ms);
/* diagnostics and tests: the largest number of results of one document that the canonical sort orders inside one
 * workgroup's LDS, without a merge pass */
uint32_t sp_matcher_finish_sort_tile(void);

/* ---- matched text: the bytes that the results and items of a finished batch cover, gathered on the device
 * (csrc/l2_text.h) or, for a batch already fetched, on the host (csrc/span_text.hpp).  The rule is the project's own,
 * unpinned by a reference vector (the reference has no such call; its tools slice the source on the host,
 * tests/utils/testUtils.cpp:125-150).  The text is the one the lexer batch ran on, all segments back to back;
 * seg_offsets[nseg+1] is the array given to sp_lexer_ctx_match_docs_device, doc_seg_offsets[ndocs+1] the one given to
 * sp_lexer_ctx_stitch_segments_device, or NULL: document d is segment d then, and nseg must be ndocs (SP_ERR_INVALID).
 * Words 3..6 of a result or item record are (origseg, origpos, origendseg, origend).  For a span of document d,
 *   s0 = doc_seg_offsets[d] + origseg, s1 = doc_seg_offsets[d] + origendseg,
 *   bytes = text[ seg_offsets[s0] + origpos, seg_offsets[s1] + origend )
 * -- ONE contiguous range also when the span crosses segments: the tail of its first segment, the whole segments between
 * and the head of its last; bytes that a segmenter removed between segments are not part of it.  A span is valid when
 *   doc_seg_offsets[d] <= doc_seg_offsets[d+1] <= nseg,   origseg <= origendseg < doc_seg_offsets[d+1] - doc_seg_offsets[d],
 *   origpos <= len(s0), origend <= len(s1),   begin <= end <= nbytes,   and the seg_offsets used ascend.
 * A document with an invalid span in a requested family, or whose spans of one family add up to 2^32 bytes or more, has
 * text status SP_DOC_ERR_RANGE and ALL its spans are empty (the stitch's rule: it fails and is empty); the other documents
 * are not affected.  A document without spans (one the matcher failed among them) has text status 0.  No byte outside
 * [0, nbytes) of the text is read and none outside the output buffers written, whatever the records hold. */
#define SP_TEXT_RESULTS 1u
#define SP_TEXT_ITEMS   2u
typedef struct sp_text_source {
	const void* d_text;            /* device: uint8_t[nbytes] */
	uint64_t nbytes;
	const void* d_seg_offsets;     /* device: uint64_t[nseg+1] */
	size_t nseg;
	const void* d_doc_seg_offsets; /* device: uint64_t[ndocs+1]; may be NULL */
} sp_text_source_t;
typedef struct sp_match_text_batch {
	size_t ndocs;
	void* d_result_text;           /* uint8_t[]: the text of result 0 of the finished d_results first */
	void* d_result_text_offsets;   /* uint64_t[nresults+1], parallel to the finished d_results; the spans of a failed
	                                  document all sit on the document's offset */
	void* d_item_text;             /* the same, parallel to the finished d_items */
	void* d_item_text_offsets;
	void* d_doc_text_status;       /* int32_t[ndocs]: 0 or SP_DOC_ERR_RANGE */
	void* d_totals;                /* uint64_t[2]: result bytes, item bytes */
} sp_match_text_batch_t;
/* host copy of a text batch (sp_match_text_free); a family that was not asked for has NULL pointers and a total of 0 */
typedef struct sp_match_text {
	size_t ndocs;
	size_t nresults;
	size_t nitems;
	char* result_text;
	uint64_t* result_text_offsets; /* nresults+1 */
	char* item_text;
	uint64_t* item_text_offsets;   /* nitems+1 */
	int32_t* doc_text_status;      /* ndocs */
	uint64_t totals[2];            /* result bytes, item bytes */
} sp_match_text_t;
/* Gathers the text of the batch finished last on this context (sp_matcher_ctx_batch_finish_device[_ex], either order; the
 * text follows the finished order).  flags: SP_TEXT_RESULTS | SP_TEXT_ITEMS; a family that is not requested has NULL
 * pointers in `out`.  Three passes per family on `stream` (count, offsets, place: csrc/l2_text.h); the call enqueues count
 * and offsets, waits for them to read the totals, sizes the buffers and enqueues the placement, which it does not wait
 * for.  The buffers belong to the context, are allocated at the first call, only grow, and are valid until the next text
 * call; the next batch or finish invalidates the state, not the buffers.  A `stream` other than the finish's is ordered
 * behind it with an event.  SP_ERR_INVALID when the last batch is not finished, for flags 0 or unknown bits, and for a
 * NULL source; SP_ERR_NOMEM when a buffer cannot be allocated (the context stays usable). */
int sp_matcher_ctx_finished_text_device(sp_matcher_ctx_t* c, const sp_text_source_t* src, uint32_t flags, void* stream, sp_match_text_batch_t* out);
/* plain copy of the buffers of the last sp_matcher_ctx_finished_text_device to the host (waits for it) */
int sp_matcher_ctx_finished_text_fetch(sp_matcher_ctx_t* c, sp_match_text_t* out);
void sp_match_text_free(sp_match_text_t* t);
/* duration of all passes of the last text call in milliseconds (HIP events on its stream round them; waits for them; the
 * host's wait for the totals between offsets and place lies inside) */
int sp_matcher_ctx_last_text_ms(sp_matcher_ctx_t* c, double* ms);
/* diagnostics and tests: spans of at least this many bytes are copied by their whole wave in a loop of their own */
uint32_t sp_matcher_text_long_span(void);
/* The same rule over host arrays, needs no device: the text of a batch already fetched (sp_matcher_ctx_finished_fetch,
 * sp_matcher_ctx_batch_fetch, sp_matcher_ctx_match_docs), and the yardstick of the device passes.  The items of document d
 * are taken to follow those of document d-1 without gaps, in result order.  Fills `out` (sp_match_text_free);
 * SP_ERR_INVALID with the message in `err` for flags 0 or unknown bits, a NULL source, nseg != ndocs without
 * doc_seg_offsets, and a batch whose offsets and item counts do not cover its results and items. */
int sp_match_batch_text(const sp_match_batch_t* mb, const char* text, uint64_t nbytes, const uint64_t* seg_offsets,
                        size_t nseg, const uint64_t* doc_seg_offsets, uint32_t flags,
                        sp_match_text_t* out, char* err, size_t errsize);

/* ---- result values: the values of the format strings of a finished batch -- what an index stores as a feature beside the
 * pattern name ("3'645 Eur" -> "EUR 3'645") -- built on the device (csrc/l2_values.h) or, for a batch already fetched, on the
 * host (csrc/result_values.hpp).  The rule is the project's own restatement of resultformat.Formatter and of the host shim,
 * unpinned by a reference vector beyond the one example of the reference's web page (PatternResultFormat lives in
 * strusAnalyzer).
 * The format table is built on the host at every sp_matcher_compile (a loaded rule set rebuilds it from its format strings;
 * the blob is unchanged; without a compile, or when format strings or variable names were added since, the first values call
 * that finds the counts changed builds it).  A context uploads the table it finds at its FIRST values call and keeps it:
 * create the contexts that build values after the last definition of the rule set, as for the rule tables themselves.  For every format handle f in 1..sp_matcher_format_count() it holds the parts of the string:
 *   - "\x" is the literal byte x (a backslash at the end stands for itself);
 *   - "{var}" and "{var|sep}" are variable parts: the name without its bytes <= 32 at both ends, the separator one blank by
 *     default and empty for an empty text behind '|'; the part holds the variable handle of the rule set for that name, or
 *     0 when the rule set has no such variable -- such a part matches no argument;
 *   - everything else is literal bytes.  Literals and separators live in one byte pool.
 * A format string that does not parse (no '}' behind a '{', an empty variable name) is no error of definePattern; it makes
 * the values calls below fail with SP_ERR_INVALID and a message that names the format.
 * A list is a range [b, e) of the finished item records.  Its top-level records are found by walking i = b: with
 * (fmt_i, nsub_i) = item_format[i], the arguments of a record with fmt_i != 0 are [i+1, i+1+nsub_i) and the next top-level
 * record is i+1+nsub_i; behind a record without a format it is i+1.  eval( f, [b,e) ) concatenates the parts of f: a literal
 * part gives its bytes; a variable part v gives, for every top-level record of the list whose word 0 is v, in list order,
 * joined by the part's separator: eval( fmt_i, its arguments ) if fmt_i != 0, else the bytes of its span under the
 * matched-text rule above (words 3..6, seg_offsets, doc_seg_offsets), unchanged.
 *   SP_VALUE_RESULTS  result r has a value iff result_format[r] != 0: eval( result_format[r], [item_begin, item_begin+item_count) )
 *   SP_VALUE_ITEMS    item record i has a value iff item_format[i][0] != 0: eval over its nsub records; for every such
 *                     record, the nested ones included
 * A record without a format has an empty value range; the format arrays tell an empty value from no value.
 * A document fails -- value status SP_DOC_ERR_RANGE, ALL its value ranges of both families empty, the other documents not
 * affected -- when the evaluation of a requested value meets one of these: a span that it uses is invalid under the text
 * rule; a format handle (of the value's record or of a top-level record of a list it walks for a variable part) exceeds the
 * format count; such a record's nsub runs beyond the list (for the value's own record: beyond the items of the document, as
 * a result's item range does); more than sp_matcher_value_max_depth() formats are under evaluation inside each other (8: the
 * value itself is level 1; the device keeps the walk's stack of 5 words per level and lane in LDS, 40 KB per workgroup);
 * the document has 2^32 items or more; or the values of one family add up to 2^32 bytes or more.  Records and spans that no
 * requested value uses are not looked at.  A document the matcher failed, or one without formatted records, has status 0; a
 * matcher without format strings yields all-empty ranges and status 0.  No byte outside [0, nbytes) of the text is read,
 * none outside the outputs written and no record at or beyond the finished totals read, whatever the records hold. */
#define SP_VALUE_RESULTS 1u
#define SP_VALUE_ITEMS   2u
typedef struct sp_match_values_batch {
	size_t ndocs;
	void* d_result_values;         /* uint8_t[]: the value of result 0 of the finished d_results first */
	void* d_result_value_offsets;  /* uint64_t[nresults+1], parallel to the finished d_results; the values of a failed
	                                  document all sit on the document's offset */
	void* d_item_values;           /* the same, parallel to the finished d_items */
	void* d_item_value_offsets;
	void* d_doc_value_status;      /* int32_t[ndocs]: 0 or SP_DOC_ERR_RANGE */
	void* d_totals;                /* uint64_t[2]: result bytes, item bytes */
} sp_match_values_batch_t;
/* host copy of a values batch (sp_match_values_free); a family that was not asked for has NULL pointers and a total of 0 */
typedef struct sp_match_values {
	size_t ndocs;
	size_t nresults;
	size_t nitems;
	char* result_values;
	uint64_t* result_value_offsets; /* nresults+1 */
	char* item_values;
	uint64_t* item_value_offsets;   /* nitems+1 */
	int32_t* doc_value_status;      /* ndocs */
	uint64_t totals[2];             /* result bytes, item bytes */
} sp_match_values_t;
/* Builds the values of the batch finished last on this context (sp_matcher_ctx_batch_finish_device[_ex], either order; the
 * values follow the finished order).  flags: SP_VALUE_RESULTS | SP_VALUE_ITEMS; a family that is not requested has NULL
 * pointers in `out`.  Three passes per family on `stream` (count, offsets, place: csrc/l2_values.h); the call enqueues count
 * and offsets, waits for them to read the totals, sizes the buffers and enqueues the placement, which it does not wait
 * for.  The buffers belong to the context, are allocated at the first call, only grow, and are valid until the next values
 * call; the format table is uploaded once per context, at the first call; the next batch or finish invalidates the state,
 * not the buffers.  A `stream` other than the finish's is ordered behind it with an event.  SP_ERR_INVALID when the last
 * batch is not finished, for flags 0 or unknown bits, for a NULL source and for a format string that does not parse;
 * SP_ERR_NOMEM when a buffer cannot be allocated (the context stays usable). */
int sp_matcher_ctx_finished_values_device(sp_matcher_ctx_t* c, const sp_text_source_t* src, uint32_t flags, void* stream, sp_match_values_batch_t* out);
/* plain copy of the buffers of the last sp_matcher_ctx_finished_values_device to the host (waits for it) */
int sp_matcher_ctx_finished_values_fetch(sp_matcher_ctx_t* c, sp_match_values_t* out);
void sp_match_values_free(sp_match_values_t* v);
/* duration of all passes of the last values call in milliseconds (HIP events on its stream round them; waits for them; the
 * host's wait for the totals between offsets and place lies inside) */
int sp_matcher_ctx_last_values_ms(sp_matcher_ctx_t* c, double* ms);
/* the number of formats that may be under evaluation inside each other (a compile-time constant) */
uint32_t sp_matcher_value_max_depth(void);
/* The same rule over host arrays, needs no device: the values of a batch already fetched (sp_matcher_ctx_finished_fetch,
 * sp_matcher_ctx_batch_fetch, sp_matcher_ctx_match_docs) of matcher `m`, and the yardstick of the device passes.  The items of
 * document d are taken to follow those of document d-1 without gaps, in result order.  Fills `out` (sp_match_values_free);
 * SP_ERR_INVALID with the message in `err` under the rules of sp_match_batch_text, and for a format string that does not parse. */
int sp_match_batch_values(const sp_matcher_t* m, const sp_match_batch_t* mb, const char* text, uint64_t nbytes,
                          const uint64_t* seg_offsets, size_t nseg, const uint64_t* doc_seg_offsets, uint32_t flags,
                          sp_match_values_t* out, char* err, size_t errsize);

/* ---- pattern frequencies: per document, which patterns matched, how often and where first and last -- the feature
 * frequency an index, a tagger or a classifier takes from a document -- and over the batch the document and collection
 * frequency per pattern; summed on the device (csrc/l2_freq.h) or, for a batch already fetched, on the host
 * (csrc/pattern_freq.hpp).  The rule is the project's own, unpinned by a reference vector (the reference has no such call).
 * Handles are the pattern handles of the rule set: valid ones run from 1 to the number of pattern names np, the handle
 * bound is np + 1 (sp_matcher_handle_bound).  For the batch finished last, `exclusive` already applied, every document d:
 *   - if every result of d has 1 <= handle < handle_bound: one record per distinct handle, ascending by handle, with
 *       count         the number of results of d with that handle,
 *       first_ordpos  the minimum of their ordpos,
 *       last_ordend   the maximum of their ordend                       (all values unsigned);
 *   - otherwise d has frequency status SP_DOC_ERR_RANGE and no records (the stitch's and the text's rule: it fails and is
 *     empty); the other documents are not affected.
 * A document that the matcher failed, or that has no results, has no records and status 0.  Over the batch:
 *   doc_offsets[ndocs+1]          the record range of every document,       totals[0]  the number of records,
 *   handle_results[handle_bound]  the sum of `count` over all records with that handle (collection frequency),
 *   handle_docs[handle_bound]     the number of records with that handle (document frequency);
 * index 0 of both stays 0, and a document with a range status contributes nothing.  Nothing depends on the order of a
 * document's results: the bytes are the same after a plain finish, after a canonical one and from result-set mode.  No byte
 * outside the output buffers is written and no record at or beyond the finished total read, whatever the records hold. */
typedef struct sp_pattern_freq {
	uint32_t handle;
	uint32_t count;
	uint32_t first_ordpos;
	uint32_t last_ordend;
} sp_pattern_freq_t;
typedef struct sp_pattern_freq_device {
	size_t ndocs;
	uint32_t handle_bound;
	void* d_records;             /* sp_pattern_freq_t[]: document 0's records first, ascending by handle inside a document */
	void* d_doc_offsets;         /* uint64_t[ndocs+1] */
	void* d_doc_freq_status;     /* int32_t[ndocs]: 0 or SP_DOC_ERR_RANGE */
	void* d_handle_results;      /* uint64_t[handle_bound] */
	void* d_handle_docs;         /* uint32_t[handle_bound] */
	void* d_totals;              /* uint64_t[1]: records */
} sp_pattern_freq_device_t;
/* host copy of a frequency batch (sp_pattern_freq_batch_free) */
typedef struct sp_pattern_freq_batch {
	size_t ndocs;
	size_t nrecords;
	uint32_t handle_bound;
	sp_pattern_freq_t* records;
	uint64_t* doc_offsets;        /* ndocs+1 */
	int32_t* doc_freq_status;     /* ndocs */
	uint64_t* handle_results;     /* handle_bound */
	uint32_t* handle_docs;        /* handle_bound */
	uint64_t totals[1];           /* records */
} sp_pattern_freq_batch_t;
/* np + 1: one more than the number of pattern names of the rule set; every result handle lies in [1, handle_bound) */
uint32_t sp_matcher_handle_bound(const sp_matcher_t* m);
/* Sums the frequencies of the batch finished last on this context (sp_matcher_ctx_batch_finish_device[_ex], either order).
 * Passes on `stream` (count, offsets, place, totals: csrc/l2_freq.h); the call enqueues count and offsets, waits for them
 * only to read the total, sizes the buffers, enqueues the rest and returns.  The buffers belong to the context, are
 * allocated at the first call, only grow, and are valid until the next frequency call; the next batch or finish
 * invalidates the state, not the buffers.  A `stream` other than the finish's is ordered behind it with an event.
 * SP_ERR_INVALID when the last batch is not finished; SP_ERR_NOMEM when a buffer cannot be allocated (the context stays
 * usable). */
int sp_matcher_ctx_finished_pattern_freq_device(sp_matcher_ctx_t* c, void* stream, sp_pattern_freq_device_t* out);
/* plain copy of the buffers of the last sp_matcher_ctx_finished_pattern_freq_device to the host (waits for it) */
int sp_matcher_ctx_finished_pattern_freq_fetch(sp_matcher_ctx_t* c, sp_pattern_freq_batch_t* out);
void sp_pattern_freq_batch_free(sp_pattern_freq_batch_t* b);
/* duration of all passes of the last frequency call in milliseconds (HIP events on its stream round them; waits for them;
 * the host's wait for the total between offsets and place lies inside) */
int sp_matcher_ctx_last_pattern_freq_ms(sp_matcher_ctx_t* c, double* ms);
/* diagnostics and tests: the handles that the device passes cover with one sweep of a document's results (the window of
 * their per-wave bitmap); a document whose handles span several windows is swept once per occupied window */
uint32_t sp_matcher_pattern_freq_window(void);
/* The same rule over host arrays, needs no device: the frequencies of a batch already fetched (results, doc_result_offsets
 * and, if given, doc_status: a document with a status has no records), and the yardstick of the device passes.  Fills `out`
 * (sp_pattern_freq_batch_free); SP_ERR_INVALID with the message in `err` for a bound of 0 and for offsets that do not
 * ascend or do not cover nresults. */
int sp_match_batch_pattern_freq(const sp_match_batch_t* mb, uint32_t handle_bound, sp_pattern_freq_batch_t* out,
                                char* err, size_t errsize);

/* ---- index terms: per document the distinct pairs (pattern, value) of its results -- the entries an inverted index stores
 * for a document, with the term frequency and the first position, and the way from every occurrence to its term; grouped on
 * the device (csrc/l2_terms.h) or, for a batch already fetched, on the host (csrc/match_terms.hpp).  The rule is the project's
 * own, unpinned by a reference vector (the reference has no such call).
 * The input is the batch finished last on a context, `exclusive` applied, in finished order (plain or canonical).  Every
 * result r has a TERM VALUE, chosen by `flags`:
 *   SP_TERM_VALUES  the bytes [result_value_offsets[r], result_value_offsets[r+1]) of the values batch built on this context
 *                   for this finished batch with SP_VALUE_RESULTS; an unformatted result has the empty value;
 *   SP_TERM_TEXT    the result's range [result_text_offsets[r], result_text_offsets[r+1]) of the text batch built on this
 *                   context for this finished batch with SP_TEXT_RESULTS;
 *   both            the value where result_format[r] != 0, else the text (a batch without format arrays: the text).
 * Two results of a document are the SAME TERM iff their handles are equal and their term values are equal byte strings: the
 * same length and the same bytes.  An empty value is a value; the same bytes under two handles are two terms.  Valid handles
 * are those of the frequency rule above: 1 <= handle < handle_bound.
 * A document d FAILS -- term status SP_DOC_ERR_RANGE, no records, all its result_term entries 0xFFFFFFFF, the other documents
 * not affected -- when a source that `flags` selects (both of them with both flags) has a non-zero value or text status for
 * d, or when one of its results has a handle outside [1, handle_bound).  A document that the matcher failed, or one without
 * results, has no records and term status 0 (results that a hand-made batch gives to a document with a matcher status keep
 * the result_term 0xFFFFFFFF).  Every other document has one record per distinct term:
 *   handle, count (its results with this term), first_ordpos (the minimum of their ordpos, unsigned), last_ordend (the
 *   maximum of their ordend), first_result (the smallest index, counted from the start of d's finished block, of a result
 *   with this term: the range of THAT result in the selected source is the term's bytes -- a term owns no bytes of its
 *   own), value_bytes (the length of the term value).
 * The records of d are ascending by handle, then by first_result; the terms of one handle are contiguous.  INVARIANT: the
 * sum of `count`, the minimum of `first_ordpos` and the maximum of `last_ordend` over the terms of a handle are that
 * handle's sp_pattern_freq_t of the same document, and the handles that occur are the same.
 *   doc_term_offsets[ndocs+1]  the record range of every document,          totals[0]  the number of records,
 *   result_term[nresults]      parallel to the finished results: the index of the result's term inside its document's
 *                              block of records (a posting list is a gather through it),
 *   doc_term_status[ndocs]     0 or SP_DOC_ERR_RANGE.
 * count, first_ordpos, last_ordend and value_bytes depend on the results only; first_result, result_term and the order
 * inside a handle follow the finished order.  After a canonical finish the whole batch is a function of the results alone:
 * the exact engines and result-set mode leave the same bytes.  A hash only chooses where the device looks for a term; two
 * results are one term only after their bytes were compared (sp_test_term_hash_bits).  No byte outside the outputs is written,
 * no record at or beyond the finished total and no source byte outside the source's total read, whatever the records hold.
 * The dictionary of the whole batch (the distinct terms across documents with their document frequency) is built from the
 * terms batch by a call of its own: "batch dictionary" below. */
#define SP_TERM_VALUES 1u
#define SP_TERM_TEXT   2u
typedef struct sp_match_term {
	uint32_t handle;
	uint32_t count;         /* results of d with this term */
	uint32_t first_ordpos;  /* minimum of their ordpos, unsigned */
	uint32_t last_ordend;   /* maximum of their ordend */
	uint32_t first_result;  /* smallest index, inside d's finished block, of a result with this term:
	                           its value range in the selected source IS the term's bytes */
	uint32_t value_bytes;   /* length of the term value */
} sp_match_term_t;
typedef struct sp_match_terms_device {
	size_t ndocs;
	uint32_t handle_bound;
	uint32_t flags;
	void* d_records;             /* sp_match_term_t[]: document 0's records first */
	void* d_doc_term_offsets;    /* uint64_t[ndocs+1] */
	void* d_result_term;         /* uint32_t[nresults], parallel to the finished d_results */
	void* d_doc_term_status;     /* int32_t[ndocs]: 0 or SP_DOC_ERR_RANGE */
	void* d_totals;              /* uint64_t[1]: records */
} sp_match_terms_device_t;
/* host copy of a terms batch (sp_match_terms_free) */
typedef struct sp_match_terms {
	size_t ndocs;
	size_t nresults;
	size_t nrecords;
	uint32_t handle_bound;
	uint32_t flags;
	sp_match_term_t* records;
	uint64_t* doc_term_offsets;   /* ndocs+1 */
	uint32_t* result_term;        /* nresults */
	int32_t* doc_term_status;     /* ndocs */
	uint64_t totals[1];           /* records */
} sp_match_terms_t;
/* Groups the results of the batch finished last on this context into terms.  flags: SP_TERM_VALUES | SP_TERM_TEXT; a source
 * that is selected must have been built on this context since that finish WITH its results family
 * (sp_matcher_ctx_finished_values_device with SP_VALUE_RESULTS, sp_matcher_ctx_finished_text_device with SP_TEXT_RESULTS): the
 * terms point into its buffers, so they are valid as long as those are.  Passes on `stream` (count, offsets, place:
 * csrc/l2_terms.h); the call enqueues count and offsets, waits for them only to read the total, sizes the records, enqueues
 * the placement and returns.  The buffers belong to the context, are allocated at the first call, only grow, and are valid
 * until the next terms call; the next batch or finish invalidates the state, not the buffers.  A `stream` other than the
 * one of the finish, the values call or the text call is ordered behind each of them with an event (their placements are
 * not waited for by their own calls).  SP_ERR_INVALID when the last batch is not finished, for flags 0 or unknown bits, and
 * when a selected source was not built since that finish or was built without the results family; SP_ERR_NOMEM when a
 * buffer cannot be allocated (the context stays usable). */
int sp_matcher_ctx_finished_terms_device(sp_matcher_ctx_t* c, uint32_t flags, void* stream, sp_match_terms_device_t* out);
/* plain copy of the buffers of the last sp_matcher_ctx_finished_terms_device to the host (waits for it) */
int sp_matcher_ctx_finished_terms_fetch(sp_matcher_ctx_t* c, sp_match_terms_t* out);
void sp_match_terms_free(sp_match_terms_t* t);
/* duration of all passes of the last terms call in milliseconds (HIP events on its stream round them; waits for them; the
 * host's wait for the total between offsets and place lies inside) */
int sp_matcher_ctx_last_terms_ms(sp_matcher_ctx_t* c, double* ms);
/* diagnostics and tests: the largest number of results of one document whose terms the device finds in a table in LDS; a
 * larger document uses working memory in HBM */
uint32_t sp_matcher_term_tile(void);
/* test hook (tests only): the device keeps only the low `bits` bits of the hash of a term (32 and more: all of them, the
 * default; 0: every term collides with every other).  The outputs do not change by a bit. */
void sp_test_term_hash_bits(unsigned bits);
/* The same rule over host arrays, needs no device, and the yardstick of the device passes: the terms of a batch already
 * fetched, with the host copies of its values (their results family, for SP_TERM_VALUES) and of its text (for SP_TERM_TEXT).
 * Fills `out` (sp_match_terms_free); SP_ERR_INVALID with the message in `err` for flags 0 or unknown bits, a NULL source or
 * one without its results family where `flags` selects it, sources whose ndocs or nresults are not those of `mb`, a bound
 * of 0, and offsets (of the documents or of a selected source) that do not ascend or do not cover their total. */
int sp_match_batch_terms(const sp_match_batch_t* mb, const sp_match_values_t* values, const sp_match_text_t* text,
                         uint32_t handle_bound, uint32_t flags, sp_match_terms_t* out, char* err, size_t errsize);

/* ---- batch dictionary: every distinct term (pattern, value) of a terms batch ONCE, across its documents, with its document
 * frequency and its collection frequency, and the way from every term record to its entry -- what an indexer needs to number
 * the new terms of a batch without de-duplicating strings on the host; built on the device (csrc/l2_dict.h) or, for a batch
 * already fetched, on the host (csrc/match_dict.hpp).  The rule is the project's own, unpinned by a reference vector.
 * INPUT: the terms batch built last on a context (sp_matcher_ctx_finished_terms_device) for the batch finished last, with the
 * sources its `flags` selected.  Write N for the number of term records.  Record i belongs to document d(i); its term is
 * (handle, value bytes), the value being the range of its first_result in the selected source, exactly as the terms rule
 * defines it.
 * SAME TERM: two term records are the same dictionary term iff their handles are equal and their values are equal byte
 * strings: the same length and the same bytes.  The empty value is a value.  The same bytes under two handles are two
 * entries.  With both flags a record may take its bytes from the values in one document and from the text in another: equal
 * bytes are one entry.
 * ORDER AND ENTRIES: one entry per distinct term, ordered by first occurrence, that is ascending by the smallest global record
 * index i of the term = (first document, index inside that document's block).  The entries first seen in document d are
 * contiguous, doc_dict_offsets[d] .. doc_dict_offsets[d+1], and ascend by handle inside that range, as the records do.  A
 * document that failed its terms (no records), that the matcher failed, or that has no results contributes nothing.
 * OUTPUTS:
 *   records[ndict]               sp_dict_term_t, below,                      totals[0]  ndict,
 *   term_dict[N]                 parallel to the term records: the entry of every record,
 *   doc_dict_offsets[ndocs+1]    the entries first seen in every document,
 *   handle_terms[handle_bound]   distinct terms per handle over the batch (a consumer that wants the entries by handle buckets
 *                                them with these counts).
 * INVARIANTS: the sum of doc_freq is N; the sum of count is the number of results of the documents that have records; per
 * handle the sum of count over its entries is handle_results[h] of the frequency pass when no document has a term or
 * frequency status; the sum of handle_terms is ndict; term_dict[i] < ndict for every i.
 * DETERMINISM: every output word is a function of the terms batch and its sources alone -- sums, maxima, minima of indices;
 * neither timing nor the hash enters (sp_test_term_hash_bits masks the dictionary's hash too).  After a canonical finish the
 * exact engines and result-set mode leave the same bytes.
 * SAFETY, as for the terms: no byte outside the outputs is written; no term record at or beyond N, no result at or beyond
 * the finished total and no source byte beyond the source's total is read, whatever the records hold; every index read from
 * working memory is compared against its bound before use.
 * LIMIT: N below 2^32 - 1 (indices are 32 bits), else SP_ERR_INVALID.
 * First-occurrence order needs only a compaction, is how an indexer numbers new terms, and is fully deterministic.  The
 * entries ranked by (handle, value bytes) are a product of their own, built from the dictionary ("dictionary order", below). */
typedef struct sp_dict_term {
	uint32_t handle;        /* pattern handle */
	uint32_t value_bytes;   /* length of the value */
	uint32_t first_doc;     /* first document with the term */
	uint32_t first_term;    /* index of the term's record inside first_doc's block; that record's first_result range IS
	                           the entry's bytes: an entry owns no bytes of its own */
	uint32_t doc_freq;      /* term records with this term = documents that contain it */
	uint32_t max_count;     /* the largest per-document count */
	uint64_t count;         /* sum of the per-document count: the collection frequency */
} sp_dict_term_t;
typedef struct sp_match_dictionary_device {
	size_t ndocs;
	uint32_t handle_bound;
	uint32_t flags;              /* those of the terms call */
	void* d_records;             /* sp_dict_term_t[ndict] */
	void* d_term_dict;           /* uint32_t[N], parallel to the term records */
	void* d_doc_dict_offsets;    /* uint64_t[ndocs+1] */
	void* d_handle_terms;        /* uint32_t[handle_bound] */
	void* d_totals;              /* uint64_t[1]: ndict */
} sp_match_dictionary_device_t;
/* host copy of a dictionary (sp_match_dictionary_free) */
typedef struct sp_match_dictionary {
	size_t ndocs;
	size_t nterms;                /* N */
	size_t ndict;
	uint32_t handle_bound;
	uint32_t flags;
	sp_dict_term_t* records;      /* ndict */
	uint32_t* term_dict;          /* nterms */
	uint64_t* doc_dict_offsets;   /* ndocs+1 */
	uint32_t* handle_terms;       /* handle_bound */
	uint64_t totals[1];           /* ndict */
} sp_match_dictionary_t;
/* Builds the dictionary of the terms built last on this context.  Five launches on `stream` (insert, resolve, offsets, place,
 * accumulate: csrc/l2_dict.h); the call enqueues the first three, waits for them only to read ndict, sizes the records,
 * enqueues the other two and returns.  The buffers belong to the context, are allocated at the first call, only grow (working
 * memory: 4 bytes x (table slots + 2N) + 4 x ndocs, the table having min(2N, 2^32 - 1) slots), and are valid until the next
 * dictionary call; the next batch, finish or terms call invalidates the state, not the buffers.  A `stream` other than the one
 * of the finish, the terms call, or the values or text call whose buffers the terms point into is ordered behind each of them
 * with an event (none of those calls waits for its own placement).  SP_ERR_INVALID when the last batch is not finished, when
 * no terms were built since that finish, when a source that the terms' flags select is not built with its results family for
 * this finish, and for N >= 2^32 - 1; SP_ERR_NOMEM when a buffer cannot be allocated (the context stays usable). */
int sp_matcher_ctx_finished_dictionary_device(sp_matcher_ctx_t* c, void* stream, sp_match_dictionary_device_t* out);
/* plain copy of the buffers of the last sp_matcher_ctx_finished_dictionary_device to the host (waits for it) */
int sp_matcher_ctx_finished_dictionary_fetch(sp_matcher_ctx_t* c, sp_match_dictionary_t* out);
void sp_match_dictionary_free(sp_match_dictionary_t* d);
/* duration of the five launches of the last dictionary call in milliseconds (HIP events on its stream round them; waits for
 * them; the host's wait for ndict between offsets and place lies inside; the hipMemsetAsync calls that clear the table, the
 * counters and handle_terms are enqueued before the first event and lie outside, as the clearing of every other product does) */
int sp_matcher_ctx_last_dictionary_ms(sp_matcher_ctx_t* c, double* ms);
/* The same rule over host arrays, needs no device, and the yardstick of the device passes: the dictionary of a terms batch
 * already fetched (or made by sp_match_batch_terms), with the batch and the host copies of the sources the terms were built
 * from; `flags` and the handle bound are those of `terms`.  Fills `out` (sp_match_dictionary_free); SP_ERR_INVALID with the
 * message in `err` for a NULL argument that the flags select or a source without its results family, for ndocs or nresults
 * that do not agree between `mb`, the sources and `terms`, for term offsets that do not ascend or do not cover nrecords, for
 * a first_result outside its document, a source range outside the source's bytes, and a value_bytes that is not the length
 * of its range; SP_ERR_NOMEM when memory runs out. */
int sp_match_batch_dictionary(const sp_match_batch_t* mb, const sp_match_values_t* values, const sp_match_text_t* text,
                              const sp_match_terms_t* terms, sp_match_dictionary_t* out, char* err, size_t errsize);

/* ---- dictionary order: the entries of the batch dictionary ranked by (pattern, value) -- the sorted run of a batch that an
 * indexer merges with the runs of other batches, searches by bisection and stores as a front-coded term block, and a listing
 * that does not depend on the order of the documents; built on the device (csrc/l2_dictorder.h) or, for a batch already
 * fetched, on the host (csrc/match_dictorder.hpp).  The rule is the project's own, unpinned by a reference vector.
 * INPUT: the dictionary built last on a context (sp_matcher_ctx_finished_dictionary_device), which implies its terms batch and
 * the sources the terms' flags selected.  Write ndict for the number of entries.  The value of entry e is the value of the
 * term record (first_doc, first_term), exactly as the dictionary rule defines it.
 * ORDER: entry a lies before entry b iff handle(a) < handle(b), unsigned, or the handles are equal and value(a) < value(b)
 * as byte strings: memcmp over the common length, every byte unsigned, and the shorter value first when one is a prefix of
 * the other.  The empty value is the first of its handle.  Entries are distinct in (handle, bytes), so the order is strict.
 * OUTPUTS:
 *   order[ndict]                    (uint32) order[k] is the entry at sorted position k,
 *   rank[ndict]                     (uint32) the inverse permutation: rank[order[k]] == k,
 *   prefix_bytes[ndict]             (uint32) parallel to `order`: 0 when k is the first position of its handle, otherwise the
 *                                   number of leading bytes that the values of order[k-1] and order[k] share: what a
 *                                   front-coded term block stores,
 *   handle_offsets[handle_bound+1]  (uint64) the exclusive prefix sums of the dictionary's handle_terms: the entries of handle
 *                                   h are order[handle_offsets[h] .. handle_offsets[h+1]), handle_offsets[handle_bound] is ndict,
 *   totals[0]                       ndict.
 * INVARIANTS: `order` is a permutation of 0..ndict-1; handles do not descend along `order`; for consecutive entries of one
 * handle prefix_bytes[k] <= min(value_bytes of both), and the byte behind the shared prefix ascends strictly or the left
 * value ends there.
 * DETERMINISM: every output word is a function of the dictionary and its sources alone, whatever algorithm produces it (the
 * device sorts fixed tiles and merges them by rank; no atomic decides where an entry goes).  After a canonical finish the
 * exact engines and result-set mode leave the same bytes.
 * SAFETY, as for the dictionary: no byte outside the outputs is written; an entry index is compared against ndict, a record
 * index against N, a result against the finished total and a source range against the source's total before use, and so is
 * every index read from working memory; a slot of an output that no valid entry reaches gets 0xFFFFFFFF.  A value whose
 * range is not inside its source compares as the empty value: it cannot come from this context's own dictionary, and the
 * host twin refuses it.
 * LIMIT: that of the dictionary, N below 2^32 - 1.
 * Neither the dictionary records nor the postings are moved: `order` is the way to them. */
typedef struct sp_match_dictionary_order_device {
	size_t ndict;
	uint32_t handle_bound;
	void* d_order;               /* uint32_t[ndict] */
	void* d_rank;                /* uint32_t[ndict] */
	void* d_prefix_bytes;        /* uint32_t[ndict], parallel to d_order */
	void* d_handle_offsets;      /* uint64_t[handle_bound+1] */
	void* d_totals;              /* uint64_t[1]: ndict */
} sp_match_dictionary_order_device_t;
/* host copy of a dictionary order (sp_match_dictionary_order_free) */
typedef struct sp_match_dictionary_order {
	size_t ndict;
	uint32_t handle_bound;
	uint32_t* order;              /* ndict */
	uint32_t* rank;               /* ndict */
	uint32_t* prefix_bytes;       /* ndict */
	uint64_t* handle_offsets;     /* handle_bound+1 */
	uint64_t totals[1];           /* ndict */
} sp_match_dictionary_order_t;
/* Ranks the entries of the dictionary built last on this context.  The host knows ndict from the dictionary call, so this call
 * enqueues every launch on `stream` and returns without waiting for anything (csrc/l2_dictorder.h): keys (a 64-bit key of the
 * handle and the first four value bytes per entry), tiles (fixed tiles of sp_matcher_dictionary_order_tile() entries sorted in
 * LDS), one merge launch per level with the run width doubling, ceil(log2(ceil(ndict / tile))) of them, place (order, rank,
 * prefix_bytes) and the handle offsets.  A comparison leaves the key only on a tie and then compares the bytes of both values
 * in their sources.  ndict <= 1 sorts nothing: no tile and no merge launch.  The buffers belong to the context, are allocated
 * at the first call, only grow (working memory: 2 x 12 x ndict bytes for the two buffers of (key, entry), 12 x ndict for where
 * the value of every entry lies and how long it is, and one cursor word), and are valid until the next order call; the next
 * batch, finish, terms or dictionary call invalidates the state, not the buffers.  Postings and positions neither need nor
 * invalidate the order, nor the reverse.  A `stream` other than the dictionary's is ordered behind the dictionary with an
 * event (its placement is not waited for by its own call).  SP_ERR_INVALID when no dictionary was built since the last terms
 * call of the last finish; SP_ERR_NOMEM when a buffer cannot be allocated (the context stays usable, `out` is empty). */
int sp_matcher_ctx_finished_dictionary_order_device(sp_matcher_ctx_t* c, void* stream, sp_match_dictionary_order_device_t* out);
/* plain copy of the buffers of the last sp_matcher_ctx_finished_dictionary_order_device to the host (waits for it) */
int sp_matcher_ctx_finished_dictionary_order_fetch(sp_matcher_ctx_t* c, sp_match_dictionary_order_t* out);
void sp_match_dictionary_order_free(sp_match_dictionary_order_t* o);
/* duration of the launches of the last order call in milliseconds (HIP events on its stream round them; waits for them; the
 * hipMemsetAsync calls that clear the cursor and the total and fill `rank` are enqueued before the first event, as the
 * clearing of every other product) */
int sp_matcher_ctx_last_dictionary_order_ms(sp_matcher_ctx_t* c, double* ms);
/* diagnostics and tests: the entries of one tile of the device's sort; tile k is always the entries [k * tile, (k+1) * tile)
 * in dictionary order, whichever workgroup takes it */
uint32_t sp_matcher_dictionary_order_tile(void);
/* The same rule over host arrays, needs no device, and the yardstick of the device passes: the order of a dictionary already
 * fetched (or made by sp_match_batch_dictionary), with the batch, the terms and the host copies of the sources the terms were
 * built from.  Fills `out` (sp_match_dictionary_order_free); SP_ERR_INVALID with the message in `err` for everything that
 * sp_match_batch_dictionary refuses about `mb`, the sources and `terms`, for a dictionary whose ndocs, nterms, handle bound or
 * flags are not those of `terms`, for an entry with a handle outside the bound, a first_doc / first_term outside its
 * document's records, a first_result outside its document, a source range outside the source's bytes, a value_bytes that is
 * not the length of its range, handle_terms that are not the number of entries of their handle, and two entries with the same
 * (handle, bytes); SP_ERR_NOMEM when memory runs out. */
int sp_match_batch_dictionary_order(const sp_match_batch_t* mb, const sp_match_values_t* values, const sp_match_text_t* text,
                                    const sp_match_terms_t* terms, const sp_match_dictionary_t* dict,
                                    sp_match_dictionary_order_t* out, char* err, size_t errsize);

/* ---- term blocks: the sorted dictionary of a batch written down as front-coded blocks -- the first product of a finished batch
 * that OWNS ITS BYTES: the immutable run of one batch that an indexer stores, merges with the run of the next batch or searches
 * later without the batch, its text or its values; built on the device (csrc/l2_termblocks.h) or, for a batch already fetched,
 * on the host (csrc/match_termblocks.hpp).  The rule is the project's own, unpinned by a reference vector.  (It is the run of
 * ONE batch: no dictionary that lives across batches is kept anywhere.)
 * INPUT: the dictionary order built last on a context (sp_matcher_ctx_finished_dictionary_order_device), which implies its
 * dictionary, its terms batch and the sources the terms' flags selected.  Write ndict for the number of entries.
 * BLOCK SIZE: B = sp_matcher_term_block_entries(), 16 by default.
 * BLOCKS: block j covers the sorted positions [j B, min((j+1) B, ndict)); nblocks = ceil(ndict / B).  Blocks are cut over the
 * sorted positions of the whole batch, not per handle.
 * THE CODE OF POSITION k: let e = order[k]; position k is the HEAD of its block iff k % B == 0.  The code is five unsigned
 * LEB128 varints followed by the suffix bytes; a varint is seven bits per byte, low bits first, the high bit set on every byte
 * but the last, in minimal length:
 *   1  hdelta     0 at a head, otherwise handle(order[k]) - handle(order[k-1]), never negative along `order`,
 *   2  shared     0 at a head, otherwise prefix_bytes[k] (already 0 at the first position of a handle),
 *   3  suffix     value_bytes(e) - shared,
 *   4  doc_freq(e),
 *   5  count(e)   64 bits, up to ten bytes,
 *   then the `suffix` bytes value(e)[shared:].
 * OUTPUTS:
 *   bytes[nbytes]              (uint8)  the codes of all positions in sorted order, without gaps,
 *   block_offsets[nblocks+1]   (uint64) where block j starts in `bytes`; the last element is nbytes,
 *   block_handles[nblocks]     (uint32) the handle of the head of block j,
 *   totals[4]                  (uint64) {nblocks, nbytes, B, the sum of value_bytes over all entries}: the fourth is what the
 *                              values cost uncoded.
 * With block_handles[j] a block decodes from its own bytes alone; a head carries its value in full.
 * INVARIANTS: decoding reproduces, for every sorted position, exactly (handle, value bytes, doc_freq, count) of order[k];
 * block_offsets ascends; a block is never empty (a code is at least five bytes).
 * DETERMINISM: every output byte is a function of the dictionary, its order and its sources alone (the one atomic of the
 * device adds to a sum).  After a canonical finish the exact engines and result-set mode leave the same bytes.
 * SAFETY, as for the order: no byte outside the outputs is written; every byte written for block j lies inside
 * [block_offsets[j], block_offsets[j+1]), and that range inside nbytes; every source byte read lies inside its source; an entry
 * index, a record index, a result and a source range are compared against their bounds before use, as the order call does.  A
 * value whose range is not inside its source is coded as the empty value, which is how the order treats it: it cannot come
 * from this context's own dictionary, and the host twin refuses it.
 * LIMIT: that of the dictionary, N below 2^32 - 1. */
/* one decoded position of a block (sp_match_term_blocks_decode_block) */
typedef struct sp_term_block_entry {
	uint32_t handle;        /* pattern handle */
	uint32_t value_bytes;   /* length of the full value */
	uint64_t value_offset;  /* where the full value starts in the `values` of the decode call */
	uint32_t doc_freq;
	uint32_t reserved;      /* 0 */
	uint64_t count;         /* the collection frequency */
} sp_term_block_entry_t;
typedef struct sp_match_term_blocks_device {
	size_t ndict;
	size_t nblocks;
	size_t nbytes;
	uint32_t block_entries;      /* B */
	void* d_bytes;               /* uint8_t[nbytes] */
	void* d_block_offsets;       /* uint64_t[nblocks+1] */
	void* d_block_handles;       /* uint32_t[nblocks] */
	void* d_totals;              /* uint64_t[4]: nblocks, nbytes, B, the sum of value_bytes */
} sp_match_term_blocks_device_t;
/* host copy of the term blocks (sp_match_term_blocks_free) */
typedef struct sp_match_term_blocks {
	size_t ndict;
	size_t nblocks;
	size_t nbytes;
	uint32_t block_entries;       /* B */
	uint8_t* bytes;               /* nbytes */
	uint64_t* block_offsets;      /* nblocks+1 */
	uint32_t* block_handles;      /* nblocks */
	uint64_t totals[4];           /* nblocks, nbytes, B, the sum of value_bytes */
} sp_match_term_blocks_t;
/* the positions of a block, B: 16 unless sp_test_term_block_entries chose another */
uint32_t sp_matcher_term_block_entries(void);
/* tests and diagnostics only, like sp_test_postings_digit_bits: B from 1, 2, 4, 8, 16, 32, 64 for the device calls and the
 * twin that follow; 0 (and any other number) restores the default.  B = 1 means no front coding at all. */
void sp_test_term_block_entries(unsigned n);
/* Writes the term blocks of the order built last on this context.  Three launches on `stream` (sizes, offsets, emit:
 * csrc/l2_termblocks.h); the call enqueues the first two, waits for them only to read nbytes, sizes `bytes`, enqueues the third
 * and returns.  block_offsets and block_handles are sized by nblocks, which the host knows, before the wait.  ndict == 0 launches
 * nothing: nblocks = nbytes = 0, block_offsets = [0].  Where a value lies and how long it is is read from the working memory of
 * the order call, which is valid as long as the order's state is.  The buffers belong to the context, are allocated at the
 * first call, only grow (working memory: 8 bytes a block), and are valid until the next term-blocks call; whatever invalidates
 * the order -- the next batch, finish, terms or dictionary call -- and a new order call invalidate the state, not the buffers.
 * Postings and positions neither need nor invalidate the blocks, nor the reverse.  A `stream` other than the order's is ordered
 * behind the order with an event.  SP_ERR_INVALID when no order was built since the last dictionary call; SP_ERR_NOMEM when a
 * buffer cannot be allocated (the context stays usable, `out` is empty). */
int sp_matcher_ctx_finished_term_blocks_device(sp_matcher_ctx_t* c, void* stream, sp_match_term_blocks_device_t* out);
/* plain copy of the buffers of the last sp_matcher_ctx_finished_term_blocks_device to the host (waits for it): this fetch
 * replaces those of the batch and of its text or values for a caller who wants the sorted dictionary with its strings */
int sp_matcher_ctx_finished_term_blocks_fetch(sp_matcher_ctx_t* c, sp_match_term_blocks_t* out);
void sp_match_term_blocks_free(sp_match_term_blocks_t* tb);
/* duration of the launches of the last term-blocks call in milliseconds (HIP events on its stream round them; waits for them;
 * the host's wait for nbytes between offsets and emit lies inside; the hipMemsetAsync calls that clear the totals are enqueued
 * before the first event, as the clearing of every other product) */
int sp_matcher_ctx_last_term_blocks_ms(sp_matcher_ctx_t* c, double* ms);
/* The same rule over host arrays, needs no device, and the yardstick of the device passes: the blocks of an order already
 * fetched (or made by sp_match_batch_dictionary_order), with the batch, the terms, the dictionary and the host copies of the
 * sources the terms were built from.  Fills `out` (sp_match_term_blocks_free); SP_ERR_INVALID with the message in `err` for
 * everything that sp_match_batch_dictionary_order refuses, for an order whose ndict or handle bound is not the dictionary's, an
 * `order` that is not a permutation, handles that descend along it, a prefix_bytes[k] above the length of either neighbour, and
 * a prefix_bytes[k] that is not what the two values share (0 at the first position of a handle); SP_ERR_NOMEM when memory
 * runs out. */
int sp_match_batch_term_blocks(const sp_match_batch_t* mb, const sp_match_values_t* values, const sp_match_text_t* text,
                               const sp_match_terms_t* terms, const sp_match_dictionary_t* dict, const sp_match_dictionary_order_t* order,
                               sp_match_term_blocks_t* out, char* err, size_t errsize);
/* The reader: decodes block j of `tb` alone, from bytes[block_offsets[j] .. block_offsets[j+1]) and block_handles[j], into
 * `entries` (room for nentries_cap records; a block holds at most block_entries) and the full values, one behind the other, into
 * `values` (room for values_cap bytes).  *nentries and *nvalues get what the block holds, also when the room does not suffice;
 * with entries == NULL and values == NULL the call only counts.  Needs no device.  SP_ERR_INVALID with the message in `err` for
 * j >= nblocks, block offsets that descend or leave `bytes`, room that does not suffice, and a malformed block: a varint that
 * runs past the block, a varint longer than ten bytes, a `shared` above the previous value's length (above 0 at the head), a
 * suffix that runs past the block, a handle or a value length that leaves 32 bits, an empty block and one of more than
 * block_entries codes. */
int sp_match_term_blocks_decode_block(const sp_match_term_blocks_t* tb, size_t j, sp_term_block_entry_t* entries, size_t nentries_cap,
                                      uint8_t* values, size_t values_cap, size_t* nentries, size_t* nvalues, char* err, size_t errsize);

/* ---- batch postings: for every entry of the batch dictionary the documents that hold it -- the list (document, term
 * frequency, first position), ascending by document, that an indexer appends to its inverted index, and the way from every
 * term record to its posting; built on the device (csrc/l2_postings.h) or, for a batch already fetched, on the host
 * (csrc/match_postings.hpp).  The rule is the project's own, unpinned by a reference vector.
 * INPUT: the dictionary built last on a context (sp_matcher_ctx_finished_dictionary_device), which implies the terms batch it
 * was built from.  Write N for the number of term records and ndict for the number of entries.  Record i lies in document
 * d(i), at index t(i) = i - doc_term_offsets[d(i)] inside that document's block, and term_dict[i] is its entry.  No source
 * byte is read: term_dict already says which records are the same term.
 * POSTING: one 16-byte record sp_posting_t per term record: {d(i), t(i), records[i].count, records[i].first_ordpos}.
 * OUTPUTS:
 *   entry_offsets[ndict+1]   (uint64) the exclusive prefix sums of doc_freq in dictionary order; entry_offsets[ndict] is N,
 *   postings[N]              the postings of entry e are [entry_offsets[e], entry_offsets[e+1]), strictly ascending by `doc`
 *                            inside an entry: a document has at most one record per term, so this is also the ascending
 *                            order of the global record index i,
 *   record_posting[N]        (uint32) parallel to the term records: the index of record i's posting, a permutation of 0..N-1,
 *   totals[0]                N.
 * INVARIANTS: postings[record_posting[i]] is {d(i), t(i), records[i].count, records[i].first_ordpos}; the first posting of
 * entry e is {first_doc, first_term, ..}; the list of e has doc_freq postings; the sum of `count` over the list of e is the
 * entry's count and the maximum its max_count; record_posting[i] lies in the range of entry term_dict[i].
 * DETERMINISM: every output word is a function of the terms batch and its dictionary alone; no timing enters (the device
 * partitions the records with a stable radix partition over fixed tiles of records, without an atomic on its data).  After a
 * canonical finish the exact engines and result-set mode leave the same bytes.
 * SAFETY, as for the terms and the dictionary: no byte outside the outputs is written; a record index is compared against N
 * before a term record is read, an entry index against ndict and a document index against ndocs before use, and so is
 * every position read from working memory.  A term_dict[i] at or beyond ndict cannot come from this context's own
 * dictionary; were it there, the device would take ndict - 1 for the record's entry and touch nothing out of bounds (the host
 * twin refuses such a dictionary).
 * LIMIT: N below 2^32 - 1, which the dictionary enforces.
 * The positions of EVERY occurrence of a term in a document are not part of a posting: they are a product of their own,
 * built from the postings ("posting positions", below).  The postings stay in dictionary order; the way to them by
 * (handle, value bytes) is `order` of the "dictionary order" product, below. */
typedef struct sp_posting {
	uint32_t doc;           /* the document */
	uint32_t term;          /* index of the term record inside doc's block: everything else about the occurrence hangs off it */
	uint32_t count;         /* that record's count: the term frequency in doc */
	uint32_t first_ordpos;  /* that record's first_ordpos */
} sp_posting_t;
typedef struct sp_match_postings_device {
	size_t ndocs;
	size_t nterms;               /* N */
	size_t ndict;
	void* d_postings;            /* sp_posting_t[N] */
	void* d_entry_offsets;       /* uint64_t[ndict+1] */
	void* d_record_posting;      /* uint32_t[N], parallel to the term records */
	void* d_totals;              /* uint64_t[1]: N */
} sp_match_postings_device_t;
/* host copy of the postings (sp_match_postings_free) */
typedef struct sp_match_postings {
	size_t ndocs;
	size_t nterms;                /* N */
	size_t ndict;
	sp_posting_t* postings;       /* nterms */
	uint64_t* entry_offsets;      /* ndict+1 */
	uint32_t* record_posting;     /* nterms */
	uint64_t totals[1];           /* N */
} sp_match_postings_t;
/* Builds the postings of the dictionary built last on this context.  The host knows N and ndict from the dictionary call, so
 * this call enqueues every launch on `stream` and returns without waiting for anything: keys, entry offsets, then per radix
 * pass histogram, scan and scatter, then place (csrc/l2_postings.h); ceil(bitwidth(ndict - 1) / 8) passes, none for ndict <= 1.
 * The buffers belong to the context, are allocated at the first call, only grow (working memory: 4N bytes for the document of
 * every record, 2 x 8N for the two buffers of (entry, record) pairs, 4 x 256 x ceil(N / tile) for the digit counts of the tiles
 * (sp_matcher_postings_tile), and 66 cursor words), and are valid until the next postings call; the next batch, finish, terms
 * or dictionary call invalidates the state, not the buffers.  A `stream` other than the dictionary's is ordered behind the
 * dictionary with an event (its placement is not waited for by its own call).  SP_ERR_INVALID when no dictionary was built
 * since the last terms call of the last finish; SP_ERR_NOMEM when a buffer cannot be allocated (the context stays usable,
 * `out` is empty). */
int sp_matcher_ctx_finished_postings_device(sp_matcher_ctx_t* c, void* stream, sp_match_postings_device_t* out);
/* plain copy of the buffers of the last sp_matcher_ctx_finished_postings_device to the host (waits for it) */
int sp_matcher_ctx_finished_postings_fetch(sp_matcher_ctx_t* c, sp_match_postings_t* out);
void sp_match_postings_free(sp_match_postings_t* p);
/* duration of the launches of the last postings call in milliseconds (HIP events on its stream round them; waits for them;
 * the hipMemsetAsync that clears the cursors is enqueued before the first event, as the clearing of every other product) */
int sp_matcher_ctx_last_postings_ms(sp_matcher_ctx_t* c, double* ms);
/* diagnostics and tests: the records of one tile of the device's partition; tile k is always the records
 * [k * tile, (k+1) * tile) in the order of the pass, whichever wave takes it */
uint32_t sp_matcher_postings_tile(void);
/* test hook (tests only): the bits of a radix digit, 1..8; anything else selects the default, 8.  The outputs do not change
 * by a bit. */
void sp_test_postings_digit_bits(unsigned bits);
/* The same rule over host arrays, needs no device, and the yardstick of the device passes: the postings of a terms batch and
 * its dictionary already fetched (or made by sp_match_batch_terms and sp_match_batch_dictionary), by a counting sort.  Fills
 * `out` (sp_match_postings_free); SP_ERR_INVALID with the message in `err` for a NULL argument, for ndocs or nterms that do not
 * agree between `terms` and `dict`, for term offsets that do not ascend or do not cover nrecords, for a term_dict[i] at or
 * beyond ndict, and for a doc_freq that is not the number of records of its entry; SP_ERR_NOMEM when memory runs out. */
int sp_match_batch_postings(const sp_match_terms_t* terms, const sp_match_dictionary_t* dict, sp_match_postings_t* out,
                            char* err, size_t errsize);

/* ---- posting positions: for every posting the list of ALL occurrences of its term in its document -- the position list that
 * an inverted index stores per posting -- without fetching the finished batch; built on the device (csrc/l2_positions.h) or,
 * for a batch already fetched, on the host (csrc/match_positions.hpp).  The rule is the project's own, unpinned by a reference
 * vector.
 * INPUT: the postings built last on a context (sp_matcher_ctx_finished_postings_device), which implies their dictionary, their
 * terms batch and the finished batch.  Write N for the number of term records = the number of postings, and doc_offsets for
 * the finished batch's result range per document.
 * PARTICIPATING RESULTS: result r of document d participates iff result_term[r] != 0xFFFFFFFF.  Its posting is
 * p(r) = record_posting[doc_term_offsets[d] + result_term[r]].  The results of documents that failed their terms, or that the
 * matcher failed, contribute nothing.  nocc is the number of participating results = the sum of `count` over the postings.
 * OCCURRENCE: one 8-byte record sp_occurrence_t {ordpos, result} per participating result; `result` is the index of the result
 * inside its document's finished block: ordend, the original positions and the items hang off it, an occurrence owns
 * nothing else.
 * OUTPUTS:
 *   posting_offsets[N+1]     (uint64) the exclusive prefix sums of postings[p].count in posting order; posting_offsets[N] is nocc,
 *   occurrences[nocc]        those of posting p are [posting_offsets[p], posting_offsets[p+1]), ascending by ordpos (unsigned),
 *                            equal positions in finished order, that is ascending `result`,
 *   posting_positions[N]     (uint32) the number of DISTINCT ordpos in the list of p: the length of the position set an index
 *                            stores; two results of a term that start at the same token and end at different ones are one position,
 *   totals[2]                (uint64) nocc, and the sum of posting_positions.
 * The postings lie entry by entry and ascend by document inside an entry, so the concatenated lists of an entry are that
 * term's positional posting list.
 * INVARIANTS: the list of p has postings[p].count records; its first ordpos is postings[p].first_ordpos; for every occurrence
 * result_term[doc_offsets[doc] + result] == postings[p].term; the smallest `result` of the list is the term record's
 * first_result; 1 <= posting_positions[p] <= count; every participating result appears exactly once.
 * DETERMINISM: every output word is a function of the finished batch, the terms and the postings; no timing enters (the device
 * partitions the results with the postings' stable radix partition over fixed tiles, without an atomic on its data).  The
 * ordpos words and posting_positions depend on the results alone; `result` follows the finished order, as first_result does.
 * After a canonical finish the exact engines and result-set mode leave the same bytes.
 * SAFETY, as for the postings: no byte outside the outputs is written; a result index is compared against the finished total
 * before a result is read, a result_term against its document's record count, a posting index against N, and a rank against
 * the number of sorted slots (the finished total on the device, where the results that do not participate are sorted behind
 * the nocc occurrences; only those are placed) before use.  A slot that no valid result reaches holds 0xFFFFFFFF words.
 * LIMIT: the finished total below 2^32 - 1, else SP_ERR_INVALID. */
typedef struct sp_occurrence {
	uint32_t ordpos;        /* ordinal position the result starts at */
	uint32_t result;        /* index of the result inside its document's finished block */
} sp_occurrence_t;
typedef struct sp_match_positions_device {
	size_t ndocs;
	size_t nterms;               /* N */
	size_t nocc;
	void* d_occurrences;         /* sp_occurrence_t[nocc] */
	void* d_posting_offsets;     /* uint64_t[N+1] */
	void* d_posting_positions;   /* uint32_t[N], parallel to the postings */
	void* d_totals;              /* uint64_t[2]: nocc, the sum of posting_positions */
} sp_match_positions_device_t;
/* host copy of the positions (sp_match_positions_free) */
typedef struct sp_match_positions {
	size_t ndocs;
	size_t nterms;                /* N */
	size_t nocc;
	sp_occurrence_t* occurrences; /* nocc */
	uint64_t* posting_offsets;    /* nterms+1 */
	uint32_t* posting_positions;  /* nterms */
	uint64_t totals[2];           /* nocc, the sum of posting_positions */
} sp_match_positions_t;
/* Builds the positions of the postings built last on this context.  Launches on `stream` (csrc/l2_positions.h): keys and
 * posting offsets; then the host waits, once, for nocc and the largest participating ordpos, which it does not know and which
 * set the passes; then ceil(bitwidth(largest ordpos) / 8) radix passes of histogram, scan and scatter by position, a rekey
 * launch, ceil(bitwidth(N - 1) / 8) passes by posting (of N where a result does not participate), and place, which nobody
 * waits for.  The buffers belong to the context, are allocated at the first call, only grow (working memory, R being the
 * finished total: 4R bytes for the document of every result, 2 x 8R for the two buffers of (key, result) pairs, 4 x 256 x
 * ceil(R / tile) for the digit counts of the tiles (sp_matcher_positions_tile), and 131 cursor words), and are valid until
 * the next positions call; the next batch, finish, terms, dictionary or postings call invalidates the state, not the buffers.
 * A `stream` other than the postings' is ordered behind the postings with an event (their placement is not waited for by
 * their own call).  SP_ERR_INVALID when no postings were built since the last dictionary call of the last finish, and for a
 * finished total of 2^32 - 1 or more; SP_ERR_NOMEM when a buffer cannot be allocated (the context stays usable, `out` is empty). */
int sp_matcher_ctx_finished_positions_device(sp_matcher_ctx_t* c, void* stream, sp_match_positions_device_t* out);
/* plain copy of the buffers of the last sp_matcher_ctx_finished_positions_device to the host (waits for it) */
int sp_matcher_ctx_finished_positions_fetch(sp_matcher_ctx_t* c, sp_match_positions_t* out);
void sp_match_positions_free(sp_match_positions_t* p);
/* duration of the launches of the last positions call in milliseconds (HIP events on its stream round them; waits for them;
 * the host's wait between the posting offsets and the first pass lies inside; the hipMemsetAsync calls that clear the cursors,
 * the totals and posting_positions are enqueued before the first event, as the clearing of every other product) */
int sp_matcher_ctx_last_positions_ms(sp_matcher_ctx_t* c, double* ms);
/* diagnostics and tests: the (key, result) pairs of one tile of the device's partition; tile k is always the pairs
 * [k * tile, (k+1) * tile) in the order of the pass, whichever wave takes it.  sp_test_postings_digit_bits selects the digit
 * of this partition too. */
uint32_t sp_matcher_positions_tile(void);
/* diagnostics (measurements only): with on != 0 every later positions call records a HIP event behind each of its launches,
 * and sp_matcher_ctx_last_positions_launch_ms gives the time of the last call's launches summed by kind, ms[0..5] = keys,
 * histogram, scan, scatter, rekey, place (the scan of the posting offsets is not among them; waits for the call).
 * SP_ERR_INVALID when the last positions call recorded none.  The outputs do not change by a bit. */
void sp_test_positions_launch_events(unsigned on);
int sp_matcher_ctx_last_positions_launch_ms(sp_matcher_ctx_t* c, double ms[6]);
/* The same rule over host arrays, needs no device, and the yardstick of the device passes: the positions of a finished batch
 * already fetched with its terms and their postings (or made by the twins), by a counting sort by posting, then a stable sort
 * by ordpos inside each list.  Fills `out` (sp_match_positions_free); SP_ERR_INVALID with the message in `err` for a NULL
 * argument, for ndocs, nresults or nterms that do not agree between `mb`, `terms` and `postings`, for document or term offsets
 * that do not ascend or do not cover their total, for a result_term at or beyond its document's records, a record_posting at
 * or beyond N, and a posting whose count is not the number of its results; SP_ERR_NOMEM when memory runs out. */
int sp_match_batch_positions(const sp_match_batch_t* mb, const sp_match_terms_t* terms, const sp_match_postings_t* postings,
                             sp_match_positions_t* out, char* err, size_t errsize);

/* ---- posting blocks: the posting lists of a batch, with their positions, written down in the sorted order of the dictionary,
 * cut into the blocks of the term blocks and delta-coded with varints -- the second product of a finished batch that OWNS ITS
 * BYTES: position k of the term blocks and list k of the posting blocks are the same term, and the two products together are
 * the index segment of the batch, which an indexer stores, merges or searches without the batch; built on the device
 * (csrc/l2_postingblocks.h) or, for arrays already fetched, on the host (csrc/match_postingblocks.hpp).  The rule is the
 * project's own, unpinned by a reference vector.  (It is the run of ONE batch: no state that lives across batches is kept.)
 * INPUT: the dictionary order, the postings and the posting positions built last on a context, all three of the current
 * dictionary.  Write ndict for the number of entries, N for the number of postings, e = order[k] for the entry at sorted
 * position k.  The LIST of k is postings[entry_offsets[e] .. entry_offsets[e+1]): doc_freq(e) postings, ascending by `doc`.
 * BLOCKS: B = sp_matcher_term_block_entries(), the switch of the term blocks (sp_test_term_block_entries); block j covers the
 * sorted positions [j B, min((j+1) B, ndict)); nblocks = ceil(ndict / B).  Block j of both products covers the same terms.
 * THE CODE OF SORTED POSITION k, in the unsigned LEB128 varints of the term blocks, minimal length:
 *   1  body       the number of bytes of the posting codes that follow, 64 bits: a reader skips a whole list with it,
 *   2  for every posting p of the list in order:
 *        ddelta     doc(p) for the first posting of the list, otherwise doc(p) - doc(p-1), at least 1,
 *        count(p)   the term frequency: the number of occurrences,
 *        npos       posting_positions[p]: the number of distinct ordinal positions,
 *        npos varints: the smallest ordpos of the posting as it is, then every later DISTINCT ordpos less the distinct one
 *                   before it, at least 1.
 * Occurrences that repeat an ordpos contribute no byte; the `result` word of an occurrence is not stored.  The number of
 * postings of a list is not stored: the list ends where `body` ends, and that number is the doc_freq that its term-block
 * position carries.
 * OUTPUTS:
 *   bytes[nbytes]              (uint8)  the codes of all sorted positions, without gaps,
 *   block_offsets[nblocks+1]   (uint64) where block j starts in `bytes`; the last element is nbytes,
 *   totals[4]                  (uint64) {nblocks, nbytes, B, the number of position varints written}: the fourth equals
 *                              totals[1] of the positions product.
 * A block decodes from its own bytes alone.
 * INVARIANTS: decoding list k reproduces, for every posting of order[k], exactly (doc, count, the distinct ordpos ascending);
 * block_offsets ascends; a block is never empty (a list is at least `body` and one posting of four varints).
 * DETERMINISM: every byte is a function of the dictionary, its order, the postings and the positions alone (the one global
 * atomic of the device adds to the fourth total).  The codes hold positions and no `result` index, so a plain and a canonical
 * finish leave the same bytes, and after a canonical finish the exact engines and result-set mode do too.
 * SAFETY, as for the term blocks: no byte outside the outputs is written; every byte written for block j lies inside
 * [block_offsets[j], block_offsets[j+1]), and that range inside the capacity the host allocated; an entry is compared
 * against ndict, a posting against N, an occurrence against nocc and a document against ndocs before use, and so is every
 * index read from working memory.  Arrays that this context cannot produce: a posting whose entry, index or document fails
 * one of those comparisons, and a posting without an occurrence (`count` 0 means an empty occurrence range here: the range,
 * not the word, says how many occurrences are walked), costs nothing and writes nothing, for nobody carries its header;
 * documents that do not ascend inside a list and positions that do not ascend inside a posting wrap in 32 bits;
 * posting_positions is written as it is, above `count` too.  The sizing and the emitting pass go through one function for what
 * a posting costs (csrc/posting_block_code.h), so they agree on all of these; such bytes need not decode, a byte of `bytes`
 * that no code reaches keeps what the buffer held, and a span of 64 occurrences one of which would leave the range of its
 * block is not written.  The host twin refuses these inputs.
 * LIMIT: those of the dictionary and the positions: N and the finished total below 2^32 - 1. */
/* one decoded posting of a block (sp_match_posting_blocks_decode_block) */
typedef struct sp_block_posting {
	uint32_t doc;
	uint32_t count;            /* the term frequency */
	uint32_t npos;             /* the number of distinct positions */
	uint32_t reserved;         /* 0 */
	uint64_t position_offset;  /* where its npos positions start in the `positions` of the decode call */
} sp_block_posting_t;
typedef struct sp_match_posting_blocks_device {
	size_t ndict;
	size_t nblocks;
	size_t nbytes;
	uint32_t block_entries;      /* B */
	void* d_bytes;               /* uint8_t[nbytes] */
	void* d_block_offsets;       /* uint64_t[nblocks+1] */
	void* d_totals;              /* uint64_t[4]: nblocks, nbytes, B, the position varints written */
} sp_match_posting_blocks_device_t;
/* host copy of the posting blocks (sp_match_posting_blocks_free) */
typedef struct sp_match_posting_blocks {
	size_t ndict;
	size_t nblocks;
	size_t nbytes;
	uint32_t block_entries;       /* B */
	uint8_t* bytes;               /* nbytes */
	uint64_t* block_offsets;      /* nblocks+1 */
	uint64_t totals[4];           /* nblocks, nbytes, B, the position varints written */
} sp_match_posting_blocks_t;
/* Writes the posting blocks of the order, the postings and the positions built last on this context.  Six launches on `stream`
 * (lists, sizes, prefix, blocks, offsets, emit: csrc/l2_postingblocks.h); the call enqueues the first five, waits for them only
 * to read nbytes, sizes `bytes`, enqueues the sixth and returns.  block_offsets is sized by nblocks, which the host knows,
 * before the wait.  ndict == 0 launches nothing: nblocks = nbytes = 0, block_offsets = [0].  The buffers belong to the context,
 * are allocated at the first call, only grow (working memory: 8 bytes a posting, 16 a sorted position, 8 a block), and are
 * valid until the next posting-blocks call; a new order, postings or positions call, and whatever invalidates those -- the next
 * batch, finish, terms or dictionary call --, invalidate the state, not the buffers.  The term blocks neither need nor
 * invalidate the posting blocks, nor the reverse.  A `stream` other than those of the order, the postings and the positions is
 * ordered behind each with an event.  SP_ERR_INVALID unless an order, postings and positions were all built since the last
 * dictionary call of the last finish; SP_ERR_NOMEM when a buffer cannot be allocated (the context stays usable, `out` is empty). */
int sp_matcher_ctx_finished_posting_blocks_device(sp_matcher_ctx_t* c, void* stream, sp_match_posting_blocks_device_t* out);
/* plain copy of the buffers of the last sp_matcher_ctx_finished_posting_blocks_device to the host (waits for it): this fetch
 * replaces those of the postings, the positions, the dictionary and the order for a caller who wants the inverted lists in the
 * order of the term blocks */
int sp_matcher_ctx_finished_posting_blocks_fetch(sp_matcher_ctx_t* c, sp_match_posting_blocks_t* out);
void sp_match_posting_blocks_free(sp_match_posting_blocks_t* pb);
/* duration of the launches of the last posting-blocks call in milliseconds (HIP events on its stream round them; waits for
 * them; the host's wait for nbytes between offsets and emit lies inside; the hipMemsetAsync calls that clear the totals are
 * enqueued before the first event, as the clearing of every other product) */
int sp_matcher_ctx_last_posting_blocks_ms(sp_matcher_ctx_t* c, double* ms);
/* The same rule over host arrays, needs no device, no batch and no source, and the yardstick of the device passes: the blocks of
 * a dictionary, its order, its postings and their positions already fetched (or made by their twins).  Fills `out`
 * (sp_match_posting_blocks_free); SP_ERR_INVALID with the message in `err` for a NULL argument; an order or postings whose ndict
 * is not the dictionary's; positions whose number of postings is not that of the postings; an `order` that is not a
 * permutation; entry offsets that do not ascend or do not cover the postings; a doc_freq that is not the length of its list;
 * posting offsets that do not ascend or do not cover the occurrences; a posting with `count` 0; a posting without an
 * occurrence; documents that do not ascend inside a list; positions
 * that do not ascend inside a posting; a posting_positions that is 0, above `count` or not the number of distinct positions;
 * SP_ERR_NOMEM when memory runs out. */
int sp_match_batch_posting_blocks(const sp_match_dictionary_t* dict, const sp_match_dictionary_order_t* order,
                                  const sp_match_postings_t* postings, const sp_match_positions_t* positions,
                                  sp_match_posting_blocks_t* out, char* err, size_t errsize);
/* The reader: decodes block j of `pb` alone, from bytes[block_offsets[j] .. block_offsets[j+1]): per list its number of postings
 * into `list_postings` (room for nlists_cap numbers; a block holds at most block_entries lists), the postings of all its lists
 * one behind the other into `postings` (room for npostings_cap records) and their positions, ascending, into `positions` (room
 * for npositions_cap numbers).  *nlists, *npostings and *npositions get what the block holds, also when the room does not
 * suffice; with the three outputs NULL the call only counts.  Needs no device.  SP_ERR_INVALID with the message in `err` for
 * j >= nblocks, block offsets that descend or leave `bytes`, room that does not suffice, and a malformed block: a varint that
 * runs past the block or is longer than ten bytes; a `body` that runs past the block; a `body` of 0; a posting that ends
 * beyond its `body`; a ddelta of 0 behind the first posting of a list, or a position gap of 0 behind the first position of a
 * posting; an npos of 0 or above `count`; a document, a count or a position that leaves 32 bits; an empty block and one of more
 * than block_entries lists. */
int sp_match_posting_blocks_decode_block(const sp_match_posting_blocks_t* pb, size_t j, uint32_t* list_postings, size_t nlists_cap,
                                         sp_block_posting_t* postings, size_t npostings_cap, uint32_t* positions, size_t npositions_cap,
                                         size_t* nlists, size_t* npostings, size_t* npositions, char* err, size_t errsize);

/* ---- segment lookups: the read side of an index segment -- the term blocks and the posting blocks of one batch -- on the device:
 * a segment object that owns device copies of the two products and holds no reference to a context, the lookup of many terms at
 * once, exact or by prefix, and the decoded posting lists of what was found (csrc/l2_segment.h); for host copies the same rule
 * without a device (csrc/match_segment.hpp).  The rule is the project's own, unpinned by a reference vector.
 * THE ORDER of a segment: handles unsigned, bytes as memcmp does, a prefix before what it is a prefix of.
 * WHAT A QUERY (h, q) MATCHES: `first` is the first sorted position whose (handle, value) is not below (h, q), ndict if there is
 * none; the matching positions are the run from `first` on whose handle is h and whose value equals q -- under SP_LOOKUP_PREFIX:
 * starts with q; the empty q then selects the whole handle.  The order makes the run contiguous.  An exact run has one position
 * at most.
 * OUTPUTS, the selection being the runs of the queries one behind the other, nsel positions (a position that two queries select
 * appears twice):
 *   q_first[nq], q_count[nq], q_status[nq]  (uint32) the run of every query and its status, 0 or an SP_LOOKUP_ERR_*,
 *   q_sel_offsets[nq+1]                     (uint64) where the run of a query starts in the selection,
 *   selections[nsel]                        one 24-byte sp_segment_selection_t per selected position,
 *   sel_value_offsets[nsel+1]               (uint64) into `values`: the full values, reconstructed,
 *   sel_posting_offsets[nsel+1]             (uint64) into `postings`,
 *   postings[npostings]                     one 16-byte sp_segment_posting_t per posting of a selected position,
 *   posting_position_offsets[npostings+1]   (uint64) into `positions`,
 *   positions[npositions]                   (uint32) the distinct ordinal positions, absolute and ascending,
 *   totals[4]                               (uint64) {nsel, npostings, npositions, the bytes of `values`}.
 * INVARIANTS: every number equals what sp_match_term_blocks_decode_block and sp_match_posting_blocks_decode_block give for that
 * position.  DETERMINISM: every output byte is a function of the segment and the queries alone.
 * SAFETY: the bytes of a segment may come from a file.  Every read of `bytes` is bounded by the range of its block and that
 * range by nbytes; nothing is written outside the outputs, and the emitting pass writes exactly what the sizing pass counted.
 * A walk that meets a malformed code ends with a status: met while the run is looked for, the query gets the status and an
 * empty run (q_first 0); met at a selected position -- the place of the run in the selection is fixed by then --, that position
 * is selected empty (all numbers of its record but `position` are 0, no value, no posting) and its query gets the status, the
 * largest of its positions.  The malformations are those of the two readers.
 * KNOWN WEAKNESS: a list is walked by one lane, so a list of a megabyte is serial.
 * LIMITS: nq, nsel, npostings and npositions below 2^32 - 1. */
#define SP_LOOKUP_PREFIX 1u
enum {
	SP_LOOKUP_ERR_VARINT = 1, /* a varint that runs past its block or its list, or is longer than ten bytes */
	SP_LOOKUP_ERR_HEAD = 2,   /* a head that does not carry its handle and its value in full */
	SP_LOOKUP_ERR_SHARED = 3, /* a `shared` above the length of the value before */
	SP_LOOKUP_ERR_SUFFIX = 4, /* a suffix that runs past the block */
	SP_LOOKUP_ERR_BODY = 5,   /* a `body` of 0 or past the block, or a posting that ends beyond its `body` */
	SP_LOOKUP_ERR_DELTA = 6,  /* a ddelta of 0 behind the first posting of a list, or a position gap of 0 behind the first position */
	SP_LOOKUP_ERR_NPOS = 7,   /* an npos of 0 or above `count` */
	SP_LOOKUP_ERR_RANGE = 8   /* a handle, a value length, a doc_freq, a document, a count or a position that leaves 32 bits */
};
typedef struct sp_segment sp_segment_t;
typedef struct sp_segment_selection {
	uint32_t position;      /* the sorted position */
	uint32_t handle;
	uint32_t doc_freq;
	uint32_t value_bytes;
	uint64_t count;         /* the collection frequency */
} sp_segment_selection_t;
typedef struct sp_segment_posting {
	uint32_t doc;
	uint32_t count;         /* the term frequency */
	uint32_t npos;          /* the number of distinct positions */
	uint32_t reserved;      /* 0 */
} sp_segment_posting_t;
typedef struct sp_segment_lookup_device {
	size_t nq;
	size_t nsel;
	size_t npostings;
	size_t npositions;
	size_t nvalue_bytes;
	uint32_t flags;
	void* d_q_first;                   /* uint32_t[nq] */
	void* d_q_count;                   /* uint32_t[nq] */
	void* d_q_status;                  /* uint32_t[nq] */
	void* d_q_sel_offsets;             /* uint64_t[nq+1] */
	void* d_selections;                /* sp_segment_selection_t[nsel] */
	void* d_sel_value_offsets;         /* uint64_t[nsel+1] */
	void* d_sel_posting_offsets;       /* uint64_t[nsel+1] */
	void* d_values;                    /* uint8_t[nvalue_bytes] */
	void* d_postings;                  /* sp_segment_posting_t[npostings] */
	void* d_posting_position_offsets;  /* uint64_t[npostings+1] */
	void* d_positions;                 /* uint32_t[npositions] */
	void* d_totals;                    /* uint64_t[4]: nsel, npostings, npositions, nvalue_bytes */
} sp_segment_lookup_device_t;
/* host copy of a lookup (sp_segment_lookup_free) */
typedef struct sp_segment_lookup {
	size_t nq;
	size_t nsel;
	size_t npostings;
	size_t npositions;
	size_t nvalue_bytes;
	uint32_t flags;
	uint32_t* q_first;
	uint32_t* q_count;
	uint32_t* q_status;
	uint64_t* q_sel_offsets;
	sp_segment_selection_t* selections;
	uint64_t* sel_value_offsets;
	uint64_t* sel_posting_offsets;
	uint8_t* values;
	sp_segment_posting_t* postings;
	uint64_t* posting_position_offsets;
	uint32_t* positions;
	uint64_t totals[4];
} sp_segment_lookup_t;
/* Uploads host copies of the two products -- fetches, twin output, or bytes read back from a file -- to the current device and
 * keeps nothing of the host arrays.  Only the tables are checked, on the host; the bytes are not decoded.  SP_ERR_INVALID with
 * the message in `err` when ndict, nblocks or block_entries differ between the two products, nblocks is not ceil(ndict / B), B is
 * not one of 1, 2, 4, .. 64, a block_offsets array descends, does not end at nbytes or has an empty block, or block_handles
 * descends; SP_ERR_NOMEM and SP_ERR_DEVICE as elsewhere.  *out is NULL after a failure.  A segment is immutable; it owns its
 * device memory and the working buffers of its lookups (sp_segment_free). */
int sp_segment_open(const sp_match_term_blocks_t* tb, const sp_match_posting_blocks_t* pb, sp_segment_t** out, char* err, size_t errsize);
/* The same of the term blocks and the posting blocks built last on a context, copied device-to-device on `stream` behind the two
 * calls; the call waits for the copies, so the segment outlives the context and its next batch.  SP_ERR_INVALID (the message is
 * the context's last error) unless both block products are valid on that context. */
int sp_segment_from_ctx(sp_matcher_ctx_t* c, void* stream, sp_segment_t** out);
void sp_segment_free(sp_segment_t* s);
const char* sp_segment_last_error(sp_segment_t* s);
/* Looks nq queries up: query i is the handle query_handles[i] with the bytes query_bytes[query_offsets[i] .. query_offsets[i+1])
 * (host arrays, uploaded by the call, of which nothing is kept); flags is 0 for exact queries or SP_LOOKUP_PREFIX.  Everything
 * runs on `stream`, kernel boundaries are the only ordering, no flag is spun on and no atomic decides where a byte goes (the one
 * atomic is a maximum into q_status).  Five launches (find, runs, sizes, offsets, emit: csrc/l2_segment.h); the host waits once,
 * behind `offsets`, for the totals that size `values`, `postings` and `positions` -- and under SP_LOOKUP_PREFIX once more behind
 * `runs` for nsel, which an exact lookup bounds by nq.  nq == 0 or ndict == 0 launches nothing.  The outputs are device buffers
 * of the segment, only grow and are valid until the next lookup on that segment.  SP_ERR_INVALID for unknown flags, query
 * offsets that descend, and -- after the wait, the segment staying usable -- a limit that is reached. */
int sp_segment_lookup_device(sp_segment_t* s, const uint32_t* query_handles, const uint64_t* query_offsets, const uint8_t* query_bytes,
                             size_t nq, uint32_t flags, void* stream, sp_segment_lookup_device_t* out);
/* plain copy of the buffers of the last lookup of the segment to the host (waits for it) */
int sp_segment_lookup_fetch(sp_segment_t* s, sp_segment_lookup_t* out);
void sp_segment_lookup_free(sp_segment_lookup_t* lk);
/* duration of the last lookup in milliseconds (HIP events on its stream round the upload of the queries and the launches; the
 * host's waits lie inside) */
int sp_segment_last_lookup_ms(sp_segment_t* s, double* ms);
/* The same rule over host copies of the two products, needs no device, and the yardstick of the device passes: the same walks
 * (csrc/segment_walk.h), the same statuses.  Fills `out` (sp_segment_lookup_free); SP_ERR_INVALID with the message in `err` for
 * what sp_segment_open and sp_segment_lookup_device refuse. */
int sp_match_segment_lookup(const sp_match_term_blocks_t* tb, const sp_match_posting_blocks_t* pb, const uint32_t* query_handles,
                            const uint64_t* query_offsets, const uint8_t* query_bytes, size_t nq, uint32_t flags,
                            sp_segment_lookup_t* out, char* err, size_t errsize);
/* copies the results of the last device batch to the host, grouped by document (as sp_matcher_ctx_match_docs
 * returns them, `exclusive` elimination included) */
int sp_matcher_ctx_batch_fetch(sp_matcher_ctx_t* c, sp_match_batch_t* out);
/* the same for the documents [first_doc, first_doc+ndocs) of the last device batch only (a caller that checks a
 * sample, or picks up the documents of one shard, does not move the whole batch over PCIe) */
int sp_matcher_ctx_batch_fetch_docs(sp_matcher_ctx_t* c, size_t first_doc, size_t ndocs, sp_match_batch_t* out);
/* waits for the stream and returns counters[0..7] = {results, items, events, failed docs, documents the LDS-resident
 * kernel handed over to the general one (diagnostics), 0..} */
int sp_matcher_ctx_batch_counters(sp_matcher_ctx_t* c, uint64_t counters[8]);
/* duration of the last rule-automaton kernel in milliseconds (HIP events on the launch stream) */
double sp_matcher_ctx_last_kernel_ms(sp_matcher_ctx_t* c);
/* which kernel the context runs its batches on: 0 general automaton, 1 LDS-resident automaton (flat rule sets),
 * 2 the join kernel of result-set mode (SP_CTX_RESULT_SETS or SPA_L2_JOIN=1 at context creation, eligible rule set; result
 * MULTISETS with their items, no order inside a document, no statistics) */
int sp_matcher_ctx_kernel_kind(const sp_matcher_ctx_t* c);
/* name of the kernel that does the work of this context's batches (what rocprofv3 lists) */
const char* sp_matcher_ctx_kernel_name(const sp_matcher_ctx_t* c);
/* copies the per-document status words of the last batch to the host (waits for the stream) */
int sp_matcher_ctx_batch_status(sp_matcher_ctx_t* c, int32_t* status, size_t ndocs);
/* doubles every per-document working-set capacity (what the host entry points do on SP_DOC_ERR_ARENA) */
int sp_matcher_ctx_grow_arena(sp_matcher_ctx_t* c);
/* minimum capacity (records) of the device result / item buffers of the batch entry points */
int sp_matcher_ctx_reserve_output(sp_matcher_ctx_t* c, uint64_t results, uint64_t items);
/* working-set capacity per in-flight document; 0 keeps a default.  Takes effect at the next launch. */
int sp_matcher_ctx_set_arena(sp_matcher_ctx_t* c, uint32_t max_rules, uint32_t max_triggers, uint32_t bucket_capacity,
                             uint32_t max_items, uint32_t max_follow);

/* ==== level 1: pattern lexer ==== */

/* strus::createPatternLexer_std + PatternLexerInterface::createInstance
 * (src/libstrus_pattern.cpp:35-47, src/patternLexer.cpp:1165-1172) */
sp_lexer_t* sp_lexer_create(void);
void sp_lexer_free(sp_lexer_t* l);
const char* sp_lexer_last_error(const sp_lexer_t* l);

/* PatternLexerInstanceInterface (src/patternLexer.cpp:971-1141), same argument meaning.
 * Expressions are NUL terminated; posbind is an sp_position_bind. */
int sp_lexer_define_lexem_name(sp_lexer_t* l, uint32_t id, const char* name);                       /* :971 */
const char* sp_lexer_get_lexem_name(const sp_lexer_t* l, uint32_t id);                              /* :983 */
int sp_lexer_define_lexem(sp_lexer_t* l, uint32_t id, const char* expression, uint32_t resultIndex,
                          uint32_t level, int posbind);                                             /* :990 */
int sp_lexer_define_symbol(sp_lexer_t* l, uint32_t symbolid, uint32_t patternid, const char* name); /* :1008 */
uint32_t sp_lexer_get_symbol(const sp_lexer_t* l, uint32_t patternid, const char* name);            /* :1020 */
int sp_lexer_define_option(sp_lexer_t* l, const char* name, double value);                          /* :1031 */
int sp_lexer_compile(sp_lexer_t* l);                                                                /* :1068 */
/* compiled lexer (automaton tables, whole-word literal table, symbol tables, lexem names) as a blob and back; only a
 * compiled lexer can be saved, a loaded one is compiled and frozen (see sp_matcher_serialize) */
int sp_lexer_serialize(const sp_lexer_t* l, void** blob, size_t* size);
sp_lexer_t* sp_lexer_deserialize(const void* blob, size_t size, char* err, size_t errsize);
/* compiled automaton tables as a flat u64 array (test hook; layout in csrc/capi_l1.cpp) */
size_t sp_lexer_dump_tables(const sp_lexer_t* l, uint64_t** out);
/* one of the table images the kernels read (test hook): which = 0 all passes, 1 the passes the scan kernel runs, 2 the words
 * kernel's; the eight word offsets {character rows, accept, start, shift, self loop, exception sources, exception targets,
 * compact shape table}, then the image.  0 when the lexer has no such image (2: a table the words kernel does not take). */
size_t sp_lexer_dump_image(const sp_lexer_t* l, int which, uint64_t** out);
/* Which kernels a context on a device of num_cus compute units launches for a batch of ndocs documents and nbytes bytes, and why
 * -- the lexer's counterpart of sp_matcher_fast_tier; needs no device.  Writes one line of key=value fields separated by blanks:
 *   route             approx | lanes | passes(N) | none: approximate literal table, lane-per-stream scan kernel, the N-pass scan
 *                     instance, nothing to scan (literals and word shapes only);  cp=1: the instances for classes by code point
 *   scan_kernel, words_kernel   what sp_lexer_ctx_scan_kernel_name / _words_kernel_name return after that launch
 *   scan_grid, scan_threads, scan_lds (bytes, 0 = tables read from global memory), lane_grid, word_grid, word_waves,
 *   word_lds_words, post_grid, post_waves (before a context bounds them by its arena), chunk_bytes, max_units (bound of the
 *   scan units), scan_words, post_clusters, image_words, scan_image_words, words_image_words (sizes of the three table images)
 * The SPA_L1_* switches of the environment count as they do for a context created and launched now.  SP_ERR_INVALID before
 * compile() or when the line does not fit bufsize. */
int sp_lexer_launch_plan(const sp_lexer_t* l, unsigned num_cus, size_t ndocs, size_t nbytes, char* buf, size_t bufsize);

/* PatternLexerInstanceInterface::createContext (:1120): an error before compile(); SP_ERR_DEVICE
 * without a usable GPU (no CPU fallback) */
sp_lexer_ctx_t* sp_lexer_ctx_create(const sp_lexer_t* l, int device);
void sp_lexer_ctx_free(sp_lexer_ctx_t* c);
const char* sp_lexer_ctx_last_error(const sp_lexer_ctx_t* c);
/* PatternLexerContextInterface::match (:858): one document, host buffers */
int sp_lexer_ctx_match(sp_lexer_ctx_t* c, const char* src, size_t srclen, sp_lexem_t** lexems, size_t* nlexems);
/* PatternLexerContextInterface::reset (:700) */
int sp_lexer_ctx_reset(sp_lexer_ctx_t* c);

/* ---- batch mode: many documents per launch ---- */
typedef struct sp_lex_batch {
	size_t ndocs;
	size_t nlexems;
	sp_lexem_t* lexems;            /* grouped by document, reference output order inside a document */
	uint64_t* doc_lexem_offsets;   /* ndocs+1 */
	int32_t* doc_status;           /* ndocs x SP_DOC_* */
} sp_lex_batch_t;
/* text: all documents back to back; doc_offsets: ndocs+1 byte offsets */
int sp_lexer_ctx_match_docs(sp_lexer_ctx_t* c, const char* text, const uint64_t* doc_offsets, size_t ndocs, sp_lex_batch_t* out);
void sp_lex_batch_free(sp_lex_batch_t* b);

typedef struct sp_lex_device_batch {
	size_t ndocs;
	void* d_lexems;        /* sp_lexem_t[], each document's lexems contiguous */
	void* d_doc_ranges;    /* uint64_t[ndocs][2] = (first lexem, count) */
	void* d_doc_status;    /* int32_t[ndocs] */
	void* d_counters;      /* uint64_t[8]: lexems, bytes, raw reports, failed docs */
} sp_lex_device_batch_t;
/* device-resident text and offsets, asynchronous on `stream` (hipStream_t); lexems stay in HBM */
int sp_lexer_ctx_match_docs_device(sp_lexer_ctx_t* c, const void* d_text, const void* d_doc_offsets,
                                   size_t ndocs, size_t nbytes, void* stream, sp_lex_device_batch_t* out);
/* host copy of the lexems of the documents [first_doc, first_doc+ndocs) of the last device batch
 * (what PatternLexerContextInterface::match returns for each of them, src/patternLexer.cpp:858) */
int sp_lexer_ctx_batch_fetch_docs(sp_lexer_ctx_t* c, size_t first_doc, size_t ndocs, sp_lex_batch_t* out);
/* ---- segmented documents: the "documents" of the last device batch are content segments (the pieces an XML, HTML or JSON
 * segmenter hands to the lexer one at a time), and document d consists of the segments
 * [doc_seg_offsets[d], doc_seg_offsets[d+1]) of that batch, in that order.  The stitch does on the device what a segmenting
 * caller does between lexer and matcher (the loop of the reference's command-line tool, `ordposOffset = lexems.back().ordpos()`;
 * that tool lives in strusAnalyzer, outside the reference repository, so the rule is this project's definition, unpinned by
 * a reference vector):
 *   - the lexems of a document are those of its segments in segment order, lexer order inside a segment;
 *   - the lexem (id, ordpos, origpos, origsize) of the document's s-th segment (s counts every segment from 0, empty ones
 *     included) becomes (id, ordpos + base_s, origpos, origsize) with origseg = s; base_0 = 0, base_{s+1} = the stitched ordpos
 *     of the last lexem of segment s, or base_s when segment s has no lexems; origpos stays relative to the segment;
 *   - a document fails and is empty when one of its segments failed in the lexer (its status: that of its first failing
 *     segment), when its segment range ends beyond the lexer batch or descends (SP_DOC_ERR_RANGE), or when a stitched ordpos
 *     or its lexem count does not fit 32 bits (SP_DOC_ERR_RANGE); a document of no segments is valid and empty.
 * The segment ranges of different documents are meant to be disjoint, as those of an ascending doc_seg_offsets are; the
 * stitched lexems then fit the lexer's lexem capacity, which sizes the buffers.  Ranges that share segments are not an
 * input this call defines lexems for: every access stays inside the buffers, and the documents that would end beyond the
 * capacity fail with SP_DOC_ERR_OUTPUT.
 * The stitched batch feeds the matcher as it is:
 *   sp_matcher_ctx_match_docs_device(mctx, out.d_lexems, out.d_origseg, out.d_doc_offsets, ndocs, nlexems, stream, &mout)
 * with nlexems = d_totals[0], or any upper bound of it such as the lexer batch's lexem counter.  A document that failed
 * in the stitch reaches the matcher as an empty document and comes back from it with status 0: the caller combines the two
 * status arrays. */
typedef struct sp_lex_stitched_batch {
	size_t ndocs;
	void* d_lexems;        /* sp_lexem_t[], document 0 first, segment order inside a document */
	void* d_origseg;       /* uint32_t[] parallel to d_lexems */
	void* d_doc_offsets;   /* uint64_t[ndocs+1] -- what sp_matcher_ctx_match_docs_device takes */
	void* d_doc_status;    /* int32_t[ndocs] */
	void* d_totals;        /* uint64_t[2]: lexems, failed documents */
} sp_lex_stitched_batch_t;
/* Enqueues the stitching passes (count, offsets, place: csrc/l1_stitch.h) for the last device batch of the context on `stream`
 * and returns without waiting for anything; d_doc_seg_offsets is a device array uint64_t[ndocs+1].  A `stream` other than the
 * batch's is ordered behind the batch with an event.  SP_ERR_INVALID before any batch has run on the context.  The buffers
 * belong to the context (allocated at the first stitch, a context that never stitches has none) and are valid until the
 * next stitch on it; the raw batch stays as it is.  The next lexer batch on the context invalidates the stitched state (not
 * the buffers).  A batch with segments that failed for lack of room is grown and rerun before it is stitched, as ever. */
int sp_lexer_ctx_stitch_segments_device(sp_lexer_ctx_t* c, const void* d_doc_seg_offsets, size_t ndocs,
                                        void* stream, sp_lex_stitched_batch_t* out);
/* plain copy of the stitched buffers to the host (waits for the stitch): the batch is released with sp_lex_batch_free, *origseg
 * (parallel to out->lexems; the parameter may be NULL) with sp_free.  SP_ERR_INVALID when the last batch has not been stitched. */
int sp_lexer_ctx_stitched_fetch(sp_lexer_ctx_t* c, sp_lex_batch_t* out, uint32_t** origseg);
/* copies the first `ndocs` status words of the stitched batch to the host (waits for the stitch; a caller that feeds the matcher
 * on the device needs only these); ndocs_stitched, if given, receives the number of documents of the stitch.  SP_ERR_INVALID
 * when the last batch has not been stitched. */
int sp_lexer_ctx_stitched_status(sp_lexer_ctx_t* c, int32_t* status, size_t ndocs, size_t* ndocs_stitched);
/* duration of the three passes of the last stitch in milliseconds (HIP events on its stream; waits for them) */
int sp_lexer_ctx_last_stitch_ms(sp_lexer_ctx_t* c, double* ms);
int sp_lexer_ctx_batch_counters(sp_lexer_ctx_t* c, uint64_t counters[8]);
int sp_lexer_ctx_batch_status(sp_lexer_ctx_t* c, int32_t* status, size_t ndocs);
double sp_lexer_ctx_last_kernel_ms(sp_lexer_ctx_t* c);
/* the same interval split at the boundary of the lexer's two kernels (automaton scan; literals + start of match +
 * handler + ordinal positions) */
int sp_lexer_ctx_last_kernel_ms_split(sp_lexer_ctx_t* c, double* scan_ms, double* post_ms);
/* the same in three parts: automaton scan; words kernel (whole-word literals and word shapes, found where runs of word
 * characters end); start of match + handler + ordinal positions */
int sp_lexer_ctx_last_kernel_ms_split3(sp_lexer_ctx_t* c, double* scan_ms, double* words_ms, double* post_ms);
/* name of the scan kernel the last launch of this context went through ("(none)" before the first launch) */
const char* sp_lexer_ctx_scan_kernel_name(const sp_lexer_ctx_t* c);
/* the same for the words kernel (whole-word literals and word shapes): its 12- or 16-wave instance, "(none)" for tables it does not take */
const char* sp_lexer_ctx_words_kernel_name(const sp_lexer_ctx_t* c);
int sp_lexer_ctx_reserve_output(sp_lexer_ctx_t* c, uint64_t lexems);
int sp_lexer_ctx_grow_arena(sp_lexer_ctx_t* c);

#ifdef __cplusplus
}
#endif
#endif
