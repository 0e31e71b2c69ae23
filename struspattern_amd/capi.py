"""ctypes binding of include/strus_pattern_amd.h (the C-ABI of libstruspattern_amd.so).

The library is the product: if it cannot be loaded this module raises -- there is no Python or
CPU fallback for the match path."""
import ctypes
import os

from . import build as _build

c_u32 = ctypes.c_uint32
c_u64 = ctypes.c_uint64
c_vp = ctypes.c_void_p
c_cp = ctypes.c_char_p
P = ctypes.POINTER


class SpLexem(ctypes.Structure):
    _fields_ = [("id", c_u32), ("ordpos", c_u32), ("origpos", c_u32), ("origsize", c_u32)]


class SpResult(ctypes.Structure):
    _fields_ = [(n, c_u32) for n in ("handle", "ordpos", "ordend", "origseg", "origpos", "origendseg", "origend", "item_begin", "item_count")]


class SpResultItem(ctypes.Structure):
    _fields_ = [(n, c_u32) for n in ("variable", "ordpos", "ordend", "origseg", "origpos", "origendseg", "origend")]


class SpMatcherStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("nofProgramsInstalled", "nofAltKeyProgramsInstalled", "nofSignalsFired", "nofTriggersAvgActive")]


class SpMatchBatch(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("nresults", ctypes.c_size_t), ("nitems", ctypes.c_size_t),
        ("results", P(SpResult)), ("items", P(SpResultItem)),
        ("doc_result_offsets", P(c_u64)), ("doc_stats", P(c_u64)), ("doc_status", P(ctypes.c_int32)),
        ("result_format", P(c_u32)), ("item_format", P(c_u32)),
    ]


class SpLexBatch(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("nlexems", ctypes.c_size_t), ("lexems", P(SpLexem)),
        ("doc_lexem_offsets", P(c_u64)), ("doc_status", P(ctypes.c_int32)),
    ]


class SpLexDeviceBatch(ctypes.Structure):
    _fields_ = [("ndocs", ctypes.c_size_t), ("d_lexems", c_vp), ("d_doc_ranges", c_vp), ("d_doc_status", c_vp), ("d_counters", c_vp)]


class SpLexStitchedBatch(ctypes.Structure):
    _fields_ = [("ndocs", ctypes.c_size_t), ("d_lexems", c_vp), ("d_origseg", c_vp), ("d_doc_offsets", c_vp), ("d_doc_status", c_vp), ("d_totals", c_vp)]


class SpMatchDeviceBatch(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("d_results", c_vp), ("d_items", c_vp), ("d_doc_result_offsets", c_vp),
        ("d_doc_stats", c_vp), ("d_doc_status", c_vp), ("d_counters", c_vp),
        ("d_result_format", c_vp), ("d_item_format", c_vp),
    ]


class SpMatchFinishedBatch(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("d_results", c_vp), ("d_items", c_vp), ("d_doc_result_offsets", c_vp),
        ("d_doc_item_offsets", c_vp), ("d_result_format", c_vp), ("d_item_format", c_vp), ("d_totals", c_vp),
    ]


class SpTextSource(ctypes.Structure):
    _fields_ = [("d_text", c_vp), ("nbytes", c_u64), ("d_seg_offsets", c_vp), ("nseg", ctypes.c_size_t), ("d_doc_seg_offsets", c_vp)]


class SpMatchTextBatch(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("d_result_text", c_vp), ("d_result_text_offsets", c_vp), ("d_item_text", c_vp),
        ("d_item_text_offsets", c_vp), ("d_doc_text_status", c_vp), ("d_totals", c_vp),
    ]


class SpMatchText(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("nresults", ctypes.c_size_t), ("nitems", ctypes.c_size_t),
        ("result_text", P(ctypes.c_uint8)), ("result_text_offsets", P(c_u64)), ("item_text", P(ctypes.c_uint8)), ("item_text_offsets", P(c_u64)),
        ("doc_text_status", P(ctypes.c_int32)), ("totals", c_u64 * 2),
    ]


class SpMatchValuesBatch(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("d_result_values", c_vp), ("d_result_value_offsets", c_vp), ("d_item_values", c_vp),
        ("d_item_value_offsets", c_vp), ("d_doc_value_status", c_vp), ("d_totals", c_vp),
    ]


class SpMatchValues(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("nresults", ctypes.c_size_t), ("nitems", ctypes.c_size_t),
        ("result_values", P(ctypes.c_uint8)), ("result_value_offsets", P(c_u64)), ("item_values", P(ctypes.c_uint8)), ("item_value_offsets", P(c_u64)),
        ("doc_value_status", P(ctypes.c_int32)), ("totals", c_u64 * 2),
    ]


class SpPatternFreq(ctypes.Structure):
    _fields_ = [(n, c_u32) for n in ("handle", "count", "first_ordpos", "last_ordend")]


class SpPatternFreqDevice(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("handle_bound", c_u32), ("d_records", c_vp), ("d_doc_offsets", c_vp), ("d_doc_freq_status", c_vp),
        ("d_handle_results", c_vp), ("d_handle_docs", c_vp), ("d_totals", c_vp),
    ]


class SpPatternFreqBatch(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("nrecords", ctypes.c_size_t), ("handle_bound", c_u32),
        ("records", P(SpPatternFreq)), ("doc_offsets", P(c_u64)), ("doc_freq_status", P(ctypes.c_int32)),
        ("handle_results", P(c_u64)), ("handle_docs", P(c_u32)), ("totals", c_u64 * 1),
    ]


class SpMatchTerm(ctypes.Structure):
    _fields_ = [(n, c_u32) for n in ("handle", "count", "first_ordpos", "last_ordend", "first_result", "value_bytes")]


class SpMatchTermsDevice(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("handle_bound", c_u32), ("flags", c_u32), ("d_records", c_vp), ("d_doc_term_offsets", c_vp),
        ("d_result_term", c_vp), ("d_doc_term_status", c_vp), ("d_totals", c_vp),
    ]


class SpMatchTerms(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("nresults", ctypes.c_size_t), ("nrecords", ctypes.c_size_t), ("handle_bound", c_u32), ("flags", c_u32),
        ("records", P(SpMatchTerm)), ("doc_term_offsets", P(c_u64)), ("result_term", P(c_u32)), ("doc_term_status", P(ctypes.c_int32)),
        ("totals", c_u64 * 1),
    ]


class SpDictTerm(ctypes.Structure):
    _fields_ = [(n, c_u32) for n in ("handle", "value_bytes", "first_doc", "first_term", "doc_freq", "max_count")] + [("count", c_u64)]


class SpMatchDictionaryDevice(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("handle_bound", c_u32), ("flags", c_u32), ("d_records", c_vp), ("d_term_dict", c_vp),
        ("d_doc_dict_offsets", c_vp), ("d_handle_terms", c_vp), ("d_totals", c_vp),
    ]


class SpMatchDictionary(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("nterms", ctypes.c_size_t), ("ndict", ctypes.c_size_t), ("handle_bound", c_u32), ("flags", c_u32),
        ("records", P(SpDictTerm)), ("term_dict", P(c_u32)), ("doc_dict_offsets", P(c_u64)), ("handle_terms", P(c_u32)),
        ("totals", c_u64 * 1),
    ]


class SpMatchDictionaryOrderDevice(ctypes.Structure):
    _fields_ = [
        ("ndict", ctypes.c_size_t), ("handle_bound", c_u32), ("d_order", c_vp), ("d_rank", c_vp), ("d_prefix_bytes", c_vp),
        ("d_handle_offsets", c_vp), ("d_totals", c_vp),
    ]


class SpMatchDictionaryOrder(ctypes.Structure):
    _fields_ = [
        ("ndict", ctypes.c_size_t), ("handle_bound", c_u32), ("order", P(c_u32)), ("rank", P(c_u32)), ("prefix_bytes", P(c_u32)),
        ("handle_offsets", P(c_u64)), ("totals", c_u64 * 1),
    ]


class SpTermBlockEntry(ctypes.Structure):
    _fields_ = [("handle", c_u32), ("value_bytes", c_u32), ("value_offset", c_u64), ("doc_freq", c_u32), ("reserved", c_u32), ("count", c_u64)]


class SpMatchTermBlocksDevice(ctypes.Structure):
    _fields_ = [
        ("ndict", ctypes.c_size_t), ("nblocks", ctypes.c_size_t), ("nbytes", ctypes.c_size_t), ("block_entries", c_u32),
        ("d_bytes", c_vp), ("d_block_offsets", c_vp), ("d_block_handles", c_vp), ("d_totals", c_vp),
    ]


class SpMatchTermBlocks(ctypes.Structure):
    _fields_ = [
        ("ndict", ctypes.c_size_t), ("nblocks", ctypes.c_size_t), ("nbytes", ctypes.c_size_t), ("block_entries", c_u32),
        ("bytes", P(ctypes.c_uint8)), ("block_offsets", P(c_u64)), ("block_handles", P(c_u32)), ("totals", c_u64 * 4),
    ]


class SpBlockPosting(ctypes.Structure):
    _fields_ = [("doc", c_u32), ("count", c_u32), ("npos", c_u32), ("reserved", c_u32), ("position_offset", c_u64)]


class SpMatchPostingBlocksDevice(ctypes.Structure):
    _fields_ = [
        ("ndict", ctypes.c_size_t), ("nblocks", ctypes.c_size_t), ("nbytes", ctypes.c_size_t), ("block_entries", c_u32),
        ("d_bytes", c_vp), ("d_block_offsets", c_vp), ("d_totals", c_vp),
    ]


class SpMatchPostingBlocks(ctypes.Structure):
    _fields_ = [
        ("ndict", ctypes.c_size_t), ("nblocks", ctypes.c_size_t), ("nbytes", ctypes.c_size_t), ("block_entries", c_u32),
        ("bytes", P(ctypes.c_uint8)), ("block_offsets", P(c_u64)), ("totals", c_u64 * 4),
    ]


class SpSegmentSelection(ctypes.Structure):
    _fields_ = [("position", c_u32), ("handle", c_u32), ("doc_freq", c_u32), ("value_bytes", c_u32), ("count", c_u64)]


class SpSegmentPosting(ctypes.Structure):
    _fields_ = [(n, c_u32) for n in ("doc", "count", "npos", "reserved")]


class SpSegmentLookupDevice(ctypes.Structure):
    _fields_ = [(n, ctypes.c_size_t) for n in ("nq", "nsel", "npostings", "npositions", "nvalue_bytes")] + [("flags", c_u32)] + [
        (n, c_vp) for n in ("d_q_first", "d_q_count", "d_q_status", "d_q_sel_offsets", "d_selections", "d_sel_value_offsets", "d_sel_posting_offsets",
                            "d_values", "d_postings", "d_posting_position_offsets", "d_positions", "d_totals")]


class SpSegmentLookup(ctypes.Structure):
    _fields_ = [(n, ctypes.c_size_t) for n in ("nq", "nsel", "npostings", "npositions", "nvalue_bytes")] + [
        ("flags", c_u32), ("q_first", P(c_u32)), ("q_count", P(c_u32)), ("q_status", P(c_u32)), ("q_sel_offsets", P(c_u64)),
        ("selections", P(SpSegmentSelection)), ("sel_value_offsets", P(c_u64)), ("sel_posting_offsets", P(c_u64)),
        ("values", P(ctypes.c_uint8)), ("postings", P(SpSegmentPosting)), ("posting_position_offsets", P(c_u64)), ("positions", P(c_u32)),
        ("totals", c_u64 * 4),
    ]


class SpPosting(ctypes.Structure):
    _fields_ = [(n, c_u32) for n in ("doc", "term", "count", "first_ordpos")]


class SpMatchPostingsDevice(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("nterms", ctypes.c_size_t), ("ndict", ctypes.c_size_t), ("d_postings", c_vp), ("d_entry_offsets", c_vp),
        ("d_record_posting", c_vp), ("d_totals", c_vp),
    ]


class SpMatchPostings(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("nterms", ctypes.c_size_t), ("ndict", ctypes.c_size_t),
        ("postings", P(SpPosting)), ("entry_offsets", P(c_u64)), ("record_posting", P(c_u32)), ("totals", c_u64 * 1),
    ]


class SpOccurrence(ctypes.Structure):
    _fields_ = [(n, c_u32) for n in ("ordpos", "result")]


class SpMatchPositionsDevice(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("nterms", ctypes.c_size_t), ("nocc", ctypes.c_size_t), ("d_occurrences", c_vp), ("d_posting_offsets", c_vp),
        ("d_posting_positions", c_vp), ("d_totals", c_vp),
    ]


class SpMatchPositions(ctypes.Structure):
    _fields_ = [
        ("ndocs", ctypes.c_size_t), ("nterms", ctypes.c_size_t), ("nocc", ctypes.c_size_t),
        ("occurrences", P(SpOccurrence)), ("posting_offsets", P(c_u64)), ("posting_positions", P(c_u32)), ("totals", c_u64 * 2),
    ]


# name -> (restype, argtypes); every symbol declared in include/strus_pattern_amd.h
SIGNATURES = {
    "sp_version": (c_cp, []),
    "sp_device_count": (ctypes.c_int, []),
    "sp_free": (None, [c_vp]),
    "sp_test_fail_alloc_above": (None, [c_u64]),
    "sp_match_batch_regroup": (ctypes.c_int, [c_vp, c_u64, c_vp, c_u64, c_vp, c_vp, c_vp, c_vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                              ctypes.c_int, c_u32, P(SpMatchBatch), ctypes.c_char_p, ctypes.c_size_t]),
    "sp_matcher_create": (c_vp, []),
    "sp_matcher_free": (None, [c_vp]),
    "sp_matcher_last_error": (c_cp, [c_vp]),
    "sp_matcher_define_term_frequency": (ctypes.c_int, [c_vp, c_u32, ctypes.c_double]),
    "sp_matcher_push_term": (ctypes.c_int, [c_vp, c_u32]),
    "sp_matcher_push_expression": (ctypes.c_int, [c_vp, ctypes.c_int, ctypes.c_size_t, c_u32, c_u32]),
    "sp_matcher_push_pattern": (ctypes.c_int, [c_vp, c_cp]),
    "sp_matcher_attach_variable": (ctypes.c_int, [c_vp, c_cp]),
    "sp_matcher_define_pattern": (ctypes.c_int, [c_vp, c_cp, c_cp, ctypes.c_int]),
    "sp_matcher_define_option": (ctypes.c_int, [c_vp, c_cp, ctypes.c_double]),
    "sp_matcher_compile": (ctypes.c_int, [c_vp]),
    "sp_matcher_pattern_id": (c_u32, [c_vp, c_cp]),
    "sp_matcher_pattern_name": (c_cp, [c_vp, c_u32]),
    "sp_matcher_variable_id": (c_u32, [c_vp, c_cp]),
    "sp_matcher_variable_name": (c_cp, [c_vp, c_u32]),
    "sp_matcher_dump_table": (ctypes.c_size_t, [c_vp, P(P(c_u32))]),
    "sp_matcher_fast_tier": (ctypes.c_int, [c_vp, ctypes.c_char_p, ctypes.c_size_t]),
    "sp_matcher_result_set_tier": (ctypes.c_int, [c_vp, ctypes.c_char_p, ctypes.c_size_t, P(c_u32)]),
    "sp_matcher_launch_plan": (ctypes.c_int, [c_vp, c_u32, ctypes.c_uint, ctypes.c_uint, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, c_u32, c_u64, c_u64, ctypes.c_char_p, ctypes.c_size_t]),
    "sp_matcher_serialize": (ctypes.c_int, [c_vp, P(c_vp), P(ctypes.c_size_t)]),
    "sp_matcher_deserialize": (c_vp, [c_vp, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]),
    "sp_lexer_serialize": (ctypes.c_int, [c_vp, P(c_vp), P(ctypes.c_size_t)]),
    "sp_lexer_deserialize": (c_vp, [c_vp, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]),
    "sp_matcher_format_count": (c_u32, [c_vp]),
    "sp_matcher_format_string": (c_cp, [c_vp, c_u32]),
    "sp_matcher_ctx_fetch_formats": (ctypes.c_int, [c_vp, P(P(c_u32)), P(P(c_u32))]),
    "sp_matcher_ctx_create": (c_vp, [c_vp, ctypes.c_int]),
    "sp_matcher_ctx_create_ex": (c_vp, [c_vp, ctypes.c_int, c_u32]),
    "sp_matcher_ctx_free": (None, [c_vp]),
    "sp_matcher_ctx_last_error": (c_cp, [c_vp]),
    "sp_matcher_ctx_put_input": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_size_t]),
    "sp_matcher_ctx_fetch_results": (ctypes.c_int, [c_vp, P(P(SpResult)), P(ctypes.c_size_t), P(P(SpResultItem)), P(ctypes.c_size_t)]),
    "sp_matcher_ctx_statistics": (ctypes.c_int, [c_vp, P(SpMatcherStats)]),
    "sp_matcher_ctx_reset": (ctypes.c_int, [c_vp]),
    "sp_matcher_ctx_match_docs": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.c_size_t, P(SpMatchBatch)]),
    "sp_match_batch_free": (None, [P(SpMatchBatch)]),
    "sp_matcher_ctx_match_docs_device": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.c_size_t, ctypes.c_size_t, c_vp, P(SpMatchDeviceBatch)]),
    "sp_matcher_ctx_match_lexed_device": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_size_t, ctypes.c_size_t, c_vp, P(SpMatchDeviceBatch)]),
    "sp_matcher_ctx_batch_fetch": (ctypes.c_int, [c_vp, P(SpMatchBatch)]),
    "sp_matcher_ctx_batch_fetch_docs": (ctypes.c_int, [c_vp, ctypes.c_size_t, ctypes.c_size_t, P(SpMatchBatch)]),
    "sp_matcher_ctx_batch_finish_device": (ctypes.c_int, [c_vp, c_vp, P(SpMatchFinishedBatch)]),
    "sp_matcher_ctx_batch_finish_device_ex": (ctypes.c_int, [c_vp, c_vp, c_u32, P(SpMatchFinishedBatch)]),
    "sp_matcher_ctx_finished_fetch": (ctypes.c_int, [c_vp, P(SpMatchBatch)]),
    "sp_matcher_ctx_last_finish_ms": (ctypes.c_int, [c_vp, P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_double)]),
    "sp_matcher_ctx_last_finish_sort_ms": (ctypes.c_int, [c_vp, P(ctypes.c_double)]),
    "sp_matcher_finish_sort_tile": (c_u32, []),
    "sp_matcher_ctx_finished_text_device": (ctypes.c_int, [c_vp, P(SpTextSource), c_u32, c_vp, P(SpMatchTextBatch)]),
    "sp_matcher_ctx_finished_text_fetch": (ctypes.c_int, [c_vp, P(SpMatchText)]),
    "sp_match_text_free": (None, [P(SpMatchText)]),
    "sp_matcher_ctx_last_text_ms": (ctypes.c_int, [c_vp, P(ctypes.c_double)]),
    "sp_matcher_text_long_span": (c_u32, []),
    "sp_matcher_ctx_finished_values_device": (ctypes.c_int, [c_vp, P(SpTextSource), c_u32, c_vp, P(SpMatchValuesBatch)]),
    "sp_matcher_ctx_finished_values_fetch": (ctypes.c_int, [c_vp, P(SpMatchValues)]),
    "sp_match_values_free": (None, [P(SpMatchValues)]),
    "sp_matcher_ctx_last_values_ms": (ctypes.c_int, [c_vp, P(ctypes.c_double)]),
    "sp_matcher_value_max_depth": (c_u32, []),
    "sp_match_batch_values": (ctypes.c_int, [c_vp, P(SpMatchBatch), c_vp, c_u64, c_vp, ctypes.c_size_t, c_vp, c_u32, P(SpMatchValues), ctypes.c_char_p, ctypes.c_size_t]),
    "sp_match_batch_text": (ctypes.c_int, [P(SpMatchBatch), c_vp, c_u64, c_vp, ctypes.c_size_t, c_vp, c_u32, P(SpMatchText), ctypes.c_char_p, ctypes.c_size_t]),
    "sp_matcher_handle_bound": (c_u32, [c_vp]),
    "sp_matcher_ctx_finished_pattern_freq_device": (ctypes.c_int, [c_vp, c_vp, P(SpPatternFreqDevice)]),
    "sp_matcher_ctx_finished_pattern_freq_fetch": (ctypes.c_int, [c_vp, P(SpPatternFreqBatch)]),
    "sp_pattern_freq_batch_free": (None, [P(SpPatternFreqBatch)]),
    "sp_matcher_ctx_last_pattern_freq_ms": (ctypes.c_int, [c_vp, P(ctypes.c_double)]),
    "sp_matcher_pattern_freq_window": (c_u32, []),
    "sp_match_batch_pattern_freq": (ctypes.c_int, [P(SpMatchBatch), c_u32, P(SpPatternFreqBatch), ctypes.c_char_p, ctypes.c_size_t]),
    "sp_matcher_ctx_finished_terms_device": (ctypes.c_int, [c_vp, c_u32, c_vp, P(SpMatchTermsDevice)]),
    "sp_matcher_ctx_finished_terms_fetch": (ctypes.c_int, [c_vp, P(SpMatchTerms)]),
    "sp_match_terms_free": (None, [P(SpMatchTerms)]),
    "sp_matcher_ctx_last_terms_ms": (ctypes.c_int, [c_vp, P(ctypes.c_double)]),
    "sp_matcher_term_tile": (c_u32, []),
    "sp_test_term_hash_bits": (None, [ctypes.c_uint]),
    "sp_match_batch_terms": (ctypes.c_int, [P(SpMatchBatch), P(SpMatchValues), P(SpMatchText), c_u32, c_u32, P(SpMatchTerms), ctypes.c_char_p, ctypes.c_size_t]),
    "sp_matcher_ctx_finished_dictionary_device": (ctypes.c_int, [c_vp, c_vp, P(SpMatchDictionaryDevice)]),
    "sp_matcher_ctx_finished_dictionary_fetch": (ctypes.c_int, [c_vp, P(SpMatchDictionary)]),
    "sp_match_dictionary_free": (None, [P(SpMatchDictionary)]),
    "sp_matcher_ctx_last_dictionary_ms": (ctypes.c_int, [c_vp, P(ctypes.c_double)]),
    "sp_match_batch_dictionary": (ctypes.c_int, [P(SpMatchBatch), P(SpMatchValues), P(SpMatchText), P(SpMatchTerms), P(SpMatchDictionary), ctypes.c_char_p, ctypes.c_size_t]),
    "sp_matcher_ctx_finished_dictionary_order_device": (ctypes.c_int, [c_vp, c_vp, P(SpMatchDictionaryOrderDevice)]),
    "sp_matcher_ctx_finished_dictionary_order_fetch": (ctypes.c_int, [c_vp, P(SpMatchDictionaryOrder)]),
    "sp_match_dictionary_order_free": (None, [P(SpMatchDictionaryOrder)]),
    "sp_matcher_ctx_last_dictionary_order_ms": (ctypes.c_int, [c_vp, P(ctypes.c_double)]),
    "sp_matcher_dictionary_order_tile": (c_u32, []),
    "sp_match_batch_dictionary_order": (ctypes.c_int, [P(SpMatchBatch), P(SpMatchValues), P(SpMatchText), P(SpMatchTerms), P(SpMatchDictionary),
                                                        P(SpMatchDictionaryOrder), ctypes.c_char_p, ctypes.c_size_t]),
    "sp_matcher_term_block_entries": (c_u32, []),
    "sp_test_term_block_entries": (None, [ctypes.c_uint]),
    "sp_matcher_ctx_finished_term_blocks_device": (ctypes.c_int, [c_vp, c_vp, P(SpMatchTermBlocksDevice)]),
    "sp_matcher_ctx_finished_term_blocks_fetch": (ctypes.c_int, [c_vp, P(SpMatchTermBlocks)]),
    "sp_match_term_blocks_free": (None, [P(SpMatchTermBlocks)]),
    "sp_matcher_ctx_last_term_blocks_ms": (ctypes.c_int, [c_vp, P(ctypes.c_double)]),
    "sp_match_batch_term_blocks": (ctypes.c_int, [P(SpMatchBatch), P(SpMatchValues), P(SpMatchText), P(SpMatchTerms), P(SpMatchDictionary),
                                                   P(SpMatchDictionaryOrder), P(SpMatchTermBlocks), ctypes.c_char_p, ctypes.c_size_t]),
    "sp_match_term_blocks_decode_block": (ctypes.c_int, [P(SpMatchTermBlocks), ctypes.c_size_t, P(SpTermBlockEntry), ctypes.c_size_t, P(ctypes.c_uint8),
                                                          ctypes.c_size_t, P(ctypes.c_size_t), P(ctypes.c_size_t), ctypes.c_char_p, ctypes.c_size_t]),
    "sp_matcher_ctx_finished_postings_device": (ctypes.c_int, [c_vp, c_vp, P(SpMatchPostingsDevice)]),
    "sp_matcher_ctx_finished_postings_fetch": (ctypes.c_int, [c_vp, P(SpMatchPostings)]),
    "sp_match_postings_free": (None, [P(SpMatchPostings)]),
    "sp_matcher_ctx_last_postings_ms": (ctypes.c_int, [c_vp, P(ctypes.c_double)]),
    "sp_matcher_postings_tile": (c_u32, []),
    "sp_test_postings_digit_bits": (None, [ctypes.c_uint]),
    "sp_match_batch_postings": (ctypes.c_int, [P(SpMatchTerms), P(SpMatchDictionary), P(SpMatchPostings), ctypes.c_char_p, ctypes.c_size_t]),
    "sp_matcher_ctx_finished_positions_device": (ctypes.c_int, [c_vp, c_vp, P(SpMatchPositionsDevice)]),
    "sp_matcher_ctx_finished_positions_fetch": (ctypes.c_int, [c_vp, P(SpMatchPositions)]),
    "sp_match_positions_free": (None, [P(SpMatchPositions)]),
    "sp_matcher_ctx_last_positions_ms": (ctypes.c_int, [c_vp, P(ctypes.c_double)]),
    "sp_matcher_positions_tile": (c_u32, []),
    "sp_test_positions_launch_events": (None, [ctypes.c_uint]),
    "sp_matcher_ctx_last_positions_launch_ms": (ctypes.c_int, [c_vp, P(ctypes.c_double)]),
    "sp_match_batch_positions": (ctypes.c_int, [P(SpMatchBatch), P(SpMatchTerms), P(SpMatchPostings), P(SpMatchPositions), ctypes.c_char_p, ctypes.c_size_t]),
    "sp_matcher_ctx_finished_posting_blocks_device": (ctypes.c_int, [c_vp, c_vp, P(SpMatchPostingBlocksDevice)]),
    "sp_matcher_ctx_finished_posting_blocks_fetch": (ctypes.c_int, [c_vp, P(SpMatchPostingBlocks)]),
    "sp_match_posting_blocks_free": (None, [P(SpMatchPostingBlocks)]),
    "sp_matcher_ctx_last_posting_blocks_ms": (ctypes.c_int, [c_vp, P(ctypes.c_double)]),
    "sp_match_batch_posting_blocks": (ctypes.c_int, [P(SpMatchDictionary), P(SpMatchDictionaryOrder), P(SpMatchPostings), P(SpMatchPositions),
                                                      P(SpMatchPostingBlocks), ctypes.c_char_p, ctypes.c_size_t]),
    "sp_match_posting_blocks_decode_block": (ctypes.c_int, [P(SpMatchPostingBlocks), ctypes.c_size_t, P(c_u32), ctypes.c_size_t, P(SpBlockPosting), ctypes.c_size_t,
                                                             P(c_u32), ctypes.c_size_t, P(ctypes.c_size_t), P(ctypes.c_size_t), P(ctypes.c_size_t),
                                                             ctypes.c_char_p, ctypes.c_size_t]),
    "sp_segment_open": (ctypes.c_int, [P(SpMatchTermBlocks), P(SpMatchPostingBlocks), P(c_vp), ctypes.c_char_p, ctypes.c_size_t]),
    "sp_segment_from_ctx": (ctypes.c_int, [c_vp, c_vp, P(c_vp)]),
    "sp_segment_free": (None, [c_vp]),
    "sp_segment_last_error": (c_cp, [c_vp]),
    "sp_segment_lookup_device": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.c_size_t, c_u32, c_vp, P(SpSegmentLookupDevice)]),
    "sp_segment_lookup_fetch": (ctypes.c_int, [c_vp, P(SpSegmentLookup)]),
    "sp_segment_lookup_free": (None, [P(SpSegmentLookup)]),
    "sp_segment_last_lookup_ms": (ctypes.c_int, [c_vp, P(ctypes.c_double)]),
    "sp_match_segment_lookup": (ctypes.c_int, [P(SpMatchTermBlocks), P(SpMatchPostingBlocks), c_vp, c_vp, c_vp, ctypes.c_size_t, c_u32,
                                                P(SpSegmentLookup), ctypes.c_char_p, ctypes.c_size_t]),
    "sp_matcher_ctx_batch_counters": (ctypes.c_int, [c_vp, P(c_u64)]),
    "sp_matcher_ctx_last_kernel_ms": (ctypes.c_double, [c_vp]),
    "sp_matcher_ctx_kernel_kind": (ctypes.c_int, [c_vp]),
    "sp_matcher_ctx_kernel_name": (ctypes.c_char_p, [c_vp]),
    "sp_matcher_ctx_batch_status": (ctypes.c_int, [c_vp, c_vp, ctypes.c_size_t]),
    "sp_matcher_ctx_grow_arena": (ctypes.c_int, [c_vp]),
    "sp_matcher_ctx_reserve_output": (ctypes.c_int, [c_vp, c_u64, c_u64]),
    "sp_matcher_ctx_set_arena": (ctypes.c_int, [c_vp, c_u32, c_u32, c_u32, c_u32, c_u32]),
    "sp_lexer_create": (c_vp, []),
    "sp_lexer_free": (None, [c_vp]),
    "sp_lexer_last_error": (c_cp, [c_vp]),
    "sp_lexer_define_lexem_name": (ctypes.c_int, [c_vp, c_u32, c_cp]),
    "sp_lexer_get_lexem_name": (c_cp, [c_vp, c_u32]),
    "sp_lexer_define_lexem": (ctypes.c_int, [c_vp, c_u32, c_cp, c_u32, c_u32, ctypes.c_int]),
    "sp_lexer_define_symbol": (ctypes.c_int, [c_vp, c_u32, c_u32, c_cp]),
    "sp_lexer_get_symbol": (c_u32, [c_vp, c_u32, c_cp]),
    "sp_lexer_define_option": (ctypes.c_int, [c_vp, c_cp, ctypes.c_double]),
    "sp_lexer_compile": (ctypes.c_int, [c_vp]),
    "sp_lexer_dump_tables": (ctypes.c_size_t, [c_vp, P(P(c_u64))]),
    "sp_lexer_dump_image": (ctypes.c_size_t, [c_vp, ctypes.c_int, P(P(c_u64))]),
    "sp_lexer_launch_plan": (ctypes.c_int, [c_vp, ctypes.c_uint, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]),
    "sp_lexer_ctx_create": (c_vp, [c_vp, ctypes.c_int]),
    "sp_lexer_ctx_free": (None, [c_vp]),
    "sp_lexer_ctx_last_error": (c_cp, [c_vp]),
    "sp_lexer_ctx_match": (ctypes.c_int, [c_vp, c_cp, ctypes.c_size_t, P(P(SpLexem)), P(ctypes.c_size_t)]),
    "sp_lexer_ctx_reset": (ctypes.c_int, [c_vp]),
    "sp_lexer_ctx_match_docs": (ctypes.c_int, [c_vp, c_cp, c_vp, ctypes.c_size_t, P(SpLexBatch)]),
    "sp_lex_batch_free": (None, [P(SpLexBatch)]),
    "sp_lexer_ctx_match_docs_device": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_size_t, ctypes.c_size_t, c_vp, P(SpLexDeviceBatch)]),
    "sp_lexer_ctx_batch_fetch_docs": (ctypes.c_int, [c_vp, ctypes.c_size_t, ctypes.c_size_t, P(SpLexBatch)]),
    "sp_lexer_ctx_stitch_segments_device": (ctypes.c_int, [c_vp, c_vp, ctypes.c_size_t, c_vp, P(SpLexStitchedBatch)]),
    "sp_lexer_ctx_stitched_fetch": (ctypes.c_int, [c_vp, P(SpLexBatch), P(P(c_u32))]),
    "sp_lexer_ctx_stitched_status": (ctypes.c_int, [c_vp, c_vp, ctypes.c_size_t, P(ctypes.c_size_t)]),
    "sp_lexer_ctx_last_stitch_ms": (ctypes.c_int, [c_vp, P(ctypes.c_double)]),
    "sp_lexer_ctx_batch_counters": (ctypes.c_int, [c_vp, P(c_u64)]),
    "sp_lexer_ctx_batch_status": (ctypes.c_int, [c_vp, c_vp, ctypes.c_size_t]),
    "sp_lexer_ctx_last_kernel_ms": (ctypes.c_double, [c_vp]),
    "sp_lexer_ctx_last_kernel_ms_split": (ctypes.c_int, [c_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "sp_lexer_ctx_scan_kernel_name": (ctypes.c_char_p, [c_vp]),
    "sp_lexer_ctx_words_kernel_name": (ctypes.c_char_p, [c_vp]),
    "sp_lexer_ctx_last_kernel_ms_split3": (ctypes.c_int, [c_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "sp_lexer_ctx_reserve_output": (ctypes.c_int, [c_vp, c_u64]),
    "sp_lexer_ctx_grow_arena": (ctypes.c_int, [c_vp]),
}

_LIB = None


def lib():
    """Loads libstruspattern_amd.so (building it first if the sources are newer)."""
    global _LIB
    if _LIB is None:
        path = _build.LIB
        if _build.needs_build():
            path = _build.build()
        L = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB
