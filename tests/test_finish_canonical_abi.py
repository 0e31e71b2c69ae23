"""The C-ABI of the canonical device finish (include/strus_pattern_amd.h: SP_FINISH_CANONICAL,
sp_matcher_ctx_batch_finish_device_ex, sp_matcher_ctx_last_finish_sort_ms, sp_matcher_finish_sort_tile) as the built library
exports it and as struspattern_amd/capi.py declares it, and the Python statement of the order (tests/canonical_order.py) on
a batch written by hand.  No GPU."""
import ctypes
import os
import re

import numpy as np

from struspattern_amd import MatchBatch, build, capi

from .canonical_order import canonical_key, in_canonical_order, sorted_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {
    "sp_matcher_ctx_batch_finish_device_ex": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(capi.SpMatchFinishedBatch)]),
    "sp_matcher_ctx_last_finish_sort_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    "sp_matcher_finish_sort_tile": (ctypes.c_uint32, []),
}


def test_the_library_exports_the_canonical_finish():
    L = ctypes.CDLL(build.build())
    for name in SYMBOLS:
        assert getattr(L, name) is not None
    tile = L.sp_matcher_finish_sort_tile
    tile.restype, tile.argtypes = SYMBOLS["sp_matcher_finish_sort_tile"]
    assert tile() >= 64            # (a wave's worth at least: the smallest class of the sort)


def test_capi_declares_it_with_the_stated_types():
    for name, (res, args) in SYMBOLS.items():
        assert name in capi.SIGNATURES
        got_res, got_args = capi.SIGNATURES[name]
        assert got_res is res and got_args == args


def test_the_header_declares_it():
    with open(os.path.join(ROOT, "include", "strus_pattern_amd.h")) as f:
        header = f.read()
    assert re.search(r"^#define SP_FINISH_CANONICAL\s+1u\s*$", header, re.M)
    assert re.search(r"\bint sp_matcher_ctx_batch_finish_device_ex\(sp_matcher_ctx_t\* c, void\* stream, uint32_t flags, sp_match_finished_batch_t\* out\);", header)
    assert re.search(r"\bint sp_matcher_ctx_last_finish_sort_ms\(sp_matcher_ctx_t\* c, double\* sort_ms\);", header)
    assert re.search(r"\buint32_t sp_matcher_finish_sort_tile\(void\);", header)


def test_the_struct_is_still_eight_pointer_sized_fields():
    assert ctypes.sizeof(capi.SpMatchFinishedBatch) == 8 * ctypes.sizeof(ctypes.c_void_p)


def _hand_written():
    """two documents.  Document 0: results a, b, c tie in words 0..6 and 8 and differ in their items only (c's item is the
    smallest), d is a true duplicate of a, e lies before all of them by ordpos, f has the position of a and a smaller
    handle but a larger origpos (words 3..6 come before the handle).  Document 1: two results already in order."""
    #        handle ordpos ordend seg pos eseg end  ib ic
    a = [7, 5, 6, 0, 50, 0, 60, 0, 1]
    b = [7, 5, 6, 0, 50, 0, 60, 1, 1]
    c = [7, 5, 6, 0, 50, 0, 60, 2, 1]
    d = [7, 5, 6, 0, 50, 0, 60, 3, 1]
    e = [9, 2, 9, 0, 20, 0, 90, 4, 2]
    f = [1, 5, 6, 0, 51, 0, 60, 6, 0]
    g = [3, 1, 2, 0, 10, 0, 20, 6, 1]
    h = [3, 1, 3, 0, 10, 0, 30, 7, 0]
    results = np.array([a, b, c, d, e, f, g, h], np.uint32)
    items = np.array([
        [2, 5, 5, 0, 50, 0, 55],      # a
        [3, 5, 5, 0, 50, 0, 55],      # b: another variable
        [1, 5, 5, 0, 50, 0, 55],      # c
        [2, 5, 5, 0, 50, 0, 55],      # d = a
        [1, 2, 2, 0, 20, 0, 25], [2, 9, 9, 0, 85, 0, 90],      # e
        [4, 1, 1, 0, 10, 0, 15],      # g
    ], np.uint32)
    return MatchBatch(results, items, np.array([0, 6, 8], np.uint64), np.zeros((2, 4), np.uint64), np.zeros(2, np.int32))


def test_sorted_batch_on_a_hand_written_batch():
    batch = _hand_written()
    assert canonical_key(batch, 0) == (5, 6, 0, 50, 0, 60, 7, 1, 2, 5, 5, 0, 50, 0, 55)
    assert canonical_key(batch, 0) == canonical_key(batch, 3) != canonical_key(batch, 1)
    assert canonical_key(batch, 0)[:8] == canonical_key(batch, 1)[:8] == canonical_key(batch, 2)[:8]
    assert not in_canonical_order(batch, 0) and in_canonical_order(batch, 1)
    s = sorted_batch(batch)
    # e, then c (item variable 1), a and d (2, the same bytes), b (3), then f (origpos 51 although its handle is 1)
    want = np.array([
        [9, 2, 9, 0, 20, 0, 90, 0, 2],
        [7, 5, 6, 0, 50, 0, 60, 2, 1],
        [7, 5, 6, 0, 50, 0, 60, 3, 1],
        [7, 5, 6, 0, 50, 0, 60, 4, 1],
        [7, 5, 6, 0, 50, 0, 60, 5, 1],
        [1, 5, 6, 0, 51, 0, 60, 6, 0],
        [3, 1, 2, 0, 10, 0, 20, 6, 1],
        [3, 1, 3, 0, 10, 0, 30, 7, 0],
    ], np.uint32)
    assert np.array_equal(s.results, want)
    assert [int(v) for v in s.items[:, 0]] == [1, 2, 1, 2, 2, 3, 4]
    assert np.array_equal(s.items[0], batch.items[4]) and np.array_equal(s.items[1], batch.items[5])
    assert np.array_equal(s.doc_offsets, batch.doc_offsets)
    assert in_canonical_order(s, 0) and in_canonical_order(s, 1)
    again = sorted_batch(s)
    assert np.array_equal(again.results, s.results) and np.array_equal(again.items, s.items)


def test_sorted_batch_carries_the_format_words():
    batch = _hand_written()
    batch.result_format = np.array([0, 0, 0, 0, 5, 0, 0, 0], np.uint32)
    batch.item_format = np.array([[1, 0], [1, 0], [1, 0], [0, 0], [2, 1], [0, 0], [3, 0]], np.uint32)
    # a and d differ in item_format only now: d (0, 0) before a (1, 0)
    assert canonical_key(batch, 3) < canonical_key(batch, 0)
    s = sorted_batch(batch)
    assert [int(v) for v in s.result_format] == [5, 0, 0, 0, 0, 0, 0, 0]
    assert [[int(x) for x in v] for v in s.item_format] == [[2, 1], [0, 0], [1, 0], [0, 0], [1, 0], [1, 0], [3, 0]]
