"""The C-ABI of the device finish (include/strus_pattern_amd.h: sp_matcher_ctx_batch_finish_device,
sp_matcher_ctx_finished_fetch) as the built library exports it and as struspattern_amd/capi.py declares it.  No GPU."""
import ctypes
import os
import re

from struspattern_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sp_matcher_ctx_batch_finish_device", "sp_matcher_ctx_finished_fetch", "sp_matcher_ctx_last_finish_ms"]


def test_the_library_exports_the_finish_entry_points():
    path = build.build()
    L = ctypes.CDLL(path)
    for name in SYMBOLS:
        assert getattr(L, name) is not None


def test_capi_declares_them():
    for name in SYMBOLS:
        assert name in capi.SIGNATURES
    res, args = capi.SIGNATURES["sp_matcher_ctx_batch_finish_device"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(capi.SpMatchFinishedBatch)]
    res, args = capi.SIGNATURES["sp_matcher_ctx_finished_fetch"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.POINTER(capi.SpMatchBatch)]


def test_the_struct_is_eight_pointer_sized_fields():
    assert ctypes.sizeof(capi.SpMatchFinishedBatch) == 8 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in capi.SpMatchFinishedBatch._fields_] == [
        "ndocs", "d_results", "d_items", "d_doc_result_offsets", "d_doc_item_offsets", "d_result_format", "d_item_format", "d_totals"]


def test_the_header_declares_what_capi_declares():
    with open(os.path.join(ROOT, "include", "strus_pattern_amd.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header)
    body = re.search(r"typedef struct sp_match_finished_batch \{(.*?)\} sp_match_finished_batch_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+);", body)
    assert fields == [n for n, _ in capi.SpMatchFinishedBatch._fields_]
    # the raw device batch says what it is: (first, count) pairs in completion order
    raw = re.search(r"typedef struct sp_match_device_batch \{(.*?)\} sp_match_device_batch_t;", header, re.S).group(1)
    assert "uint64_t[ndocs][2]" in raw and "COMPLETION order" in raw and "sp_..._finish" not in raw
