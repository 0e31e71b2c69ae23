"""The C-ABI of the segment stitch (include/strus_pattern_amd.h: sp_lexer_ctx_stitch_segments_device,
sp_lexer_ctx_stitched_fetch, sp_lexer_ctx_last_stitch_ms) as the built library exports it and as struspattern_amd/capi.py
declares it.  No GPU."""
import ctypes
import os
import re

from struspattern_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sp_lexer_ctx_stitch_segments_device", "sp_lexer_ctx_stitched_fetch", "sp_lexer_ctx_last_stitch_ms", "sp_lexer_ctx_stitched_status"]
FIELDS = ["ndocs", "d_lexems", "d_origseg", "d_doc_offsets", "d_doc_status", "d_totals"]


def test_the_library_exports_the_stitch_entry_points():
    path = build.build()
    L = ctypes.CDLL(path)
    for name in SYMBOLS:
        assert getattr(L, name) is not None


def test_capi_declares_them():
    for name in SYMBOLS:
        assert name in capi.SIGNATURES
    vp, P = ctypes.c_void_p, ctypes.POINTER
    assert capi.SIGNATURES["sp_lexer_ctx_stitch_segments_device"] == (ctypes.c_int, [vp, vp, ctypes.c_size_t, vp, P(capi.SpLexStitchedBatch)])
    assert capi.SIGNATURES["sp_lexer_ctx_stitched_fetch"] == (ctypes.c_int, [vp, P(capi.SpLexBatch), P(P(ctypes.c_uint32))])
    assert capi.SIGNATURES["sp_lexer_ctx_last_stitch_ms"] == (ctypes.c_int, [vp, P(ctypes.c_double)])
    assert capi.SIGNATURES["sp_lexer_ctx_stitched_status"] == (ctypes.c_int, [vp, vp, ctypes.c_size_t, P(ctypes.c_size_t)])


def test_the_struct_is_six_pointer_sized_fields():
    assert ctypes.sizeof(capi.SpLexStitchedBatch) == 6 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in capi.SpLexStitchedBatch._fields_] == FIELDS


def test_the_header_declares_what_capi_declares():
    with open(os.path.join(ROOT, "include", "strus_pattern_amd.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header)
    body = re.search(r"typedef struct sp_lex_stitched_batch \{(.*?)\} sp_lex_stitched_batch_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == FIELDS
    # the header says how the stitched batch feeds the matcher, what a failed document looks like there, and what the rule rests on
    assert "sp_matcher_ctx_match_docs_device(mctx, out.d_lexems, out.d_origseg, out.d_doc_offsets, ndocs, nlexems" in header
    assert "reaches the matcher as an empty document" in header and "unpinned by" in header
    # the segment index no longer "always 0 out of the lexer" without saying where it comes from
    assert "sp_lexer_ctx_stitch_segments_device" in re.search(r"/\* analyzer::PatternLexem\(.*?\*/", header, re.S).group(0)
