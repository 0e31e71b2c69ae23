"""Index terms without a device (sp_match_batch_terms, csrc/match_terms.hpp): the twin equals the model (tests/terms_model.py)
on hand-made batches, field by field and byte for byte; every error return of the header; the range rule; and the invariant
that ties the terms of a handle to the handle's pattern frequency record."""
import ctypes

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from tests import terms_model as model
from tests.finished_support import _batch, _family

V, T = spa.SP_TERM_VALUES, spa.SP_TERM_TEXT


def _check(mb, bound, flags, mv=None, mt=None):
    got = spa.batchTerms(mb, values=mv, text=mt, handle_bound=bound, flags=flags)
    want = model.of_batch(mb, bound, flags, mv, mt)
    model.assert_same(got, want)
    return got


DOCS = [
    [(3, 1, 2), (1, 2, 3), (3, 3, 5), (3, 9, 10), (1, 4, 5), (2, 0, 1)],
    [],
    [(2, 7, 8)],
    [(1, 5, 6), (1, 1, 9), (1, 3, 4)],
]
TEXT = [b"eur", b"x", b"usd", b"eur", b"x", b"x", b"", b"ab", b"abc", b"ab"]
VALUES = [b"EUR", b"", b"EUR", b"EUR", b"", b"q", b"v", b"", b"", b""]
FORMATS = [1, 0, 1, 2, 0, 3, 1, 0, 0, 0]


def test_symbols_and_signatures():
    vp, u32, P = ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER
    for name in ("sp_matcher_ctx_finished_terms_device", "sp_matcher_ctx_finished_terms_fetch", "sp_match_terms_free",
                 "sp_matcher_ctx_last_terms_ms", "sp_matcher_term_tile", "sp_test_term_hash_bits", "sp_match_batch_terms"):
        assert name in capi.SIGNATURES and hasattr(capi.lib(), name)
    assert capi.SIGNATURES["sp_matcher_ctx_finished_terms_device"] == (ctypes.c_int, [vp, u32, vp, P(capi.SpMatchTermsDevice)])
    assert ctypes.sizeof(capi.SpMatchTerm) == 24
    assert capi.lib().sp_matcher_term_tile() >= 64


@pytest.mark.parametrize("flags", [V, T, V | T])
def test_three_flag_combinations_equal_the_model(flags):
    mb = _batch(DOCS, FORMATS)
    mv, mt = _family(spa.MatchValues, VALUES, 4), _family(spa.MatchText, TEXT, 4)
    got = _check(mb, 4, flags, mv, mt)
    assert not got.status.any()
    if flags == T:
        # document 0: (1,"x") twice, (2,"x") -- the same bytes under another handle --, (3,"eur") twice, (3,"usd")
        assert got.doc(0).tolist() == [[1, 2, 2, 5, 1, 1], [2, 1, 0, 1, 5, 1], [3, 2, 1, 10, 0, 3], [3, 1, 3, 5, 2, 3]]
        assert got.result_term[:6].tolist() == [2, 0, 3, 2, 0, 1]
        assert got.doc(3).tolist() == [[1, 2, 3, 6, 0, 2], [1, 1, 1, 9, 1, 3]]      # "ab" is a prefix of "abc"; an empty text in document 2
        assert got.doc(2).tolist() == [[2, 1, 7, 8, 0, 0]]
    if flags == V:
        assert got.doc(0).tolist() == [[1, 2, 2, 5, 1, 0], [2, 1, 0, 1, 5, 1], [3, 3, 1, 10, 0, 3]]
    if flags == V | T:
        # a formatted result takes its value, also an empty one; an unformatted one its text
        assert got.doc(0).tolist() == [[1, 2, 2, 5, 1, 1], [2, 1, 0, 1, 5, 1], [3, 3, 1, 10, 0, 3]]
        assert got.doc(2).tolist() == [[2, 1, 7, 8, 0, 1]]
    # both flags without format arrays: the text
    if flags == V | T:
        model.assert_same(_check(_batch(DOCS), 4, flags, mv, mt), _check(_batch(DOCS), 4, T, None, mt))
    # the helper
    terms = list(got.terms(3, mb, mv, mt))
    assert [t[1] for t in terms] == {V: [b""], T: [b"ab", b"abc"], V | T: [b"ab", b"abc"]}[flags]


def test_first_result_is_not_the_least_ordpos_and_empty_is_a_value():
    docs = [[(1, 9, 10), (1, 5, 6), (1, 2, 30), (1, 7, 8)]]
    mt = _family(spa.MatchText, [b"b", b"", b"b", b""], 1)
    got = _check(_batch(docs), 2, T, None, mt)
    assert got.records.tolist() == [[1, 2, 2, 30, 0, 1], [1, 2, 5, 8, 1, 0]] and got.result_term.tolist() == [0, 1, 0, 1]


def test_range_rule():
    docs = [[(1, 1, 2)], [(1, 1, 2), (2, 3, 4)], [(2, 1, 2)]]
    strings = [b"a", b"b", b"c", b"d"]
    mt = _family(spa.MatchText, strings, 3)
    # a handle equal to the bound
    got = _check(_batch(docs), 2, T, None, mt)
    assert got.status.tolist() == [0, 5, 5] and got.doc_offsets.tolist() == [0, 1, 1, 1]
    assert got.result_term.tolist() == [0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]
    # handle 0
    zero = [[(1, 1, 2)], [(0, 1, 2), (2, 3, 4)], [(2, 1, 2)]]
    got = _check(_batch(zero), 3, T, None, mt)
    assert got.status.tolist() == [0, 5, 0] and got.result_term.tolist() == [0, 0xFFFFFFFF, 0xFFFFFFFF, 0]
    # a source status on one document between two good ones: only a selected source counts
    bad_text = _family(spa.MatchText, strings, 3, status=[0, 5, 0])
    mv = _family(spa.MatchValues, strings, 3)
    got = _check(_batch(docs, [1, 1, 1, 1]), 3, V | T, mv, bad_text)
    assert got.status.tolist() == [0, 5, 0] and got.doc_offsets.tolist() == [0, 1, 1, 2]
    got = _check(_batch(docs, [1, 1, 1, 1]), 3, V, mv, bad_text)
    assert got.status.tolist() == [0, 0, 0] and len(got.records) == 4
    bad_values = _family(spa.MatchValues, strings, 3, status=[0, 5, 0])
    assert _check(_batch(docs), 3, V, bad_values, None).status.tolist() == [0, 5, 0]
    # a document the matcher failed: no records, status 0
    got = _check(_batch(docs, status=[0, 1, 0]), 3, T, None, mt)
    assert got.status.tolist() == [0, 0, 0] and got.doc_offsets.tolist() == [0, 1, 1, 2]


def test_frequency_invariant():
    rng = np.random.default_rng(7)
    docs, strings = [], []
    for d in range(6):
        n = int(rng.integers(0, 120))
        docs.append([(int(rng.integers(1, 9)), int(rng.integers(0, 1000)), int(rng.integers(0, 1000))) for _ in range(n)])
        strings += [bytes(rng.integers(97, 100, int(rng.integers(0, 3))).astype(np.uint8)) for _ in range(n)]
    mb = _batch(docs)
    mt = _family(spa.MatchText, strings, 6)
    got = _check(mb, 9, T, None, mt)
    freq = spa.batchPatternFreq(mb, 9)
    assert len(got.records) > len(freq.records) > 0
    for d in range(6):
        terms, want = got.doc(d), freq.doc(d)
        handles = terms[:, 0]
        assert np.all(np.diff(handles.astype(np.int64)) >= 0)                      # the terms of a handle are contiguous
        assert sorted(set(handles.tolist())) == want[:, 0].tolist()
        for h, count, first, last in want.tolist():
            mine = terms[handles == h]
            assert int(mine[:, 1].sum()) == count and int(mine[:, 2].min()) == first and int(mine[:, 3].max()) == last
            assert np.all(np.diff(mine[:, 4].astype(np.int64)) > 0)                # ascending by first_result inside a handle


def _raw(mb, mv, mt, bound, flags, break_=None):
    """sp_match_batch_terms over hand-filled C structs; break_( b, v, x) may damage them.  Returns (rc, message)."""
    L = capi.lib()
    res = np.array(mb.results, np.uint32)
    offs = np.array(mb.doc_offsets, np.uint64)          # (copies: break_ writes into them)
    b = capi.SpMatchBatch()
    b.ndocs, b.nresults = len(offs) - 1, len(res)
    b.results = ctypes.cast(res.ctypes.data, ctypes.POINTER(capi.SpResult))
    b.doc_result_offsets = ctypes.cast(offs.ctypes.data, ctypes.POINTER(ctypes.c_uint64))
    keep = []

    def fill(c, data, family_offsets, status, names):
        ro, st = np.array(family_offsets, np.uint64), np.array(status, np.int32)
        buf = ctypes.create_string_buffer(bytes(data), len(data) + 1)
        keep.extend([ro, st, buf])
        c.ndocs, c.nresults = len(st), len(ro) - 1
        setattr(c, names[0], ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint8)))
        setattr(c, names[1], ctypes.cast(ro.ctypes.data, ctypes.POINTER(ctypes.c_uint64)))
        setattr(c, names[2], ctypes.cast(st.ctypes.data, ctypes.POINTER(ctypes.c_int32)))
        c.totals[0] = len(data)
        return c
    v = fill(capi.SpMatchValues(), mv.result_values, mv.result_offsets, mv.status, ("result_values", "result_value_offsets", "doc_value_status")) if mv else None
    x = fill(capi.SpMatchText(), mt.result_text, mt.result_offsets, mt.status, ("result_text", "result_text_offsets", "doc_text_status")) if mt else None
    if break_:
        break_(b, v, x, keep)
    t = capi.SpMatchTerms()
    err = ctypes.create_string_buffer(256)
    rc = L.sp_match_batch_terms(ctypes.byref(b), ctypes.byref(v) if v else None, ctypes.byref(x) if x else None, bound, flags, ctypes.byref(t), err, 256)
    if rc == 0:
        L.sp_match_terms_free(ctypes.byref(t))
    else:
        assert not t.records and not t.result_term and not t.doc_term_offsets
    return rc, err.value.decode()


def test_error_returns():
    mb = _batch(DOCS, FORMATS)
    mv, mt = _family(spa.MatchValues, VALUES, 4), _family(spa.MatchText, TEXT, 4)
    assert _raw(mb, mv, mt, 4, V | T)[0] == 0
    # flags 0 or unknown bits
    for flags in (0, 4, V | 8):
        rc, msg = _raw(mb, mv, mt, 4, flags)
        assert rc == -1 and "flags" in msg
    # a NULL source that the flags select, and one without its results family
    assert _raw(mb, None, mt, 4, V)[0] == -1 and _raw(mb, mv, None, 4, T)[0] == -1 and _raw(mb, None, mt, 4, V | T)[0] == -1
    assert _raw(mb, None, mt, 4, T)[0] == 0 and _raw(mb, mv, None, 4, V)[0] == 0

    def no_family(b, v, x, keep):
        x.result_text_offsets = None
    assert _raw(mb, mv, mt, 4, T, no_family)[0] == -1
    # sizes that do not agree with the batch
    short_text = _family(spa.MatchText, TEXT[:-1], 4)
    assert _raw(mb, mv, short_text, 4, T)[0] == -1
    assert _raw(mb, mv, _family(spa.MatchText, TEXT, 3), 4, T)[0] == -1
    assert _raw(mb, _family(spa.MatchValues, VALUES + [b""], 4), mt, 4, V)[0] == -1
    # a bound of 0
    rc, msg = _raw(mb, mv, mt, 0, T)
    assert rc == -1 and "bound" in msg

    # offsets that do not ascend or do not cover
    def descending(b, v, x, keep):
        x.result_text_offsets[3], x.result_text_offsets[4] = x.result_text_offsets[4], x.result_text_offsets[3] + 100
    assert _raw(mb, mv, mt, 4, T, descending)[0] == -1

    def uncovered(b, v, x, keep):
        x.totals[0] += 1
    assert _raw(mb, mv, mt, 4, T, uncovered)[0] == -1
    assert _raw(mb, mv, mt, 4, V, uncovered)[0] == 0                              # (the text is not selected)

    def doc_offsets_descend(b, v, x, keep):
        b.doc_result_offsets[1], b.doc_result_offsets[2] = 7, 6
    assert _raw(mb, mv, mt, 4, T, doc_offsets_descend)[0] == -1

    def doc_offsets_short(b, v, x, keep):
        b.doc_result_offsets[4] = 9
    assert _raw(mb, mv, mt, 4, T, doc_offsets_short)[0] == -1
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        spa.batchTerms(mb, values=None, text=mt, handle_bound=4, flags=V)
