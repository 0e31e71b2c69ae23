"""Batch dictionary without a device (sp_match_batch_dictionary, csrc/match_dict.hpp): the twin equals the model
(tests/dictionary_model.py) on hand-made batches, with every expected entry written out by hand; every error return of the
header; and the invariants that tie the dictionary to its terms and to the pattern frequencies of the batch."""
import ctypes

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from tests import dictionary_model as model
from tests.finished_support import (_batch, DICT_BOUND as BOUND, DICT_DOCS as DOCS, DICT_EXPECTED as EXPECTED, DICT_FORMATS as FORMATS,
                                    _dict_inputs as _inputs, DICT_TEXT as TEXT, _family)

V, T = spa.SP_TERM_VALUES, spa.SP_TERM_TEXT


def _entries(d):
    """the entries as [handle, value_bytes, first_doc, first_term, doc_freq, max_count, count]"""
    return [row[:6] + [count] for row, count in zip(d.records.tolist(), d.counts.tolist())]


def _check(mb, terms, mv=None, mt=None):
    got = spa.batchDictionary(mb, terms, values=mv, text=mt)
    want = model.of_batch(mb, terms, terms.handle_bound, mv, mt)
    model.assert_same(got, want)
    model.check_invariants(got, terms, mb)
    return got


def test_symbols_and_signatures():
    vp, P = ctypes.c_void_p, ctypes.POINTER
    for name in ("sp_matcher_ctx_finished_dictionary_device", "sp_matcher_ctx_finished_dictionary_fetch", "sp_match_dictionary_free",
                 "sp_matcher_ctx_last_dictionary_ms", "sp_match_batch_dictionary"):
        assert name in capi.SIGNATURES and hasattr(capi.lib(), name)
    assert capi.SIGNATURES["sp_matcher_ctx_finished_dictionary_device"] == (ctypes.c_int, [vp, vp, P(capi.SpMatchDictionaryDevice)])
    assert capi.SIGNATURES["sp_match_batch_dictionary"][1][:5] == [P(capi.SpMatchBatch), P(capi.SpMatchValues), P(capi.SpMatchText), P(capi.SpMatchTerms), P(capi.SpMatchDictionary)]
    assert ctypes.sizeof(capi.SpDictTerm) == 32 and capi.SpDictTerm.count.offset == 24
    for name in ("finishedDictionaryDevice", "finishedDictionaryFetch", "lastDictionaryMs"):
        assert hasattr(spa.PatternMatcherContext, name)


@pytest.mark.parametrize("flags", [V, T, V | T])
def test_three_flag_combinations_equal_the_model_and_the_entries_written_out(flags):
    mb, mv, mt, terms = _inputs(flags)
    assert terms.handle_bound == BOUND and not terms.status.any()
    got = _check(mb, terms, mv, mt)
    entries, term_dict, doc_offsets, handle_terms = EXPECTED[flags]
    assert _entries(got) == entries
    assert got.records[:, 7].tolist() == [0] * len(entries)
    assert got.term_dict.tolist() == term_dict and got.doc_offsets.tolist() == doc_offsets and got.handle_terms.tolist() == handle_terms
    assert got.counts.dtype == np.uint64 and int(got.counts.sum()) == len(TEXT)
    # the helper: the bytes of an entry are those of its first record
    listed = [(h, v) for h, v, _, _, _ in got.entries(mb, terms, values=mv, text=mt)]
    want = {T: [(1, b"eur"), (1, b"ab"), (2, b"x"), (3, b""), (1, b"abc"), (2, b"eur")],
            V: [(1, b"EUR"), (1, b""), (2, b""), (3, b""), (1, b"eur"), (2, b"x")],
            V | T: [(1, b"EUR"), (1, b"ab"), (2, b"x"), (3, b""), (1, b"eur"), (2, b"eur")]}[flags]
    assert listed == want
    assert [(df, c, mx) for _, _, df, c, mx in got.entries(mb, terms, values=mv, text=mt)] == [(e[4], e[6], e[5]) for e in entries]


def test_a_document_with_a_term_status_between_two_good_ones_contributes_nothing():
    mb, mv, mt, terms = _inputs(T, text_status=[0, 5, 0, 0])
    assert terms.status.tolist() == [0, 5, 0, 0] and terms.doc_offsets.tolist() == [0, 4, 4, 6, 8]
    got = _check(mb, terms, None, mt)
    # without document 1 nothing is first seen behind document 0: the entries of "abc" and of "eur" under handle 2 are gone
    assert _entries(got) == [[1, 3, 0, 0, 3, 3, 6], [1, 2, 0, 1, 1, 1, 1], [2, 1, 0, 2, 2, 1, 2], [3, 0, 0, 3, 2, 1, 2]]
    assert got.doc_offsets.tolist() == [0, 4, 4, 4, 4] and got.term_dict.tolist() == [0, 1, 2, 3, 0, 3, 0, 2]
    assert int(got.counts.sum()) == len(TEXT) - 2
    # a failing document in front: the entries first seen behind it follow directly, from 0
    mb, mv, mt, terms = _inputs(T, text_status=[5, 0, 0, 0])
    got = _check(mb, terms, None, mt)
    assert got.doc_offsets.tolist() == [0, 0, 2, 4, 5]
    assert _entries(got) == [[1, 3, 1, 0, 1, 1, 1], [2, 3, 1, 1, 1, 1, 1], [1, 3, 2, 0, 2, 3, 4], [3, 0, 2, 1, 1, 1, 1], [2, 1, 3, 1, 1, 1, 1]]
    # a document the matcher failed has no records either
    mb = _batch(DOCS, FORMATS, status=[0, 0, 1, 0])
    mt = _family(spa.MatchText, TEXT, 4)
    terms = spa.batchTerms(mb, text=mt, handle_bound=BOUND, flags=T)
    got = _check(mb, terms, None, mt)
    assert got.doc_offsets.tolist() == [0, 4, 6, 6, 6] and got.records[0].tolist() == [1, 3, 0, 0, 2, 2, 3, 0]


def test_handle_bound_of_hand_made_terms_is_not_guessed():
    mb, mv, mt, terms = _inputs(T)
    by_hand = spa.MatchTerms(terms.records, terms.doc_offsets, terms.result_term, terms.status, T)
    with pytest.raises(spa.PatternError, match="handle bound"):
        spa.batchDictionary(mb, by_hand, text=mt)
    got = spa.batchDictionary(mb, by_hand, text=mt, handle_bound=7)
    assert got.handle_terms.tolist() == [0, 3, 2, 1, 0, 0, 0] and _entries(got) == EXPECTED[T][0]


def test_no_documents_and_no_records():
    mb = _batch([])
    mt = _family(spa.MatchText, [], 0)
    terms = spa.batchTerms(mb, text=mt, handle_bound=3, flags=T)
    got = _check(mb, terms, None, mt)
    assert len(got.records) == 0 and got.doc_offsets.tolist() == [0] and got.handle_terms.tolist() == [0, 0, 0] and len(got.term_dict) == 0
    mb = _batch([[], []])
    mt = _family(spa.MatchText, [], 2)
    got = _check(mb, spa.batchTerms(mb, text=mt, handle_bound=3, flags=T), None, mt)
    assert len(got.records) == 0 and got.doc_offsets.tolist() == [0, 0, 0]


def test_invariants_against_the_pattern_frequencies():
    rng = np.random.default_rng(11)
    docs, strings = [], []
    for d in range(6):
        n = int(rng.integers(1, 121))
        docs.append([(int(rng.integers(1, 9)), int(rng.integers(0, 1000)), int(rng.integers(0, 1000))) for _ in range(n)])
        strings += [bytes(rng.integers(97, 100, int(rng.integers(0, 3))).astype(np.uint8)) for _ in range(n)]
    mb = _batch(docs)
    mt = _family(spa.MatchText, strings, 6)
    terms = spa.batchTerms(mb, text=mt, handle_bound=9, flags=T)
    got = _check(mb, terms, None, mt)
    freq = spa.batchPatternFreq(mb, 9)
    assert not terms.status.any() and not freq.status.any()
    n, ndict = len(terms.records), len(got.records)
    assert 0 < ndict < n < len(mb.results)                                       # terms repeat across the documents
    assert int(got.records[:, 4].sum()) == n and int(got.counts.sum()) == len(mb.results)
    assert int(got.handle_terms.sum()) == ndict and int(got.term_dict.max()) < ndict
    for h in range(9):
        mine = got.records[:, 0] == h
        assert int(got.counts[mine].sum()) == int(freq.handle_results[h]) and int(mine.sum()) == int(got.handle_terms[h])
    assert int(got.records[:, 4].max()) > 1 and np.all(got.records[:, 5] <= got.counts) and np.all(got.records[:, 4] <= 6)
    # inside the range of a document the entries ascend by handle
    for d in range(6):
        handles = got.records[int(got.doc_offsets[d]):int(got.doc_offsets[d + 1]), 0].astype(np.int64)
        assert np.all(np.diff(handles) >= 0)


def _raw(mb, mv, mt, terms, break_=None, null=()):
    """sp_match_batch_dictionary over hand-filled C structs; break_( b, v, x, t) may damage them, `null` names the arguments
    passed as NULL.  Returns (rc, message)."""
    L = capi.lib()
    res = np.array(mb.results, np.uint32)
    offs = np.array(mb.doc_offsets, np.uint64)          # (copies: break_ writes into them)
    rf = np.array(mb.result_format, np.uint32)
    b = capi.SpMatchBatch()
    b.ndocs, b.nresults = len(offs) - 1, len(res)
    b.results = ctypes.cast(res.ctypes.data, ctypes.POINTER(capi.SpResult))
    b.doc_result_offsets = ctypes.cast(offs.ctypes.data, ctypes.POINTER(ctypes.c_uint64))
    b.result_format = ctypes.cast(rf.ctypes.data, ctypes.POINTER(ctypes.c_uint32))
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
    v = fill(capi.SpMatchValues(), mv.result_values, mv.result_offsets, mv.status, ("result_values", "result_value_offsets", "doc_value_status"))
    x = fill(capi.SpMatchText(), mt.result_text, mt.result_offsets, mt.status, ("result_text", "result_text_offsets", "doc_text_status"))
    rec, toffs = np.array(terms.records, np.uint32), np.array(terms.doc_offsets, np.uint64)
    rt, st = np.array(terms.result_term, np.uint32), np.array(terms.status, np.int32)
    t = capi.SpMatchTerms()
    t.ndocs, t.nresults, t.nrecords, t.handle_bound, t.flags = len(toffs) - 1, len(rt), len(rec), terms.handle_bound, terms.flags
    t.records = ctypes.cast(rec.ctypes.data, ctypes.POINTER(capi.SpMatchTerm))
    t.doc_term_offsets = ctypes.cast(toffs.ctypes.data, ctypes.POINTER(ctypes.c_uint64))
    t.result_term = ctypes.cast(rt.ctypes.data, ctypes.POINTER(ctypes.c_uint32))
    t.doc_term_status = ctypes.cast(st.ctypes.data, ctypes.POINTER(ctypes.c_int32))
    t.totals[0] = len(rec)
    if break_:
        break_(b, v, x, t)
    args = {"mb": b, "values": v, "text": x, "terms": t}
    d = capi.SpMatchDictionary()
    d.ndict = 77                                        # (the call clears `out` first)
    err = ctypes.create_string_buffer(256)
    rc = L.sp_match_batch_dictionary(*[None if k in null else ctypes.byref(a) for k, a in args.items()], ctypes.byref(d), err, 256)
    if rc == 0:
        assert d.ndict == len(EXPECTED[terms.flags][0]) and d.nterms == len(rec) and d.totals[0] == d.ndict
        L.sp_match_dictionary_free(ctypes.byref(d))
    else:
        assert not d.records and not d.term_dict and not d.doc_dict_offsets and not d.handle_terms and d.ndict == 0 and d.totals[0] == 0
    return rc, err.value.decode()


def test_error_returns():
    mb, mv, mt, both = _inputs(V | T)
    text_terms, value_terms = _inputs(T)[3], _inputs(V)[3]
    assert _raw(mb, mv, mt, both) == (0, "") and _raw(mb, mv, mt, text_terms)[0] == 0 and _raw(mb, mv, mt, value_terms)[0] == 0
    # a NULL argument that the flags select; one they do not select may be NULL
    assert _raw(mb, mv, mt, both, null=("mb",))[0] == -1 and _raw(mb, mv, mt, both, null=("terms",))[0] == -1
    rc, msg = _raw(mb, mv, mt, both, null=("values",))
    assert rc == -1 and "values" in msg
    rc, msg = _raw(mb, mv, mt, both, null=("text",))
    assert rc == -1 and "text" in msg
    assert _raw(mb, mv, mt, text_terms, null=("text",))[0] == -1 and _raw(mb, mv, mt, value_terms, null=("values",))[0] == -1
    assert _raw(mb, mv, mt, text_terms, null=("values",))[0] == 0 and _raw(mb, mv, mt, value_terms, null=("text",))[0] == 0

    # a source without its results family
    def no_text_family(b, v, x, t):
        x.result_text_offsets = None

    def no_values_family(b, v, x, t):
        v.result_value_offsets = None
    assert _raw(mb, mv, mt, both, no_text_family)[0] == -1 and _raw(mb, mv, mt, both, no_values_family)[0] == -1
    assert _raw(mb, mv, mt, value_terms, no_text_family)[0] == 0

    # ndocs or nresults that do not agree between the batch, the sources and the terms
    def count(which, field, by):
        def damage(b, v, x, t):
            target = {"b": b, "v": v, "x": x, "t": t}[which]
            setattr(target, field, getattr(target, field) + by)
        return damage
    for which in "vxt":
        for field in ("ndocs", "nresults"):
            rc, msg = _raw(mb, mv, mt, both, count(which, field, -1))
            assert rc == -1 and "counts" in msg, (which, field)
    assert _raw(mb, mv, mt, text_terms, count("v", "nresults", 1))[0] == 0        # (the values are not selected)

    # term offsets that do not ascend or do not cover nrecords
    def descending(b, v, x, t):
        t.doc_term_offsets[1], t.doc_term_offsets[2] = 6, 4

    def uncovered(b, v, x, t):
        t.doc_term_offsets[4] -= 1

    def beyond(b, v, x, t):
        t.doc_term_offsets[4] += 1

    def late_start(b, v, x, t):
        t.doc_term_offsets[0] = 1
    for damage in (descending, uncovered, beyond, late_start, count("t", "nrecords", -1)):
        rc, msg = _raw(mb, mv, mt, both, damage)
        assert rc == -1 and "offsets" in msg, damage.__name__

    # a first_result outside its document: document 1 has two results
    def first_result_outside(b, v, x, t):
        t.records[4].first_result = 2
    rc, msg = _raw(mb, mv, mt, both, first_result_outside)
    assert rc == -1 and "first_result" in msg

    # a value_bytes that is not the length of its range
    def wrong_length(b, v, x, t):
        t.records[1].value_bytes += 1
    rc, msg = _raw(mb, mv, mt, both, wrong_length)
    assert rc == -1 and "value_bytes" in msg

    # the message is cut to the buffer; the Python call raises
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        spa.batchDictionary(mb, both, values=None, text=mt)
