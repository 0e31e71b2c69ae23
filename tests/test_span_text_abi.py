"""sp_match_batch_text (csrc/span_text.hpp), the device-free twin of the text passes: the C++ statement of the rule against
the numpy one (tests/span_text_model.py) over hand-made batches -- plain and segmented documents, empty and zero-length
spans, every validity condition violated in turn, the flags, and the arguments that are refused.  Needs no device."""
import ctypes

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from tests import span_text_model as model

SP_ERR_INVALID = -1


def make_batch(docs, failed=()):
    """docs: per document a list of results (span, [item spans]), span = (origseg, origpos, origendseg, origend) -> MatchBatch
    in the finished layout (document order, items without gaps in result order)"""
    results, items, offs = [], [], [0]
    for doc in docs:
        for k, (span, its) in enumerate(doc):
            results.append([7, k, k + 1, *span, len(items), len(its)])
            items += [[3, k, k + 1, *s] for s in its]
        offs.append(len(results))
    status = np.zeros(len(docs), np.int32)
    status[list(failed)] = 2
    return spa.MatchBatch(np.array(results, np.uint32).reshape(-1, 9), np.array(items, np.uint32).reshape(-1, 7),
                          np.array(offs, np.uint64), np.zeros((len(docs), 4), np.uint64), status)


def both(mb, text, so, dso=None, results=True, items=True):
    """(twin, model) of one batch"""
    flags = (model.SP_TEXT_RESULTS if results else 0) | (model.SP_TEXT_ITEMS if items else 0)
    got = spa.batchText(mb, text, so, dso, results=results, items=items)
    want = model.batch_text(mb.results, mb.items, mb.doc_offsets, text, np.asarray(so, np.uint64),
                            None if dso is None else np.asarray(dso, np.uint64), flags)
    return got, want


def assert_same(got, want):
    assert np.array_equal(got.status, want["status"])
    for fam in ("result", "item"):
        if want[fam + "_offsets"] is None:
            assert getattr(got, fam + "_text") is None and getattr(got, fam + "_offsets") is None
        else:
            assert np.array_equal(getattr(got, fam + "_offsets"), want[fam + "_offsets"])
            assert getattr(got, fam + "_text") == want[fam + "_text"]


def check(mb, text, so, dso=None, **kw):
    got, want = both(mb, text, so, dso, **kw)
    assert_same(got, want)
    return got


def test_symbols_and_signatures():
    for name in ("sp_matcher_ctx_finished_text_device", "sp_matcher_ctx_finished_text_fetch", "sp_matcher_ctx_last_text_ms",
                 "sp_match_text_free", "sp_match_batch_text", "sp_matcher_text_long_span"):
        assert name in capi.SIGNATURES and hasattr(capi.lib(), name)
    vp, P = ctypes.c_void_p, ctypes.POINTER
    assert capi.SIGNATURES["sp_matcher_ctx_finished_text_device"] == (ctypes.c_int, [vp, P(capi.SpTextSource), ctypes.c_uint32, vp, P(capi.SpMatchTextBatch)])
    assert [n for n, _ in capi.SpTextSource._fields_] == ["d_text", "nbytes", "d_seg_offsets", "nseg", "d_doc_seg_offsets"]
    assert [n for n, _ in capi.SpMatchTextBatch._fields_] == ["ndocs", "d_result_text", "d_result_text_offsets", "d_item_text", "d_item_text_offsets",
                                                              "d_doc_text_status", "d_totals"]
    assert capi.lib().sp_matcher_text_long_span() >= 1024


def test_plain_documents():
    text = b"the quick brown fox|jumps over|the lazy dog"
    so = [0, 19, 30, 43]
    docs = [
        [((0, 4, 0, 9), [(0, 4, 0, 9)]), ((0, 0, 0, 19), [(0, 0, 0, 3), (0, 16, 0, 19)])],
        [((0, 1, 0, 6), [])],
        [((0, 5, 0, 9), [(0, 9, 0, 13)]), ((0, 9, 0, 13), [(0, 9, 0, 12)])],     # the last span ends on the last byte of the text
    ]
    got = check(make_batch(docs), text, so)
    assert [got.result(i) for i in range(5)] == [b"quick", b"the quick brown fox", b"jumps", b"lazy", b" dog"]
    assert [got.item(i) for i in range(5)] == [b"quick", b"the", b"fox", b" dog", b" do"]
    assert not got.status.any()


def test_segmented_documents_cross_borders_and_empty_segments():
    pieces = [b"alpha beta", b"", b"gamma", b"delta eps", b"", b"", b"zeta", b"eta theta"]
    text = b"".join(pieces)
    so = np.concatenate([[0], np.cumsum([len(p) for p in pieces])])
    dso = [0, 3, 7, 7, 8]            # document 2 has no segments
    docs = [
        [((0, 6, 0, 10), [(0, 6, 0, 10)]),          # inside one segment
         ((0, 6, 2, 3), [(0, 6, 1, 0), (2, 0, 2, 3)]),  # over an empty segment: two borders
         ((1, 0, 1, 0), [])],                        # an empty span in an empty segment
        [((0, 6, 3, 2), [(0, 6, 1, 0), (1, 0, 2, 0), (3, 0, 3, 2)]),   # three borders, two of empty segments
         ((0, 9, 3, 0), [])],                        # from the end of a segment to the start of a later one: empty
        [],
        [((0, 0, 0, 9), [(0, 4, 0, 9)])],
    ]
    got = check(make_batch(docs), text, so, dso)
    assert [got.result(i) for i in range(6)] == [b"beta", b"betagam", b"", b"epsze", b"", b"eta theta"]
    assert [got.item(i) for i in range(7)] == [b"beta", b"beta", b"gam", b"eps", b"", b"ze", b"theta"]
    assert not got.status.any()


def test_zero_length_spans_and_no_documents():
    text = b"abcdef"
    docs = [[((0, k, 0, k), [(0, k, 0, k)]) for k in range(4)], [((0, 3, 0, 3), [])]]
    got = check(make_batch(docs), text, [0, 3, 6])
    assert got.result_text == b"" and not got.result_offsets.any() and len(got.result_offsets) == 6
    got = check(make_batch([]), text, [0], None)
    assert len(got.status) == 0 and got.result_text == b"" and list(got.result_offsets) == [0] and list(got.item_offsets) == [0]
    got = check(make_batch([]), b"", [0, 0, 0], [0])
    assert len(got.status) == 0


# every validity condition violated in turn by the middle document: (text, seg_offsets, doc_seg_offsets, span of the middle document)
_GOOD = dict(text=b"0123456789abcdefghijABCDEFGHIJ", so=[0, 10, 15, 20, 30], dso=[0, 1, 3, 4])
VIOLATIONS = {
    "valid":                    dict(span=(0, 2, 1, 3), status=0),
    "origseg > origendseg":     dict(span=(1, 0, 0, 3)),
    "origendseg outside":       dict(span=(0, 2, 2, 0)),
    "origpos > len(s0)":        dict(span=(0, 6, 1, 3)),
    "origend > len(s1)":        dict(span=(0, 2, 1, 6)),
    "begin > end":              dict(span=(0, 3, 0, 2)),
    "docSeg descends":          dict(span=(0, 0, 0, 0), dso=[0, 3, 1, 2], so=[0, 10, 20, 30, 30]),
    "docSeg beyond nseg":       dict(span=(0, 0, 0, 0), dso=[0, 1, 9, 4], docs3=True),
    "end > nbytes":             dict(span=(0, 0, 0, 15), so=[0, 10, 30, 10, 20], dso=[0, 1, 2, 4], text=b"0123456789abcdefghij", last=(1, 2, 1, 9)),
    "segOffsets descend":       dict(span=(0, 0, 0, 0), so=[0, 10, 5, 15], dso=[0, 1, 2, 3], text=b"0123456789abcde", last=(0, 1, 0, 9)),
    "segOffsets descend between": dict(span=(0, 1, 2, 1), so=[0, 10, 20, 15, 25, 30], dso=[0, 1, 4, 5], last=(0, 0, 0, 5)),
}


@pytest.mark.parametrize("name", list(VIOLATIONS))
def test_violation_in_the_middle_document(name):
    v = dict(_GOOD, **VIOLATIONS[name])
    first = [((0, 1, 0, 9), [(0, 1, 0, 4)]), ((0, 0, 0, 10), [])]
    last = [((*v.get("last", (0, 3, 0, 10)),), [(*v.get("last", (0, 3, 0, 10)),)])]
    middle = [((0, 0, 0, 1), [(0, 0, 0, 1)]), (v["span"], [(0, 1, 0, 2)]), ((0, 1, 0, 1), [])]
    docs = [first, middle, last]
    if v.get("docs3"):
        docs = [first, middle, [], last]             # (the document behind the bad range has no spans: dso = [0, 1, 9, 4, ...])
        v["dso"] = [0, 1, 9, 3, 4]
    got = check(make_batch(docs), v["text"], v["so"], v["dso"])
    want_status = v.get("status", model.SP_DOC_ERR_RANGE)
    assert list(got.status) == [0, want_status] + [0] * (len(docs) - 2)
    # the run without the middle document's spans: the others byte for byte, the failed document empty
    without = check(make_batch([first, []] + docs[2:]), v["text"], v["so"], v["dso"])
    if want_status:
        assert got.result_text == without.result_text and got.item_text == without.item_text
        assert np.array_equal(got.result_offsets[:3], without.result_offsets[:3])
        assert np.all(got.result_offsets[2:5] == got.result_offsets[2]) and np.all(got.item_offsets[1:3] == got.item_offsets[1])
        assert np.array_equal(got.result_offsets[5:], without.result_offsets[2:])
        assert np.array_equal(got.item_offsets[3:], without.item_offsets[1:])
    else:
        assert len(got.result_text) > len(without.result_text)
    assert got.result(0) == without.result(0) and got.result(len(got.result_offsets) - 2) == without.result(len(without.result_offsets) - 2)


def test_invalid_item_empties_the_document_only_when_items_are_asked_for():
    text, so = b"0123456789abcdefghij", [0, 10, 20]
    docs = [[((0, 0, 0, 4), [(0, 0, 0, 99)])], [((0, 1, 0, 5), [(0, 1, 0, 5)])]]
    mb = make_batch(docs)
    got = check(mb, text, so)
    assert list(got.status) == [5, 0] and got.result_text == b"bcde" and got.item_text == b"bcde"
    got = check(mb, text, so, items=False)
    assert list(got.status) == [0, 0] and got.result_text == b"0123bcde" and got.item_text is None and got.item_offsets is None
    got = check(mb, text, so, results=False)
    assert list(got.status) == [5, 0] and got.result_text is None and got.item_text == b"bcde"


def test_matcher_failed_document_has_no_spans_and_status_0():
    text, so = b"0123456789abcdefghij", [0, 10, 15, 20]
    docs = [[((0, 0, 0, 4), [])], [], [((0, 0, 0, 5), [(0, 1, 0, 2)])]]
    got = check(make_batch(docs, failed=[1]), text, so)
    assert list(got.status) == [0, 0, 0] and got.result_text == b"0123fghij" and got.item_text == b"g"


def test_refused_arguments():
    text, so = b"0123456789", [0, 5, 10]
    mb = make_batch([[((0, 0, 0, 4), [])]])
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        spa.batchText(mb, text, so)                       # nseg = 2, ndocs = 1, no doc_seg_offsets
    spa.batchText(mb, text, so, [0, 2])
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        spa.batchText(mb, text, so, [0, 2], results=False, items=False)
    L = capi.lib()
    b, t = capi.SpMatchBatch(), capi.SpMatchText()
    offs = (ctypes.c_uint64 * 1)(0)
    b.doc_result_offsets = offs
    err = ctypes.create_string_buffer(128)
    seg = (ctypes.c_uint64 * 1)(0)
    assert L.sp_match_batch_text(ctypes.byref(b), b"", 0, seg, 0, None, 4, ctypes.byref(t), err, 128) == SP_ERR_INVALID and err.value
    assert L.sp_match_batch_text(ctypes.byref(b), b"", 0, None, 0, None, 1, ctypes.byref(t), err, 128) == SP_ERR_INVALID
    assert L.sp_match_batch_text(ctypes.byref(b), b"", 0, seg, 0, None, 3, ctypes.byref(t), err, 128) == 0
    assert t.ndocs == 0 and t.totals[0] == 0 and t.result_text_offsets[0] == 0
    L.sp_match_text_free(ctypes.byref(t))
    assert not t.result_text_offsets
    # a batch whose item counts do not add up to its items is not a finished batch
    mb = make_batch([[((0, 0, 0, 4), [(0, 0, 0, 1)])]])
    mb.items = mb.items[:0]
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        spa.batchText(mb, text, so, [0, 2])


def test_random_batches_against_the_model():
    rng = np.random.default_rng(5)
    for _ in range(20):
        nseg = int(rng.integers(1, 12))
        lens = rng.integers(0, 9, nseg)
        so = np.concatenate([[0], np.cumsum(lens)])
        text = bytes(rng.integers(97, 123, int(so[-1]), dtype=np.uint8))
        cuts = np.sort(rng.integers(0, nseg + 1, int(rng.integers(0, 5))))
        dso = np.concatenate([[0], cuts, [nseg]])
        docs = []
        for d in range(len(dso) - 1):
            k = int(dso[d + 1] - dso[d])
            doc = []
            for _ in range(int(rng.integers(0, 6)) if k else 0):
                spans = []
                for _ in range(int(rng.integers(1, 4))):
                    s0 = int(rng.integers(0, k))
                    s1 = int(rng.integers(s0, k))
                    slack = 1 if rng.random() < 0.05 else 0      # now and then one byte too far
                    spans.append((s0, int(rng.integers(0, lens[dso[d] + s0] + 1 + slack)), s1, int(rng.integers(0, lens[dso[d] + s1] + 1 + slack))))
                doc.append((spans[0], spans[1:]))
            docs.append(doc)
        check(make_batch(docs), text, so, dso)
