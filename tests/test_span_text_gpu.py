"""Matched text on the device (sp_matcher_ctx_finished_text_device, csrc/l2_text.h): the bytes, offsets and status that the
text passes leave must EQUAL what the device-free twin (sp_match_batch_text) makes of the fetched finished batch, and
for valid spans the plain slices of the source.  The chosen spans come from hand-made lexems (and a hand-made origseg)
through a two-term rule, so that a test sets every span itself: the result of the pair (a, b) covers a's begin to b's
end, its items are a and b."""
import ctypes
import json
import os

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi, rulelang, segments
from tests import span_text_model as model
from tests.finished_support import _ctx, _from_device, _pairs, _random_text, Run, Source, _stream, _torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _assert_text(ctx, src, out=None, results=True, items=True):
    """the fetched text batch equals the twin's and the model's on the fetched finished batch; returns (batch, text)"""
    mb = ctx.finishedFetch()
    got = ctx.finishedTextFetch()
    twin = spa.batchText(mb, src.text, src.so, src.dso, results=results, items=items)
    flags = (model.SP_TEXT_RESULTS if results else 0) | (model.SP_TEXT_ITEMS if items else 0)
    want = model.batch_text(mb.results, mb.items, mb.doc_offsets, src.text, src.so, src.dso, flags)
    assert np.array_equal(got.status, twin.status) and np.array_equal(got.status, want["status"])
    for fam in ("result", "item"):
        g_text, g_offs = getattr(got, fam + "_text"), getattr(got, fam + "_offsets")
        if want[fam + "_offsets"] is None:
            assert g_text is None and g_offs is None and getattr(twin, fam + "_text") is None
            continue
        assert np.array_equal(g_offs, getattr(twin, fam + "_offsets")) and np.array_equal(g_offs, want[fam + "_offsets"])
        assert g_text == getattr(twin, fam + "_text")
        assert g_text == want[fam + "_text"]                   # (the plain slices of the source, for the valid spans)
        assert b"\xff" not in g_text
    if out is not None:
        # the device arrays themselves
        totals = _from_device(out.d_totals, 2, np.uint64)
        assert int(totals[0]) == (len(got.result_text) if results else 0) and int(totals[1]) == (len(got.item_text) if items else 0)
        assert np.array_equal(_from_device(out.d_doc_text_status, out.ndocs, np.int32), got.status)
        assert bool(out.d_result_text) == results and bool(out.d_result_text_offsets) == results
        assert bool(out.d_item_text) == items and bool(out.d_item_text_offsets) == items
        if results:
            assert np.array_equal(_from_device(out.d_result_text_offsets, len(mb.results) + 1, np.uint64), got.result_offsets)
    return mb, got


def _slice(src, d, span):
    s0, pos, s1, end = span
    d0 = d if src.dso is None else int(src.dso[d])
    return src.text[int(src.so[d0 + s0]) + pos:int(src.so[d0 + s1]) + end]


def _assert_chosen(src, mb, got, want):
    """what the test chose is what came out: per document the texts of its results and of its items (as multisets: the
    order inside a document is the engine's)"""
    ioffs = model.item_offsets(mb.results, mb.doc_offsets)
    for d, w in enumerate(want):
        r0, r1 = int(mb.doc_offsets[d]), int(mb.doc_offsets[d + 1])
        assert r1 - r0 == len(w)
        assert sorted(got.result(i) for i in range(r0, r1)) == sorted(_slice(src, d, s[0]) for s in w)
        assert sorted(got.item(i) for i in range(ioffs[d], ioffs[d + 1])) == sorted(_slice(src, d, x) for s in w for x in s[1:])


# ---- 1. round and copy edges
LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257]


def test_round_and_copy_edges():
    rng = np.random.default_rng(3)
    long_span = capi.lib().sp_matcher_text_long_span()
    counts = [0, 1, 63, 64, 65, 129]
    docs, seglens = [], []
    k = 0
    for n in counts:
        spans = []
        for _ in range(n):
            length = LENGTHS[k % len(LENGTHS)]
            pos = int(rng.integers(0, 40))
            spans.append((0, pos, 0, pos + length))
            k += 1
        docs.append(spans)
        seglens.append([300])
    # every source alignment against every destination alignment: spans of 13 bytes move the destination by one (mod 4)
    docs.append([(0, 4 * (i % 5) + i // 4, 0, 4 * (i % 5) + i // 4 + 13) for i in range(16)])
    seglens.append([64])
    # long spans: below, at and above the threshold, between short ones; the block ends mid-dword
    docs.append([(0, 1, 0, 4), (0, 3, 0, 3 + long_span - 1), (0, 2, 0, 2 + long_span), (0, 5, 0, 6), (0, 1, 0, 1 + long_span + 1),
                 (0, 7, 0, 7 + 2 * long_span + 3), (0, 0, 0, 2)])
    seglens.append([2 * long_span + 64])
    docs.append([(0, 0, 0, 3)])                                # a document of three bytes between two others
    seglens.append([5])
    docs.append([(0, 2, 0, 9), (0, 30, 0, 41)])                # the last span ends on the last byte of the text
    seglens.append([41])
    src = Source([_random_text(rng, lens[0]) for lens in seglens])
    lex, seg, offs, want = _pairs(docs, seglens)
    ctx = _ctx()
    Run(ctx, lex, seg, offs)
    out = src.gather(ctx)
    mb, got = _assert_text(ctx, src, out)
    assert not got.status.any()
    _assert_chosen(src, mb, got, want)
    assert ctx.lastTextMs() >= 0.0
    # what the shapes are there for
    assert np.diff(mb.doc_offsets.astype(np.int64)).tolist() == counts + [16, 7, 1, 2]
    assert got.result(len(mb.results) - 1) == src.text[-11:]
    assert {got.item(len(mb.items) - 2), got.item(len(mb.items) - 1)} == {src.text[-11:-6], src.text[-6:]}
    ro = got.result_offsets.astype(np.int64)
    lens = np.diff(ro)
    assert set(LENGTHS) | {long_span - 1, long_span, long_span + 1, 2 * long_span + 3} <= set(lens.tolist())
    begin = np.array([int(src.so[d]) for d in range(len(docs)) for _ in docs[d]]) + mb.results[:, 4].astype(np.int64)
    assert {(int(s) % 4, int(t) % 4) for s, t, n in zip(begin, ro[:-1], lens) if n >= 13} == {(s, t) for s in range(4) for t in range(4)}
    doc_at = ro[mb.doc_offsets.astype(np.int64)]
    assert any(doc_at[d] % 4 and doc_at[d + 1] % 4 and doc_at[d] > 0 and doc_at[d + 1] < ro[-1] for d in range(len(docs)))


# ---- 2. an invalid span on the device
@pytest.mark.parametrize("bad", [(0, 10, 0, 61), (0, 10, 1, 3)], ids=["origend beyond its segment", "origendseg beyond the document"])
def test_invalid_span_empties_its_document_only(bad):
    rng = np.random.default_rng(4)
    good = [(0, i % 50, 0, i % 50 + 7) for i in range(70)]
    docs = [good, good[:40] + [bad] + good[40:], good[:3]]
    seglens = [[60], [60], [60]]
    src = Source([_random_text(rng, 60) for _ in docs])
    lex, seg, offs, want = _pairs(docs, seglens)
    ctx = _ctx()
    Run(ctx, lex, seg, offs)
    src.gather(ctx)
    mb, got = _assert_text(ctx, src)
    assert got.status.tolist() == [0, 5, 0] and np.diff(mb.doc_offsets.astype(np.int64)).tolist() == [70, 71, 3]
    ro = got.result_offsets
    assert np.all(ro[70:142] == ro[70]) and got.result_text == b"".join(_slice(src, d, s) for d in (0, 2) for s in docs[d])
    io = got.item_offsets
    assert np.all(io[140:283] == io[140]) and len(got.item_text) == len(got.result_text)
    _assert_chosen(src, mb, got, want[:1])


@pytest.mark.parametrize("ndocs", [1025, 2049])
def test_document_counts_beyond_the_tile_of_the_offsets_pass(ndocs):
    """the offsets pass scans the documents in tiles of 1024: documents of 0..2 spans into the second and the third tile, one
    of the second tile with an invalid span (it counts 0 there, in both families)"""
    rng = np.random.default_rng(5)
    bad = 1030 if ndocs > 1030 else 1024
    docs = []
    for d in range(ndocs):
        spans = []
        for _ in range(int(rng.integers(0, 3))):
            pos = int(rng.integers(0, 12))
            spans.append((0, pos, 0, pos + int(rng.integers(0, 9))))
        docs.append(spans)
    docs[1022], docs[-1] = [], [(0, 0, 0, 20)]
    docs[bad - 1] = [(0, 2, 0, 9)]
    docs[bad] = [(0, 1, 0, 5), (0, 10, 0, 21)]             # origend beyond its segment
    seglens = [[20]] * ndocs
    src = Source([_random_text(rng, 20) for _ in docs])
    lex, seg, offs, want = _pairs(docs, seglens)
    ctx = _ctx()
    Run(ctx, lex, seg, offs)
    out = src.gather(ctx)
    mb, got = _assert_text(ctx, src, out)
    assert np.flatnonzero(got.status).tolist() == [bad] and int(got.status[bad]) == 5
    assert np.diff(mb.doc_offsets.astype(np.int64)).tolist() == [len(s) for s in docs]
    _assert_chosen(src, mb, got, want[:bad])
    # what lies behind the failed document follows the document before it; the last span ends the text
    r0, r1 = int(mb.doc_offsets[bad]), int(mb.doc_offsets[bad + 1])
    assert np.all(got.result_offsets[r0:r1 + 1] == got.result_offsets[r0]) and got.result(r0 - 1) == _slice(src, bad - 1, (0, 2, 0, 9))
    assert len(got.item_text) == len(got.result_text) == sum(s[3] - s[1] for d, spans in enumerate(docs) if d != bad for s in spans)
    if bad < ndocs - 1:
        assert got.result(len(mb.results) - 1) == src.text[-20:]


# ---- 3. the documented example end to end: lexer -> matcher -> finish -> text
def _example():
    with open(os.path.join(HERE, "golden", "doc_example.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("canonical", [False, True])
def test_example_end_to_end(canonical):
    case = _example()
    lx, mt = spa.PatternLexerInstance(), spa.PatternMatcherInstance()
    rulelang.load(case["program"], lx, mt)
    doc = case["text"].encode()
    pieces = [doc, b"", doc.splitlines(keepends=True)[0], doc]
    src = Source(pieces)
    lctx, mctx = lx.createContext(), mt.createContext()
    lex = lctx.matchDocsDevice(src.d_text.data_ptr(), src.d_so.data_ptr(), src.nseg, len(src.text), _stream())
    assert lctx.batchCounters()["failed_docs"] == 0
    mctx.matchLexedDevice(lex.d_lexems, lex.d_doc_ranges, src.nseg, int(lctx.batchCounters()["lexems"]), _stream())
    assert mctx.batchCounters()["failed_docs"] == 0
    mctx.batchFinishDevice(_stream(), canonical=canonical)
    out = src.gather(mctx)
    mb, got = _assert_text(mctx, src, out)
    assert len(mb.results) and len(mb.items) and not got.status.any()
    # the text follows the finished order: result i's text is the slice of its own record
    for d in range(src.nseg):
        for i in range(int(mb.doc_offsets[d]), int(mb.doc_offsets[d + 1])):
            assert got.result(i) == pieces[d][int(mb.results[i, 4]):int(mb.results[i, 6])]
    assert np.array_equal(mb.doc(0)[:, :7], mb.doc(3)[:, :7]) and got.result(0) == got.result(int(mb.doc_offsets[3]))
    if canonical:
        keys = [tuple(int(x) for x in r[1:7]) for r in mb.doc(0)]
        assert keys == sorted(keys)


# ---- 4. segmented documents
def test_segmented_example_and_cross_segment_span():
    case = _example()
    first, second = case["text"].splitlines(keepends=True)
    doc = (second + "\n  \n" + first).encode()
    lx, mt = spa.PatternLexerInstance(), spa.PatternMatcherInstance()
    rulelang.load(case["program"], lx, mt)
    text, so, dso, posmaps = segments.segmented_batch([doc, b"", doc])
    plain = spa.matchSegmentedDocs(lx.createContext(), mt.createContext(), text, so, dso)
    mb, mt_ = spa.matchSegmentedDocs(lx.createContext(), mt.createContext(), text, so, dso, with_text=True)
    assert np.array_equal(mb.results, plain.results) and np.array_equal(mb.items, plain.items) and np.array_equal(mb.status, plain.status)
    assert len(mb.results) and np.all(mb.results[:, 3] == 1) and not mt_.status.any()
    twin = spa.batchText(mb, text, so, dso)
    assert mt_.result_text == twin.result_text and mt_.item_text == twin.item_text
    assert np.array_equal(mt_.result_offsets, twin.result_offsets) and np.array_equal(mt_.item_offsets, twin.item_offsets)
    # the text of a result is the slice of the document between its absolute positions
    for d in (0, 2):
        r0, r1 = int(mb.doc_offsets[d]), int(mb.doc_offsets[d + 1])
        ab = segments.absolute_records(mb.results[r0:r1], posmaps[d])
        assert [mt_.result(r0 + i) for i in range(r1 - r0)] == [doc[int(a[4]):int(a[6])] for a in ab]
    # hand-made spans across one and across three segment borders, two of them of empty segments
    rng = np.random.default_rng(6)
    seglens = [[10, 0, 5, 9], [7], [4, 0, 0, 6]]
    docs = [[(0, 6, 0, 10), (0, 6, 2, 3), (1, 0, 1, 0), (0, 2, 3, 9), (2, 5, 3, 0)], [(0, 1, 0, 7)], [(0, 1, 3, 2), (3, 0, 3, 6)]]
    src = Source([_random_text(rng, n) for lens in seglens for n in lens], doc_seg_offsets=[0, 4, 5, 9])
    lex, seg, offs, want = _pairs(docs, seglens)
    ctx = _ctx()
    Run(ctx, lex, seg, offs)
    src.gather(ctx)
    mb, got = _assert_text(ctx, src)
    assert not got.status.any() and np.count_nonzero(mb.results[:, 3] != mb.results[:, 5]) == 4
    _assert_chosen(src, mb, got, want)
    assert sorted(len(got.result(i)) for i in range(5)) == [0, 0, 4, 7, 22]


# ---- 5. a random batch, on a stream of its own
def test_random_batch_on_another_stream():
    torch = _torch()
    rng = np.random.default_rng(7)
    docs, seglens = [], []
    for _ in range(200):
        lens = [int(x) for x in rng.integers(0, 50, int(rng.integers(1, 5)))]
        spans = []
        for _ in range(int(rng.integers(0, 90))):
            s0 = int(rng.integers(0, len(lens)))
            s1 = int(rng.integers(s0, len(lens)))
            pos = int(rng.integers(0, lens[s0] + 1))
            end = int(rng.integers(pos if s0 == s1 else 0, lens[s1] + 1))
            spans.append((s0, pos, s1, end))
        docs.append(spans)
        seglens.append(lens)
    dso = np.concatenate([[0], np.cumsum([len(lens) for lens in seglens])])
    src = Source([_random_text(rng, n) for lens in seglens for n in lens], doc_seg_offsets=dso)
    lex, seg, offs, want = _pairs(docs, seglens)
    ctx = _ctx()
    Run(ctx, lex, seg, offs)
    other = torch.cuda.Stream()
    out = src.gather(ctx, stream=other.cuda_stream)
    mb, got = _assert_text(ctx, src, out)
    assert not got.status.any() and len(mb.results) == sum(len(d) for d in docs)
    _assert_chosen(src, mb, got, want)
    # each family alone
    for results, items in ((True, False), (False, True)):
        out = src.gather(ctx, stream=other.cuda_stream, results=results, items=items)
        _assert_text(ctx, src, out, results=results, items=items)


# ---- 6. call order
def test_call_order_and_buffer_reuse():
    rng = np.random.default_rng(8)
    docs = [[(0, i, 0, i + 5) for i in range(20)], [(0, 0, 0, 9)]]
    seglens = [[40], [40]]
    src = Source([_random_text(rng, 40) for _ in docs])
    lex, seg, offs, want = _pairs(docs, seglens)
    ctx = _ctx()
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):       # before any batch
        src.gather(ctx)
    with pytest.raises(spa.PatternError):
        ctx.finishedTextFetch()
    with pytest.raises(spa.PatternError):
        ctx.lastTextMs()
    run = Run(ctx, lex, seg, offs)
    for kw in (dict(results=False, items=False),):
        with pytest.raises(spa.PatternError, match=r"\(-1\)"):
            src.gather(ctx, **kw)
    L = capi.lib()
    out = capi.SpMatchTextBatch()
    ok_src = capi.SpTextSource(src.d_text.data_ptr(), len(src.text), src.d_so.data_ptr(), src.nseg, None)
    assert L.sp_matcher_ctx_finished_text_device(ctx._h, ctypes.byref(ok_src), 4, None, ctypes.byref(out)) == -1      # an unknown bit
    assert L.sp_matcher_ctx_finished_text_device(ctx._h, None, 3, None, ctypes.byref(out)) == -1
    bad = capi.SpTextSource(src.d_text.data_ptr(), len(src.text), None, src.nseg, None)
    assert L.sp_matcher_ctx_finished_text_device(ctx._h, ctypes.byref(bad), 3, None, ctypes.byref(out)) == -1
    bad = capi.SpTextSource(src.d_text.data_ptr(), len(src.text), src.d_so.data_ptr(), src.nseg + 1, None)      # nseg != ndocs
    assert L.sp_matcher_ctx_finished_text_device(ctx._h, ctypes.byref(bad), 3, None, ctypes.byref(out)) == -1
    # an allocation that fails, then a normal call
    L.sp_test_fail_alloc_above(1)
    try:
        assert L.sp_matcher_ctx_finished_text_device(ctx._h, ctypes.byref(ok_src), 3, None, ctypes.byref(out)) == -2  # SP_ERR_NOMEM
    finally:
        L.sp_test_fail_alloc_above(0)
    first = src.gather(ctx)
    mb, got = _assert_text(ctx, src, first)
    _assert_chosen(src, mb, got, want)
    # a second call reuses the buffers
    second = src.gather(ctx)
    for name, _ in capi.SpMatchTextBatch._fields_:
        assert getattr(first, name) == getattr(second, name)
    _assert_text(ctx, src, second)
    # the next batch invalidates the state until it is finished again
    run.match()
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        src.gather(ctx)
    with pytest.raises(spa.PatternError):
        ctx.finishedTextFetch()
    ctx.batchFinishDevice(_stream())
    with pytest.raises(spa.PatternError):                       # finished, but no text of this finish yet
        ctx.finishedTextFetch()
    third = src.gather(ctx)
    assert third.d_result_text == first.d_result_text
    _assert_text(ctx, src, third)
