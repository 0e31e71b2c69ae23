"""Index terms on the device (sp_matcher_ctx_finished_terms_device, csrc/l2_terms.h): the records, offsets, result_term,
status and total that the passes leave must EQUAL what the device-free twin (sp_match_batch_terms) makes of the fetched
finished batch with its fetched text and values, and the model (tests/terms_model.py).  Bare-term matchers over hand-made
lexems as in tests/test_pattern_freq_gpu.py: the lexem (h, p, origpos, origsize) gives the result with handle h whose text is
[origpos, origpos + origsize) of the document's crafted text, so with SP_TERM_TEXT a test sets every handle and value itself.

The device tests feed valid handles only: the matcher produces no others.  The handle-range rule is covered through the twin
(tests/test_terms_abi.py, tests/micro/match_terms_san.cpp) and by the bound check being the first use of a handle in every
kernel (validHandle in countTerms and placeTerms, csrc/l2_terms_kernel.hip)."""
import ctypes

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from tests import terms_model as model
from tests.finished_support import (_bare, _build, _from_device, Lexems, _matcher, MONEY, Run, RunAny, Source, _stream, T_LIT, T_PLAIN_A, T_PLAIN_B,
                                    T_SPAN, _torch, _values)

pytestmark = pytest.mark.gpu

V, T = spa.SP_TERM_VALUES, spa.SP_TERM_TEXT
NONE = 0xFFFFFFFF


def _assert_terms(ctx, bound, flags, out=None):
    """the fetched terms equal the twin's and the model's on the fetched batch, text and values; returns (batch, terms)"""
    mb = ctx.finishedFetch()
    mt = ctx.finishedTextFetch() if flags & T else None
    mv = ctx.finishedValuesFetch() if flags & V else None
    got = ctx.finishedTermsFetch()
    want = model.of_batch(mb, bound, flags, mv, mt)
    model.assert_same(spa.batchTerms(mb, values=mv, text=mt, handle_bound=bound, flags=flags), want)
    model.assert_same(got, want)
    if out is not None:
        assert out.ndocs == len(mb.doc_offsets) - 1 and out.handle_bound == bound and out.flags == flags
        assert int(_from_device(out.d_totals, 1, np.uint64)[0]) == len(got.records)
        assert np.array_equal(_from_device(out.d_doc_term_status, out.ndocs, np.int32), got.status)
        assert np.array_equal(_from_device(out.d_doc_term_offsets, out.ndocs + 1, np.uint64), got.doc_offsets)
        assert np.array_equal(_from_device(out.d_records, 6 * len(got.records), np.uint32).reshape(-1, 6), got.records)
        assert np.array_equal(_from_device(out.d_result_term, len(mb.results), np.uint32), got.result_term)
    return mb, got


def _go(docs, nhandles=8, canonical=False, stream=None):
    """the text terms of hand-made documents: (context, source, batch, terms)"""
    m = _bare(nhandles)
    pieces, lex, seg, offs = _build(docs)
    ctx = m.createContext()
    src = Source(pieces)
    Run(ctx, lex, seg, offs, canonical=canonical)
    src.gather(ctx, items=False)
    out = ctx.finishedTermsDevice(T, _stream() if stream is None else stream)
    mb, got = _assert_terms(ctx, nhandles + 1, T, out)
    assert len(mb.results) == len(lex)
    return ctx, src, mb, got


def _values_of(mb, mt, got, d):
    return [(h, v, c) for h, v, c, _, _ in got.terms(d, mb, text=mt)]


def _mixed(n, seed):
    """n results over 5 handles and 37 values of the lengths 0 .. 36"""
    rng = np.random.default_rng(seed)
    pool = [bytes(rng.integers(65, 91, k, dtype=np.uint8)) for k in range(37)]
    return [(1 + int(rng.integers(0, 5)), pool[int(rng.integers(0, 37))]) for _ in range(n)]


def _shape_docs():
    tile = capi.lib().sp_matcher_term_tile()
    docs = [_mixed(n, 100 + n) for n in (5, 0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1)]
    docs.append([(3, b"same value")] * 130)                                               # all results one term
    docs.append([(1 + k % 4, b"v%03d" % k) for k in range(200)])                           # all results distinct terms
    return docs


# ---- 1. batch shapes
def test_no_documents():
    m = _bare(8)
    ctx = m.createContext()
    src = Source([])
    Run(ctx, np.zeros((0, 4), np.uint32), np.zeros(0, np.uint32), np.zeros(1, np.uint64))
    src.gather(ctx, items=False)
    out = ctx.finishedTermsDevice(T, _stream())
    mb, got = _assert_terms(ctx, 9, T, out)
    assert len(got.records) == 0 and got.doc_offsets.tolist() == [0] and len(got.result_term) == 0


def test_trip_and_tile_edges_one_term_and_distinct_terms():
    tile = capi.lib().sp_matcher_term_tile()
    docs = _shape_docs()
    ctx, src, mb, got = _go(docs)
    assert np.diff(mb.doc_offsets.astype(np.int64)).tolist() == [5, 0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1, 130, 200]
    assert not got.status.any() and len(got.doc(1)) == 0 and len(got.doc(2)) == 1
    assert got.doc(10).tolist() == [[3, 130, 1, 131, 0, 10]]
    assert len(got.doc(11)) == 200 and np.all(got.doc(11)[:, 1] == 1)
    assert 100 < len(got.doc(9)) <= 5 * 37 and int(got.doc(9)[:, 1].sum()) == 2 * tile + 1
    assert ctx.lastTermsMs() >= 0.0
    # the invariant against the frequency pass of the same finish
    ctx.finishedPatternFreqDevice(_stream())
    freq = ctx.finishedPatternFreqFetch()
    for d in range(len(docs)):
        terms = got.doc(d)
        for h, count, first, last in freq.doc(d).tolist():
            mine = terms[terms[:, 0] == h]
            assert int(mine[:, 1].sum()) == count and int(mine[:, 2].min()) == first and int(mine[:, 3].max()) == last
        assert sorted(set(terms[:, 0].tolist())) == freq.doc(d)[:, 0].tolist()


# ---- 2. values
def test_value_edges():
    base = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefg"                        # 33 bytes
    lengths = [0, 1, 15, 16, 17, 33]
    docs = [
        [(1, base[:n]) for n in lengths] * 3,                           # every length three times, at three places
        [(2, b"same"), (5, b"same"), (2, b"same"), (5, b"same")],       # identical bytes under two handles
        [(1, base[:16]), (1, base[:17]), (1, base[:16]), (1, base[:17] + b"x")],          # one a prefix of the other
        [(1, base[:32] + b"A"), (1, base[:32] + b"B"), (1, base[:32] + b"A"), (1, b"A" + base[:32]), (1, b"B" + base[:32])],  # last byte, first byte
        [(4, base[:17])] * 40 + [(4, base[:16] + b"!")] * 3,            # 17 bytes: the copies start at every offset modulo 16
    ]
    ctx, src, mb, got = _go(docs)
    mt = ctx.finishedTextFetch()
    assert not got.status.any()
    assert _values_of(mb, mt, got, 0) == [(1, base[:n], 3) for n in lengths]
    assert _values_of(mb, mt, got, 1) == [(2, b"same", 2), (5, b"same", 2)]
    assert _values_of(mb, mt, got, 2) == [(1, base[:16], 2), (1, base[:17], 1), (1, base[:17] + b"x", 1)]
    assert [c for _, _, c in _values_of(mb, mt, got, 3)] == [2, 1, 1, 1]
    assert _values_of(mb, mt, got, 4) == [(4, base[:17], 40), (4, base[:16] + b"!", 3)]
    assert got.doc(4)[:, 4].tolist() == [0, 40]
    starts = {(int(src.so[4]) + 17 * k) % 16 for k in range(40)}
    assert starts == set(range(16))


# ---- 3. a hash decides nothing
def test_hash_bits_leave_identical_bytes():
    docs = _shape_docs()
    L = capi.lib()
    fields = []
    try:
        for bits in (0, 2, 32):
            L.sp_test_term_hash_bits(bits)
            ctx, src, mb, got = _go(docs)
            fields.append([getattr(got, f).tobytes() for f in ("records", "doc_offsets", "result_term", "status")])
    finally:
        L.sp_test_term_hash_bits(32)
    assert fields[0] == fields[1] == fields[2] and len(fields[2][0]) > 24 * 400


# ---- 4. values as the source, and both sources
def test_values_alone_and_both_flags_on_a_matcher_with_formats():
    m = _matcher()
    bound = m.handleBound()
    text = b"eur usd eur chf usd eur ab cd ab cd"
    L = Lexems()
    for pos in (0, 4, 8, 12, 16, 20):
        L.add(T_SPAN, pos, 3).gap()                                     # Span: formatted "{a}" -> eur usd eur chf usd eur
    L.add(T_LIT, 0, 3).gap().add(T_LIT, 4, 3).gap()                     # Lit: formatted, the value is "CHF" whatever the text
    L.add(T_PLAIN_A, 24, 2).add(T_PLAIN_B, 27, 2).gap().add(T_PLAIN_A, 30, 2).add(T_PLAIN_B, 33, 2)   # Plain: no format, text "ab cd" twice
    L.doc()
    L.add(T_SPAN, 33, 2).doc()
    L.add(T_SPAN, 40, 3).add(T_SPAN, 0, 3).doc()                        # a span outside the text: the values of the document fail
    L.add(T_LIT, 1, 1).add(T_SPAN, 4, 3).doc()
    for flags in (V, V | T):
        ctx = m.createContext()
        src = Source([text] * 4)
        RunAny(ctx, *L.arrays())
        with pytest.raises(spa.PatternError, match=r"\(-1\)"):          # before the values call
            ctx.finishedTermsDevice(flags, _stream())
        _values(ctx, src, flags=model.SP_TERM_VALUES)                   # (SP_VALUE_RESULTS)
        if flags & T:
            with pytest.raises(spa.PatternError, match=r"\(-1\)"):      # values, but no text yet
                ctx.finishedTermsDevice(flags, _stream())
            src.gather(ctx, items=False)
        out = ctx.finishedTermsDevice(flags, _stream())
        mb, got = _assert_terms(ctx, bound, flags, out)
        mv = ctx.finishedValuesFetch()
        mt = ctx.finishedTextFetch() if flags & T else None
        assert got.status.tolist() == [0, 0, 5, 0] and mv.status.tolist() == [0, 0, 5, 0]
        r2 = slice(int(mb.doc_offsets[2]), int(mb.doc_offsets[3]))
        assert len(got.doc(2)) == 0 and len(mb.results[r2]) == 2 and np.all(got.result_term[r2] == NONE)
        assert len(got.doc(1)) == 1 and len(got.doc(3)) == 2 and not np.any(got.result_term[:r2.start] == NONE)
        name = lambda h: m.patternName(h)
        terms = sorted((name(h), v, c) for h, v, c, _, _ in got.terms(0, mb, values=mv, text=mt))
        plain = (b"", 2) if flags == V else (b"ab cd", 2)               # an unformatted result: the empty value, or its text
        assert terms == sorted([("Lit", b"CHF", 2), ("Plain",) + plain, ("Span", b"eur", 3), ("Span", b"usd", 2), ("Span", b"chf", 1)])


# ---- 5. the order of the results
def test_plain_against_canonical_finish():
    docs = _shape_docs()[:8]
    per_doc = []
    for canonical in (False, True):
        ctx, src, mb, got = _go(docs, canonical=canonical)
        mt = ctx.finishedTextFetch()
        per_doc.append([sorted(got.terms(d, mb, text=mt)) for d in range(len(docs))])
    assert per_doc[0] == per_doc[1] and len(per_doc[0][7]) > 100


# ---- 6. call order, buffers, streams
def test_call_order_second_batch_and_another_stream():
    torch = _torch()
    m = _bare(8)
    docs = _shape_docs()[:7]
    pieces, lex, seg, offs = _build(docs)
    ctx = m.createContext()
    src = Source(pieces)
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):              # before any batch
        ctx.finishedTermsDevice(T, _stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedTermsFetch()
    with pytest.raises(spa.PatternError):
        ctx.lastTermsMs()
    run = Run(ctx, lex, seg, offs)
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):              # finished, but no text
        ctx.finishedTermsDevice(T, _stream())
    src.gather(ctx, results=False)
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):              # a text without the results family
        ctx.finishedTermsDevice(T, _stream())
    src.gather(ctx, items=False)
    for flags in (0, 4, V):                                             # bad flags; values that were never built
        with pytest.raises(spa.PatternError, match=r"\(-1\)"):
            ctx.finishedTermsDevice(flags, _stream())
    # an allocation that fails, then a normal call
    L = capi.lib()
    out = capi.SpMatchTermsDevice()
    L.sp_test_fail_alloc_above(1)
    try:
        assert L.sp_matcher_ctx_finished_terms_device(ctx._h, T, None, ctypes.byref(out)) == -2      # SP_ERR_NOMEM
    finally:
        L.sp_test_fail_alloc_above(0)
    first = ctx.finishedTermsDevice(T, _stream())
    mb, got = _assert_terms(ctx, 9, T, first)
    # a stream other than the finish's and the text's
    other = torch.cuda.Stream()
    second = ctx.finishedTermsDevice(T, other.cuda_stream)
    assert second.d_records == first.d_records
    model.assert_same(_assert_terms(ctx, 9, T, second)[1], got)
    # the text gathered on a third stream, not waited for, and the terms on the second
    third = torch.cuda.Stream()
    src.gather(ctx, stream=third.cuda_stream, items=False)
    model.assert_same(_assert_terms(ctx, 9, T, ctx.finishedTermsDevice(T, other.cuda_stream))[1], got)
    # a new finish: the old text does not count
    run.match()
    ctx.batchFinishDevice(_stream())
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        ctx.finishedTermsDevice(T, _stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedTermsFetch()
    # a second, smaller batch on the same context
    small = docs[:3]
    pieces, lex, seg, offs = _build(small)
    src = Source(pieces)
    Run(ctx, lex, seg, offs)
    src.gather(ctx, items=False)
    fourth = ctx.finishedTermsDevice(T, _stream())
    assert fourth.d_records == first.d_records and fourth.d_result_term == first.d_result_term
    mb, got = _assert_terms(ctx, 9, T, fourth)
    assert len(mb.results) == 6 and got.doc_offsets[-1] == len(got.records) > 0


# ---- 7. segmented documents end to end
def test_segmented_documents_with_terms():
    from struspattern_amd import rulelang, segments
    docs = [b"He paid 3'645 Eur\n\nand 3'645 Eur again or 12 sFr. he paid", b"nothing", b"12 sFr. in the year 1984 something happened"]
    lx, m = spa.PatternLexerInstance(), spa.PatternMatcherInstance()
    rulelang.load(MONEY, lx, m)
    text, so, dso, _ = segments.segmented_batch(docs)
    assert len(so) - 1 > len(docs)                                      # (a document of two segments)
    mb, mt, mv, terms = spa.matchSegmentedDocs(lx.createContext(), m.createContext(), text, so, dso, with_terms=True)
    assert not mb.status.any() and not mv.status.any() and not mt.status.any()
    flags = V | T
    model.assert_same(terms, model.of_batch(mb, m.handleBound(), flags, mv, mt))
    model.assert_same(spa.batchTerms(mb, values=mv, text=mt, handle_bound=m.handleBound(), flags=flags), terms)
    assert not terms.status.any() and len(terms.records) > 0
    found = {(m.patternName(h), v): c for h, v, c, _, _ in terms.terms(0, mb, values=mv, text=mt)}
    assert found[("MoneyAmount", b"EUR 3'645")] == 2 and found[("MoneyAmount", b"CHF 12")] == 1


# ---- 8. minimum and maximum against first_result: results whose ordpos does not ascend in engine order
def test_first_result_is_not_the_result_with_the_least_ordpos():
    m = spa.PatternMatcherInstance()
    for a, b in ((1, 2), (3, 4)):
        m.pushTerm(a)
        m.pushTerm(b)
        m.pushExpression("within", 2, 5, 0)
        m.definePattern("w", "", True)
    m.compile()
    assert m.handleBound() == 2
    # every lexem of document 0 covers the same three bytes: all its results are one term, whatever their positions
    docs = [[(1, 1), (3, 2), (4, 3), (2, 4), (4, 5), (3, 6)], [(3, 1), (4, 2)]]
    lex, offs = [], [0]
    for doc in docs:
        lex += [[t, p, 0, 3] for t, p in doc]
        offs.append(len(lex))
    lex, offs = np.array(lex, np.uint32).reshape(-1, 4), np.array(offs, np.uint64)
    ctx = m.createContext()
    src = Source([b"abc", b"xyz"])
    Run(ctx, lex, np.zeros(len(lex), np.uint32), offs)
    src.gather(ctx, items=False)
    out = ctx.finishedTermsDevice(T, _stream())
    mb, got = _assert_terms(ctx, 2, T, out)
    mt = ctx.finishedTextFetch()
    first = mb.doc(0)
    assert len(first) == 4 and all(mt.result(r) == b"abc" for r in range(4))
    assert got.doc(0).tolist() == [[1, 4, int(first[:, 1].min()), int(first[:, 2].max()), 0, 3]]
    assert int(first[0, 1]) != int(first[:, 1].min()) and int(first[0, 2]) != int(first[:, 2].max())    # (else the case shows nothing)
    assert got.doc(1).tolist() == [[1, 1, 1, 3, 0, 3]] and got.result_term.tolist() == [0] * 5


# ---- 9. after a canonical finish the same bytes from the exact engine and from result-set mode
def test_exact_engine_against_result_set_mode_after_a_canonical_finish():
    from struspattern_amd import synth
    rules = synth.random_rules(400, 30, 2)
    lex, offs = synth.random_documents(24, 500, 30, 102)
    m = spa.PatternMatcherInstance()
    synth.apply_rules(m, rules)
    assert m.resultSetTier()[0]
    bound = m.handleBound()
    rng = np.random.default_rng(5)
    pieces = [bytes(rng.integers(97, 99, int(offs[d + 1] - offs[d]), dtype=np.uint8)) for d in range(24)]   # texts over "ab": values repeat
    src = Source(pieces)
    got = []
    for result_sets in (False, True):
        ctx = m.createContext(result_sets=result_sets)
        assert ctx.kernelKind() == (2 if result_sets else 1)
        Run(ctx, lex, np.zeros(len(lex), np.uint32), offs, canonical=True)
        src.gather(ctx, items=False)
        out = ctx.finishedTermsDevice(T, _stream())
        got.append(_assert_terms(ctx, bound, T, out))
    (mb_a, a), (mb_b, b) = got
    assert np.array_equal(mb_a.results, mb_b.results) and len(mb_a.results) > 1000
    assert len(a.records) > 500 and int(a.records[:, 1].max()) > 1 and len(a.records) < len(mb_a.results) and not a.status.any()
    for f in ("records", "doc_offsets", "result_term", "status"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes()


# ---- 10. the command line
def test_match_terms_listing(capsys):
    import json
    import os
    from struspattern_amd import match, rulelang
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "doc_example.json")) as f:
        case = json.load(f)
    prog, fn = os.path.join(here, "golden", "doc_example.rul"), os.path.join(here, "golden", "doc_example.txt")
    assert match.main(["-p", prog, "-o", str(case["origin"]), "--device-values", fn]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert plain[0] == "%s:" % fn and plain[1:5] == case["results"] and plain[-1] == "OK done"
    assert match.main(["-p", prog, "-o", str(case["origin"]), "--device-values", "--terms", fn]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[:5] == plain[:5] and lines[-1] == "OK done" and len(lines) > 6
    # the same lines by the model, from the batch and the values that --device-values builds and the text of the results
    lx, mt = spa.PatternLexerInstance(), spa.PatternMatcherInstance()
    rulelang.load(case["program"], lx, mt)
    with open(fn, "rb") as f:
        doc = f.read()
    offs = np.array([0, len(doc)], np.uint64)
    lb = lx.createContext().matchDocs(doc, offs)
    mctx = mt.createContext()
    mb = mctx.matchDocs(lb.lexems, lb.doc_offsets)
    mv = match.device_values(mctx, doc, offs)
    mtext = spa.batchText(mb, doc, offs, items=False)
    want = model.of_batch(mb, mt.handleBound(), V | T, mv, mtext)
    formatted = mb.result_format is not None
    expected = []
    for h, count, pos, end, fr, size in want.records.tolist():
        value = mv.result(fr) if formatted and int(mb.result_format[fr]) else mtext.result(fr)
        expected.append("term %s '%s': count %d first %d" % (mt.patternName(h), value.decode(), count, pos))
    assert lines[5:-1] == expected
    names = [line.split(" '")[0] for line in lines[5:-1]]
    assert names == sorted(names, key=lambda n: mt.patternId(n[5:])) and sum(int(l.split("count ")[1].split()[0]) for l in lines[5:-1]) == 4
