"""Batch dictionary on the device (sp_matcher_ctx_finished_dictionary_device, csrc/l2_dict.h): the records, term_dict, offsets,
handle_terms and total that the five launches leave must EQUAL what the device-free twin (sp_match_batch_dictionary) makes of
the fetched batch, sources and terms, and the model (tests/dictionary_model.py); the device pointers of `out` hold the same
bytes.  Bare-term matchers over hand-made lexems as in tests/test_terms_gpu.py: with SP_TERM_TEXT a test sets every handle
and value itself, and since every occurrence has its own copy of its value, equal values lie at different addresses.

A pattern name defined twice, once with a format string and once without, is ONE handle whose results are formatted or not by
the definition that fired: that is how a formatted value meets an unformatted text under the same handle (section 5)."""
import ctypes

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from tests import dictionary_model as model
from tests.finished_support import (_bare, _build, EVERY, _from_device, Lexems, _matcher, MONEY, Run, RunAny, Source, _stream, T_LIT, T_PLAIN_A,
                                    T_PLAIN_B, T_SPAN, _torch, _trip_docs, TRIP_RECORDS, _values)

pytestmark = pytest.mark.gpu

V, T = spa.SP_TERM_VALUES, spa.SP_TERM_TEXT


def _assert_dictionary(ctx, bound, out=None):
    """the fetched dictionary equals the twin's and the model's on the fetched batch, sources and terms, and so do the bytes
    behind the device pointers; returns (batch, terms, dictionary)"""
    mb = ctx.finishedFetch()
    terms = ctx.finishedTermsFetch()
    mt = ctx.finishedTextFetch() if terms.flags & T else None
    mv = ctx.finishedValuesFetch() if terms.flags & V else None
    got = ctx.finishedDictionaryFetch()
    want = model.of_batch(mb, terms, bound, mv, mt)
    model.assert_same(spa.batchDictionary(mb, terms, values=mv, text=mt), want)
    model.assert_same(got, want)
    model.check_invariants(got, terms, mb)
    if out is not None:
        assert out.ndocs == len(mb.doc_offsets) - 1 and out.handle_bound == bound and out.flags == terms.flags
        assert int(_from_device(out.d_totals, 1, np.uint64)[0]) == len(got.records)
        assert np.array_equal(_from_device(out.d_records, 8 * len(got.records), np.uint32).reshape(-1, 8), got.records)
        assert np.array_equal(_from_device(out.d_term_dict, len(terms.records), np.uint32), got.term_dict)
        assert np.array_equal(_from_device(out.d_doc_dict_offsets, out.ndocs + 1, np.uint64), got.doc_offsets)
        assert np.array_equal(_from_device(out.d_handle_terms, bound, np.uint32), got.handle_terms)
    return mb, terms, got


def _go(docs, nhandles=8, canonical=False):
    """the dictionary of the text terms of hand-made documents: (context, batch, terms, dictionary)"""
    m = _bare(nhandles)
    pieces, lex, seg, offs = _build(docs)
    ctx = m.createContext()
    src = Source(pieces)
    Run(ctx, lex, seg, offs, canonical=canonical)
    src.gather(ctx, items=False)
    ctx.finishedTermsDevice(T, _stream())
    out = ctx.finishedDictionaryDevice(_stream())
    mb, terms, got = _assert_dictionary(ctx, nhandles + 1, out)
    assert len(mb.results) == len(lex)
    return ctx, mb, terms, got


def _by_term(ctx, mb, terms, got):
    """(handle, value) -> (doc_freq, count, max_count, first_doc)"""
    mt = ctx.finishedTextFetch()
    return {(h, v): (df, c, mx, int(first)) for (h, v, df, c, mx), first in zip(got.entries(mb, terms, text=mt), got.records[:, 2])}


# ---- 1. empty shapes
def test_no_documents_empty_documents_and_a_single_document():
    m = _bare(8)
    ctx = m.createContext()
    src = Source([])
    Run(ctx, np.zeros((0, 4), np.uint32), np.zeros(0, np.uint32), np.zeros(1, np.uint64))
    src.gather(ctx, items=False)
    ctx.finishedTermsDevice(T, _stream())
    out = ctx.finishedDictionaryDevice(_stream())
    mb, terms, got = _assert_dictionary(ctx, 9, out)
    assert len(got.records) == 0 and got.doc_offsets.tolist() == [0] and len(got.term_dict) == 0 and not got.handle_terms.any()
    ctx, mb, terms, got = _go([[], [], []])
    assert len(got.records) == 0 and got.doc_offsets.tolist() == [0, 0, 0, 0] and not got.handle_terms.any()
    doc = [(2, b"b"), (1, b"a"), (2, b"b"), (2, b""), (3, b"a"), (2, b"b")]
    ctx, mb, terms, got = _go([doc])
    assert len(got.records) == len(terms.records) == 4 and got.term_dict.tolist() == [0, 1, 2, 3] and got.doc_offsets.tolist() == [0, 4]
    assert np.all(got.records[:, 4] == 1) and got.counts.tolist() == terms.records[:, 1].tolist() == [1, 3, 1, 1]
    assert got.records[:, 5].tolist() == [1, 3, 1, 1] and got.records[:, 3].tolist() == [0, 1, 2, 3] and not got.records[:, 2].any()


# ---- 2. trip edges
def test_trip_edges_with_terms_repeated_across_documents():
    docs = _trip_docs()
    ctx, mb, terms, got = _go(docs)
    assert np.diff(terms.doc_offsets.astype(np.int64)).tolist() == TRIP_RECORDS
    found = _by_term(ctx, mb, terms, got)
    assert found[EVERY] == (6, sum(d.count(EVERY) for d in docs), 2, 1) and found[EVERY][1] == 10
    new = np.diff(got.doc_offsets.astype(np.int64)).tolist()
    assert new[0] == 0 and new[1] == 1 and new[6] == 0 and all(0 < new[k] < TRIP_RECORDS[k] for k in (2, 3, 4, 5))
    assert len(got.records) < len(terms.records) and int(got.records[:, 4].max()) == 6 and int(got.records[:, 5].max()) == 2
    assert ctx.lastDictionaryMs() >= 0.0


# ---- 3. value edges across documents
def test_value_edges_across_documents():
    base = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefg"                        # 33 bytes
    lengths = [0, 1, 15, 16, 17, 33]
    seventeen = b"seventeen bytes.."
    assert len(seventeen) == 17
    docs = [
        [(1, base[:n]) for n in lengths],
        [(1, base[:n]) for n in reversed(lengths)] + [(1, base[:n]) for n in lengths],
        # each pair split over two documents: the last byte, the first byte, a prefix, the handle
        [(1, base[:32] + b"A"), (1, b"A" + base[:32]), (3, base[:16]), (2, b"same"), (3, b"")],
        [(1, base[:32] + b"B"), (1, b"B" + base[:32]), (3, base[:17]), (5, b"same"), (3, b"\0")],
    ]
    # one value of 17 bytes in 16 documents, its copies at the 16 start offsets modulo 16
    running = sum(len(v) for doc in docs for _, v in doc)
    for k in range(16):
        pad = (k - running) % 16
        docs.append([(4, b"p" * pad), (4, seventeen)])
        running += pad + 17
    ctx, mb, terms, got = _go(docs)
    mt = ctx.finishedTextFetch()
    starts = {int(mt.result_offsets[r]) % 16 for r in range(len(mb.results)) if mt.result(r) == seventeen}
    assert starts == set(range(16))
    found = _by_term(ctx, mb, terms, got)
    for n in lengths:
        assert found[(1, base[:n])] == (2, 3, 2, 0)
    for key in ((1, base[:32] + b"A"), (1, b"A" + base[:32]), (3, base[:16]), (2, b"same"), (3, b"")):
        assert found[key] == (1, 1, 1, 2)
    for key in ((1, base[:32] + b"B"), (1, b"B" + base[:32]), (3, base[:17]), (5, b"same"), (3, b"\0")):
        assert found[key] == (1, 1, 1, 3)
    assert found[(4, seventeen)] == (16, 16, 1, 4)
    assert len(found) == len(got.records) and int(got.handle_terms[4]) == 1 + len({len(d[0][1]) for d in docs[4:]})


# ---- 4. a hash decides nothing
def test_hash_bits_leave_identical_bytes():
    docs = _trip_docs()
    L = capi.lib()
    fields = []
    try:
        for bits in (0, 2, 32):
            L.sp_test_term_hash_bits(bits)
            ctx, mb, terms, got = _go(docs)
            assert len(terms.records) == sum(TRIP_RECORDS) < 1500
            fields.append([getattr(got, f).tobytes() for f in model.FIELDS])
    finally:
        L.sp_test_term_hash_bits(32)
    assert fields[0] == fields[1] == fields[2] and len(fields[2][0]) > 32 * 150


# ---- 5. formats and failed documents
def test_values_alone_and_both_flags_with_a_document_whose_values_fail():
    m = _matcher()
    bound = m.handleBound()
    text = b"eur usd eur chf usd eur ab cd ab cd CHF"
    L = Lexems()
    for pos in (0, 4, 8):
        L.add(T_SPAN, pos, 3).gap()                                     # Span: formatted "{a}" -> eur usd eur
    L.add(T_LIT, 0, 3).gap()                                            # Lit: formatted, the value is "CHF" whatever the text
    L.add(T_PLAIN_A, 24, 2).add(T_PLAIN_B, 27, 2)                       # Plain: no format, text "ab cd"
    L.doc()
    L.add(T_SPAN, 36, 3).gap().add(T_SPAN, 4, 3).doc()                  # the text "CHF" as the value of a Span, and usd again
    L.add(T_SPAN, 50, 3).add(T_SPAN, 0, 3).add(T_LIT, 0, 3).doc()       # a span outside the text: the values of the document fail
    L.add(T_LIT, 1, 1).gap().add(T_LIT, 5, 1).gap().add(T_SPAN, 0, 3).gap().add(T_PLAIN_A, 30, 2).add(T_PLAIN_B, 33, 2).doc()
    for flags in (V, V | T):
        ctx = m.createContext()
        src = Source([text] * 4)
        RunAny(ctx, *L.arrays())
        _values(ctx, src, flags=1)                                      # (SP_VALUE_RESULTS)
        if flags & T:
            src.gather(ctx, items=False)
        ctx.finishedTermsDevice(flags, _stream())
        out = ctx.finishedDictionaryDevice(_stream())
        mb, terms, got = _assert_dictionary(ctx, bound, out)
        mv = ctx.finishedValuesFetch()
        mt = ctx.finishedTextFetch() if flags & T else None
        assert terms.status.tolist() == [0, 0, 5, 0] and mv.status.tolist() == [0, 0, 5, 0] and len(mb.doc(2)) == 3
        name = m.patternName
        found = {(name(h), v): (df, c, mx, int(first)) for (h, v, df, c, mx), first in zip(got.entries(mb, terms, values=mv, text=mt), got.records[:, 2])}
        plain = b"" if flags == V else b"ab cd"                         # an unformatted result: the empty value, or its text
        assert found == {("Span", b"eur"): (2, 3, 2, 0), ("Span", b"usd"): (2, 2, 1, 0), ("Lit", b"CHF"): (2, 3, 2, 0), ("Plain", plain): (2, 2, 1, 0),
                         ("Span", b"CHF"): (1, 1, 1, 1)}
        assert got.doc_offsets.tolist() == [0, 4, 5, 5, 5] and not np.any(got.records[:, 2] == 2)


_TWICE = []


def _defined_twice():
    """X = any(term 1) with the format "CHF", and X = sequence(term 2, term 3) without a format: one name, one handle"""
    if not _TWICE:
        m = spa.PatternMatcherInstance()
        m.pushTerm(1)
        m.attachVariable("a")
        m.pushExpression("any", 1, 1, 0)
        m.definePattern("X", "CHF", True)
        m.pushTerm(2)
        m.pushTerm(3)
        m.pushExpression("sequence", 2, 1, 0)
        m.definePattern("X", "", True)
        m.compile()
        assert m.handleBound() == 2 and m.patternId("X") == 1
        _TWICE.append(m)
    return _TWICE[0]


def test_formatted_value_of_one_document_equals_the_text_of_another_under_the_same_handle():
    m = _defined_twice()
    text = b"eur CHF"
    L = Lexems()
    L.add(1, 0, 3).doc()                                                # formatted: the value is "CHF", the text "eur"
    L.add(2, 4, 2).add(3, 6, 1).doc()                                   # unformatted: the text is "CHF"
    L.add(1, 0, 3).gap().add(2, 4, 2).add(3, 6, 1).gap().add(1, 4, 3).doc()   # both in one document, and a formatted one over "CHF"
    L.add(2, 0, 2).add(3, 2, 1).doc()                                   # unformatted: the text is "eur"
    want = {V: {b"CHF": (2, 3, 2, 0), b"": (3, 3, 1, 1)},
            V | T: {b"CHF": (3, 5, 3, 0), b"eur": (1, 1, 1, 3)},
            T: {b"eur": (3, 3, 1, 0), b"CHF": (2, 3, 2, 1)}}
    for flags in (V, V | T, T):
        ctx = m.createContext()
        src = Source([text] * 4)
        RunAny(ctx, *L.arrays())
        if flags & V:
            _values(ctx, src, flags=1)                                  # (SP_VALUE_RESULTS)
        if flags & T:
            src.gather(ctx, items=False)
        ctx.finishedTermsDevice(flags, _stream())
        out = ctx.finishedDictionaryDevice(_stream())
        mb, terms, got = _assert_dictionary(ctx, 2, out)
        assert np.diff(mb.doc_offsets.astype(np.int64)).tolist() == [1, 1, 3, 1] and not terms.status.any()
        assert np.all(mb.results[:, 0] == 1) and sorted((mb.result_format != 0).tolist()) == [False] * 3 + [True] * 3
        mv = ctx.finishedValuesFetch() if flags & V else None
        mt = ctx.finishedTextFetch() if flags & T else None
        found = {v: (df, c, mx, int(first)) for (h, v, df, c, mx), first in zip(got.entries(mb, terms, values=mv, text=mt), got.records[:, 2])}
        assert found == want[flags] and int(got.handle_terms[1]) == 2


# ---- 6. call order, buffers and streams
def test_call_order_second_batch_and_other_streams():
    torch = _torch()
    m = _bare(8)
    docs = _trip_docs()
    pieces, lex, seg, offs = _build(docs)
    ctx = m.createContext()
    src = Source(pieces)
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):              # before any batch
        ctx.finishedDictionaryDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedDictionaryFetch()
    with pytest.raises(spa.PatternError):
        ctx.lastDictionaryMs()
    run = Run(ctx, lex, seg, offs)
    src.gather(ctx, items=False)
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):              # finished, but no terms
        ctx.finishedDictionaryDevice(_stream())
    ctx.finishedTermsDevice(T, _stream())
    # an allocation that fails, then a normal call
    L = capi.lib()
    out = capi.SpMatchDictionaryDevice()
    L.sp_test_fail_alloc_above(1)
    try:
        assert L.sp_matcher_ctx_finished_dictionary_device(ctx._h, None, ctypes.byref(out)) == -2       # SP_ERR_NOMEM
    finally:
        L.sp_test_fail_alloc_above(0)
    assert not out.d_records
    with pytest.raises(spa.PatternError):
        ctx.finishedDictionaryFetch()
    first = ctx.finishedDictionaryDevice(_stream())
    mb, terms, got = _assert_dictionary(ctx, 9, first)
    assert ctx.lastDictionaryMs() >= 0.0
    # a stream other than the terms'; the text gathered on a third stream and not waited for
    other, third = torch.cuda.Stream(), torch.cuda.Stream()
    src.gather(ctx, stream=third.cuda_stream, items=False)
    ctx.finishedTermsDevice(T, _stream())
    with pytest.raises(spa.PatternError):                               # a new terms call: the dictionary is gone until it is rebuilt
        ctx.finishedDictionaryFetch()
    second = ctx.finishedDictionaryDevice(other.cuda_stream)
    assert second.d_records == first.d_records and second.d_term_dict == first.d_term_dict
    model.assert_same(_assert_dictionary(ctx, 9, second)[2], got)
    # a new finish: the old terms do not count
    run.match()
    ctx.batchFinishDevice(_stream())
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        ctx.finishedDictionaryDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedDictionaryFetch()
    # a second, smaller batch on the same context: the buffers stay where they are
    pieces, lex, seg, offs = _build(docs[:3])
    src = Source(pieces)
    Run(ctx, lex, seg, offs)
    src.gather(ctx, items=False)
    ctx.finishedTermsDevice(T, _stream())
    fourth = ctx.finishedDictionaryDevice(_stream())
    for field in ("d_records", "d_term_dict", "d_doc_dict_offsets", "d_handle_terms", "d_totals"):
        assert getattr(fourth, field) == getattr(first, field)
    mb, terms, got = _assert_dictionary(ctx, 9, fourth)
    assert len(terms.records) == 64 and len(got.records) == 63 and ctx.lastDictionaryMs() >= 0.0


# ---- 7. the order of the results
def test_plain_against_canonical_finish():
    docs = _trip_docs()
    found = []
    for canonical in (False, True):
        ctx, mb, terms, got = _go(docs, canonical=canonical)
        found.append(_by_term(ctx, mb, terms, got))
    assert found[0] == found[1] and len(found[0]) > 150


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
        ctx.finishedTermsDevice(T, _stream())
        out = ctx.finishedDictionaryDevice(_stream())
        got.append(_assert_dictionary(ctx, bound, out))
        # 8. the invariants against the frequency pass of the same finish
        ctx.finishedPatternFreqDevice(_stream())
        freq = ctx.finishedPatternFreqFetch()
        mb, terms, d = got[-1]
        assert not terms.status.any() and not freq.status.any()
        sums = np.zeros(bound, np.uint64)
        np.add.at(sums, d.records[:, 0], d.counts)
        assert np.array_equal(sums, freq.handle_results) and int(d.counts.sum()) == len(mb.results)
        assert np.array_equal(np.bincount(d.records[:, 0], minlength=bound), d.handle_terms)
    (mb_a, terms_a, a), (mb_b, terms_b, b) = got
    assert np.array_equal(mb_a.results, mb_b.results)
    assert len(a.records) < len(terms_a.records) < len(mb_a.results) and len(a.records) > 100
    for f in model.FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes()


# ---- 9. end to end
def test_segmented_documents_with_dictionary():
    from struspattern_amd import rulelang, segments
    docs = [b"He paid 3'645 Eur\n\nand 3'645 Eur again or 12 sFr. he paid", b"nothing", b"12 sFr. in the year 1984 something happened"]
    for extra, doc_freq in (([], 1), ([b"later 3'645 Eur were paid"], 2)):
        lx, m = spa.PatternLexerInstance(), spa.PatternMatcherInstance()
        rulelang.load(MONEY, lx, m)
        text, so, dso, _ = segments.segmented_batch(docs + extra)
        mb, mt, mv, terms, d = spa.matchSegmentedDocs(lx.createContext(), m.createContext(), text, so, dso, with_dictionary=True)
        assert not mb.status.any() and not terms.status.any() and len(d.records) > 0
        want = model.of_batch(mb, terms, m.handleBound(), mv, mt)
        model.assert_same(d, want)
        model.assert_same(spa.batchDictionary(mb, terms, values=mv, text=mt), want)
        model.check_invariants(d, terms, mb)
        found = {(m.patternName(h), v): (df, c) for h, v, df, c, _ in d.entries(mb, terms, values=mv, text=mt)}
        assert found[("MoneyAmount", b"EUR 3'645")] == (doc_freq, 1 + doc_freq) and found[("MoneyAmount", b"CHF 12")] == (2, 2)


def test_match_dictionary_listing(capsys):
    import json
    import os
    from struspattern_amd import match, rulelang
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "doc_example.json")) as f:
        case = json.load(f)
    prog, fn = os.path.join(here, "golden", "doc_example.rul"), os.path.join(here, "golden", "doc_example.txt")
    common = ["-p", prog, "-o", str(case["origin"]), "--device-values"]
    assert match.main(common + [fn, fn]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert plain[0] == "%s:" % fn and plain[1:5] == case["results"] and plain[-1] == "OK done"
    assert match.main(common + ["--dictionary", fn, fn]) == 0
    lines = capsys.readouterr().out.splitlines()
    n = len(plain) - 1
    assert lines[:n] == plain[:n] and lines[-1] == "OK done" and len(lines) > n + 1
    entries = lines[n:-1]
    assert all(line.startswith("dict ") and " docs 2 count " in line for line in entries)
    # the same lines by the model, from the batch, the values and the text of the results of the two copies
    lx, mt = spa.PatternLexerInstance(), spa.PatternMatcherInstance()
    rulelang.load(case["program"], lx, mt)
    with open(fn, "rb") as f:
        doc = f.read()
    offs = np.array([0, len(doc), 2 * len(doc)], np.uint64)
    lb = lx.createContext().matchDocs(doc + doc, offs)
    mctx = mt.createContext()
    mb = mctx.matchDocs(lb.lexems, lb.doc_offsets)
    mv = match.device_values(mctx, doc + doc, offs)
    mtext = spa.batchText(mb, doc + doc, offs, items=False)
    terms = spa.batchTerms(mb, values=mv, text=mtext, handle_bound=mt.handleBound(), flags=V | T)
    want = model.of_batch(mb, terms, mt.handleBound(), mv, mtext)
    expected = []
    for (h, size, d, t, df, mx, _, _), count in zip(want.records.tolist(), want.counts.tolist()):
        r = int(mb.doc_offsets[d]) + int(terms.doc(d)[t][4])
        value = mv.result(r) if mb.result_format is not None and int(mb.result_format[r]) else mtext.result(r)
        expected.append("dict %s '%s': docs %d count %d" % (mt.patternName(h), value.decode(), df, count))
    assert entries == expected and sum(int(line.rsplit(" ", 1)[1]) for line in entries) == len(mb.results) == 8
