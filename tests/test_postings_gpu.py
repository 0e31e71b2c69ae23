"""Batch postings on the device (sp_matcher_ctx_finished_postings_device, csrc/l2_postings.h): the postings, entry offsets,
record_posting and total that the launches leave must EQUAL what the device-free twin (sp_match_batch_postings) makes of the
fetched terms and dictionary, and the model (tests/postings_model.py); the device pointers of `out` hold the same bytes.
Bare-term matchers over hand-made lexems as in tests/test_dictionary_gpu.py: with SP_TERM_TEXT a test sets every handle and
value itself, so it decides the number of term records N, of entries ndict, and which documents share a term."""
import ctypes

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from tests import postings_model as model
from tests.finished_support import (_bare, _build, EVERY, _from_device, Lexems, _matcher, MONEY, Run, RunAny, Source, _stream, T_LIT, T_PLAIN_A,
                                    T_PLAIN_B, T_SPAN, _torch, _trip_docs, TRIP_RECORDS, _values)

pytestmark = pytest.mark.gpu

V, T = spa.SP_TERM_VALUES, spa.SP_TERM_TEXT


def _assert_postings(ctx, out=None):
    """the fetched postings equal the twin's and the model's on the fetched terms and dictionary, and so do the bytes behind
    the device pointers; returns (terms, dictionary, postings)"""
    terms = ctx.finishedTermsFetch()
    d = ctx.finishedDictionaryFetch()
    got = ctx.finishedPostingsFetch()
    want = model.of_batch(terms, d)
    model.assert_same(spa.batchPostings(terms, d), want)
    model.assert_same(got, want)
    model.check_invariants(got, terms, d)
    if out is not None:
        n, ndict = len(terms.records), len(d.records)
        assert out.ndocs == len(terms.doc_offsets) - 1 and out.nterms == n and out.ndict == ndict
        assert int(_from_device(out.d_totals, 1, np.uint64)[0]) == n
        assert np.array_equal(_from_device(out.d_postings, 4 * n, np.uint32).reshape(-1, 4), got.records)
        assert np.array_equal(_from_device(out.d_entry_offsets, ndict + 1, np.uint64), got.entry_offsets)
        assert np.array_equal(_from_device(out.d_record_posting, n, np.uint32), got.record_posting)
    return terms, d, got


def _go(docs, nhandles=8, canonical=False):
    """the postings of the text terms of hand-made documents: (context, terms, dictionary, postings)"""
    m = _bare(nhandles)
    pieces, lex, seg, offs = _build(docs)
    ctx = m.createContext()
    src = Source(pieces)
    Run(ctx, lex, seg, offs, canonical=canonical)
    src.gather(ctx, items=False)
    ctx.finishedTermsDevice(T, _stream())
    ctx.finishedDictionaryDevice(_stream())
    out = ctx.finishedPostingsDevice(_stream())
    terms, d, got = _assert_postings(ctx, out)
    return ctx, terms, d, got


def _lists(ctx, terms, d, got):
    """(handle, value) -> [(doc, count, first_ordpos)], the list of every entry"""
    mb, mt = ctx.finishedFetch(), ctx.finishedTextFetch()
    return {(h, v): [(doc, count, first) for doc, _, count, first in got.entry(e).tolist()]
            for e, (h, v, _, _, _) in enumerate(d.entries(mb, terms, text=mt))}


def _term(k):
    return (1 + k % 7, b"t%06d" % k)


# ---- 1. empty shapes
def test_no_documents_empty_documents_and_a_single_document():
    m = _bare(8)
    ctx = m.createContext()
    src = Source([])
    Run(ctx, np.zeros((0, 4), np.uint32), np.zeros(0, np.uint32), np.zeros(1, np.uint64))
    src.gather(ctx, items=False)
    ctx.finishedTermsDevice(T, _stream())
    ctx.finishedDictionaryDevice(_stream())
    out = ctx.finishedPostingsDevice(_stream())
    terms, d, got = _assert_postings(ctx, out)
    assert got.records.shape == (0, 4) and got.entry_offsets.tolist() == [0] and len(got.record_posting) == 0
    ctx, terms, d, got = _go([[], [], []])
    assert got.records.shape == (0, 4) and got.entry_offsets.tolist() == [0] and len(got.record_posting) == 0
    # one document: ndict = N and the postings are the identity
    doc = [(2, b"b"), (1, b"a"), (2, b"b"), (2, b""), (3, b"a"), (2, b"b")]
    ctx, terms, d, got = _go([doc])
    assert len(d.records) == len(terms.records) == 4
    assert got.record_posting.tolist() == [0, 1, 2, 3] and got.entry_offsets.tolist() == [0, 1, 2, 3, 4]
    assert got.records[:, :3].tolist() == [[0, 0, 1], [0, 1, 3], [0, 2, 1], [0, 3, 1]]
    assert ctx.lastPostingsMs() >= 0.0


# ---- 2. key width edges: no pass, one pass of one bit, a full byte, a second pass of one bit
@pytest.mark.parametrize("ndict", [1, 2, 256, 257])
def test_key_width_edges(ndict):
    first = [_term(k) for k in range(ndict)]
    again = first[::2][::-1]                                            # every second term once more, the other way round
    ctx, terms, d, got = _go([first, again, first[-1:]])
    assert len(d.records) == ndict and len(terms.records) == ndict + len(again) + 1
    lists = _lists(ctx, terms, d, got)
    for k, key in enumerate(first):
        docs = [0] + ([1] if k % 2 == 0 else []) + ([2] if k == ndict - 1 else [])
        assert [doc for doc, _, _ in lists[key]] == docs, k


# ---- 3. tile edges
def _tile_docs(n):
    """documents of at most 257 term records, n in all: a third of the terms of a document are those of every document of its
    size, the others occur once"""
    docs, fresh = [], 0
    while n:
        size = min(n, 257)
        doc = [(1 + k % 7, b"s%04d" % k) for k in range(size // 3)]
        while len(doc) < size:
            doc.append((1 + fresh % 7, b"u%06d" % fresh))
            fresh += 1
        docs.append(doc)
        n -= size
    return docs


@pytest.mark.parametrize("edge", ["tile-1", "tile", "tile+1", "2*tile+1"])
def test_tile_edges_with_a_third_of_the_terms_repeated(edge):
    tile = capi.lib().sp_matcher_postings_tile()
    n = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2*tile+1": 2 * tile + 1}[edge]
    docs = _tile_docs(n)
    ctx, terms, d, got = _go(docs)
    assert len(terms.records) == n and len(d.records) < n - n // 4
    assert int(d.records[:, 4].max()) == len(docs) > 1                  # the shared terms
    assert got.docs(0).tolist() == list(range(len(docs)))               # (1, "s0000") is in every document


# ---- 4. a list longer than a tile, with skew
def test_a_list_longer_than_a_tile_and_a_list_that_spans_the_records():
    tile = capi.lib().sp_matcher_postings_tile()
    ndocs = tile + 1
    span = (3, b"first and last")
    docs = [[EVERY] + ([_term(k)] if k % 3 else []) for k in range(ndocs)]
    docs[0].append(span)
    docs[-1].append(span)
    ctx, terms, d, got = _go(docs)
    lists = _lists(ctx, terms, d, got)
    assert [doc for doc, _, _ in lists[EVERY]] == list(range(ndocs)) and len(lists[EVERY]) > tile
    assert [doc for doc, _, _ in lists[span]] == [0, ndocs - 1]
    assert all([p[:2] for p in lists[_term(k)]] == [(k, 1)] for k in range(ndocs) if k % 3)
    assert len(terms.records) == ndocs + len([k for k in range(ndocs) if k % 3]) + 2 > tile


# ---- 5. the digit width changes nothing
def test_digit_bits_leave_identical_bytes():
    docs = _trip_docs()
    L = capi.lib()
    fields = []
    try:
        for bits in (1, 3, 8):
            L.sp_test_postings_digit_bits(bits)
            ctx, terms, d, got = _go(docs)
            assert len(terms.records) == sum(TRIP_RECORDS) and len(d.records) > 128        # eight passes of one bit or more, three of three
            fields.append([getattr(got, f).tobytes() for f in model.FIELDS])
    finally:
        L.sp_test_postings_digit_bits(8)
    assert fields[0] == fields[1] == fields[2] and len(fields[2][0]) == 16 * sum(TRIP_RECORDS)


# ---- 6. failed documents
def test_a_document_whose_values_fail_has_no_posting():
    m = _matcher()
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
        ctx.finishedDictionaryDevice(_stream())
        out = ctx.finishedPostingsDevice(_stream())
        terms, d, got = _assert_postings(ctx, out)
        assert terms.status.tolist() == [0, 0, 5, 0] and len(terms.doc(2)) == 0
        assert not np.any(got.records[:, 0] == 2) and sorted(set(got.records[:, 0].tolist())) == [0, 1, 3]
        mb, mv = ctx.finishedFetch(), ctx.finishedValuesFetch()
        mt = ctx.finishedTextFetch() if flags & T else None
        found = {(m.patternName(h), v): got.docs(e).tolist() for e, (h, v, _, _, _) in enumerate(d.entries(mb, terms, values=mv, text=mt))}
        plain = b"" if flags == V else b"ab cd"
        assert found == {("Span", b"eur"): [0, 3], ("Span", b"usd"): [0, 1], ("Lit", b"CHF"): [0, 3], ("Plain", plain): [0, 3], ("Span", b"CHF"): [1]}


# ---- 7. call order, buffers and streams
def test_call_order_second_batch_and_other_streams():
    torch = _torch()
    m = _bare(8)
    docs = _trip_docs()
    pieces, lex, seg, offs = _build(docs)
    ctx = m.createContext()
    src = Source(pieces)
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):              # before any batch
        ctx.finishedPostingsDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedPostingsFetch()
    with pytest.raises(spa.PatternError):
        ctx.lastPostingsMs()
    run = Run(ctx, lex, seg, offs)
    src.gather(ctx, items=False)
    ctx.finishedTermsDevice(T, _stream())
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):              # terms, but no dictionary
        ctx.finishedPostingsDevice(_stream())
    ctx.finishedDictionaryDevice(_stream())
    # an allocation that fails, then a normal call
    L = capi.lib()
    out = capi.SpMatchPostingsDevice()
    L.sp_test_fail_alloc_above(1)
    try:
        assert L.sp_matcher_ctx_finished_postings_device(ctx._h, None, ctypes.byref(out)) == -2       # SP_ERR_NOMEM
    finally:
        L.sp_test_fail_alloc_above(0)
    assert not out.d_postings and out.nterms == 0
    with pytest.raises(spa.PatternError):
        ctx.finishedPostingsFetch()
    first = ctx.finishedPostingsDevice(_stream())
    terms, d, got = _assert_postings(ctx, first)
    assert ctx.lastPostingsMs() >= 0.0
    # a new dictionary call invalidates the fetch; a stream other than the dictionary's, which is not waited for
    ctx.finishedDictionaryDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedPostingsFetch()
    other = torch.cuda.Stream()
    second = ctx.finishedPostingsDevice(other.cuda_stream)
    assert second.d_postings == first.d_postings and second.d_record_posting == first.d_record_posting
    model.assert_same(_assert_postings(ctx, second)[2], got)
    # a new terms call: neither the dictionary nor the postings count
    ctx.finishedTermsDevice(T, _stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedPostingsFetch()
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        ctx.finishedPostingsDevice(_stream())
    # a new finish: the old dictionary does not count
    ctx.finishedDictionaryDevice(_stream())
    ctx.finishedPostingsDevice(_stream())
    run.match()
    ctx.batchFinishDevice(_stream())
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        ctx.finishedPostingsDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedPostingsFetch()
    # a second, smaller batch on the same context: the buffers stay where they are
    pieces, lex, seg, offs = _build(docs[:3])
    src = Source(pieces)
    Run(ctx, lex, seg, offs)
    src.gather(ctx, items=False)
    ctx.finishedTermsDevice(T, _stream())
    ctx.finishedDictionaryDevice(_stream())
    fourth = ctx.finishedPostingsDevice(_stream())
    for field in ("d_postings", "d_entry_offsets", "d_record_posting", "d_totals"):
        assert getattr(fourth, field) == getattr(first, field)
    terms, d, got = _assert_postings(ctx, fourth)
    assert len(terms.records) == 64 and len(d.records) == 63 and ctx.lastPostingsMs() >= 0.0


# ---- 8. the order of the results
def test_plain_against_canonical_finish():
    docs = _trip_docs()
    found = []
    for canonical in (False, True):
        ctx, terms, d, got = _go(docs, canonical=canonical)
        found.append(_lists(ctx, terms, d, got))
    assert found[0] == found[1] and len(found[0]) > 150
    assert [doc for doc, _, _ in found[0][EVERY]] == [1, 2, 3, 4, 5, 6]


def test_exact_engine_against_result_set_mode_after_a_canonical_finish():
    from struspattern_amd import synth
    rules = synth.random_rules(400, 30, 2)
    lex, offs = synth.random_documents(24, 500, 30, 102)
    m = spa.PatternMatcherInstance()
    synth.apply_rules(m, rules)
    assert m.resultSetTier()[0]
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
        ctx.finishedDictionaryDevice(_stream())
        out = ctx.finishedPostingsDevice(_stream())
        got.append(_assert_postings(ctx, out))
    (terms_a, da, a), (terms_b, db, b) = got
    assert 100 < len(da.records) < len(terms_a.records) and int(da.records[:, 4].max()) > 1
    for f in model.FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes()


# ---- 9. end to end
def test_segmented_documents_with_postings():
    from struspattern_amd import rulelang, segments
    docs = [b"He paid 3'645 Eur\n\nand 3'645 Eur again or 12 sFr. he paid", b"nothing", b"12 sFr. in the year 1984 something happened",
            b"later 3'645 Eur were paid"]
    lx, m = spa.PatternLexerInstance(), spa.PatternMatcherInstance()
    rulelang.load(MONEY, lx, m)
    text, so, dso, _ = segments.segmented_batch(docs)
    mb, mt, mv, terms, d, p = spa.matchSegmentedDocs(lx.createContext(), m.createContext(), text, so, dso, with_postings=True)
    assert not mb.status.any() and not terms.status.any() and len(d.records) > 0
    want = model.of_batch(terms, d)
    model.assert_same(p, want)
    model.assert_same(spa.batchPostings(terms, d), want)
    model.check_invariants(p, terms, d)
    found = {(m.patternName(h), v): (p.docs(e).tolist(), p.entry(e)[:, 2].tolist()) for e, (h, v, _, _, _) in enumerate(d.entries(mb, terms, values=mv, text=mt))}
    assert found[("MoneyAmount", b"EUR 3'645")] == ([0, 3], [2, 1]) and found[("MoneyAmount", b"CHF 12")] == ([0, 2], [1, 1])
    assert not any(1 in docs_of for docs_of, _ in found.values())


def test_match_postings_listing(capsys):
    import json
    import os
    from struspattern_amd import match
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "doc_example.json")) as f:
        case = json.load(f)
    prog, fn = os.path.join(here, "golden", "doc_example.rul"), os.path.join(here, "golden", "doc_example.txt")
    common = ["-p", prog, "-o", str(case["origin"]), "--device-values"]
    assert match.main(common + ["--dictionary", fn, fn]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert match.main(common + ["--postings", fn, fn]) == 0             # (implies --dictionary)
    lines = capsys.readouterr().out.splitlines()
    n = len(plain) - 1
    assert lines[:n] == plain[:n] and lines[-1] == "OK done"
    entries = [line for line in plain if line.startswith("dict ")]
    posts = lines[n:-1]
    assert len(posts) == len(entries) > 0
    total = 0
    for entry, post in zip(entries, posts):
        name = entry[len("dict "):entry.rindex("': docs ") + 1]          # NAME 'VALUE'
        assert post.startswith("post " + name + ": ")
        cells = post[len("post " + name + ": "):].split(" ")
        assert [c.split(":")[0] for c in cells] == ["0", "1"]           # both files, in the order given
        counts = [int(c.split(":")[1].split("@")[0]) for c in cells]
        assert counts[0] == counts[1] and cells[0].split("@")[1] == cells[1].split("@")[1]
        assert sum(counts) == int(entry.rsplit(" ", 1)[1])
        total += sum(counts)
    assert total == 2 * len(case["results"]) == 8
