"""Posting positions on the device (sp_matcher_ctx_finished_positions_device, csrc/l2_positions.h): the occurrences, posting
offsets, posting_positions and totals that the launches leave must EQUAL what the device-free twin (sp_match_batch_positions)
makes of the fetched batch, terms and postings, and the model (tests/positions_model.py); the device pointers of `out` hold
the same bytes.  Bare-term matchers over hand-made lexems as in tests/test_postings_gpu.py; here a test also chooses the
ordinal position of every lexem, so it decides every ordpos, the width of the position key and the length of every list."""
import ctypes

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from tests import positions_model as model
from tests.finished_support import (_bare, _from_device, Lexems, _matcher, MONEY, Run, RunAny, Source, _stream, T_LIT, T_SPAN, _torch, _trip_docs,
                                    TRIP_RECORDS, _values)

pytestmark = pytest.mark.gpu

V, T = spa.SP_TERM_VALUES, spa.SP_TERM_TEXT


def _build_at(docs):
    """docs: per document a list of (handle, value bytes, ordpos), the positions not descending: every occurrence gets its own
    copy of the value in the document's text -> pieces, lexems (n, 4), origseg, document offsets"""
    pieces, lex, offs = [], [], [0]
    for doc in docs:
        text = b""
        for h, value, pos in doc:
            lex.append([h, pos, len(text), len(value)])
            text += value
        pieces.append(text)
        offs.append(len(lex))
    return pieces, np.array(lex, np.uint32).reshape(-1, 4), np.zeros(len(lex), np.uint32), np.array(offs, np.uint64)


def _counted(docs):
    """(handle, value) documents at the positions 1, 2, .."""
    return [[(h, v, k + 1) for k, (h, v) in enumerate(doc)] for doc in docs]


def _assert_positions(ctx, out=None):
    """the fetched positions equal the twin's and the model's on the fetched batch, terms and postings, and so do the bytes
    behind the device pointers; returns (batch, terms, postings, positions)"""
    mb, terms = ctx.finishedFetch(), ctx.finishedTermsFetch()
    postings = ctx.finishedPostingsFetch()
    got = ctx.finishedPositionsFetch()
    want = model.of_batch(mb, terms, postings)
    model.assert_same(spa.batchPositions(mb, terms, postings), want)
    model.assert_same(got, want)
    model.check_invariants(got, mb, terms, postings)
    if out is not None:
        n, nocc = len(postings.records), len(got.occurrences)
        assert out.ndocs == len(terms.doc_offsets) - 1 and out.nterms == n and out.nocc == nocc
        assert _from_device(out.d_totals, 2, np.uint64).tolist() == got.totals.tolist() == [nocc, int(got.posting_positions.sum())]
        assert np.array_equal(_from_device(out.d_occurrences, 2 * nocc, np.uint32).reshape(-1, 2), got.occurrences)
        assert np.array_equal(_from_device(out.d_posting_offsets, n + 1, np.uint64), got.posting_offsets)
        assert np.array_equal(_from_device(out.d_posting_positions, n, np.uint32), got.posting_positions)
    return mb, terms, postings, got


def _products(ctx, flags=T):
    ctx.finishedTermsDevice(flags, _stream())
    ctx.finishedDictionaryDevice(_stream())
    ctx.finishedPostingsDevice(_stream())
    return ctx.finishedPositionsDevice(_stream())


def _go(docs, nhandles=8, canonical=False):
    """the positions of the text terms of hand-made documents: (context, batch, terms, postings, positions)"""
    m = _bare(nhandles)
    pieces, lex, seg, offs = _build_at(docs)
    ctx = m.createContext()
    src = Source(pieces)
    Run(ctx, lex, seg, offs, canonical=canonical)
    src.gather(ctx, items=False)
    out = _products(ctx)
    return (ctx,) + _assert_positions(ctx, out)


# ---- 1. empty shapes
def test_no_documents_empty_documents_and_a_single_document():
    m = _bare(8)
    ctx = m.createContext()
    src = Source([])
    Run(ctx, np.zeros((0, 4), np.uint32), np.zeros(0, np.uint32), np.zeros(1, np.uint64))
    src.gather(ctx, items=False)
    out = _products(ctx)
    mb, terms, postings, got = _assert_positions(ctx, out)
    assert got.occurrences.shape == (0, 2) and got.posting_offsets.tolist() == [0] and got.totals.tolist() == [0, 0]
    ctx, mb, terms, postings, got = _go([[], [], []])
    assert got.occurrences.shape == (0, 2) and got.posting_offsets.tolist() == [0] and got.totals.tolist() == [0, 0]
    # one document: (2,"b") three times, the others once
    doc = [(2, b"b", 1), (1, b"a", 2), (2, b"b", 3), (2, b"", 4), (3, b"a", 5), (2, b"b", 9)]
    ctx, mb, terms, postings, got = _go([doc])
    assert postings.records[:, 2].tolist() == [1, 3, 1, 1]
    assert got.posting_offsets.tolist() == [0, 1, 4, 5, 6] and got.posting_positions.tolist() == [1, 3, 1, 1]
    assert got.occurrences.tolist() == [[2, 1], [1, 0], [3, 2], [9, 5], [4, 3], [5, 4]]
    assert got.positions(1).tolist() == [1, 3, 9] and ctx.lastPositionsMs() >= 0.0


# ---- 2. the width of the position key: no pass, one bit, a full byte, a second and a third pass
@pytest.mark.parametrize("largest", [0, 1, 255, 256, 65535, 65536])
def test_position_key_width(largest):
    low = min(largest, 1)
    docs = [[(1, b"a", 0), (2, b"b", 0), (1, b"a", low), (1, b"a", largest), (2, b"b", largest)],
            [(1, b"a", low), (3, b"c", largest), (1, b"a", largest)]]
    ctx, mb, terms, postings, got = _go(docs)
    assert int(mb.results[:, 1].max()) == largest and len(got.occurrences) == 8
    assert got.posting(0)[:, 0].tolist() == [0, low, largest] and got.posting(1)[:, 0].tolist() == [low, largest]
    assert got.posting(2)[:, 0].tolist() == [0, largest]
    if largest == 0:
        assert got.posting_positions.tolist() == [1] * len(postings.records)
    else:
        assert got.posting_positions.tolist() == [len(set(got.posting(p)[:, 0].tolist())) for p in range(len(postings.records))]


# ---- 3. tile edges of the occurrences
def _result_docs(n):
    """documents of at most 257 results, n in all: a third of the results of a document are terms that every document of its
    size has, twice each, the others occur once"""
    docs, fresh = [], 0
    while n:
        size = min(n, 257)
        doc = [(1 + (k // 2) % 7, b"s%04d" % (k // 2)) for k in range(size // 3)]
        while len(doc) < size:
            doc.append((1 + fresh % 7, b"u%06d" % fresh))
            fresh += 1
        docs.append(doc)
        n -= size
    return docs


@pytest.mark.parametrize("edge", ["tile-1", "tile", "tile+1", "2*tile+1"])
def test_tile_edges_with_a_third_of_the_terms_shared(edge):
    tile = capi.lib().sp_matcher_positions_tile()
    n = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2*tile+1": 2 * tile + 1}[edge]
    docs = _result_docs(n)
    ctx, mb, terms, postings, got = _go(_counted(docs))
    assert len(got.occurrences) == n == len(mb.results) and len(postings.records) < n
    assert int(postings.records[:, 2].max()) == 2 and len(docs) > 1


# ---- 4. one list longer than a tile, beside lists of length 1
def test_a_list_longer_than_a_tile_beside_lists_of_one():
    tile = capi.lib().sp_matcher_positions_tile()
    long = [(1, b"x") if k % 5 else (2, b"y%05d" % k) for k in range((tile + 40) * 5 // 4)]
    docs = [[(3, b"one%04d" % k)] for k in range(70)] + [long] + [[(4, b"z%04d" % k), (1, b"x")] for k in range(70)]
    ctx, mb, terms, postings, got = _go(_counted(docs))
    counts = postings.records[:, 2]
    p = int(np.argmax(counts))
    assert int(counts[p]) > tile and int(postings.records[p, 0]) == 70
    assert int(np.count_nonzero(counts == 1)) == len(counts) - 1
    assert np.array_equal(got.posting(p)[:, 0], np.array([k + 1 for k in range(len(long)) if k % 5], np.uint32))
    assert int(got.posting_positions[p]) == int(counts[p])


# ---- 5. the digit width changes nothing
def test_digit_bits_leave_identical_bytes():
    docs = _counted(_trip_docs())
    L = capi.lib()
    fields, parities = [], [set(), set()]
    try:
        for bits in range(1, 9):
            L.sp_test_postings_digit_bits(bits)
            ctx, mb, terms, postings, got = _go(docs)
            widths = (int(mb.results[:, 1].max()).bit_length(), (len(postings.records) - 1).bit_length())
            for group in range(2):
                parities[group].add(((widths[group] + bits - 1) // bits) & 1)
            fields.append([getattr(got, f).tobytes() for f in model.FIELDS])
    finally:
        L.sp_test_postings_digit_bits(8)
    assert len(mb.results) > sum(TRIP_RECORDS) and all(f == fields[0] for f in fields)
    assert parities == [{0, 1}, {0, 1}]                                 # both ends of the ping-pong, in both groups


# ---- 6. a plain finish leaves the results out of position order
def _twice():
    """the pattern W twice with the constant value "w": the bare term 1, and the sequence of the terms 2 and 3, which fires at
    its last term and starts at its first"""
    m = spa.PatternMatcherInstance()
    m.pushTerm(1); m.pushExpression("any", 1, 1, 0); m.definePattern("W", "w", True)
    m.pushTerm(2); m.pushTerm(3); m.pushExpression("sequence", 2, 8, 0); m.definePattern("W", "w", True)
    m.compile()
    return m


def test_plain_finish_out_of_position_order():
    m = _twice()
    # term, ordpos: the sequences start at 1 and at 10, fire at 6 and at 12, behind the bare terms at 1, 3, 4 and 11
    doc = [(2, 1), (1, 1), (1, 3), (1, 4), (3, 6), (2, 10), (1, 11), (3, 12)]
    docs = [doc, [(1, 2)], doc[:5]]
    lex, offs = [], [0]
    for d in docs:
        lex += [[t, p, 2 * k, 1] for k, (t, p) in enumerate(d)]
        offs.append(len(lex))
    lex, offs = np.array(lex, np.uint32).reshape(-1, 4), np.array(offs, np.uint64)
    pieces = [b"ab" * len(d) for d in docs]
    found = []
    for canonical in (False, True):
        ctx = m.createContext()
        src = Source(pieces)
        Run(ctx, lex, np.zeros(len(lex), np.uint32), offs, canonical=canonical)
        _values(ctx, src, flags=1)                                      # (SP_VALUE_RESULTS)
        out = _products(ctx, V)
        found.append(_assert_positions(ctx, out))
    (mb, terms, postings, plain), (cmb, cterms, cpostings, canon) = found
    first = mb.results[int(mb.doc_offsets[0]):int(mb.doc_offsets[1]), 1].astype(np.int64)
    assert len(first) == 6 and np.any(np.diff(first) < 0)               # the plain finish is in firing order, not in position order
    assert len(postings.records) == 3 and postings.records[:, 2].tolist() == [6, 1, 4]   # one term, "W" with the value "w", per document
    for q in (plain, canon):
        assert q.posting(0)[:, 0].tolist() == [1, 1, 3, 4, 10, 11] and q.posting(2)[:, 0].tolist() == [1, 1, 3, 4]
    # the ordpos words and posting_positions are those after a canonical finish; `result` follows the finished order
    assert np.array_equal(plain.occurrences[:, 0], canon.occurrences[:, 0])
    assert np.array_equal(plain.posting_positions, canon.posting_positions) and plain.totals.tolist() == canon.totals.tolist()
    assert np.array_equal(plain.posting_offsets, canon.posting_offsets)
    # the bare term and the sequence at position 1 end at different tokens: one position, two results
    ends = [int(mb.results[int(mb.doc_offsets[0]) + r, 2]) for _, r in plain.posting(0)[:2].tolist()]
    assert ends[0] != ends[1] and plain.posting_positions.tolist() == [5, 1, 3]
    assert int(plain.posting_positions[0]) < int(postings.records[0, 2])


# ---- 7. a failed document
def test_a_document_whose_values_fail_has_no_occurrences():
    m = _matcher()
    text = b"eur usd eur chf usd eur ab cd ab cd CHF"

    def lexems(middle_fails):
        L = Lexems()
        for pos in (0, 4, 8):
            L.add(T_SPAN, pos, 3).gap()
        L.add(T_LIT, 0, 3).doc()
        if middle_fails:
            L.add(T_SPAN, 50, 3).add(T_SPAN, 0, 3).add(T_LIT, 0, 3).doc()   # a span outside the text: the values of the document fail
        else:
            L.doc()
        L.add(T_SPAN, 4, 3).gap().add(T_SPAN, 0, 3).gap().add(T_SPAN, 4, 3).doc()
        return L.arrays()

    found = []
    for middle_fails in (True, False):
        ctx = m.createContext()
        src = Source([text] * 3)
        RunAny(ctx, *lexems(middle_fails))
        _values(ctx, src, flags=1)
        out = _products(ctx, V)
        found.append(_assert_positions(ctx, out))
    (mb, terms, postings, got), (_, _, neighbours, want) = found
    assert terms.status.tolist() == [0, 5, 0] and len(mb.doc(1)) == 3 and np.all(terms.result_term[4:7] == 0xFFFFFFFF)
    assert not np.any(postings.records[:, 0] == 1) and len(got.occurrences) == len(mb.results) - 3 == 7
    # the neighbours are what they are without the failed document between them
    assert np.array_equal(postings.records, neighbours.records)
    for f in model.FIELDS:
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes()


# ---- 8. call order, buffers and streams
def test_call_order_second_batch_and_other_streams():
    torch = _torch()
    m = _bare(8)
    docs = _counted(_trip_docs())
    pieces, lex, seg, offs = _build_at(docs)
    ctx = m.createContext()
    src = Source(pieces)
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):              # before any batch
        ctx.finishedPositionsDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedPositionsFetch()
    with pytest.raises(spa.PatternError):
        ctx.lastPositionsMs()
    run = Run(ctx, lex, seg, offs)
    src.gather(ctx, items=False)
    ctx.finishedTermsDevice(T, _stream())
    ctx.finishedDictionaryDevice(_stream())
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):              # a dictionary, but no postings
        ctx.finishedPositionsDevice(_stream())
    ctx.finishedPostingsDevice(_stream())
    # an allocation that fails, then a normal call
    L = capi.lib()
    out = capi.SpMatchPositionsDevice()
    L.sp_test_fail_alloc_above(1)
    try:
        assert L.sp_matcher_ctx_finished_positions_device(ctx._h, None, ctypes.byref(out)) == -2      # SP_ERR_NOMEM
    finally:
        L.sp_test_fail_alloc_above(0)
    assert not out.d_occurrences and out.nocc == 0 and out.nterms == 0
    with pytest.raises(spa.PatternError):
        ctx.finishedPositionsFetch()
    first = ctx.finishedPositionsDevice(_stream())
    mb, terms, postings, got = _assert_positions(ctx, first)
    assert ctx.lastPositionsMs() >= 0.0
    # a new postings call invalidates the fetch; a stream other than the postings', which are not waited for
    ctx.finishedPostingsDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedPositionsFetch()
    other = torch.cuda.Stream()
    second = ctx.finishedPositionsDevice(other.cuda_stream)
    assert second.d_occurrences == first.d_occurrences and second.d_posting_positions == first.d_posting_positions
    model.assert_same(_assert_positions(ctx, second)[3], got)
    # postings on another stream, the positions on the first one
    ctx.finishedPostingsDevice(other.cuda_stream)
    model.assert_same(_assert_positions(ctx, ctx.finishedPositionsDevice(_stream()))[3], got)
    # a new dictionary call, a new terms call: the postings do not count, nor do the positions
    for again in ("dictionary", "terms"):
        if again == "terms":
            ctx.finishedTermsDevice(T, _stream())
        ctx.finishedDictionaryDevice(_stream())
        with pytest.raises(spa.PatternError):
            ctx.finishedPositionsFetch()
        with pytest.raises(spa.PatternError, match=r"\(-1\)"):
            ctx.finishedPositionsDevice(_stream())
        ctx.finishedPostingsDevice(_stream())
        model.assert_same(_assert_positions(ctx, ctx.finishedPositionsDevice(_stream()))[3], got)
    # a new finish: the old postings do not count
    run.match()
    ctx.batchFinishDevice(_stream())
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        ctx.finishedPositionsDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedPositionsFetch()
    # a second, smaller batch on the same context: the buffers stay where they are
    pieces, lex, seg, offs = _build_at(docs[:3])
    src = Source(pieces)
    Run(ctx, lex, seg, offs)
    src.gather(ctx, items=False)
    fourth = _products(ctx)
    for field in ("d_occurrences", "d_posting_offsets", "d_posting_positions", "d_totals"):
        assert getattr(fourth, field) == getattr(first, field)
    mb, terms, postings, got = _assert_positions(ctx, fourth)
    assert len(terms.records) == 64 and len(got.occurrences) == len(mb.results) > 64 and ctx.lastPositionsMs() >= 0.0


# ---- 9. the engines
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
        out = _products(ctx)
        got.append(_assert_positions(ctx, out))
    (mb, terms, postings, a), (_, _, _, b) = got
    assert len(a.occurrences) == len(mb.results) > len(postings.records) > 100
    for f in model.FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes()


# ---- 10. end to end
def test_segmented_documents_with_positions():
    from struspattern_amd import rulelang, segments
    docs = [b"He paid 3'645 Eur\n\nand 3'645 Eur again or 12 sFr. he paid", b"nothing", b"12 sFr. in the year 1984 something happened",
            b"later 3'645 Eur were paid"]
    lx, m = spa.PatternLexerInstance(), spa.PatternMatcherInstance()
    rulelang.load(MONEY, lx, m)
    text, so, dso, _ = segments.segmented_batch(docs)
    mb, mt, mv, terms, d, p, q = spa.matchSegmentedDocs(lx.createContext(), m.createContext(), text, so, dso, with_positions=True)
    assert not mb.status.any() and not terms.status.any() and len(d.records) > 0
    want = model.of_batch(mb, terms, p)
    model.assert_same(q, want)
    model.assert_same(spa.batchPositions(mb, terms, p), want)
    model.check_invariants(q, mb, terms, p)
    found = {(m.patternName(h), v): [(int(p.entry(e)[k, 0]), q.positions(int(p.entry_offsets[e]) + k).tolist()) for k in range(len(p.entry(e)))]
             for e, (h, v, _, _, _) in enumerate(d.entries(mb, terms, values=mv, text=mt))}
    eur = found[("MoneyAmount", b"EUR 3'645")]
    assert [doc for doc, _ in eur] == [0, 3] and len(eur[0][1]) == 2 and len(eur[1][1]) == 1 and eur[0][1][0] < eur[0][1][1]


def test_match_positions_listing(capsys):
    import json
    import os
    import re
    from struspattern_amd import match
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "doc_example.json")) as f:
        case = json.load(f)
    prog, fn = os.path.join(here, "golden", "doc_example.rul"), os.path.join(here, "golden", "doc_example.txt")
    common = ["-p", prog, "-o", str(case["origin"]), "--device-values"]
    assert match.main(common + ["--postings", fn, fn]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert match.main(common + ["--positions", fn, fn]) == 0            # (implies --postings)
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == len(plain) and lines[-1] == "OK done"
    posts = 0
    for a, b in zip(plain, lines):
        if not a.startswith("post "):
            assert a == b
            continue
        posts += 1
        assert re.sub(r"\[[0-9,]*\]", "", b) == a                        # the posting line with the positions behind every file
        for cell in b[b.rindex("': ") + 3:].split(" "):
            count, first, positions = re.fullmatch(r"\d+:(\d+)@(\d+)\[([0-9,]+)\]", cell).groups()
            positions = [int(x) for x in positions.split(",")]
            assert positions == sorted(set(positions)) and positions[0] == int(first) and 1 <= len(positions) <= int(count)
    assert posts > 0
