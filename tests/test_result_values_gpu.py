"""Result values on the device (sp_matcher_ctx_finished_values_device, csrc/l2_values.h): the bytes, offsets, statuses and
totals that the value passes leave must EQUAL what the device-free twin (sp_match_batch_values) makes of the fetched finished
batch.  The harness is that of tests/test_span_text_gpu.py: hand-made lexems and a hand-made origseg through small rules, so
that a test sets every span itself; 64 bytes of 0xFF stand behind the text on the device and no value may hold one."""
import ctypes
import os

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi, rulelang, segments
from tests import result_values_model as model
from tests.finished_support import (_ctx, _from_device, Lexems, _matcher, MONEY, _pairs, _random_text, Run, RunAny, Source, _stream, T_EV, T_J1,
                                    T_J2, T_J3, T_LIT, T_NONE, T_PLAIN_A, T_PLAIN_B, T_SPAN, T_X1, T_X2, T_YEAR, TEXT, _torch, _values)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BOTH = model.SP_VALUE_RESULTS | model.SP_VALUE_ITEMS
RANGE = model.SP_DOC_ERR_RANGE


def _assert_values(m, ctx, src, out=None, flags=BOTH):
    """the fetched values batch equals the twin's on the fetched finished batch; returns (batch, values)"""
    mb = ctx.finishedFetch()
    got = ctx.finishedValuesFetch()
    twin = spa.batchValues(m, mb, src.text, src.so, src.dso, flags=flags)
    assert np.array_equal(got.status, twin.status)
    for fam, bit in (("result", 1), ("item", 2)):
        g_values, g_offs = getattr(got, fam + "_values"), getattr(got, fam + "_offsets")
        if not flags & bit:
            assert g_values is None and g_offs is None and getattr(twin, fam + "_values") is None
            continue
        assert np.array_equal(g_offs, getattr(twin, fam + "_offsets"))
        assert g_values == getattr(twin, fam + "_values")
        assert b"\xff" not in g_values
    if out is not None:
        totals = _from_device(out.d_totals, 2, np.uint64)
        assert int(totals[0]) == (len(got.result_values) if flags & 1 else 0) and int(totals[1]) == (len(got.item_values) if flags & 2 else 0)
        assert np.array_equal(_from_device(out.d_doc_value_status, out.ndocs, np.int32), got.status)
        assert bool(out.d_result_values) == bool(flags & 1) and bool(out.d_result_value_offsets) == bool(flags & 1)
        assert bool(out.d_item_values) == bool(flags & 2) and bool(out.d_item_value_offsets) == bool(flags & 2)
        if flags & 1:
            assert np.array_equal(_from_device(out.d_result_value_offsets, len(mb.results) + 1, np.uint64), got.result_offsets)
    return mb, got


def _doc_values(m, mb, got, d):
    """the (pattern name, value) pairs of document d, sorted"""
    return sorted((m.patternName(int(mb.results[r][0])), got.result(r)) for r in range(int(mb.doc_offsets[d]), int(mb.doc_offsets[d + 1])))


def _go(L, pieces, dso=None, key="rules", flags=BOTH, canonical=False, result_sets=False):
    m = _matcher(key)
    ctx = m.createContext(result_sets=result_sets)
    src = Source(pieces, doc_seg_offsets=dso)
    RunAny(ctx, *L.arrays(), canonical=canonical)
    out = _values(ctx, src, flags)
    mb, got = _assert_values(m, ctx, src, out, flags)
    return m, ctx, src, mb, got


# ---- 1. batch shapes
def test_batch_shapes():
    rng = np.random.default_rng(1)
    m = _matcher()
    ctx, src = m.createContext(), Source([])                                            # no documents
    ctx.matchDocs(np.zeros((0, 4), np.uint32), np.zeros(1, np.uint64))
    ctx.batchFinishDevice(_stream())
    mb, got = _assert_values(m, ctx, src, _values(ctx, src))
    assert len(mb.results) == 0 and got.result_values == b"" and list(got.result_offsets) == [0]
    text = _random_text(rng, 30)
    m, ctx, src, mb, got = _go(Lexems().add(T_SPAN, 3, 5).doc(), [text])                # one document, one result
    assert _doc_values(m, mb, got, 0) == [("Span", text[3:8])] and not got.status.any()
    # a document without results, and one that the matcher fails (lexems out of order) between two good ones
    L = Lexems().add(T_SPAN, 0, 4).doc().add(99, 0, 1).doc().add(T_LIT, 0, 1).doc()
    L.gap().add(T_SPAN, 0, 2); L.lex.append([T_SPAN, 1, 2, 2]); L.seg.append(0); L.doc()
    L.add(T_SPAN, 1, 3).add(T_LIT, 5, 1).doc()
    pieces = [_random_text(rng, 8) for _ in range(5)]
    m, ctx, src, mb, got = _go(L, pieces)
    assert mb.status[3] != 0 and not got.status.any()
    assert [_doc_values(m, mb, got, d) for d in range(5)] == [[("Span", pieces[0][:4])], [], [("Lit", b"CHF")], [],
                                                              [("Lit", b"CHF"), ("Span", pieces[4][1:4])]]


# ---- 2. round edges
@pytest.mark.parametrize("n", [63, 64, 65])
def test_formatted_results_at_the_round_edge(n):
    rng = np.random.default_rng(n)
    text = _random_text(rng, 3 * n + 8)
    L = Lexems()
    for k in range(n):
        L.add(T_SPAN if k % 3 else T_LIT, 3 * k, k % 5)
    L.doc().add(T_LIT, 0, 1).doc()
    m, ctx, src, mb, got = _go(L, [text, b"ab"])
    assert int(mb.doc_offsets[1]) == n and not got.status.any()
    assert _doc_values(m, mb, got, 0) == sorted(("Span", text[3 * k:3 * k + k % 5]) if k % 3 else ("Lit", b"CHF") for k in range(n))
    assert _doc_values(m, mb, got, 1) == [("Lit", b"CHF")]


def test_formatted_record_is_the_65th_item():
    rng = np.random.default_rng(5)
    text = _random_text(rng, 200)
    L = Lexems()
    for k in range(32):
        L.add(T_PLAIN_A, 2 * k, 1).add(T_PLAIN_B, 2 * k + 1, 1).gap()
    L.add(T_YEAR, 100, 4).add(T_EV, 105, 3).doc()
    m, ctx, src, mb, got = _go(L, [text])
    assert len(mb.items) >= 65 and int(mb.item_format[64][0]) != 0 and int(mb.item_format[:64, 0].max()) == 0
    assert got.item(64) == text[100:104] and ("Event", text[100:104]) in _doc_values(m, mb, got, 0)


# ---- 3. alignment
def test_every_length_at_every_output_alignment():
    rng = np.random.default_rng(9)
    lengths, at = [], 0
    for r in range(4):
        for n in range(10):
            pad = (r - at) % 4
            if pad:
                lengths.append(pad); at += pad
            lengths.append(n); at += n
    text = _random_text(rng, 12 * len(lengths))
    L = Lexems()
    for k, n in enumerate(lengths):
        L.add(T_SPAN, 12 * k, n).gap()
    L.add(T_LIT, 0, 1).doc()
    m, ctx, src, mb, got = _go(L, [text])
    seen = set()
    for r in range(len(mb.results)):
        seen.add((len(got.result(r)), int(got.result_offsets[r]) % 4))
        if m.patternName(int(mb.results[r][0])) == "Span":
            assert got.result(r) == text[int(mb.results[r][4]):int(mb.results[r][6])]
    assert seen >= {(n, r) for n in range(10) for r in range(4)}
    assert b"" in [got.result(r) for r in range(len(mb.results))] and ("Lit", b"CHF") in _doc_values(m, mb, got, 0)


# ---- 4. separators, a variable that matches nothing
def test_separators_and_unmatched_variables():
    text = b"one two three four"
    L = Lexems().add(T_J1, 0, 3).add(T_J2, 4, 3).add(T_J3, 8, 5).gap().add(T_NONE, 14, 4).doc()
    m, ctx, src, mb, got = _go(L, [text])
    # (the items of a result are in the engine's order: the latest first)
    assert _doc_values(m, mb, got, 0) == sorted([("J2", b"two, one"), ("E2", b"twoone"), ("J3", b"three, two, one"), ("E3", b"<threetwoone>"),
                                                 ("None", b"[]")])


# ---- 5. nesting
def test_year_inside_event():
    text = b"in 1984 happened"
    L = Lexems().add(T_YEAR, 3, 4).add(T_EV, 8, 8).doc()
    m, ctx, src, mb, got = _go(L, [text])
    assert _doc_values(m, mb, got, 0) == [("Event", b"1984")]
    when = [i for i in range(len(mb.items)) if int(mb.item_format[i][0])]
    assert when and all(got.item(i) == b"1984" for i in when)


def test_depth_at_the_limit_and_beyond():
    """the chain's document between two neighbours that have values in both families: Q's result "<..>", and R's item `q`,
    bound to Q, with the same value"""
    limit = capi.lib().sp_matcher_value_max_depth()
    pieces = [b"abcdef", b"b", b"uvwxyz"]
    L = Lexems().add(2, 1, 3).add(3, 5, 1).doc().add(1, 0, 1).doc().add(2, 0, 4).add(3, 5, 1).doc()
    want = [[("Q", b"<bcd>"), ("R", b"")], None, [("Q", b"<uvwx>"), ("R", b"")]]

    def neighbours(mb, got):
        assert _doc_values(m, mb, got, 0) == want[0] and _doc_values(m, mb, got, 2) == want[2]
        ioffs = model.item_offsets(mb.results, mb.doc_offsets)
        items = [sorted(got.item(i) for i in range(ioffs[d], ioffs[d + 1]) if int(mb.item_format[i][0])) for d in (0, 2)]
        assert items == [[b"<bcd>"], [b"<uvwx>"]]
        return ioffs

    m, ctx, src, mb, got = _go(L, pieces, key=limit)
    assert not got.status.any() and _doc_values(m, mb, got, 1) == [("P%d" % k, b"x") for k in range(limit)]
    neighbours(mb, got)
    # one level more: the document of the chain is empty in both families, its neighbours are intact and document 2's
    # values follow directly behind document 0's bytes
    m, ctx, src, mb, got = _go(L, pieces, key=limit + 1)
    assert list(got.status) == [0, RANGE, 0] and int(mb.doc_offsets[2]) - int(mb.doc_offsets[1]) == limit + 1
    ioffs = neighbours(mb, got)
    r1, r2 = int(mb.doc_offsets[1]), int(mb.doc_offsets[2])
    assert got.result_values == b"<bcd><uvwx>" and got.item_values == b"<bcd><uvwx>"
    assert np.all(got.result_offsets[r1:r2 + 1] == 5) and np.all(got.item_offsets[ioffs[1]:ioffs[2] + 1] == 5)
    assert int(got.result_offsets[-1]) == 11 and int(got.item_offsets[-1]) == 11
    m, ctx, src, mb, got = _go(L, pieces, key=limit + 1, flags=model.SP_VALUE_ITEMS)     # the items alone start one level further in
    assert not got.status.any() and got.item_values.count(b"x") > 0 and b"<bcd>" in got.item_values and b"<uvwx>" in got.item_values


# ---- 6. spans
def test_invalid_span_used_by_a_value():
    rng = np.random.default_rng(12)
    pieces = [_random_text(rng, 10) for _ in range(3)]
    L = Lexems().add(T_SPAN, 1, 3).doc().add(T_LIT, 0, 1).add(T_SPAN, 11, 2).add(T_YEAR, 0, 2).add(T_EV, 3, 2).doc().add(T_SPAN, 2, 8).doc()
    m, ctx, src, mb, got = _go(L, pieces)
    assert list(got.status) == [0, RANGE, 0] and int(mb.doc_offsets[2]) - int(mb.doc_offsets[1]) == 3
    assert got.result_offsets[1] == got.result_offsets[4] and _doc_values(m, mb, got, 2) == [("Span", pieces[2][2:10])]
    # an invalid span that no value uses: Plain has no format
    L = Lexems().add(T_PLAIN_A, 11, 2).add(T_PLAIN_B, 3, 2).add(T_SPAN, 1, 3).doc()
    m, ctx, src, mb, got = _go(L, pieces[:1])
    assert not got.status.any() and ("Span", pieces[0][1:4]) in _doc_values(m, mb, got, 0)


def test_span_across_segments_and_long_span():
    rng = np.random.default_rng(13)
    long_span = capi.lib().sp_matcher_text_long_span()
    pieces = [_random_text(rng, 12), b"", _random_text(rng, 9), _random_text(rng, long_span + 7)]
    L = Lexems().add(T_X1, 8, 2, seg=0).add(T_X2, 1, 3, seg=2).doc().add(T_LIT, 0, 1).add(T_SPAN, 3, long_span).add(T_SPAN, 1, 2).doc()
    m, ctx, src, mb, got = _go(L, pieces, dso=[0, 3, 4])
    assert not got.status.any()
    assert _doc_values(m, mb, got, 0) == [("Cross", b"(" + pieces[0][8:] + pieces[2][:4] + b")")]
    assert ("Span", pieces[3][3:3 + long_span]) in _doc_values(m, mb, got, 1)


# ---- 7. families and contexts
def test_families_alone_and_a_matcher_without_formats():
    rng = np.random.default_rng(14)
    text = _random_text(rng, 40)
    L = Lexems().add(T_YEAR, 3, 4).add(T_EV, 8, 8).gap().add(T_SPAN, 20, 7).add(T_PLAIN_A, 30, 2).add(T_PLAIN_B, 33, 2).doc()
    for flags in (model.SP_VALUE_RESULTS, model.SP_VALUE_ITEMS):
        m, ctx, src, mb, got = _go(L, [text], flags=flags)
        assert not got.status.any() and (got.result_values if flags == 1 else got.item_values)
    lex, seg, offs, want = _pairs([[(0, 1, 0, 9)]], [[40]])
    ctx = _ctx()
    src = Source([text])
    Run(ctx, lex, seg, offs)
    _values(ctx, src)
    got = ctx.finishedValuesFetch()
    assert not got.status.any() and got.result_values == b"" and got.item_values == b""
    assert list(got.result_offsets) == [0, 0] and list(got.item_offsets) == [0, 0, 0]


def test_call_order_grown_batch_and_foreign_stream():
    torch = _torch()
    rng = np.random.default_rng(15)
    m = _matcher()
    ctx = m.createContext()
    small = Source([_random_text(rng, 30)])
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):       # before any batch
        _values(ctx, small)
    with pytest.raises(spa.PatternError):
        ctx.finishedValuesFetch()
    with pytest.raises(spa.PatternError):
        ctx.lastValuesMs()
    L = Lexems().add(T_SPAN, 3, 5).add(T_LIT, 9, 1).doc()
    lex, seg, offs = L.arrays()
    run = RunAny.__new__(RunAny)
    run.ctx, run.ndocs, run.nlex = ctx, 1, len(lex)
    run.d_lex = torch.from_numpy(lex.view(np.int32).reshape(-1)).cuda()
    run.d_seg = torch.from_numpy(seg.view(np.int32)).cuda()
    run.d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    run.match()
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):       # a batch that is not finished
        _values(ctx, small)
    ctx.batchFinishDevice(_stream())
    for flags in (0, 4):
        with pytest.raises(spa.PatternError, match=r"\(-1\)"):
            _values(ctx, small, flags=flags)
    out = capi.SpMatchValuesBatch()
    assert capi.lib().sp_matcher_ctx_finished_values_device(ctx._h, None, 3, None, ctypes.byref(out)) == -1
    first = _values(ctx, small)
    _assert_values(m, ctx, small, first)
    assert ctx.lastValuesMs() > 0
    # a second, larger batch on the same context: the buffers grow; on another stream than the finish's
    big = Lexems()
    pieces = []
    for d in range(70):
        n = int(rng.integers(0, 80))
        for k in range(n):
            big.add(T_SPAN if k % 2 else T_LIT, 3 * k, int(rng.integers(0, 4))).gap()
        big.add(T_YEAR, 0, 2).add(T_EV, 2, 2).doc()
        pieces.append(_random_text(rng, 3 * n + 8))
    src = Source(pieces)
    RunAny(ctx, *big.arrays())
    other = torch.cuda.Stream()
    out = _values(ctx, src, stream=other.cuda_stream)
    mb, got = _assert_values(m, ctx, src, out)
    assert not got.status.any() and len(got.result_values) > 1000
    ctx.matchDocsDevice(run.d_lex.data_ptr(), run.d_offs.data_ptr(), 1, run.nlex, _stream(), run.d_seg.data_ptr())
    with pytest.raises(spa.PatternError):                         # the next batch invalidates the values
        ctx.finishedValuesFetch()


def test_failed_allocation_then_a_normal_call():
    """a device allocation that fails is SP_ERR_NOMEM (-2) and leaves no values; the context stays usable, and a second
    call on the same batch reuses the buffers of the first"""
    rng = np.random.default_rng(17)
    m = _matcher()
    ctx = m.createContext()
    pieces = [_random_text(rng, 20) for _ in range(3)]
    L = Lexems().add(T_SPAN, 3, 5).add(T_LIT, 9, 1).doc().add(T_J1, 0, 2).add(T_J2, 4, 3).doc().add(T_YEAR, 1, 4).add(T_EV, 6, 2).doc()
    src = Source(pieces)
    RunAny(ctx, *L.arrays())
    lib = capi.lib()
    out = capi.SpMatchValuesBatch()
    c_src = capi.SpTextSource(src.d_text.data_ptr(), len(src.text), src.d_so.data_ptr(), src.nseg, None)
    lib.sp_test_fail_alloc_above(1)
    try:
        assert lib.sp_matcher_ctx_finished_values_device(ctx._h, ctypes.byref(c_src), BOTH, None, ctypes.byref(out)) == -2
    finally:
        lib.sp_test_fail_alloc_above(0)
    with pytest.raises(spa.PatternError):                         # the failed call left nothing to fetch
        ctx.finishedValuesFetch()
    first = _values(ctx, src)
    mb, got = _assert_values(m, ctx, src, first)
    assert len(mb.results) >= 3 and len(got.result_values) > 0 and not got.status.any()
    second = _values(ctx, src)
    for name, _ in capi.SpMatchValuesBatch._fields_:
        assert getattr(first, name) == getattr(second, name)
    _assert_values(m, ctx, src, second)


# ---- 8. finish modes
def test_plain_against_canonical_finish():
    rng = np.random.default_rng(16)
    L, pieces = Lexems(), []
    for d in range(20):
        for k in range(int(rng.integers(10, 60))):
            L.add(int(rng.choice([T_LIT, T_SPAN, T_J1, T_J2, T_J3, T_YEAR, T_EV, T_PLAIN_A, T_PLAIN_B])), 2 * k, int(rng.integers(0, 3)))
        L.doc()
        pieces.append(_random_text(rng, 130))
    per_mode = []
    for canonical in (False, True):
        m, ctx, src, mb, got = _go(L, pieces, canonical=canonical)
        assert not got.status.any()
        ioffs = model.item_offsets(mb.results, mb.doc_offsets)
        per_mode.append([(sorted((mb.results[r].tobytes(), got.result(r)) for r in range(int(mb.doc_offsets[d]), int(mb.doc_offsets[d + 1]))),
                          sorted((mb.items[i].tobytes(), got.item(i)) for i in range(ioffs[d], ioffs[d + 1])))
                         for d in range(len(pieces))])
    strip = lambda docs: [(sorted((r[:28] + r[32:], v) for r, v in rs), its) for rs, its in docs]      # (item_begin is assigned by the finish)
    assert strip(per_mode[0]) == strip(per_mode[1]) and sum(len(rs) for rs, _ in per_mode[0]) > 100


def test_exact_engine_against_result_set_mode():
    m = spa.PatternMatcherInstance()
    for k, fmt in enumerate(["{a}-{b}", "{b|;}", ""]):
        m.pushTerm(1 + k); m.attachVariable("a"); m.pushTerm(2 + k); m.attachVariable("b")
        m.pushExpression("sequence", 2, 3, 0); m.definePattern("p%d" % k, fmt, True)
    m.compile()
    assert m.resultSetTier()[0], m.resultSetTier()[1]           # (two-term sequences: eligible for the join kernel)
    rng = np.random.default_rng(17)
    L, pieces = Lexems(), []
    for d in range(12):
        for k in range(int(rng.integers(0, 40))):
            L.add(int(rng.integers(1, 5)), 2 * k, int(rng.integers(0, 3)))
        L.doc()
        pieces.append(_random_text(rng, 90))
    got = []
    for result_sets in (False, True):
        ctx = m.createContext(result_sets=result_sets)
        assert ctx.kernelKind() == (2 if result_sets else ctx.kernelKind())
        src = Source(pieces)
        RunAny(ctx, *L.arrays(), canonical=True)
        out = _values(ctx, src)
        mb, v = _assert_values(m, ctx, src, out)
        got.append((mb.results.tobytes(), v.result_values, v.item_values, v.result_offsets.tobytes(), v.status.tobytes()))
    assert got[0] == got[1] and len(got[0][1]) > 50


# ---- 9. end to end
def _segmented(program, docs):
    """-> (matcher, MatchBatch, MatchValues, text, seg_offsets, doc_seg_offsets) of matchSegmentedDocs(.., with_values=True)"""
    lx, mt = spa.PatternLexerInstance(), spa.PatternMatcherInstance()
    prg = rulelang.load(program, lx, mt)
    text, so, dso, _ = segments.segmented_batch(docs)
    mb, mv = spa.matchSegmentedDocs(lx.createContext(), mt.createContext(), text, so, dso, with_values=True)
    assert not mb.status.any() and not mv.status.any()
    twin = spa.batchValues(mt, mb, text, so, dso)
    assert twin.result_values == mv.result_values and twin.item_values == mv.item_values
    assert np.array_equal(twin.result_offsets, mv.result_offsets) and np.array_equal(twin.item_offsets, mv.item_offsets)
    return prg, mt, mb, mv


def test_segmented_example_end_to_end():
    with open(os.path.join(HERE, "golden", "doc_example.rul")) as f:
        program = f.read()
    with open(os.path.join(HERE, "golden", "doc_example.txt"), "rb") as f:
        text = f.read()
    # the example's program has no format strings: its listing has no values, and so has the device
    prg, mt, mb, mv = _segmented(program, [text])
    assert len(mb.results) > 0 and mv.result_values == b"" and mv.item_values == b""
    # the documented program with format strings, the text as two paragraphs: the values of the listing
    prg, mt, mb, mv = _segmented(MONEY, [TEXT.replace(b" and ", b"\n\n")])
    names = [mt.patternName(int(r[0])) for r in mb.results]
    got = sorted((names[r], mv.result(r)) for r in range(len(names)) if int(mb.result_format[r]))
    assert ("MoneyAmount", b"EUR 3'645") in got and ("MoneyAmount", b"CHF 12") in got and ("Event", b"1984") in got
    when = [i for i in range(len(mb.items)) if int(mb.item_format[i][0]) and mt.variableName(int(mb.items[i][0])) == "when"]
    assert when and all(mv.item(i) == b"1984" for i in when)


def test_listing_with_device_values_is_the_listing(tmp_path, capsys):
    """match.py --device-values prints what match.py prints, plain and with --paragraphs"""
    from struspattern_amd import match
    prog, doc = tmp_path / "money.rul", tmp_path / "money.txt"
    prog.write_text(MONEY)
    doc.write_bytes(TEXT.replace(b" and ", b"\n\n"))
    for extra in ([], ["--paragraphs"]):
        outs = []
        for dv in ([], ["--device-values"]):
            assert match.main(["-p", str(prog), *extra, *dv, str(doc)]) == 0
            outs.append(capsys.readouterr().out)
        assert outs[0] == outs[1] and "'EUR 3'645'" in outs[0] and "OK done" in outs[0]
