"""Dictionary order on the device (sp_matcher_ctx_finished_dictionary_order_device, csrc/l2_dictorder.h): order, rank,
prefix_bytes, handle_offsets and the total that the launches leave must EQUAL what the device-free twin
(sp_match_batch_dictionary_order) makes of the fetched batch, terms and dictionary, and the model (tests/dictorder_model.py); the
device pointers of `out` hold the same bytes.  Bare-term matchers over hand-made lexems as in tests/test_postings_gpu.py: with
SP_TERM_TEXT a test sets every handle and value itself, so it decides ndict, the arrival order and every byte compared."""
import ctypes

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from tests import dictorder_cases as cases
from tests import dictorder_model as model
from tests import postings_model
from tests.finished_support import (_bare, _build, _from_device, Lexems, _matcher, MONEY, Run, Source, _stream, T_LIT, T_PLAIN_A, T_PLAIN_B, T_SPAN, _torch,
                                    _trip_docs, _values)

pytestmark = pytest.mark.gpu

V, T = spa.SP_TERM_VALUES, spa.SP_TERM_TEXT


def _assert_order(ctx, out=None, values=False, text=True):
    """the fetched order equals the twin's and the model's on the fetched batch, terms and dictionary, the invariants hold, and
    the bytes behind the device pointers are the fetched ones; returns (entries, order)"""
    mb, terms, d = ctx.finishedFetch(), ctx.finishedTermsFetch(), ctx.finishedDictionaryFetch()
    mv = ctx.finishedValuesFetch() if values else None
    mt = ctx.finishedTextFetch() if text else None
    got = ctx.finishedDictionaryOrderFetch()
    entries = model.entries_of(mb, terms, d, mv, mt)
    want = model.dictionary_order(entries, d.handle_terms)
    model.assert_same(spa.batchDictionaryOrder(mb, terms, d, values=mv, text=mt), want)
    model.assert_same(got, want)
    model.check_invariants(got, entries, d.handle_terms)
    if out is not None:
        n, bound = len(d.records), len(d.handle_terms)
        assert out.ndict == n and out.handle_bound == bound
        assert int(_from_device(out.d_totals, 1, np.uint64)[0]) == n
        assert np.array_equal(_from_device(out.d_order, n, np.uint32), got.order)
        assert np.array_equal(_from_device(out.d_rank, n, np.uint32), got.rank)
        assert np.array_equal(_from_device(out.d_prefix_bytes, n, np.uint32), got.prefix_bytes)
        assert np.array_equal(_from_device(out.d_handle_offsets, bound + 1, np.uint64), got.handle_offsets)
    return entries, got


def _go(docs, nhandles=8, canonical=False):
    """the order of the dictionary of the text terms of hand-made documents: (context, entries, order)"""
    m = _bare(nhandles)
    pieces, lex, seg, offs = _build(docs)
    ctx = m.createContext()
    src = Source(pieces)
    Run(ctx, lex, seg, offs, canonical=canonical)
    src.gather(ctx, items=False)
    ctx.finishedTermsDevice(T, _stream())
    ctx.finishedDictionaryDevice(_stream())
    out = ctx.finishedDictionaryOrderDevice(_stream())
    entries, got = _assert_order(ctx, out)
    return ctx, entries, got


def _sorted(entries, got):
    return [entries[int(e)] for e in got.order]


# ---- 1. empty shapes
def test_no_documents_empty_documents_and_one_entry():
    m = _bare(8)
    ctx = m.createContext()
    src = Source([])
    Run(ctx, np.zeros((0, 4), np.uint32), np.zeros(0, np.uint32), np.zeros(1, np.uint64))
    src.gather(ctx, items=False)
    ctx.finishedTermsDevice(T, _stream())
    ctx.finishedDictionaryDevice(_stream())
    out = ctx.finishedDictionaryOrderDevice(_stream())
    entries, got = _assert_order(ctx, out)
    assert len(got.order) == 0 and got.handle_offsets.tolist() == [0] * 10
    ctx, entries, got = _go([[], [], []])
    assert len(got.order) == len(got.rank) == len(got.prefix_bytes) == 0 and got.handle_offsets.tolist() == [0] * 10
    ctx, entries, got = _go([[(3, b"only")], [], [(3, b"only"), (3, b"only")]])
    assert got.order.tolist() == [0] and got.rank.tolist() == [0] and got.prefix_bytes.tolist() == [0]
    assert got.handle_offsets.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1]
    assert ctx.lastDictionaryOrderMs() >= 0.0


# ---- 2. wave and tile edges
def _edge(name):
    tile = capi.lib().sp_matcher_dictionary_order_tile()
    return {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2*tile+1": 2 * tile + 1, "3*tile": 3 * tile, "4*tile+1": 4 * tile + 1,
            "5*tile-3": 5 * tile - 3}.get(name) or int(name)


@pytest.mark.parametrize("edge,arrival", [("2", "descending"), ("63", "shuffle"), ("64", "descending"), ("65", "shuffle"), ("tile-1", "shuffle"),
                                          ("tile", "descending"), ("tile+1", "shuffle"), ("2*tile+1", "ascending"), ("3*tile", "shuffle"),
                                          ("4*tile+1", "descending"), ("5*tile-3", "shuffle")])
def test_wave_and_tile_edges(edge, arrival):
    """3 tiles: a run without a partner at the first level; 5 tiles less 3 entries: three levels with a partial last run"""
    n = _edge(edge)
    pairs = cases.numbered(n, arrival=arrival)
    ctx, entries, got = _go(cases.in_documents(pairs, 257))
    assert len(entries) == n and _sorted(entries, got) == sorted(pairs)
    if arrival == "ascending":
        assert got.order.tolist() == list(range(n))
    assert int(got.handle_offsets[-1]) == n and np.diff(got.handle_offsets.astype(np.int64)).tolist()[1:8] == [len(range(h, n, 7)) for h in range(7)]


# ---- 3. comparator edges
def test_comparator_edges_and_a_long_shared_prefix():
    pairs = cases.comparator_values() + cases.long_prefix_group()
    # (a one-byte term in front of a document moves every value behind it to another address: odd ones among them)
    docs = [[(7, b"!")] * (k % 2) + doc for k, doc in enumerate(cases.in_documents(pairs, 9))]
    ctx, entries, got = _go(docs)
    assert _sorted(entries, got) == sorted(set(pairs) | {(7, b"!")})
    group = got.handle(3)
    assert len(group) == 70 and got.prefix_bytes[int(got.handle_offsets[3]):int(got.handle_offsets[4])].tolist() == [0] + [300] * 69
    k = int(got.rank[entries.index((2, b"a\0\0\0\0"))])
    assert [entries[int(e)][1] for e in got.order[k - 3:k + 2]] == [b"a", b"a\0", b"a\0\0\0", b"a\0\0\0\0", b"ab"]
    assert got.prefix_bytes[k - 3:k + 2].tolist() == [0, 1, 2, 4, 1]
    assert [v for h, v in _sorted(entries, got) if h == 2][-3:] == [b"\x7f", b"\x80", b"\xfe\x01"]


# ---- 4. one handle holds all entries; every entry has its own handle
def test_one_handle_for_all_entries_and_a_handle_per_entry():
    ctx, entries, got = _go([[(299, b"v%03d" % ((k * 37) % 300)) for k in range(d, 300, 3)] for d in range(3)], nhandles=299)
    assert len(got.handle(299)) == 300 and int(got.handle_offsets[299]) == 0 and len(got.handle_offsets) == 301
    assert [entries[int(e)][1] for e in got.order] == [b"v%03d" % k for k in range(300)]
    ctx, entries, got = _go([[(1 + (k * 37) % 299, b"same") for k in range(d, 299, 2)] for d in range(2)], nhandles=299)
    assert got.handle_offsets.tolist() == [0] + list(range(300)) and not got.prefix_bytes.any()
    assert [entries[int(e)][0] for e in got.order] == list(range(1, 300))


# ---- 5. both sources
def test_values_and_text_in_one_batch():
    m = _matcher()
    text = b"eur usd eur chf usd eur ab cd ab cd CHF"
    L = Lexems()
    for pos in (4, 0, 8):
        L.add(T_SPAN, pos, 3).gap()                                     # Span: formatted "{a}" -> usd eur eur
    L.add(T_LIT, 0, 3).gap()                                            # Lit: formatted, the value is "CHF" whatever the text
    L.add(T_PLAIN_A, 24, 2).add(T_PLAIN_B, 27, 2)                       # Plain: no format, text "ab cd"
    L.doc()
    L.add(T_SPAN, 36, 3).gap().add(T_SPAN, 12, 3).doc()                 # the text "CHF" as the value of a Span, and chf
    L.add(T_PLAIN_A, 30, 2).add(T_PLAIN_B, 33, 2).gap().add(T_SPAN, 4, 3).doc()
    ctx = m.createContext()
    src = Source([text] * 3)
    Run(ctx, *L.arrays())
    _values(ctx, src, flags=1)                                          # (SP_VALUE_RESULTS)
    src.gather(ctx, items=False)
    ctx.finishedTermsDevice(V | T, _stream())
    ctx.finishedDictionaryDevice(_stream())
    out = ctx.finishedDictionaryOrderDevice(_stream())
    entries, got = _assert_order(ctx, out, values=True)
    found = [(m.patternName(h), v) for h, v in _sorted(entries, got)]
    by_handle = sorted(set(found), key=lambda t: (m.patternId(t[0]), t[1]))
    assert found == by_handle and len(found) == 6
    assert set(found) == {("Lit", b"CHF"), ("Span", b"CHF"), ("Span", b"chf"), ("Span", b"eur"), ("Span", b"usd"), ("Plain", b"ab cd")}


# ---- 6. the order of the results
def test_plain_against_canonical_finish():
    docs = _trip_docs()
    found = []
    for canonical in (False, True):
        ctx, entries, got = _go(docs, canonical=canonical)
        found.append((_sorted(entries, got), got.prefix_bytes.tobytes(), got.handle_offsets.tobytes()))
    assert found[0] == found[1] and len(found[0][0]) > 150


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
        out = ctx.finishedDictionaryOrderDevice(_stream())
        got.append(_assert_order(ctx, out))
    (entries_a, a), (entries_b, b) = got
    assert len(entries_a) > 100 and entries_a == entries_b
    for f in model.FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes()


# ---- 7. call order, buffers and streams
def test_call_order_other_products_buffers_and_streams():
    torch = _torch()
    m = _bare(8)
    docs = cases.in_documents(cases.numbered(700), 97)
    pieces, lex, seg, offs = _build(docs)
    ctx = m.createContext()
    src = Source(pieces)
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):              # before any batch
        ctx.finishedDictionaryOrderDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedDictionaryOrderFetch()
    with pytest.raises(spa.PatternError):
        ctx.lastDictionaryOrderMs()
    run = Run(ctx, lex, seg, offs)
    src.gather(ctx, items=False)
    ctx.finishedTermsDevice(T, _stream())
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):              # terms, but no dictionary
        ctx.finishedDictionaryOrderDevice(_stream())
    ctx.finishedDictionaryDevice(_stream())
    # an allocation that fails, then a normal call
    L = capi.lib()
    out = capi.SpMatchDictionaryOrderDevice()
    L.sp_test_fail_alloc_above(1)
    try:
        assert L.sp_matcher_ctx_finished_dictionary_order_device(ctx._h, None, ctypes.byref(out)) == -2       # SP_ERR_NOMEM
    finally:
        L.sp_test_fail_alloc_above(0)
    assert not out.d_order and out.ndict == 0
    with pytest.raises(spa.PatternError):
        ctx.finishedDictionaryOrderFetch()
    first = ctx.finishedDictionaryOrderDevice(_stream())
    entries, got = _assert_order(ctx, first)
    assert len(entries) == 700 and ctx.lastDictionaryOrderMs() >= 0.0
    # postings and positions built after the order leave it as it is, and the reverse
    ctx.finishedPostingsDevice(_stream())
    ctx.finishedPositionsDevice(_stream())
    postings, positions = ctx.finishedPostingsFetch(), ctx.finishedPositionsFetch()
    model.assert_same(ctx.finishedDictionaryOrderFetch(), got)
    again = ctx.finishedDictionaryOrderDevice(_stream())
    model.assert_same(_assert_order(ctx, again)[1], got)
    postings_model.assert_same(ctx.finishedPostingsFetch(), postings)
    assert ctx.finishedPositionsFetch().occurrences.tobytes() == positions.occurrences.tobytes()
    # a new dictionary call invalidates the fetch; a stream other than the dictionary's, which is not waited for
    ctx.finishedDictionaryDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedDictionaryOrderFetch()
    other = torch.cuda.Stream()
    second = ctx.finishedDictionaryOrderDevice(other.cuda_stream)
    assert second.d_order == first.d_order and second.d_rank == first.d_rank
    model.assert_same(_assert_order(ctx, second)[1], got)
    # a new terms call: neither the dictionary nor the order count
    ctx.finishedTermsDevice(T, _stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedDictionaryOrderFetch()
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        ctx.finishedDictionaryOrderDevice(_stream())
    ctx.finishedDictionaryDevice(_stream())
    ctx.finishedDictionaryOrderDevice(_stream())
    # a new finish: the old dictionary does not count
    run.match()
    ctx.batchFinishDevice(_stream())
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        ctx.finishedDictionaryOrderDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedDictionaryOrderFetch()
    # a smaller and then a larger batch on the same context: the buffers stay where they are while they are large enough
    for part, same in ((docs[:2], True), (cases.in_documents(cases.numbered(2500, arrival="descending"), 97), False)):
        pieces, lex, seg, offs = _build(part)
        src = Source(pieces)
        Run(ctx, lex, seg, offs)
        src.gather(ctx, items=False)
        ctx.finishedTermsDevice(T, _stream())
        ctx.finishedDictionaryDevice(_stream())
        later = ctx.finishedDictionaryOrderDevice(_stream())
        for field in ("d_order", "d_rank", "d_prefix_bytes"):          # (the larger batch makes them grow: where to is the allocator's business)
            assert getattr(later, field) == getattr(first, field) or not same, field
        assert later.d_handle_offsets == first.d_handle_offsets and later.d_totals == first.d_totals
        entries, got = _assert_order(ctx, later)
        assert len(entries) == sum(len(doc) for doc in part) and ctx.lastDictionaryOrderMs() >= 0.0


# ---- 8. end to end
def test_segmented_documents_with_the_order():
    from struspattern_amd import rulelang, segments
    docs = [b"He paid 3'645 Eur\n\nand 3'645 Eur again or 12 sFr. he paid", b"nothing", b"12 sFr. in the year 1984 something happened",
            b"later 3'645 Eur were paid"]
    lx, m = spa.PatternLexerInstance(), spa.PatternMatcherInstance()
    rulelang.load(MONEY, lx, m)
    text, so, dso, _ = segments.segmented_batch(docs)
    found = spa.matchSegmentedDocs(lx.createContext(), m.createContext(), text, so, dso, with_dictionary_order=True)
    assert len(found) == 6                                              # (no postings, no positions: the order is the last element)
    mb, mt, mv, terms, d, o = found
    assert isinstance(o, spa.MatchDictionaryOrder) and isinstance(d, spa.MatchDictionary)
    entries = model.entries_of(mb, terms, d, mv, mt)
    model.assert_same(o, model.dictionary_order(entries, d.handle_terms))
    model.assert_same(spa.batchDictionaryOrder(mb, terms, d, values=mv, text=mt), o)
    model.check_invariants(o, entries, d.handle_terms)
    e = o.find(m.patternId("MoneyAmount"), b"EUR 3'645", mb, terms, d, values=mv, text=mt)
    assert e is not None and entries[e] == (m.patternId("MoneyAmount"), b"EUR 3'645") and int(d.records[e, 4]) == 2
    assert o.find(m.patternId("MoneyAmount"), b"EUR 3'646", mb, terms, d, values=mv, text=mt) is None
    everything = spa.matchSegmentedDocs(lx.createContext(), m.createContext(), text, so, dso, with_positions=True, with_dictionary_order=True)
    assert len(everything) == 8 and isinstance(everything[6], spa.MatchPositions)
    model.assert_same(everything[7], o)


def _listing(capsys, argv):
    from struspattern_amd import match
    assert match.main(argv) == 0
    return capsys.readouterr().out.splitlines()


def test_match_sorted_listing(capsys, tmp_path):
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    prog = os.path.join(here, "golden", "doc_example.rul")
    a, b = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    with open(os.path.join(here, "golden", "doc_example.txt"), "rb") as f:
        example = f.read()
    example = example.replace(b"\n", b" ")                              # (no value spans a line: the listing is read line by line)
    with open(a, "wb") as f:
        f.write(example)
    with open(b, "wb") as f:
        f.write(b"Prof. Anna B. Smith wrote to anna@etc.com. " + example[:len(example) // 2])
    common = ["-p", prog, "--device-values"]
    for paragraphs in ([], ["--paragraphs"]):
        lines, today = {}, {}
        for name, files in (("ab", [a, b]), ("ba", [b, a])):
            plain = _listing(capsys, common + paragraphs + ["--postings", "--positions"] + files)
            lines[name] = _listing(capsys, common + paragraphs + ["--sorted", "--postings", "--positions"] + files)
            only_sorted = _listing(capsys, common + paragraphs + ["--sorted"] + files)                  # (implies --dictionary)
            assert only_sorted == [line for line in lines[name] if not line.startswith("post ")]
            # with the flag the same lines, the term lines in another order
            assert sorted(plain) == sorted(lines[name])
            today[name] = [line for line in plain if line.startswith("dict ")]
            head = [line for line in plain if not line.startswith(("dict ", "post "))]
            assert [line for line in lines[name] if not line.startswith(("dict ", "post "))] == head
        dicts = {name: [line for line in out if line.startswith("dict ")] for name, out in lines.items()}
        posts = {name: [line for line in out if line.startswith("post ")] for name, out in lines.items()}
        assert dicts["ab"] == dicts["ba"] and len(dicts["ab"]) > 3
        assert today["ab"] != today["ba"] and sorted(today["ab"]) == sorted(today["ba"])         # (first occurrence depends on the order of the files)
        # the term lines are identical apart from the file indices
        assert [line.split("': ")[0] for line in posts["ab"]] == [line.split("': ")[0] for line in posts["ba"]] and len(posts["ab"]) == len(dicts["ab"])

        def cells(line, other_file):
            """the FILEINDEX:COUNT@FIRSTPOS[..] cells of a post line, sorted; other_file: with the two file indices exchanged"""
            found = line.split("': ", 1)[1].split(" ")
            if other_file:
                found = [re.sub(r"^(\d+):", lambda mo: "%d:" % (1 - int(mo.group(1))), cell) for cell in found]
            return sorted(found)
        assert [cells(line, True) for line in posts["ab"]] == [cells(line, False) for line in posts["ba"]]
