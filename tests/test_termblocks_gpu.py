"""Term blocks on the device (sp_matcher_ctx_finished_term_blocks_device, csrc/l2_termblocks.h): the bytes, block_offsets,
block_handles and totals that the launches leave must EQUAL what the device-free twin (sp_match_batch_term_blocks) makes of the
fetched batch, terms, dictionary and order, and the model (tests/termblocks_model.py); they decode to the sorted entries, and the
device pointers of `out` hold the same bytes.  Bare-term matchers over hand-made lexems as in tests/test_dictorder_gpu.py: with
SP_TERM_TEXT a test sets every handle and value itself, so it decides ndict, every length and every byte coded."""
import ctypes

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from tests import dictorder_cases
from tests import dictorder_model
from tests import postings_model
from tests import termblocks_cases as cases
from tests import termblocks_model as model
from tests.finished_support import (_bare, _build, _from_device, Lexems, _matcher, MONEY, Run, Source, _stream, T_LIT, T_PLAIN_A, T_PLAIN_B, T_SPAN, _torch,
                                    _trip_docs, _values)

pytestmark = pytest.mark.gpu

V, T = spa.SP_TERM_VALUES, spa.SP_TERM_TEXT


def _assert_blocks(ctx, out=None, values=False, text=True):
    """the fetched blocks equal the twin's and the model's on the fetched batch, terms, dictionary and order, decode to the sorted
    entries, and the bytes behind the device pointers are the fetched ones; returns (sorted entries, blocks)"""
    mb, terms, d, order = ctx.finishedFetch(), ctx.finishedTermsFetch(), ctx.finishedDictionaryFetch(), ctx.finishedDictionaryOrderFetch()
    mv = ctx.finishedValuesFetch() if values else None
    mt = ctx.finishedTextFetch() if text else None
    got = ctx.finishedTermBlocksFetch()
    B = int(got.block_entries)
    assert B == capi.lib().sp_matcher_term_block_entries()
    want_entries = model.sorted_entries(d, dictorder_model.entries_of(mb, terms, d, mv, mt), order)
    want = model.term_blocks(want_entries, B)
    model.assert_same(spa.batchTermBlocks(mb, terms, d, order, values=mv, text=mt), want)
    model.assert_same(got, want)
    model.check_invariants(got, want_entries)
    assert got.entries() == want_entries                                # the library's reader
    if out is not None:
        nblocks, nbytes = len(got.block_handles), len(got.bytes)
        assert (out.ndict, out.nblocks, out.nbytes, out.block_entries) == (len(want_entries), nblocks, nbytes, B)
        assert np.array_equal(_from_device(out.d_totals, 4, np.uint64), got.totals)
        assert np.array_equal(_from_device(out.d_bytes, nbytes, np.uint8), got.bytes)
        assert np.array_equal(_from_device(out.d_block_offsets, nblocks + 1, np.uint64), got.block_offsets)
        assert np.array_equal(_from_device(out.d_block_handles, nblocks, np.uint32), got.block_handles)
    return want_entries, got


def _ordered(ctx):
    """terms, dictionary and order of the text terms of the finished batch of `ctx`"""
    ctx.finishedTermsDevice(T, _stream())
    ctx.finishedDictionaryDevice(_stream())
    ctx.finishedDictionaryOrderDevice(_stream())


def _go(docs, nhandles=8, canonical=False):
    """the term blocks of the text terms of hand-made documents: (context, sorted entries, blocks)"""
    m = _bare(nhandles)
    pieces, lex, seg, offs = _build(docs)
    ctx = m.createContext()
    src = Source(pieces)
    Run(ctx, lex, seg, offs, canonical=canonical)
    src.gather(ctx, items=False)
    _ordered(ctx)
    out = ctx.finishedTermBlocksDevice(_stream())
    entries, got = _assert_blocks(ctx, out)
    return ctx, entries, got


# ---- 1. empty shapes
def test_no_documents_empty_documents_and_one_entry():
    m = _bare(8)
    ctx = m.createContext()
    src = Source([])
    Run(ctx, np.zeros((0, 4), np.uint32), np.zeros(0, np.uint32), np.zeros(1, np.uint64))
    src.gather(ctx, items=False)
    _ordered(ctx)
    out = ctx.finishedTermBlocksDevice(_stream())
    entries, got = _assert_blocks(ctx, out)
    assert entries == [] and got.block_offsets.tolist() == [0] and got.totals.tolist() == [0, 0, 16, 0] and len(got.bytes) == 0
    ctx, entries, got = _go([[], [], []])
    assert entries == [] and got.block_offsets.tolist() == [0] and got.totals.tolist() == [0, 0, 16, 0]
    ctx, entries, got = _go([[(3, b"only")], [], [(3, b"only"), (3, b"only")]])
    assert entries == [(3, b"only", 2, 3)] and bytes(got.bytes) == b"\0\0\4\2\3only" and got.block_offsets.tolist() == [0, 9] and got.block_handles.tolist() == [3]
    assert ctx.lastTermBlocksMs() >= 0.0


# ---- 2. wave and block edges
@pytest.mark.parametrize("n,arrival", [(2, "descending"), (15, "shuffle"), (16, "descending"), (17, "shuffle"), (63, "shuffle"), (64, "descending"),
                                       (65, "shuffle"), (128, "descending"), (129, "shuffle"), (64 * 5 - 3, "shuffle")])
def test_wave_and_block_edges(n, arrival):
    """a partial block, a partial wave, several waves"""
    pairs = dictorder_cases.numbered(n, arrival=arrival)
    ctx, entries, got = _go(dictorder_cases.in_documents(pairs, 97))
    assert [e[:2] for e in entries] == sorted(pairs) and len(got.block_handles) == (n + 15) // 16


# ---- 3. alignment
@pytest.mark.parametrize("shift", [0, 1])
def test_spans_that_start_at_every_alignment(shift):
    """values of the lengths 0..9 in turn: the codes, and the spans of consecutive waves, start at every alignment mod 4; with a
    one-byte term in front every source address moves by one"""
    pairs = cases.lengths_in_turn()
    docs = [[(15, b"!")] * shift + doc for doc in dictorder_cases.in_documents(pairs, 50)]
    ctx, entries, got = _go(docs, nhandles=15)
    assert len(entries) == 140 + shift and [len(e[1]) for e in entries[:140]] == list(range(10)) * 14
    starts, at = set(), 0
    for e, (_, same, suffix) in zip(entries, [f for j in range(len(got.block_handles)) for f in model.decode_block(got, j)[1]]):
        starts.add(at % 4)
        at += 5 + suffix
    assert starts == {0, 1, 2, 3}


# ---- 4. long and skewed
def test_a_value_far_longer_than_any_staging():
    long = bytes(range(33, 127)) * 213
    assert len(long) > 20000
    long = long[:20000]
    pairs = [(2, b"k%03d" % k) for k in range(40)] + [(2, b"k019" + long)] + [(2, b"k019" + long[:9000] + b"!")]
    ctx, entries, got = _go([pairs[:20], pairs[20:]])
    assert len(entries) == 42 and entries[20][1] == b"k019" + long[:9000] + b"!" and entries[21][1] == b"k019" + long
    assert model.decode_block(got, 1)[1][4:6] == [(0, 4, 9001), (0, 9004, 11000)]


def test_long_prefixes_a_handle_per_entry_and_far_handles():
    ctx, entries, got = _go(dictorder_cases.in_documents(dictorder_cases.long_prefix_group(), 9))
    fields = [f for j in range(len(got.block_handles)) for f in model.decode_block(got, j)[1]]
    assert [s for _, s, _ in fields] == [0 if k % 16 == 0 else 300 for k in range(70)]
    ctx, entries, got = _go([cases.handle_per_entry()[:35], cases.handle_per_entry()[35:]], nhandles=70)
    fields = [f for j in range(len(got.block_handles)) for f in model.decode_block(got, j)[1]]
    assert [h for h, _, _ in fields] == [0 if k % 16 == 0 else 1 for k in range(70)]
    ctx, entries, got = _go([cases.far_handles()], nhandles=299)
    assert bytes(got.bytes) == b"\0\0\4\1\1left" + b"\xc7\1\0\5\1\1right" + b"\0\5\1\1\1s"


def test_frequencies_of_two_and_three_bytes():
    """A term in 130 documents: a doc_freq of two bytes; a term 16 384 times in one document: a count of three bytes.  Longer codes
    of `count` (2^32 and above) are covered by tests/test_termblocks_abi.py: csrc/term_block_code.h composes the header for the
    twin and the device alike."""
    docs = [[(1, b"often")] for _ in range(130)] + [[(2, b"many")] * 16384]
    ctx, entries, got = _go(docs)
    assert entries == [(1, b"often", 130, 130), (2, b"many", 1, 16384)]
    assert bytes(got.bytes) == b"\0\0\5\x82\1\x82\1often" + b"\1\0\4\1\x80\x80\1many"


# ---- 5. every block size of the switch
@pytest.mark.parametrize("B", model.SIZES)
def test_every_block_size_on_the_device(B):
    pairs = dictorder_cases.numbered(250) + dictorder_cases.comparator_values() + cases.shared_lengths(7)
    with cases.block_entries(B):
        ctx, entries, got = _go(dictorder_cases.in_documents(pairs, 97))
        assert int(got.block_entries) == B and len(entries) > 280 and len(got.block_handles) == (len(entries) + B - 1) // B


# ---- 6. both sources
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
    ctx.finishedDictionaryOrderDevice(_stream())
    out = ctx.finishedTermBlocksDevice(_stream())
    entries, got = _assert_blocks(ctx, out, values=True)
    assert {(m.patternName(h), v) for h, v, _, _ in entries} == {("Lit", b"CHF"), ("Span", b"CHF"), ("Span", b"chf"), ("Span", b"eur"), ("Span", b"usd"), ("Plain", b"ab cd")}


# ---- 7. / 8. the order of the results
def test_plain_against_canonical_finish():
    docs = _trip_docs()
    found = []
    for canonical in (False, True):
        ctx, entries, got = _go(docs, canonical=canonical)
        found.append((entries, [getattr(got, f).tobytes() for f in model.FIELDS]))
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
        _ordered(ctx)
        out = ctx.finishedTermBlocksDevice(_stream())
        got.append(_assert_blocks(ctx, out))
    (entries_a, a), (entries_b, b) = got
    assert len(entries_a) > 100 and entries_a == entries_b
    for f in model.FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes()


# ---- 9. call order, buffers and streams
def test_call_order_other_products_buffers_and_streams():
    torch = _torch()
    m = _bare(8)
    docs = dictorder_cases.in_documents(dictorder_cases.numbered(700), 97)
    pieces, lex, seg, offs = _build(docs)
    ctx = m.createContext()
    src = Source(pieces)
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):              # before any batch
        ctx.finishedTermBlocksDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedTermBlocksFetch()
    with pytest.raises(spa.PatternError):
        ctx.lastTermBlocksMs()
    run = Run(ctx, lex, seg, offs)
    src.gather(ctx, items=False)
    ctx.finishedTermsDevice(T, _stream())
    ctx.finishedDictionaryDevice(_stream())
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):              # a dictionary, but no order
        ctx.finishedTermBlocksDevice(_stream())
    ctx.finishedDictionaryOrderDevice(_stream())
    # an allocation that fails, then a normal call
    L = capi.lib()
    out = capi.SpMatchTermBlocksDevice()
    L.sp_test_fail_alloc_above(1)
    try:
        assert L.sp_matcher_ctx_finished_term_blocks_device(ctx._h, None, ctypes.byref(out)) == -2       # SP_ERR_NOMEM
    finally:
        L.sp_test_fail_alloc_above(0)
    assert not out.d_bytes and out.ndict == 0 and out.nbytes == 0
    with pytest.raises(spa.PatternError):
        ctx.finishedTermBlocksFetch()
    first = ctx.finishedTermBlocksDevice(_stream())
    entries, got = _assert_blocks(ctx, first)
    assert len(entries) == 700 and ctx.lastTermBlocksMs() >= 0.0
    # postings and positions built after the blocks leave them as they are, and the reverse
    ctx.finishedPostingsDevice(_stream())
    ctx.finishedPositionsDevice(_stream())
    postings, positions = ctx.finishedPostingsFetch(), ctx.finishedPositionsFetch()
    model.assert_same(ctx.finishedTermBlocksFetch(), got)
    again = ctx.finishedTermBlocksDevice(_stream())
    model.assert_same(_assert_blocks(ctx, again)[1], got)
    postings_model.assert_same(ctx.finishedPostingsFetch(), postings)
    assert ctx.finishedPositionsFetch().occurrences.tobytes() == positions.occurrences.tobytes()
    # a new order call invalidates the fetch; a stream other than the order's, which is not waited for
    ctx.finishedDictionaryOrderDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedTermBlocksFetch()
    other = torch.cuda.Stream()
    second = ctx.finishedTermBlocksDevice(other.cuda_stream)
    assert second.d_bytes == first.d_bytes and second.d_block_offsets == first.d_block_offsets
    model.assert_same(_assert_blocks(ctx, second)[1], got)
    # a new dictionary, a new terms call: neither the order nor the blocks count
    for again in (lambda: ctx.finishedDictionaryDevice(_stream()), lambda: ctx.finishedTermsDevice(T, _stream())):
        again()
        with pytest.raises(spa.PatternError):
            ctx.finishedTermBlocksFetch()
        with pytest.raises(spa.PatternError, match=r"\(-1\)"):
            ctx.finishedTermBlocksDevice(_stream())
        _ordered(ctx)
        ctx.finishedTermBlocksDevice(_stream())
    # a new finish: the old order does not count
    run.match()
    ctx.batchFinishDevice(_stream())
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        ctx.finishedTermBlocksDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedTermBlocksFetch()
    # a smaller and then a larger batch on the same context: the buffers stay where they are while they are large enough
    for part, same in ((docs[:2], True), (dictorder_cases.in_documents(dictorder_cases.numbered(2500, arrival="descending"), 97), False)):
        pieces, lex, seg, offs = _build(part)
        src = Source(pieces)
        Run(ctx, lex, seg, offs)
        src.gather(ctx, items=False)
        _ordered(ctx)
        later = ctx.finishedTermBlocksDevice(_stream())
        for field in ("d_bytes", "d_block_offsets", "d_block_handles"):          # (the larger batch makes them grow: where to is the allocator's business)
            assert getattr(later, field) == getattr(first, field) or not same, field
        assert later.d_totals == first.d_totals
        entries, got = _assert_blocks(ctx, later)
        assert len(entries) == sum(len(doc) for doc in part) and ctx.lastTermBlocksMs() >= 0.0


# ---- 10. end to end
def test_segmented_documents_with_the_blocks():
    from struspattern_amd import rulelang, segments
    docs = [b"He paid 3'645 Eur\n\nand 3'645 Eur again or 12 sFr. he paid", b"nothing", b"12 sFr. in the year 1984 something happened",
            b"later 3'645 Eur were paid"]
    lx, m = spa.PatternLexerInstance(), spa.PatternMatcherInstance()
    rulelang.load(MONEY, lx, m)
    text, so, dso, _ = segments.segmented_batch(docs)
    found = spa.matchSegmentedDocs(lx.createContext(), m.createContext(), text, so, dso, with_term_blocks=True)
    assert len(found) == 7                                              # (no postings, no positions: the order and the blocks are the last elements)
    mb, mt, mv, terms, d, o, blocks = found
    assert isinstance(blocks, spa.MatchTermBlocks) and isinstance(o, spa.MatchDictionaryOrder)
    want = model.sorted_entries(d, dictorder_model.entries_of(mb, terms, d, mv, mt), o)
    model.assert_same(blocks, model.term_blocks(want, 16))
    model.assert_same(spa.batchTermBlocks(mb, terms, d, o, values=mv, text=mt), blocks)
    money = m.patternId("MoneyAmount")
    k = blocks.find(money, b"EUR 3'645")                                # (on the product alone)
    assert k is not None and blocks.entries()[k][:3] == (money, b"EUR 3'645", 2)
    assert blocks.find(money, b"EUR 3'646") is None
    everything = spa.matchSegmentedDocs(lx.createContext(), m.createContext(), text, so, dso, with_positions=True, with_term_blocks=True)
    assert len(everything) == 9 and isinstance(everything[6], spa.MatchPositions) and isinstance(everything[7], spa.MatchDictionaryOrder)
    model.assert_same(everything[8], blocks)


def _listing(capsys, argv):
    from struspattern_amd import match
    assert match.main(argv) == 0
    return capsys.readouterr().out.splitlines()


def test_match_blocks_listing(capsys, tmp_path):
    import os
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
        lines = {name: _listing(capsys, common + paragraphs + ["--blocks"] + files) for name, files in (("ab", [a, b]), ("ba", [b, a]))}
        blocks = {name: [line for line in out if line.startswith(("block ", "blocks "))] for name, out in lines.items()}
        assert blocks["ab"] == blocks["ba"]                             # the block lines do not depend on the order of the files
        # --blocks implies --sorted: the same listing, and the blocks behind it
        sorted_only = _listing(capsys, common + paragraphs + ["--sorted", a, b])
        assert [line for line in lines["ab"] if line not in blocks["ab"]] == sorted_only and lines["ab"][-len(blocks["ab"]) - 1:-1] == blocks["ab"]
        found = blocks["ab"]
        dicts = [line for line in sorted_only if line.startswith("dict ")]
        assert len(found) == (len(dicts) + 15) // 16 + 1 and all(line.startswith("block %d " % j) for j, line in enumerate(found[:-1]))
        assert found[-1].startswith("blocks %d bytes " % (len(found) - 1)) and " uncoded value bytes " in found[-1]
        assert sum(int(line.split(": entries ")[1].split(" ")[0]) for line in found[:-1]) == len(dicts)
        # the head of block j is the entry of dict line 16 j
        for j, line in enumerate(found[:-1]):
            name, value = dicts[16 * j][len("dict "):].split(" '", 1)
            assert line.startswith("block %d %s: " % (j, name)) and line.endswith(" head '" + value.rsplit("': docs ", 1)[0] + "'")
