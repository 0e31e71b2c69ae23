"""Posting blocks on the device (sp_matcher_ctx_finished_posting_blocks_device, csrc/l2_postingblocks.h): the bytes,
block_offsets and totals that the launches leave must EQUAL what the device-free twin (sp_match_batch_posting_blocks) makes of
the fetched dictionary, order, postings and positions, and the model (tests/postingblocks_model.py); they decode to the lists,
and the device pointers of `out` hold the same bytes.  Bare-term matchers over hand-made lexems as in
tests/test_termblocks_gpu.py: a test sets every handle, value and position itself, so it decides every list and every byte."""
import ctypes

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from tests import postingblocks_cases as cases
from tests import postingblocks_model as model
from tests.finished_support import _bare, _from_device, MONEY, Run, Source, _stream, _torch, _trip_docs

pytestmark = pytest.mark.gpu

T = spa.SP_TERM_TEXT


def _assert_blocks(ctx, out=None):
    """the fetched blocks equal the twin's and the model's on the fetched dictionary, order, postings and positions, decode to
    the lists, and the bytes behind the device pointers are the fetched ones; returns (lists, blocks)"""
    d, order, postings, positions = ctx.finishedDictionaryFetch(), ctx.finishedDictionaryOrderFetch(), ctx.finishedPostingsFetch(), ctx.finishedPositionsFetch()
    got = ctx.finishedPostingBlocksFetch()
    B = int(got.block_entries)
    assert B == capi.lib().sp_matcher_term_block_entries()
    want_lists = model.lists_of(order, postings, positions)
    want = model.posting_blocks(want_lists, B)
    model.assert_same(spa.batchPostingBlocks(d, order, postings, positions), want)
    model.assert_same(got, want)
    model.check_invariants(got, want_lists)
    assert int(got.totals[3]) == int(positions.totals[1])
    assert got.lists() == want_lists                                   # the library's reader
    if out is not None:
        nblocks, nbytes = len(got.block_offsets) - 1, len(got.bytes)
        assert (out.ndict, out.nblocks, out.nbytes, out.block_entries) == (len(want_lists), nblocks, nbytes, B)
        assert np.array_equal(_from_device(out.d_totals, 4, np.uint64), got.totals)
        assert np.array_equal(_from_device(out.d_bytes, nbytes, np.uint8), got.bytes)
        assert np.array_equal(_from_device(out.d_block_offsets, nblocks + 1, np.uint64), got.block_offsets)
    return want_lists, got


def _inputs(ctx, order=True, postings=True, positions=True):
    """terms and dictionary of the text terms of the finished batch of `ctx`, and its order, postings and positions"""
    ctx.finishedTermsDevice(T, _stream())
    ctx.finishedDictionaryDevice(_stream())
    if order:
        ctx.finishedDictionaryOrderDevice(_stream())
    if postings:
        ctx.finishedPostingsDevice(_stream())
    if postings and positions:
        ctx.finishedPositionsDevice(_stream())


def _start(docs, nhandles=8, canonical=False, ctx=None):
    m = _bare(nhandles)
    pieces, lex, seg, offs = cases.build_at(docs)
    ctx = ctx or m.createContext()
    src = Source(pieces)
    run = Run(ctx, lex, seg, offs, canonical=canonical)
    src.gather(ctx, items=False)
    return ctx, run


def _go(docs, nhandles=8, canonical=False):
    """the posting blocks of the text terms of hand-made documents of (handle, value, ordpos): (context, lists, blocks)"""
    ctx, _ = _start(docs, nhandles, canonical)
    _inputs(ctx)
    out = ctx.finishedPostingBlocksDevice(_stream())
    lists, got = _assert_blocks(ctx, out)
    return ctx, lists, got


# ---- 1. empty shapes
def test_no_documents_empty_documents_and_one_term_once():
    m = _bare(8)
    ctx = m.createContext()
    src = Source([])
    Run(ctx, np.zeros((0, 4), np.uint32), np.zeros(0, np.uint32), np.zeros(1, np.uint64))
    src.gather(ctx, items=False)
    _inputs(ctx)
    out = ctx.finishedPostingBlocksDevice(_stream())
    lists, got = _assert_blocks(ctx, out)
    assert lists == [] and got.block_offsets.tolist() == [0] and got.totals.tolist() == [0, 0, 16, 0] and len(got.bytes) == 0
    ctx, lists, got = _go([[], [], []])
    assert lists == [] and got.block_offsets.tolist() == [0] and got.totals.tolist() == [0, 0, 16, 0]
    ctx, lists, got = _go([[], [(3, b"only", 7)]])
    assert lists == [[(1, 1, [7])]] and bytes(got.bytes) == b"\4\1\1\1\7" and got.block_offsets.tolist() == [0, 5] and got.totals.tolist() == [1, 5, 16, 1]
    assert ctx.lastPostingBlocksMs() >= 0.0


# ---- 2. posting wave edges
@pytest.mark.parametrize("n,arrival", [(63, "shuffle"), (64, "descending"), (65, "shuffle"), (129, "descending"), (64 * 5 - 3, "shuffle")])
def test_posting_wave_edges(n, arrival):
    ctx, lists, got = _go(cases.postings_in(n, arrival), nhandles=3)
    assert len(lists) == n and sum(len(e) for e in lists) == n


# ---- 3. list edges
@pytest.mark.parametrize("ndocs", [65, 130])
def test_a_list_that_crosses_waves(ndocs):
    """a term in 65 and in 130 documents, every second document skipped twice over: the list crosses waves, and a ddelta of 130
    takes two bytes"""
    docs, at = [], 0
    for k in range(ndocs):
        docs += [[]] * (130 if k == ndocs // 2 else k % 2)
        docs.append([(2, b"often", k % 5 + 1), (1, b"n%03d" % k, k % 5 + 2)])
    ctx, lists, got = _go(docs)
    long = [e for e in lists if len(e) == ndocs]
    assert len(long) == 1 and len(lists) == ndocs + 1 and any(b[0] - a[0] == 131 for a, b in zip(long[0], long[0][1:]))


def test_a_list_that_begins_on_the_last_lane_of_a_wave():
    """63 terms of one posting each sort in front of a term in 70 documents: its list begins at sorted posting 63"""
    docs = [[(1, b"a%02d" % k, 1) for k in range(63)]] + [[(2, b"zz", d + 1)] for d in range(70)]
    ctx, lists, got = _go(docs)
    assert [len(e) for e in lists] == [1] * 63 + [70]


# ---- 4. trip edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_a_posting_of_n_occurrences(n):
    docs = [[(1, b"before", 1)], [(2, b"many", 2 * i + 1) for i in range(n)] + [(3, b"behind", 2 * n)]]
    ctx, lists, got = _go(docs)
    assert lists == [[(0, 1, [1])], [(1, n, [2 * i + 1 for i in range(n)])], [(1, 1, [2 * n])]]


def test_sixty_four_postings_of_one_occurrence():
    """every lane of the trip carries a header"""
    ctx, lists, got = _go(cases.postings_in(64, "shuffle", per_doc=64), nhandles=3)
    assert len(lists) == 64 and all(len(e) == 1 and e[0][1] == 1 for e in lists)


# ---- 5. repeated ordpos
def test_repeated_positions_at_the_start_the_middle_and_the_end_of_a_trip():
    """count > npos: a run of occurrences at one position gives lanes without a byte; runs of 10 at the occurrences 1.., 27.. and
    54.. of the first trip of a posting of 64 + 30 occurrences, whose second trip starts inside a run"""
    pos, x = [], 1
    for i in range(94):
        if not (1 <= i <= 10 or 27 <= i <= 36 or 54 <= i <= 68):
            x += 3
        pos.append(x)
    docs = [[(1, b"t", p) for p in pos], [(1, b"t", 4), (1, b"t", 4), (2, b"u", 4)]]
    ctx, lists, got = _go(docs)
    assert lists == [[(0, 94, sorted(set(pos))), (1, 2, [4])], [(1, 1, [4])]] and len(set(pos)) == 94 - 35


# ---- 6. alignment
def test_spans_that_start_at_every_alignment():
    """postings of 64 occurrences whose gaps take one byte but for k two-byte gaps in posting k: the spans of consecutive trips
    are 4 + 64 + k bytes (body and header in front of the first), so they start at every alignment mod 4"""
    docs = []
    for k in range(6):
        x, doc = 0, []
        for i in range(64):
            x += 200 if i and i <= k else 1
            doc.append((1, b"v%d" % k, x))
        docs.append(doc)
    ctx, lists, got = _go(docs)
    codes = [model.list_code(e) for e in lists]
    starts = set(int(np.sum([len(c) for c in codes[:k]])) % 4 for k in range(len(codes)))
    assert starts == {0, 1, 2, 3} and all(len(e) == 1 and e[0][1] == 64 for e in lists)


# ---- 7. every block size of the switch
@pytest.mark.parametrize("B", model.SIZES)
def test_every_block_size_on_the_device(B):
    docs = cases.postings_in(150, "shuffle") + [[(2, b"w%05d" % k, 3), (2, b"w%05d" % k, 3), (2, b"w%05d" % (k + 1), 900)] for k in range(0, 100, 7)]
    with cases.block_entries(B):
        ctx, _ = _start(docs, nhandles=3)
        _inputs(ctx)
        out = ctx.finishedPostingBlocksDevice(_stream())
        lists, got = _assert_blocks(ctx, out)
        ctx.finishedTermBlocksDevice(_stream())
        terms = ctx.finishedTermBlocksFetch()
    assert int(got.block_entries) == B == int(terms.block_entries) and len(got.block_offsets) - 1 == len(terms.block_handles) == (len(lists) + B - 1) // B
    assert got.ndict == terms.ndict == len(lists)
    for j in range(len(terms.block_handles)):
        entries, block = terms.block(j), got.block(j)
        assert [e[2] for e in entries] == [len(e) for e in block]      # the doc_freq of a term-block position is the length of its list


# ---- 8. the order of the results
def test_plain_against_canonical_finish():
    docs = cases.counted(_trip_docs())
    found = []
    for canonical in (False, True):
        ctx, lists, got = _go(docs, canonical=canonical)
        found.append((lists, [getattr(got, f).tobytes() for f in model.FIELDS]))
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
        _inputs(ctx)
        out = ctx.finishedPostingBlocksDevice(_stream())
        got.append(_assert_blocks(ctx, out))
    (lists_a, a), (lists_b, b) = got
    assert len(lists_a) > 100 and lists_a == lists_b
    for f in model.FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes()


# ---- 9. call order, buffers and streams
def test_call_order_other_products_buffers_and_streams():
    torch = _torch()
    docs = cases.postings_in(700, "shuffle")
    h, v, _ = docs[0][0]
    docs.append([(h, v, 2), (h, v, 2), (h, v, 5)])                      # (a term of the first document again: 700 entries, 701 postings)
    ctx = _bare(3).createContext()
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):              # before any batch
        ctx.finishedPostingBlocksDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedPostingBlocksFetch()
    with pytest.raises(spa.PatternError):
        ctx.lastPostingBlocksMs()
    ctx, run = _start(docs, nhandles=3, ctx=ctx)
    # one of the three inputs missing
    for missing in ("order", "postings", "positions"):
        _inputs(ctx, **{missing: False})
        with pytest.raises(spa.PatternError, match=r"\(-1\)"):
            ctx.finishedPostingBlocksDevice(_stream())
    _inputs(ctx)
    # an allocation that fails, then a normal call
    L = capi.lib()
    out = capi.SpMatchPostingBlocksDevice()
    L.sp_test_fail_alloc_above(1)
    try:
        assert L.sp_matcher_ctx_finished_posting_blocks_device(ctx._h, None, ctypes.byref(out)) == -2       # SP_ERR_NOMEM
    finally:
        L.sp_test_fail_alloc_above(0)
    assert not out.d_bytes and out.ndict == 0 and out.nbytes == 0
    with pytest.raises(spa.PatternError):
        ctx.finishedPostingBlocksFetch()
    first = ctx.finishedPostingBlocksDevice(_stream())
    lists, got = _assert_blocks(ctx, first)
    assert len(lists) == 700 and ctx.lastPostingBlocksMs() >= 0.0
    # term blocks built after the posting blocks leave them as they are, and the reverse
    ctx.finishedTermBlocksDevice(_stream())
    terms = ctx.finishedTermBlocksFetch()
    model.assert_same(ctx.finishedPostingBlocksFetch(), got)
    again = ctx.finishedPostingBlocksDevice(_stream())
    model.assert_same(_assert_blocks(ctx, again)[1], got)
    assert ctx.finishedTermBlocksFetch().bytes.tobytes() == terms.bytes.tobytes()
    # a rebuilt order, postings or positions invalidates the fetch; a stream other than theirs, which is not waited for
    other = torch.cuda.Stream()
    for rebuild in (lambda: ctx.finishedDictionaryOrderDevice(_stream()), lambda: ctx.finishedPositionsDevice(_stream()),
                    lambda: (ctx.finishedPostingsDevice(_stream()), ctx.finishedPositionsDevice(_stream()))):
        rebuild()
        with pytest.raises(spa.PatternError):
            ctx.finishedPostingBlocksFetch()
        second = ctx.finishedPostingBlocksDevice(other.cuda_stream)
        assert second.d_bytes == first.d_bytes and second.d_block_offsets == first.d_block_offsets
        model.assert_same(_assert_blocks(ctx, second)[1], got)
    # new postings without their positions: refused
    ctx.finishedPostingsDevice(_stream())
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        ctx.finishedPostingBlocksDevice(_stream())
    # a new finish: the old inputs do not count
    run.match()
    ctx.batchFinishDevice(_stream())
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        ctx.finishedPostingBlocksDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedPostingBlocksFetch()
    # a smaller and then a larger batch on the same context
    for part in (docs[:2], cases.postings_in(2500, "descending")):
        _start(part, nhandles=3, ctx=ctx)
        _inputs(ctx)
        later = ctx.finishedPostingBlocksDevice(_stream())
        assert later.d_totals == first.d_totals
        lists, got = _assert_blocks(ctx, later)
        assert len(lists) == sum(len(doc) for doc in part) and ctx.lastPostingBlocksMs() >= 0.0


# ---- 10. end to end
def test_segmented_documents_with_the_posting_blocks():
    from struspattern_amd import rulelang, segments
    docs = [b"He paid 3'645 Eur\n\nand 3'645 Eur again or 12 sFr. he paid", b"nothing", b"12 sFr. in the year 1984 something happened",
            b"later 3'645 Eur were paid"]
    lx, m = spa.PatternLexerInstance(), spa.PatternMatcherInstance()
    rulelang.load(MONEY, lx, m)
    text, so, dso, _ = segments.segmented_batch(docs)
    found = spa.matchSegmentedDocs(lx.createContext(), m.createContext(), text, so, dso, with_term_blocks=True, with_posting_blocks=True)
    assert len(found) == 10
    mb, mt, mv, terms, d, p, q, o, blocks, pblocks = found
    assert isinstance(blocks, spa.MatchTermBlocks) and isinstance(pblocks, spa.MatchPostingBlocks) and isinstance(q, spa.MatchPositions)
    want = model.lists_of(o, p, q)
    model.assert_same(pblocks, model.posting_blocks(want, 16))
    model.assert_same(spa.batchPostingBlocks(d, o, p, q), pblocks)
    k = blocks.find(m.patternId("MoneyAmount"), b"EUR 3'645")               # (on the two products alone)
    e = int(o.order[k])
    held = [(int(p.entry(e)[i, 0]), int(p.entry(e)[i, 2]), q.positions(int(p.entry_offsets[e]) + i).tolist()) for i in range(len(p.entry(e)))]
    assert pblocks.postings(k) == held and [doc for doc, _, _ in held] == [0, 3] and len(held[0][2]) == 2
    alone = spa.matchSegmentedDocs(lx.createContext(), m.createContext(), text, so, dso, with_posting_blocks=True)
    assert len(alone) == 9 and isinstance(alone[7], spa.MatchDictionaryOrder)
    model.assert_same(alone[8], pblocks)


def _listing(capsys, argv):
    from struspattern_amd import match
    assert match.main(argv) == 0
    return capsys.readouterr().out.splitlines()


def test_match_posting_blocks_listing(capsys, tmp_path):
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    prog = os.path.join(here, "golden", "doc_example.rul")
    a, b = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    with open(os.path.join(here, "golden", "doc_example.txt"), "rb") as f:
        example = f.read().replace(b"\n", b" ")
    with open(a, "wb") as f:
        f.write(example)
    with open(b, "wb") as f:
        f.write(b"Prof. Anna B. Smith wrote to anna@etc.com. " + example[:len(example) // 2])
    common = ["-p", prog, "--device-values"]
    for paragraphs in ([], ["--paragraphs"]):
        lines = {name: _listing(capsys, common + paragraphs + ["--posting-blocks"] + files) for name, files in (("ab", [a, b]), ("ba", [b, a]))}
        found = {name: [line for line in out if line.startswith(("postblock ", "postblocks "))] for name, out in lines.items()}
        blocks = [line for line in lines["ab"] if line.startswith("block ")]
        assert len(found["ab"]) == len(blocks) + 1 and lines["ab"][-len(found["ab"]) - 1:-1] == found["ab"]
        assert found["ab"] == found["ba"]                               # the lines do not depend on the order of the files
        assert sum(int(line.split(": lists ")[1].split(" ")[0]) for line in found["ab"][:-1]) == len([line for line in lines["ab"] if line.startswith("dict ")])
        # --posting-blocks implies --blocks and --positions: the same listing without the new lines
        assert [line for line in lines["ab"] if line not in found["ab"]] == _listing(capsys, common + paragraphs + ["--blocks", "--positions", a, b])
