"""The canonical order of a finished device batch (SP_FINISH_CANONICAL, include/strus_pattern_amd.h): every case runs a
batch through a device entry point, finishes it on the GPU with canonical=True and compares the plain copy of the
finished buffers (finishedFetch) EXACTLY, every document of it, with tests/canonical_order.py applied to what the host
regroup of the same batch returns (batchFetch) or to the oracle's results."""
import ctypes
import random

import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from struspattern_amd import capi, synth

from .canonical_order import canonical_key, in_canonical_order, sorted_batch
from .finished_support import _apply, _docs, _from_device, _random_program

pytestmark = pytest.mark.gpu


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class _Uploaded:
    """lexems and document offsets in device memory (kept alive as long as the batch is looked at)"""

    def __init__(self, lex, offs):
        import torch
        self.lex = torch.from_numpy(np.ascontiguousarray(lex, dtype=np.uint32).view(np.int32).reshape(-1)).cuda()
        self.offs = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.uint64).view(np.int64)).cuda()
        self.ndocs, self.nlex = len(offs) - 1, len(lex)

    def run(self, ctx, stream=None):
        return ctx.matchDocsDevice(self.lex.data_ptr(), self.offs.data_ptr(), self.ndocs, self.nlex, _stream() if stream is None else stream)


def _sized(ctx, run, ndocs, what, failing=()):
    """the device protocol (bench.py size_until_ok): a batch whose output did not fit is rerun with the counted sizes.
    `failing`: documents that are to fail with status 1 (lexems out of order), whatever the sizes"""
    for _ in range(8):
        run()
        c = ctx.batchCounters()
        status = ctx.batchStatus(ndocs)
        bad = set(int(d) for d in np.nonzero(status)[0])
        if bad == set(failing):
            assert all(int(status[d]) == 1 for d in failing), what
            return c
        assert set(int(status[d]) for d in bad - set(failing)) <= {2, 9}, what    # arena / output capacity only
        if "lexems" in c:
            ctx.reserveOutput(int(c["lexems"] * 1.2) + 1024)
        else:
            ctx.reserveOutput(int(c["results"] * 1.2) + 1024, int(c["items"] * 1.2) + 1024)
        ctx.growArena()
    raise AssertionError("%s: documents still failing after resizing" % what)


def _assert_layout(fin, got):
    """the finished arrays themselves: offsets from 0 to the totals, items in result order without gaps"""
    ndocs = fin.ndocs
    totals = _from_device(fin.d_totals, 2, np.uint64)
    roffs = _from_device(fin.d_doc_result_offsets, ndocs + 1, np.uint64)
    ioffs = _from_device(fin.d_doc_item_offsets, ndocs + 1, np.uint64)
    assert np.array_equal(roffs, got.doc_offsets)
    assert int(roffs[0]) == 0 and int(ioffs[0]) == 0
    assert np.all(np.diff(roffs.astype(np.int64)) >= 0) and np.all(np.diff(ioffs.astype(np.int64)) >= 0)
    assert int(roffs[-1]) == int(totals[0]) == len(got.results)
    assert int(ioffs[-1]) == int(totals[1]) == len(got.items)
    counts = got.results[:, 8].astype(np.int64)
    running = np.cumsum(counts) - counts
    assert np.array_equal(got.results[:, 7].astype(np.int64), running)
    if len(counts):
        assert int(got.results[-1, 7]) + int(got.results[-1, 8]) == int(totals[1])
    nonempty = np.diff(roffs.astype(np.int64)) > 0
    first = roffs[:-1][nonempty].astype(np.int64)
    assert np.array_equal(got.results[first, 7].astype(np.int64), ioffs[:-1][nonempty].astype(np.int64))


def _assert_same_results(got, ref, formats=False):
    assert np.array_equal(got.doc_offsets, ref.doc_offsets)
    assert np.array_equal(got.results, ref.results)              # all nine columns
    assert np.array_equal(got.items, ref.items)
    if formats:
        assert ref.result_format is not None and ref.item_format is not None
        assert np.array_equal(got.result_format, ref.result_format)
        assert np.array_equal(got.item_format, ref.item_format)
    else:
        assert got.result_format is None and got.item_format is None


def _canonical(ctx, formats=False, stream=None):
    """the canonical finish of the context's batch, compared with the sorted host regroup of the same batch"""
    engine = ctx.batchFetch()
    want = sorted_batch(engine)
    fin = ctx.batchFinishDevice(_stream() if stream is None else stream, canonical=True)
    got = ctx.finishedFetch()
    _assert_same_results(got, want, formats)
    assert np.array_equal(got.status, engine.status) and np.array_equal(got.stats, engine.stats)
    _assert_layout(fin, got)
    assert ctx.lastFinishSortMs() > 0.0 and all(ms >= 0.0 for ms in ctx.lastFinishMs())
    return engine, got


RULES = (2, 400, 30, 500)          # seed, rules, features, lexems per document: the size of tests/test_result_sets_gpu.py


def _rule_set(with_and=False):
    seed, nrules, nfeat, _ = RULES
    rules = synth.random_rules(nrules, nfeat, seed)
    if with_and:
        rules.append(("and_%d" % nrules, "and", 3, [1, 2]))     # (not a flat rule set: the general kernel)
    m = spa.PatternMatcherInstance()
    synth.apply_rules(m, rules, compile=True)
    return m


def _shared_position_docs():
    seed, _, nfeat, n = RULES
    return _docs(np.random.default_rng(100 + seed), 24, n, nfeat, True)


# ---- 1. against the host, all three kernels
@pytest.mark.parametrize("kind", [1, 2, 0])
def test_canonical_finish_equals_the_sorted_host_regroup(kind):
    m = _rule_set(with_and=(kind == 0))
    ctx = m.createContext(result_sets=(kind == 2))
    assert ctx.kernelKind() == kind
    up = _Uploaded(*_shared_position_docs())
    c = _sized(ctx, lambda: up.run(ctx), up.ndocs, "matchDocsDevice")
    engine, got = _canonical(ctx)
    assert len(got.results) == c["results"] > 1000
    assert not all(in_canonical_order(engine, d) for d in range(up.ndocs))     # (else the case shows nothing)
    assert all(in_canonical_order(got, d) for d in range(up.ndocs))


# ---- 2. same bytes from both engines
def test_both_engines_finish_to_the_same_bytes():
    m = _rule_set()
    up = _Uploaded(*_shared_position_docs())
    finished = []
    for result_sets, kind in ((False, 1), (True, 2)):
        ctx = m.createContext(result_sets=result_sets)
        assert ctx.kernelKind() == kind
        _sized(ctx, lambda: up.run(ctx), up.ndocs, "matchDocsDevice")
        fin = ctx.batchFinishDevice(_stream(), canonical=True)
        got = ctx.finishedFetch()
        ioffs = _from_device(fin.d_doc_item_offsets, up.ndocs + 1, np.uint64)
        finished.append((got, ioffs))
    (a, ai), (b, bi) = finished
    assert len(a.results) > 1000
    _assert_same_results(a, b)
    assert np.array_equal(ai, bi)


def test_both_engines_finish_to_the_same_bytes_on_the_fused_pipeline():
    """lexer matchDocsDevice -> matchLexedDevice -> canonical finish"""
    import torch
    vocab = synth.vocabulary(2000, 5)
    pats, rules = synth.pipeline_workload(200, 500, vocab, 1)
    text, offs = synth.text_documents(16, 3000, vocab, 2, utf8=True)
    ndocs = len(offs) - 1
    lx = spa.PatternLexerInstance()
    synth.apply_lexer_patterns(lx, pats)
    m = spa.PatternMatcherInstance()
    synth.apply_rules(m, rules, compile=True)
    stream = _stream()
    lctx = lx.createContext()
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    lo = []
    lc = _sized(lctx, lambda: lo.append(lctx.matchDocsDevice(d_text.data_ptr(), d_offs.data_ptr(), ndocs, len(text), stream)), ndocs, "lexer")
    finished = []
    for result_sets, kind in ((False, 1), (True, 2)):
        fctx = m.createContext(result_sets=result_sets)
        assert fctx.kernelKind() == kind
        _sized(fctx, lambda: fctx.matchLexedDevice(lo[-1].d_lexems, lo[-1].d_doc_ranges, ndocs, int(lc["lexems"]), stream), ndocs, "matchLexedDevice")
        engine, got = _canonical(fctx)
        finished.append(got)
    assert len(finished[0].results) > 0
    _assert_same_results(finished[0], finished[1])


# ---- 3. size edges
def _edge_rules(m):
    """a few two-term `any` rules (a lexem of a covered id gives one result per rule), two of them over the same terms
    under one pattern name with different variables (their results tie in words 0..6 and 8: the items decide), and a
    `within` rule, whose result lies before results that fired earlier"""
    for name, op, rg, terms, var in (("dup", "any", 1, (1, 2), "A"), ("dup", "any", 1, (1, 2), "B"),
                                     ("one", "any", 1, (5, 6), "A"), ("win", "within", 3, (3, 4), "A")):
        for i, t in enumerate(terms):
            m.pushTerm(t)
            m.attachVariable("%s%d" % (var, i))
        m.pushExpression(op, len(terms), rg, 0)
        m.definePattern(name, "", True)
    m.compile()


def _edge_document(count, one_position):
    """lexems (n,4) of a document with exactly `count` results under _edge_rules"""
    ids, pos = [], []
    p = 1
    if not one_position:
        for _ in range(min(count // 8, 5)):            # 3 results each: the within pair and the two `dup` results between its ends
            ids += [3, 1, 4]
            pos += [p, p + 1, p + 2]
            p += 10
    rest = count - len(ids)
    for i in range(rest // 2):
        ids.append(1 + i % 2)
        pos.append(p)
        p += i % 3 != 0                                # (some lexems share a position)
    if rest % 2:
        ids.append(5)
        pos.append(p)
    lex = np.zeros((len(ids), 4), np.uint32)
    lex[:, 0] = ids
    lex[:, 1] = 1 if one_position else pos
    lex[:, 2] = np.arange(len(ids)) * 3
    lex[:, 3] = 2
    return lex


def _edge_batch():
    """the documents of the size edges: (result counts, index of the failed document, lexems, offsets)"""
    tile = int(capi.lib().sp_matcher_finish_sort_tile())
    counts = [0, 1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 200, 2 * tile + 3, 5 * tile + 1, 65, tile + 1]
    one_position = [False] * 12 + [True, True]
    failed = 9
    parts = [_edge_document(c, f) for c, f in zip(counts, one_position)]
    parts[failed][:, 1] = parts[failed][:, 1][::-1].copy()          # descending ordpos: status 1
    counts[failed] = 0
    offs = np.zeros(len(parts) + 1, np.uint64)
    offs[1:] = np.cumsum([len(p) for p in parts])
    return counts, failed, np.concatenate(parts), offs


@pytest.mark.parametrize("result_sets", [False, True])
def test_size_edges_of_the_sort(result_sets):
    counts, failed, lex, offs = _edge_batch()
    m = spa.PatternMatcherInstance()
    _edge_rules(m)
    ctx = m.createContext(result_sets=result_sets)
    assert ctx.kernelKind() == (2 if result_sets else 1)
    up = _Uploaded(lex, offs)
    _sized(ctx, lambda: up.run(ctx), up.ndocs, "matchDocsDevice", failing=(failed,))
    engine = ctx.batchFetch()
    assert [int(x) for x in np.diff(engine.doc_offsets.astype(np.int64))] == counts
    # a tie in words 0..6 and 8 that the items decide
    keys = [canonical_key(engine, r) for r in range(int(engine.doc_offsets[4]), int(engine.doc_offsets[5]))]
    assert any(a[:8] == b[:8] and a != b for a in keys for b in keys)
    # the documents at one position: one key64 for all their results
    for d in (12, 13):
        assert len(np.unique(engine.doc(d)[:, 1:3], axis=0)) == 1
    assert not all(in_canonical_order(engine, d) for d in range(up.ndocs))
    engine, got = _canonical(ctx)
    assert int(got.status[failed]) == 1 and not np.any(np.delete(got.status, failed))
    assert got.doc_offsets[failed] == got.doc_offsets[failed + 1]
    assert all(in_canonical_order(got, d) for d in range(up.ndocs))


# ---- 4. `exclusive`
@pytest.mark.parametrize("rules_docs,max_result_size", [
    (((300, 20, 3), (60, 200, 20, 4)), 30),
    (((300, 20, 3), (60, 200, 20, 4)), 200),
    (((400, 30, 3), (300, 600, 30, 4)), 30),               # 2 695 868 raw results, up to 10 073 in one document: several tiles
])
def test_exclusive_survivors_are_sorted(rules_docs, max_result_size):
    rules = synth.random_rules(*rules_docs[0])
    lex, offs = synth.random_documents(*rules_docs[1])
    m = spa.PatternMatcherInstance()
    m.defineOption("exclusive")
    m.defineOption("maxResultSize", max_result_size)
    synth.apply_rules(m, rules)
    up = _Uploaded(lex, offs)
    ctx = m.createContext()
    c = _sized(ctx, lambda: up.run(ctx), up.ndocs, "matchDocsDevice")
    engine, got = _canonical(ctx)
    assert 0 < len(got.results) < c["results"]             # finished < raw
    assert not all(in_canonical_order(engine, d) for d in range(up.ndocs))


# ---- 5. format strings
def test_format_words_travel_with_their_records():
    rng = random.Random(9100 + 2)
    nterms = 6
    calls = _random_program(rng, nterms)
    mt = spa.PatternMatcherInstance()
    _apply(mt, calls)
    lex, offs = synth.random_documents(200, 150, nterms, seed=52)
    up = _Uploaded(lex, offs)
    ctx = mt.createContext()
    assert ctx.kernelKind() == 0
    _sized(ctx, lambda: up.run(ctx), up.ndocs, "matchDocsDevice")
    engine, got = _canonical(ctx, formats=True)
    assert len(got.results) > 50 and int(got.item_format[:, 1].max()) > 0        # items with sub-records
    assert int(got.item_format[:, 0].max()) > 0 or int(got.result_format.max()) > 0
    assert not all(in_canonical_order(engine, d) for d in range(up.ndocs))


# ---- 6. interface rules
def test_interface_rules():
    import torch
    rules = synth.random_rules(300, 20, 3)
    m = spa.PatternMatcherInstance()
    synth.apply_rules(m, rules)
    lex, offs = synth.random_documents(10, 100, 20, 5)
    up = _Uploaded(lex, offs)
    ctx = m.createContext()
    L, out = capi.lib(), capi.SpMatchFinishedBatch()
    # before any batch
    assert L.sp_matcher_ctx_batch_finish_device_ex(ctx._h, None, spa.SP_FINISH_CANONICAL, ctypes.byref(out)) == -1      # SP_ERR_INVALID
    with pytest.raises(spa.PatternError, match="no batch"):
        ctx.batchFinishDevice(_stream(), canonical=True)
    _sized(ctx, lambda: up.run(ctx), up.ndocs, "matchDocsDevice")
    # an unknown flag
    assert L.sp_matcher_ctx_batch_finish_device_ex(ctx._h, None, 2, ctypes.byref(out)) == -1
    assert L.sp_matcher_ctx_batch_finish_device_ex(ctx._h, None, spa.SP_FINISH_CANONICAL | 0x80000000, ctypes.byref(out)) == -1
    engine, small = _canonical(ctx)
    # without the flag after with it: the engine's order again, and no sorting time
    ctx.batchFinishDevice(_stream())
    plain = ctx.finishedFetch()
    _assert_same_results(plain, engine)
    assert ctx.lastFinishSortMs() == 0.0
    # flags == 0 is the old entry point
    assert L.sp_matcher_ctx_batch_finish_device_ex(ctx._h, None, 0, ctypes.byref(out)) == 0
    _assert_same_results(ctx.finishedFetch(), engine)
    # a larger batch on the same context: the working memory grows
    lex2, offs2 = synth.random_documents(40, 200, 20, 4)
    up2 = _Uploaded(lex2, offs2)
    _sized(ctx, lambda: up2.run(ctx), up2.ndocs, "matchDocsDevice")
    engine2, large = _canonical(ctx)
    assert len(large.results) > 4 * len(small.results)
    # on another stream than the batch's
    other = torch.cuda.Stream()
    up2.run(ctx)
    engine3, again = _canonical(ctx, stream=other.cuda_stream)
    _assert_same_results(again, large)


# ---- 7. against the oracle
def test_canonical_finish_equals_the_sorted_oracle_results():
    rules = synth.random_rules(300, 20, 3)
    m, o = spa.PatternMatcherInstance(), oracle.L2Matcher()
    for x in (m, o):
        synth.apply_rules(x, rules)
    lex, offs = synth.random_documents(12, 200, 20, 4)
    up = _Uploaded(lex, offs)
    ctx = m.createContext()
    _sized(ctx, lambda: up.run(ctx), up.ndocs, "matchDocsDevice")
    ctx.batchFinishDevice(_stream(), canonical=True)
    got = ctx.finishedFetch()
    want = sorted_batch(o.run(synth.lexems5(lex), offs))
    assert len(want.results) > 1000
    _assert_same_results(got, want)
