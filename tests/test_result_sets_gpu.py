"""Result-set mode through the public interface (createContext(result_sets=True), sp_matcher_ctx_create_ex with
SP_CTX_RESULT_SETS) on COMPILED rule sets: per-document multisets of results with their items against the oracle and
against the exact engine, every batch entry point, the fallback of ineligible rule sets, the statistics that do not exist,
and the default context left as it was."""
from collections import Counter

import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from struspattern_amd import synth

from .result_set_model import results_multiset
from .finished_support import _docs, _sized

pytestmark = pytest.mark.gpu

SIZES = [(1, 50, 8, 300), (2, 400, 30, 500), (3, 3000, 200, 1000), (4, 20, 3, 200)]


def _pair(rules, weight_factor=None):
    m, o = spa.PatternMatcherInstance(), oracle.L2Matcher()
    for x in (m, o):
        if weight_factor is not None:
            x.defineOption("weightFactor", weight_factor)
        synth.apply_rules(x, rules, compile=True)
    return m, o


def _assert_same_multisets(got, ref, ndocs):
    assert np.array_equal(np.diff(got.doc_offsets.astype(np.int64)), np.diff(ref.doc_offsets.astype(np.int64)))
    for d in range(ndocs):
        a, b = results_multiset(got, d), results_multiset(ref, d)
        assert a == b, (d, list((a - b).items())[:2], list((b - a).items())[:2])
    assert len(got.items) == len(ref.items)


# `any` programs are never alt-keyed; they run in the operator mix (op None)
@pytest.mark.parametrize("op", ["sequence", "within", "sequence_struct", "within_struct", None])
@pytest.mark.parametrize("seed,nrules,nfeat,n", SIZES)
def test_result_sets_equal_the_oracle_on_compiled_rule_sets(seed, nrules, nfeat, n, op):
    rules = synth.random_rules(nrules, nfeat, seed, op=op)
    m, o = _pair(rules, 1.5)
    ok, why, alt = m.resultSetTier()
    assert ok and alt > 0, why
    ctx = m.createContext(result_sets=True)
    assert ctx.kernelKind() == 2
    rng = np.random.default_rng(100 + seed)
    lex, offs = _docs(rng, 24, n, nfeat, True)
    got = ctx.matchDocs(lex, offs)
    ref = o.run(synth.lexems5(lex), offs)
    assert ref.stats[:, 1].sum() > 0                       # the oracle replayed moved keys
    assert len(ref.results) > 100
    _assert_same_multisets(got, ref, len(offs) - 1)


@pytest.mark.parametrize("seed,nrules,nfeat,n", SIZES[1:3])
def test_result_sets_with_default_options(seed, nrules, nfeat, n):
    rules = synth.random_rules(nrules, nfeat, seed)
    m, o = _pair(rules)
    ctx = m.createContext(result_sets=True)
    assert ctx.kernelKind() == 2
    lex, offs = _docs(np.random.default_rng(100 + seed), 24, n, nfeat, True)
    got = ctx.matchDocs(lex, offs)
    ref = o.run(synth.lexems5(lex), offs)
    assert ref.stats[:, 1].sum() > 0
    _assert_same_multisets(got, ref, len(offs) - 1)
    assert ctx.getStatistics() is None


def _headline():
    vocab = synth.vocabulary(30000, 1)
    pats, rules = synth.pipeline_workload(10000, 10000, vocab, seed=4)
    text, offs = synth.text_documents(48, 16384, vocab, seed=1000, utf8=True)
    return pats, rules, text, offs


def test_result_sets_on_the_compiled_headline_rule_set():
    """bench.py's 10k + 10k pipeline workload, compiled: set mode equals the exact engine document by document"""
    pats, rules, text, offs = _headline()
    lxi = spa.PatternLexerInstance()
    synth.apply_lexer_patterns(lxi, pats)
    lex = lxi.createContext().matchDocs(text, offs)
    m = spa.PatternMatcherInstance()
    synth.apply_rules(m, rules, compile=True)
    ok, why, alt = m.resultSetTier()
    assert ok and alt > 0, why
    ctx, ectx = m.createContext(result_sets=True), m.createContext()
    assert ctx.kernelKind() == 2 and ectx.kernelKind() == 1
    got = ctx.matchDocs(lex.lexems, lex.doc_offsets)
    ref = ectx.matchDocs(lex.lexems, lex.doc_offsets)
    assert len(got.results) == len(ref.results) > 100000
    assert int(ref.stats[:, 1].sum()) > 0
    _assert_same_multisets(got, ref, len(offs) - 1)


def test_result_sets_on_the_device_entry_points():
    """matchDocsDevice, and matchLexedDevice behind the lexer kernel (the fused pipeline), in set mode"""
    import torch
    vocab = synth.vocabulary(2000, 5)
    pats, rules = synth.pipeline_workload(200, 500, vocab, 1)
    text, offs = synth.text_documents(16, 3000, vocab, 2, utf8=True)
    ndocs = len(offs) - 1
    lx = spa.PatternLexerInstance()
    synth.apply_lexer_patterns(lx, pats)
    m = spa.PatternMatcherInstance()
    synth.apply_rules(m, rules, compile=True)
    assert m.resultSetTier()[0]
    hl = lx.createContext().matchDocs(text, offs)
    ref = m.createContext().matchDocs(hl.lexems, hl.doc_offsets)
    assert len(ref.results) > 0
    stream = torch.cuda.current_stream().cuda_stream
    # host lexems uploaded, matchDocsDevice
    ctx = m.createContext(result_sets=True)
    assert ctx.kernelKind() == 2
    d_lex = torch.from_numpy(hl.lexems.astype(np.int32).reshape(-1)).cuda()
    d_off = torch.from_numpy(hl.doc_offsets.view(np.int64)).cuda()
    c = _sized(ctx, lambda: ctx.matchDocsDevice(d_lex.data_ptr(), d_off.data_ptr(), ndocs, len(hl.lexems), stream), ndocs, "matchDocsDevice")
    assert c["results"] == len(ref.results)
    _assert_same_multisets(ctx.batchFetch(), ref, ndocs)
    # the fused pipeline: lexer kernel -> lexems stay on the device -> join kernel
    lctx, fctx = lx.createContext(), m.createContext(result_sets=True)
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    lo = []
    lc = _sized(lctx, lambda: lo.append(lctx.matchDocsDevice(d_text.data_ptr(), d_offs.data_ptr(), ndocs, len(text), stream)), ndocs, "lexer")
    fc = _sized(fctx, lambda: fctx.matchLexedDevice(lo[-1].d_lexems, lo[-1].d_doc_ranges, ndocs, int(lc["lexems"]), stream), ndocs, "matchLexedDevice")
    assert fc["results"] == len(ref.results)
    _assert_same_multisets(fctx.batchFetch(), ref, ndocs)


def test_result_sets_through_put_input_and_fetch_results():
    rules = synth.random_rules(400, 30, 2)
    m, o = _pair(rules, 1.5)
    lex, offs = _docs(np.random.default_rng(7), 1, 500, 30, True)
    ref = o.run(synth.lexems5(lex), offs)
    assert ref.stats[:, 1].sum() > 0
    ctx = m.createContext(result_sets=True)
    assert ctx.kernelKind() == 2
    for lx in lex:
        ctx.putInput(int(lx[0]), int(lx[1]), int(lx[2]), int(lx[3]))
    res, items = ctx.fetchResults()
    got = Counter()
    for r in res.tolist():
        got[tuple(r[:7]) + (r[8],) + tuple(items[r[7]:r[7] + r[8]].reshape(-1).tolist())] += 1
    assert got == results_multiset(ref, 0) and len(res) > 100
    assert ctx.getStatistics() is None


def test_an_ineligible_rule_set_in_set_mode_runs_the_exact_engine():
    rules = synth.random_rules(200, 20, 5)
    m, o = spa.PatternMatcherInstance(), oracle.L2Matcher()
    for x in (m, o):
        synth.apply_rules(x, rules, compile=False)
        x.pushTerm(1); x.pushTerm(2); x.pushTerm(3)
        x.pushExpression("sequence", 3, 10, 0)                   # three terms: not for the join kernel
        x.definePattern("three", "", True)
        x.compile()
    ok, why, _ = m.resultSetTier()
    assert not ok and why
    ctx = m.createContext(result_sets=True)
    assert ctx.kernelKind() != 2
    lex, offs = _docs(np.random.default_rng(8), 8, 300, 20, True)
    got = ctx.matchDocs(lex, offs)
    ref = o.run(synth.lexems5(lex), offs)
    assert np.array_equal(got.doc_offsets, ref.doc_offsets) and len(ref.results) > 100
    assert np.array_equal(got.results[:, :7], ref.results[:, :7]) and np.array_equal(got.items, ref.items)
    assert ctx.getStatistics() is not None


def test_the_default_context_is_unchanged():
    """kind 1 on a flat set, the oracle's results in the oracle's order with its statistics"""
    rules = synth.random_rules(400, 30, 2)
    m, o = _pair(rules, 1.5)
    ctx = m.createContext()
    assert ctx.kernelKind() == 1
    lex, offs = _docs(np.random.default_rng(9), 12, 400, 30, True)
    got = ctx.matchDocs(lex, offs)
    ref = o.run(synth.lexems5(lex), offs)
    assert ref.stats[:, 1].sum() > 0
    assert np.array_equal(got.doc_offsets, ref.doc_offsets)
    assert np.array_equal(got.results[:, :7], ref.results[:, :7]) and np.array_equal(got.items, ref.items)
    assert np.array_equal(got.stats, ref.stats)
