"""Finishing a device batch on the device (sp_matcher_ctx_batch_finish_device, csrc/l2_finish.h): every case runs a batch
through a device entry point, finishes it on the GPU and compares the plain copy of the finished buffers
(finishedFetch) EXACTLY with what the host regroup of the same batch returns (batchFetch), and with the oracle where a
run of it is cheap."""
import random

import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from struspattern_amd import synth

from .canonical_order import sorted_batch
from .finished_support import _apply, _docs, _from_device, _random_program, _sized, _stream, _Uploaded

pytestmark = pytest.mark.gpu


def _raw_ranges(ctx, dev):
    ctx.batchCounters()      # (waits for the batch)
    return _from_device(dev.d_doc_result_offsets, 2 * dev.ndocs, np.uint64).reshape(-1, 2)


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
    # the item offsets of the documents are the item_begin of their first result
    first = roffs[:-1][np.diff(roffs.astype(np.int64)) > 0].astype(np.int64)
    assert np.array_equal(got.results[first, 7].astype(np.int64), ioffs[:-1][np.diff(roffs.astype(np.int64)) > 0].astype(np.int64))


def _assert_same_batch(got, ref, formats):
    assert np.array_equal(got.doc_offsets, ref.doc_offsets)
    assert np.array_equal(got.results, ref.results)              # all nine columns
    assert np.array_equal(got.items, ref.items)
    assert np.array_equal(got.status, ref.status)
    assert np.array_equal(got.stats, ref.stats)
    if formats:
        assert ref.result_format is not None and ref.item_format is not None
        assert np.array_equal(got.result_format, ref.result_format)
        assert np.array_equal(got.item_format, ref.item_format)
    else:
        assert got.result_format is None and got.item_format is None and ref.result_format is None


def _finish_and_compare(ctx, formats=False, stream=None):
    fin = ctx.batchFinishDevice(_stream() if stream is None else stream)
    got = ctx.finishedFetch()
    ref = ctx.batchFetch()
    _assert_same_batch(got, ref, formats)
    _assert_layout(fin, got)
    return fin, got


def _assert_oracle(got, ref):
    assert np.array_equal(got.doc_offsets, ref.doc_offsets)
    assert np.array_equal(got.results[:, :7], ref.results[:, :7])
    assert np.array_equal(got.items, ref.items)


def _uneven_documents(nfeat, seed):
    """300 documents of uneven length, three empty ones and one of 3 000 lexems among them"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(5, 400, size=300)
    sizes[[7, 150, 299]] = 0
    sizes[42] = 3000
    parts = []
    for n in sizes:
        lex, _ = _docs(rng, 1, int(n), nfeat, True)
        parts.append(lex)
    offs = np.zeros(len(sizes) + 1, np.uint64)
    offs[1:] = np.cumsum(sizes)
    return np.concatenate(parts), offs


def test_flat_rule_set_is_regrouped_in_document_order():
    rules = synth.random_rules(400, 30, 2)
    m, o = spa.PatternMatcherInstance(), oracle.L2Matcher()
    for x in (m, o):
        synth.apply_rules(x, rules, compile=True)
    lex, offs = _uneven_documents(30, 11)
    up = _Uploaded(lex, offs)
    ctx = m.createContext()
    assert ctx.kernelKind() == 1
    dev = []
    _sized(ctx, lambda: dev.append(up.run(ctx)), up.ndocs, "matchDocsDevice")
    raw = _raw_ranges(ctx, dev[-1])
    nonempty = raw[raw[:, 1] > 0]
    # the raw batch is in completion order: without this the test shows nothing about regrouping
    assert np.any(np.diff(nonempty[:, 0].astype(np.int64)) < 0)
    fin, got = _finish_and_compare(ctx)
    ref = o.run(synth.lexems5(lex), offs, nthreads=4)
    assert len(ref.results) > 10000
    _assert_oracle(got, ref)
    for d in (7, 150, 299):
        assert got.doc_offsets[d] == got.doc_offsets[d + 1]


@pytest.mark.parametrize("max_result_size", [30, 200])
@pytest.mark.parametrize("rules_docs,finished_count", [
    (((300, 20, 3), (60, 200, 20, 4)), 6571),              # of 188 520 raw results
    (((400, 30, 3), (300, 600, 30, 4)), 92883),            # of 2 695 868, up to 10 073 in one document
])
def test_exclusive_is_applied_on_the_device(rules_docs, finished_count, max_result_size):
    rules = synth.random_rules(*rules_docs[0])
    lex, offs = synth.random_documents(*rules_docs[1])

    def build(x):
        x.defineOption("exclusive")
        x.defineOption("maxResultSize", max_result_size)
        synth.apply_rules(x, rules)
    m, o = spa.PatternMatcherInstance(), oracle.L2Matcher()
    build(m)
    build(o)
    up = _Uploaded(lex, offs)
    ctx = m.createContext()
    c = _sized(ctx, lambda: up.run(ctx), up.ndocs, "matchDocsDevice")
    fin, got = _finish_and_compare(ctx)
    ref = o.run(synth.lexems5(lex), offs, nthreads=4)
    assert len(ref.results) == finished_count
    _assert_oracle(got, ref)
    assert len(got.results) < c["results"]                 # finished < raw


def test_general_kernel_with_format_strings():
    rng = random.Random(9100 + 2)
    nterms = 6
    calls = _random_program(rng, nterms)
    mt, omt = spa.PatternMatcherInstance(), oracle.L2Matcher()
    _apply(mt, calls)
    _apply(omt, calls)
    lex, offs = synth.random_documents(200, 150, nterms, seed=52)
    up = _Uploaded(lex, offs)
    ctx = mt.createContext()
    assert ctx.kernelKind() == 0
    _sized(ctx, lambda: up.run(ctx), up.ndocs, "matchDocsDevice")
    fin, got = _finish_and_compare(ctx, formats=True)
    assert fin.d_result_format and fin.d_item_format
    ref = omt.run(synth.lexems5(lex), offs, nthreads=4)
    assert len(ref.results) > 50 and int(ref.item_format[:, 1].max()) > 0        # items with sub-records
    assert int(ref.item_format[:, 0].max()) > 0 or int(ref.result_format.max()) > 0
    _assert_oracle(got, ref)
    assert np.array_equal(got.results, ref.results)
    assert np.array_equal(got.result_format, ref.result_format) and np.array_equal(got.item_format, ref.item_format)


@pytest.mark.parametrize("seed,nrules,nfeat,n", [(2, 400, 30, 500), (3, 3000, 200, 1000)])
def test_result_set_context(seed, nrules, nfeat, n):
    rules = synth.random_rules(nrules, nfeat, seed)
    m = spa.PatternMatcherInstance()
    synth.apply_rules(m, rules, compile=True)
    ctx = m.createContext(result_sets=True)
    assert ctx.kernelKind() == 2
    lex, offs = _docs(np.random.default_rng(100 + seed), 24, n, nfeat, True)
    up = _Uploaded(lex, offs)
    c = _sized(ctx, lambda: up.run(ctx), up.ndocs, "matchDocsDevice")
    fin, got = _finish_and_compare(ctx)
    assert len(got.results) == c["results"] > 100


def test_fused_pipeline():
    """lexer matchDocsDevice -> matchLexedDevice -> finish, exact engine and result-set mode"""
    import torch
    vocab = synth.vocabulary(2000, 5)
    pats, rules = synth.pipeline_workload(200, 500, vocab, 1)
    text, offs = synth.text_documents(16, 3000, vocab, 2, utf8=True)
    ndocs = len(offs) - 1
    lx = spa.PatternLexerInstance()
    synth.apply_lexer_patterns(lx, pats)
    m = spa.PatternMatcherInstance()
    synth.apply_rules(m, rules, compile=True)
    hl = lx.createContext().matchDocs(text, offs)
    ref = m.createContext().matchDocs(hl.lexems, hl.doc_offsets)
    assert len(ref.results) > 0
    stream = _stream()
    lctx = lx.createContext()
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    lo = []
    lc = _sized(lctx, lambda: lo.append(lctx.matchDocsDevice(d_text.data_ptr(), d_offs.data_ptr(), ndocs, len(text), stream)), ndocs, "lexer")
    for result_sets, kind in ((False, 1), (True, 2)):
        fctx = m.createContext(result_sets=result_sets)
        assert fctx.kernelKind() == kind
        fc = _sized(fctx, lambda: fctx.matchLexedDevice(lo[-1].d_lexems, lo[-1].d_doc_ranges, ndocs, int(lc["lexems"]), stream), ndocs, "matchLexedDevice")
        assert fc["results"] == len(ref.results)
        fin, got = _finish_and_compare(fctx)
        if not result_sets:
            _assert_same_batch(got, ref, False)


def test_a_failed_document_is_empty_and_its_neighbours_are_intact():
    rules = synth.random_rules(300, 20, 3)
    m, o = spa.PatternMatcherInstance(), oracle.L2Matcher()
    for x in (m, o):
        synth.apply_rules(x, rules)
    lex, offs = synth.random_documents(12, 200, 20, 4)
    bad = lex.copy()
    b, e = int(offs[5]), int(offs[6])
    bad[b:e, 1] = bad[b:e, 1][::-1]                     # document 5: descending ordpos
    up = _Uploaded(bad, offs)
    ctx = m.createContext()
    ctx.reserveOutput(400000, 1200000)                 # (every good document fits: the only failure is the order)
    up.run(ctx)
    fin, got = _finish_and_compare(ctx)
    assert int(got.status[5]) == 1 and not np.any(np.delete(got.status, 5))
    assert got.doc_offsets[5] == got.doc_offsets[6]
    ref = o.run(synth.lexems5(lex), offs)
    for d in (4, 6):
        mine, theirs = got.doc(d), ref.doc(d)
        assert len(theirs) > 0 and np.array_equal(mine[:, :7], theirs[:, :7])
        mi = got.items[int(mine[0, 7]):int(mine[-1, 7]) + int(mine[-1, 8])]
        ti = ref.items[int(theirs[0, 7]):int(theirs[-1, 7]) + int(theirs[-1, 8])]
        assert np.array_equal(mi, ti)


# ---- the offsets pass scans the documents in tiles of 1024: batches around the tile boundary and into a third tile
TILE_RULES = [("seq_12", "sequence", 1, [1, 2]), ("seq_23", "sequence", 1, [2, 3]), ("seq_24", "sequence", 2, [2, 4]), ("seq_123", "sequence", 2, [1, 2, 3])]
TILE_FAILING = 1000                 # the document whose lexems are out of order
_TILE_DOCS = []


def _tile_documents():
    """2049 documents of 0..3 lexems (terms 1..4 at the positions 1, 2, 3); document 1024, the first of the second tile, is
    1 2 3 between empty ones; document TILE_FAILING is 1 2 3 with descending positions"""
    if not _TILE_DOCS:
        rng = np.random.default_rng(77)
        sizes = rng.integers(1, 4, 2049)
        sizes[rng.random(2049) < 0.1] = 0
        sizes[[3, 1021, 1023, 1025, 1027, 2047]] = 0
        sizes[[TILE_FAILING, 1024]] = 3
        offs = np.zeros(2050, np.uint64)
        offs[1:] = np.cumsum(sizes)
        lex = np.zeros((int(offs[-1]), 4), np.uint32)
        for d, n in enumerate(sizes):
            b = int(offs[d])
            # half of the documents that can hold it are 1 2 (3): they have results, two of the three rules or all of them
            ids = [1, 2, 3][:n] if rng.random() < 0.5 or d == 1024 else rng.integers(1, 5, n)
            for k in range(n):
                lex[b + k] = (ids[k], k + 1, k, 1)
        b = int(offs[TILE_FAILING])
        lex[b:b + 3, 0] = (1, 2, 3)
        lex[b:b + 3, 1] = (3, 2, 1)
        _TILE_DOCS.append((lex, offs))
    return _TILE_DOCS[0]


@pytest.mark.parametrize("ndocs,exclusive,canonical", [(1023, False, False), (1024, False, False), (1025, False, False), (2049, False, False),
                                                       (2049, True, False), (1025, False, True)])
def test_document_counts_around_the_tile_of_the_offsets_pass(ndocs, exclusive, canonical):
    lex, offs = _tile_documents()
    lex, offs = lex[:int(offs[ndocs])], offs[:ndocs + 1]
    m = spa.PatternMatcherInstance()
    if exclusive:
        m.defineOption("exclusive")
        m.defineOption("maxResultSize", 30)
    synth.apply_rules(m, TILE_RULES)
    up = _Uploaded(lex, offs)
    ctx = m.createContext()
    ctx.reserveOutput(4 * ndocs, 12 * ndocs)             # (at most 3 results of at most 3 items per document: the only failure is the order)
    up.run(ctx)
    ref = ctx.batchFetch()
    assert np.flatnonzero(ref.status).tolist() == [TILE_FAILING] and int(ref.status[TILE_FAILING]) == 1
    per_doc = np.diff(ref.doc_offsets.astype(np.int64))
    items_before = np.concatenate([[0], np.cumsum(ref.results[:, 8].astype(np.int64))])
    items_per_doc = np.diff(items_before[ref.doc_offsets.astype(np.int64)])
    # what the batch is there for: 0 to 3 results per document (`exclusive` drops the two that seq_123 covers), item counts
    # that are no multiple of them, results behind the first tile
    assert set(per_doc.tolist()) == ({0, 1, 2} if exclusive else {0, 1, 2, 3}) and per_doc[TILE_FAILING] == 0
    assert len(set((items_per_doc[per_doc > 0] / per_doc[per_doc > 0]).tolist())) > 1
    assert ndocs <= 1024 or per_doc[1024] > 0
    if canonical:
        want = sorted_batch(ref)
        fin = ctx.batchFinishDevice(_stream(), canonical=True)
        got = ctx.finishedFetch()
        assert np.array_equal(got.doc_offsets, want.doc_offsets) and np.array_equal(got.results, want.results)
        assert np.array_equal(got.items, want.items) and np.array_equal(got.status, ref.status)
        _assert_layout(fin, got)
    else:
        _finish_and_compare(ctx)


def test_a_batch_whose_output_did_not_fit_is_finished_as_it_is():
    """before the rerun: the documents that overflowed the output are empty, the others are whole"""
    rules = synth.random_rules(400, 30, 3)
    m = spa.PatternMatcherInstance()
    synth.apply_rules(m, rules)
    lex, offs = synth.random_documents(300, 600, 30, 4)
    up = _Uploaded(lex, offs)
    ctx = m.createContext()
    ctx.reserveOutput(1000, 1000)                      # (a minimum; the launch sizes the output from the input: too small here)
    up.run(ctx)
    c = ctx.batchCounters()
    status = ctx.batchStatus(up.ndocs)
    codes = set(int(x) for x in status if x)
    assert c["failed_docs"] > 0 and 9 in codes and codes <= {2, 9}
    assert np.any(status == 0)
    fin, got = _finish_and_compare(ctx)
    sizes = np.diff(got.doc_offsets.astype(np.int64))
    assert np.all(sizes[status != 0] == 0) and np.any(sizes[status == 0] > 0)
    assert len(got.results) < c["results"]
    # the protocol's rerun with the counted sizes, finished again: the whole batch
    c = _sized(ctx, lambda: up.run(ctx), up.ndocs, "matchDocsDevice")
    fin, got = _finish_and_compare(ctx)
    assert len(got.results) == c["results"]


def test_interface_rules():
    import torch
    rules = synth.random_rules(300, 20, 3)
    m = spa.PatternMatcherInstance()
    synth.apply_rules(m, rules)
    lex, offs = synth.random_documents(40, 200, 20, 4)
    up = _Uploaded(lex, offs)
    ctx = m.createContext()
    with pytest.raises(spa.PatternError, match="no batch"):
        ctx.batchFinishDevice(_stream())
    with pytest.raises(spa.PatternError, match="not been finished"):
        ctx.finishedFetch()
    _sized(ctx, lambda: up.run(ctx), up.ndocs, "matchDocsDevice")
    with pytest.raises(spa.PatternError, match="not been finished"):
        ctx.finishedFetch()
    fin, first = _finish_and_compare(ctx)
    # twice on the same batch: the same bytes
    fin2, second = _finish_and_compare(ctx)
    _assert_same_batch(second, first, False)
    assert fin2.d_results == fin.d_results
    # a second batch invalidates
    lex2, offs2 = synth.random_documents(10, 100, 20, 5)
    up2 = _Uploaded(lex2, offs2)
    up2.run(ctx)
    with pytest.raises(spa.PatternError, match="not been finished"):
        ctx.finishedFetch()
    fin3, third = _finish_and_compare(ctx)
    assert fin3.ndocs == 10 and len(third.doc_offsets) == 11
    # finish on another stream than the batch's
    other = torch.cuda.Stream()
    up.run(ctx)
    fin4, fourth = _finish_and_compare(ctx, stream=other.cuda_stream)
    _assert_same_batch(fourth, first, False)
    # a batch of the host entry point can be finished too
    host = ctx.matchDocs(lex, offs)
    ctx.batchFinishDevice(_stream())
    _assert_same_batch(ctx.finishedFetch(), host, False)
