"""Pattern frequencies on the device (sp_matcher_ctx_finished_pattern_freq_device, csrc/l2_freq.h): the records, offsets,
status, both handle arrays and the total that the passes leave must EQUAL what the device-free twin
(sp_match_batch_pattern_freq) makes of the fetched finished batch, and the numpy model (tests/pattern_freq_model.py).
The handles come from hand-made lexems through rule sets of one bare-term pattern per handle: the lexem (h, p) gives the
result (handle h, ordpos p, ordend p + 1), so that a test sets every handle and position itself.

The device tests feed valid handles only: the matcher produces no others.  The range rule is covered through the twin
(tests/test_pattern_freq_abi.py, tests/micro/pattern_freq_san.cpp) and by the bound check being the first use of a handle
in both kernels (validHandle in markWindow and in the sweeps of count and place, csrc/l2_freq_kernel.hip)."""
import contextlib
import ctypes
import io
import json
import os

import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from struspattern_amd import capi, match, rulelang, synth
from tests import pattern_freq_model as model
from tests.finished_support import _bare, _from_device, _stream, _torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("records", "doc_offsets", "status", "handle_results", "handle_docs")


def _lexems(docs):
    """docs: per document a list of (term, ordpos) -> lexems (n, 4), document offsets"""
    lex, offs = [], [0]
    for doc in docs:
        lex += [[t, p, 2 * p, 1] for t, p in doc]
        offs.append(len(lex))
    return np.array(lex, np.uint32).reshape(-1, 4), np.array(offs, np.uint64)


class Run:
    """a rule set over hand-made lexems on the device, finished; `failing`: the documents that are to fail with status 1"""

    def __init__(self, ctx, lex, offs, canonical=False, failing=()):
        torch = _torch()
        self.ctx, self.failing = ctx, set(failing)
        self.d_lex = torch.from_numpy(np.ascontiguousarray(lex).view(np.int32).reshape(-1)).cuda()
        self.d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
        self.ndocs, self.nlex = len(offs) - 1, len(lex)
        self.counters = self.match()
        self.fin = ctx.batchFinishDevice(_stream(), canonical=canonical)

    def match(self):
        for _ in range(6):
            self.ctx.matchDocsDevice(self.d_lex.data_ptr(), self.d_offs.data_ptr(), self.ndocs, self.nlex, _stream())
            c = self.ctx.batchCounters()
            status = self.ctx.batchStatus(self.ndocs)
            bad = set(int(d) for d in np.flatnonzero(status))
            if bad == self.failing:
                assert all(int(status[d]) == 1 for d in bad)
                return c
            assert set(int(status[d]) for d in bad - self.failing) <= {2, 9}
            self.ctx.reserveOutput(int(c["results"] * 1.2) + 1024, int(c["items"] * 1.2) + 1024)
            self.ctx.growArena()
        raise AssertionError("documents still failing after resizing")


def _same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in FIELDS)


def _assert_freq(ctx, bound, out=None):
    """the fetched frequencies equal the twin's and the model's on the fetched finished batch; returns (batch, frequencies)"""
    mb = ctx.finishedFetch()
    got = ctx.finishedPatternFreqFetch()
    twin = spa.batchPatternFreq(mb, bound)
    model.assert_same(twin, model.batch_pattern_freq(mb.results, mb.doc_offsets, bound, mb.status))
    model.assert_same(got, model.batch_pattern_freq(mb.results, mb.doc_offsets, bound, mb.status))
    assert _same(got, twin)
    if out is not None:
        # the device arrays themselves
        assert out.ndocs == len(mb.doc_offsets) - 1 and out.handle_bound == bound
        assert int(_from_device(out.d_totals, 1, np.uint64)[0]) == len(got.records)
        assert np.array_equal(_from_device(out.d_doc_freq_status, out.ndocs, np.int32), got.status)
        assert np.array_equal(_from_device(out.d_doc_offsets, out.ndocs + 1, np.uint64), got.doc_offsets)
        assert np.array_equal(_from_device(out.d_records, 4 * len(got.records), np.uint32).reshape(-1, 4), got.records)
        assert np.array_equal(_from_device(out.d_handle_results, bound, np.uint64), got.handle_results)
        assert np.array_equal(_from_device(out.d_handle_docs, bound, np.uint32), got.handle_docs)
    return mb, got


def _freq(ctx, bound, stream=None, check_device=True):
    out = ctx.finishedPatternFreqDevice(_stream() if stream is None else stream)
    return _assert_freq(ctx, bound, out if check_device else None)


# ---- 1. trips of 64 results, one handle many times, many handles once
def test_trip_edges_contention_and_distinct_handles():
    m = _bare(200)
    counts = [0, 1, 63, 64, 65, 129]
    docs = [[(1 + (k * 5) % 7, 3 + 2 * k) for k in range(n)] for n in counts]
    docs.append([(5, 10 + k) for k in range(129)])                              # one handle 129 times
    perm = np.random.default_rng(1).permutation(129)
    docs.append([(1 + int(perm[k]), 1 + k) for k in range(129)])                # 129 distinct handles, not in handle order
    lex, offs = _lexems(docs)
    ctx = m.createContext()
    Run(ctx, lex, offs)
    mb, got = _freq(ctx, 201)
    assert np.diff(mb.doc_offsets.astype(np.int64)).tolist() == counts + [129, 129] and not got.status.any()
    assert np.diff(got.doc_offsets.astype(np.int64)).tolist() == [0, 1, 7, 7, 7, 7, 1, 129]
    assert got.doc(6).tolist() == [[5, 129, 10, 10 + 128 + 1]]
    assert got.doc(7)[:, 0].tolist() == list(range(1, 130)) and np.all(got.doc(7)[:, 1] == 1)
    assert np.array_equal(got.doc(7)[np.array(perm), 2], np.arange(1, 130))    # the record of handle perm[k]+1 starts at k+1
    assert int(got.handle_results.sum()) == len(mb.results) and int(got.handle_docs[5]) == 6
    assert ctx.lastPatternFreqMs() >= 0.0


# ---- 2. bitmap words and windows
def test_bitmap_word_and_window_edges():
    W = capi.lib().sp_matcher_pattern_freq_window()
    m = _bare(2 * W + 2)
    bound = m.handleBound()
    assert bound == 2 * W + 3
    edges = [1, 31, 32, 33, 63, 64, 65, W - 1, W, W + 1, 2 * W - 1, 2 * W, bound - 1]
    docs = [
        [(h, 1 + k) for k, h in enumerate(edges)] + [(h, 50 + k) for k, h in enumerate(reversed(edges))],   # every edge, twice
        [(W, 1), (2 * W - 1, 2), (W + 1, 3), (W, 4)],               # handles of the second window only
        [(2 * W, 1), (bound - 1, 2), (2 * W + 1, 2)],               # of the third window only
        [(1, 1), (2 * W + 1, 2), (1, 3)],                           # the first and the third: the second is not swept
        [(bound - 1, 7)],
        [(W - 1, 1), (W, 2)],                                       # neighbours across the window border
    ]
    lex, offs = _lexems(docs)
    ctx = m.createContext()
    Run(ctx, lex, offs)
    mb, got = _freq(ctx, bound)
    assert not got.status.any() and len(mb.results) == len(lex)
    assert got.doc(0)[:, 0].tolist() == edges and np.all(got.doc(0)[:, 1] == 2)
    assert got.doc(0)[:, 2].tolist() == [1 + k for k in range(len(edges))]
    assert got.doc(0)[:, 3].tolist() == [50 + (len(edges) - 1 - k) + 1 for k in range(len(edges))]
    assert got.doc(1).tolist() == [[W, 2, 1, 5], [W + 1, 1, 3, 4], [2 * W - 1, 1, 2, 3]]
    assert got.doc(2)[:, 0].tolist() == [2 * W, 2 * W + 1, bound - 1]
    assert got.doc(3).tolist() == [[1, 2, 1, 4], [2 * W + 1, 1, 2, 3]]
    assert got.doc(4).tolist() == [[bound - 1, 1, 7, 8]] and got.doc(5)[:, 0].tolist() == [W - 1, W]
    assert int(got.handle_docs[bound - 1]) == 3 and int(got.handle_docs[W]) == 3 and int(got.handle_results[W]) == 5


# ---- 3. a wave serves several documents: nothing of the document before is left in its bitmap
def test_more_documents_than_waves_with_disjoint_handle_sets():
    m = _bare(200)
    waves = 16 * _torch().cuda.get_device_properties(0).multi_processor_count
    ndocs = waves + 257
    docs = [[(1 + (7 * d + 3 * j) % 200, 1 + j) for j in range(3)] for d in range(ndocs)]
    for d in range(ndocs - 1):
        assert not {t for t, _ in docs[d]} & {t for t, _ in docs[d + 1]}
    lex, offs = _lexems(docs)
    ctx = m.createContext()
    Run(ctx, lex, offs)
    mb, got = _freq(ctx, 201, check_device=False)
    assert not got.status.any() and len(got.records) == 3 * ndocs == len(mb.results)
    assert np.all(got.records[:, 1] == 1) and int(got.handle_docs.sum()) == 3 * ndocs


# ---- 4. the tiles of the offsets pass
@pytest.mark.parametrize("ndocs", [1, 1023, 1024, 1025])
def test_document_counts_around_the_tile_of_the_offsets_pass(ndocs):
    m = _bare(200)
    docs = [[(1 + (d + 11 * j) % 200, 1 + j) for j in range((d + 1) % 4)] for d in range(ndocs)]
    failing = []
    if ndocs > 1:
        # an empty document and one the matcher fails (ordpos descends) at the end of the first tile
        edge = min(ndocs, 1024) - 1
        docs[edge - 2] = [(8, 1), (8, 2)]
        docs[edge - 1] = []
        docs[edge] = [(3, 5), (4, 2)]
        failing = [edge]
    lex, offs = _lexems(docs)
    ctx = m.createContext()
    run = Run(ctx, lex, offs, failing=failing)
    mb, got = _freq(ctx, 201)
    assert not got.status.any()
    assert np.flatnonzero(mb.status).tolist() == failing and run.counters["failed_docs"] == len(failing)
    per_doc = np.diff(got.doc_offsets.astype(np.int64))
    want = [0 if d in failing else len({t for t, _ in doc}) for d, doc in enumerate(docs)]
    assert per_doc.tolist() == want and (ndocs <= 1024 or per_doc[1024] > 0)
    if ndocs > 1:
        assert per_doc[edge - 2:edge + 1].tolist() == [1, 0, 0] and got.doc(edge - 2).tolist() == [[8, 2, 1, 3]]


# ---- 5. minimum and maximum: results whose ordpos does not ascend in engine order
def test_within_results_with_descending_ordpos():
    m = spa.PatternMatcherInstance()
    for a, b in ((1, 2), (3, 4)):
        m.pushTerm(a)
        m.pushTerm(b)
        m.pushExpression("within", 2, 5, 0)
        m.definePattern("w", "", True)
    m.compile()
    assert m.handleBound() == 2
    docs = [[(1, 1), (3, 2), (4, 3), (2, 4), (4, 5), (3, 6)], [(3, 1), (4, 2)]]
    lex, offs = _lexems(docs)
    ctx = m.createContext()
    Run(ctx, lex, offs)
    mb, got = _freq(ctx, 2)
    first = mb.doc(0)
    assert first[:, 1].tolist() != sorted(first[:, 1].tolist())               # (else the case shows nothing)
    assert got.records.tolist() == [[1, 4, 1, 7], [1, 1, 1, 3]]
    assert int(first[0, 1]) != 1 and got.handle_results.tolist() == [0, 5] and got.handle_docs.tolist() == [0, 2]


# ---- 6. `exclusive`: the counts are over the survivors
def test_exclusive_counts_the_survivors():
    m = spa.PatternMatcherInstance()
    m.defineOption("exclusive")
    m.pushTerm(1)
    m.definePattern("a", "", True)
    m.pushTerm(2)
    m.definePattern("b", "", True)
    m.pushTerm(1)
    m.pushTerm(2)
    m.pushExpression("sequence", 2, 1, 0)
    m.definePattern("ab", "", True)
    m.compile()
    docs = [[(1, 1), (2, 2), (1, 5), (1, 7), (2, 8), (2, 11)], [(2, 1), (1, 2), (2, 3)]]
    lex, offs = _lexems(docs)
    ctx = m.createContext()
    run = Run(ctx, lex, offs)
    mb, got = _freq(ctx, 4)
    assert run.counters["results"] == 8 + 4 and len(mb.results) == 4 + 2      # (the raw batch holds what `exclusive` drops)
    assert got.doc(0).tolist() == [[1, 1, 5, 6], [2, 1, 11, 12], [3, 2, 1, 9]]
    assert got.doc(1).tolist() == [[2, 1, 1, 2], [3, 1, 2, 4]]
    assert got.handle_results.tolist() == [0, 1, 2, 3] and got.handle_docs.tolist() == [0, 1, 2, 2]


# ---- 7. the same bytes from every engine and either finish
def test_engine_independence():
    rules = synth.random_rules(400, 30, 2)
    lex, offs = synth.random_documents(24, 500, 30, 102)
    m = spa.PatternMatcherInstance()
    synth.apply_rules(m, rules)
    assert m.resultSetTier()[0]
    bound = m.handleBound()
    got = []
    for result_sets, canonical in ((False, False), (False, True), (True, False)):
        ctx = m.createContext(result_sets=result_sets)
        assert ctx.kernelKind() == (2 if result_sets else 1)
        Run(ctx, lex, offs, canonical=canonical)
        mb, f = _freq(ctx, bound)
        got.append((mb, f))
    plain, canon, sets = got
    assert len(plain[1].records) > 1000 and int(plain[1].records[:, 1].max()) > 1 and not plain[1].status.any()
    assert not np.array_equal(plain[0].results, canon[0].results) and not np.array_equal(plain[0].results, sets[0].results)
    assert _same(plain[1], canon[1]) and _same(plain[1], sets[1])
    for f in FIELDS:
        assert getattr(plain[1], f).tobytes() == getattr(sets[1], f).tobytes() == getattr(canon[1], f).tobytes()


# ---- 8. call order
def test_call_order_buffer_reuse_and_another_stream():
    torch = _torch()
    m = _bare(200)
    docs = [[(1 + (3 * k) % 50, 1 + k) for k in range(70)], [], [(7, 1), (7, 2)]]
    lex, offs = _lexems(docs)
    ctx = m.createContext()
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):       # before any batch
        ctx.finishedPatternFreqDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedPatternFreqFetch()
    with pytest.raises(spa.PatternError):
        ctx.lastPatternFreqMs()
    run = Run(ctx, lex, offs)
    # an allocation that fails, then a normal call
    L = capi.lib()
    out = capi.SpPatternFreqDevice()
    L.sp_test_fail_alloc_above(1)
    try:
        assert L.sp_matcher_ctx_finished_pattern_freq_device(ctx._h, None, ctypes.byref(out)) == -2      # SP_ERR_NOMEM
    finally:
        L.sp_test_fail_alloc_above(0)
    first = ctx.finishedPatternFreqDevice(_stream())
    mb, got = _assert_freq(ctx, 201, first)
    assert np.diff(got.doc_offsets.astype(np.int64)).tolist() == [50, 0, 1]
    # a second call on the same finish reuses the buffers and gives the same bytes
    second = ctx.finishedPatternFreqDevice(_stream())
    for name, _ in capi.SpPatternFreqDevice._fields_:
        assert getattr(first, name) == getattr(second, name)
    assert _same(_assert_freq(ctx, 201, second)[1], got)
    # a stream other than the finish's
    other = torch.cuda.Stream()
    third = ctx.finishedPatternFreqDevice(other.cuda_stream)
    assert _same(_assert_freq(ctx, 201, third)[1], got)
    # the next batch invalidates the state until it is finished again
    run.match()
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        ctx.finishedPatternFreqDevice(_stream())
    with pytest.raises(spa.PatternError):
        ctx.finishedPatternFreqFetch()
    ctx.batchFinishDevice(_stream())
    with pytest.raises(spa.PatternError):                       # finished, but no frequencies of this finish yet
        ctx.finishedPatternFreqFetch()
    fourth = ctx.finishedPatternFreqDevice(_stream())
    assert fourth.d_records == first.d_records
    assert _same(_assert_freq(ctx, 201, fourth)[1], got)


# ---- 9. the command line
def test_match_frequencies_listing():
    with open(os.path.join(HERE, "golden", "doc_example.json")) as f:
        case = json.load(f)
    prog, fn = os.path.join(HERE, "golden", "doc_example.rul"), os.path.join(HERE, "golden", "doc_example.txt")
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert match.main(["-p", prog, "-o", str(case["origin"]), "--frequencies", fn]) == 0
    lines = out.getvalue().splitlines()
    assert lines[0] == "%s:" % fn and lines[1:5] == case["results"] and lines[-1] == "OK done"
    # what follows from the four results of the committed listing: per name how many, and the first position
    want = {}
    for line in case["results"]:
        name, pos = line.split(" [")[0], int(line.split(" [")[1].split(",")[0])
        n, first = want.get(name, (0, pos))
        want[name] = (n + 1, min(first, pos))
    assert want == {"Name": (2, 8), "Contact": (2, 8)}
    # the last position from the oracle's results
    lx, mt = oracle.L1Lexer(), oracle.L2Matcher()
    prg = rulelang.load(case["program"], lx, mt)
    doc = case["text"].encode()
    lex, offs = lx.matchDocs(doc, np.array([0, len(doc)], np.uint64))
    res = mt.run(synth.lexems5(lex), offs)
    pn, _ = rulelang.name_tables(prg, mt)
    last = {}
    for r in res.results:
        last[pn(int(r[0]))] = max(last.get(pn(int(r[0])), 0), int(r[2]))
    handles = sorted({int(r[0]) for r in res.results})
    assert lines[5:-1] == ["frequency %s: count %d first %d last %d" % (pn(h), *want[pn(h)], last[pn(h)]) for h in handles]
    # without the option nothing changes
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert match.main(["-p", prog, "-o", str(case["origin"]), fn]) == 0
    assert out.getvalue().splitlines() == lines[:5] + ["OK done"]
