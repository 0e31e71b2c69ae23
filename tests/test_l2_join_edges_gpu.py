"""The join kernel of result-set mode (struspattern_amd/csrc/l2_join_kernel.hip) on the edges of its own mechanics: the
constructed cases of tests/l2_join_cases.py (tests/test_l2_join_cases.py shows on the CPU which edge each one crosses and
that the expected values are the oracle's) through the growing host entry and through the device entry with batchFetch --
status, result ranges, per-document multisets of results with their items, the number of items and the batch counters.
The count array, the output capacity, segments and format strings get the assertions of their own below."""
import functools
from collections import Counter

import numpy as np
import pytest

import oracle
import struspattern_amd as spa

from . import l2_join_cases as cases
from .l2_join_cases import SP_DOC_ERR_OUTPUT
from .result_set_model import results_multiset
from .finished_support import _sized, _stream, _Uploaded

pytestmark = pytest.mark.gpu


def _waves_of_the_device(m):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return int(m.launchPlan(cus, 1 << 20, 1 << 22, result_sets=True)["join_blocks"])


@functools.lru_cache(maxsize=None)
def _built(name):
    """the case, the product's instance of its rule set and the oracle's output (computed once, never changed)"""
    builder = cases.CASES[name]
    if name == "more_docs_than_waves":
        probe = spa.PatternMatcherInstance()
        builder()[0](probe)
        waves = _waves_of_the_device(probe)
        build, lex4, offs, seg, _ = builder(waves)
        assert len(offs) - 1 > 2 * (4 * ((waves + 3) // 4))          # launchL2Join: blocks of 4 waves
    else:
        build, lex4, offs, seg, _ = builder()
    m, o = spa.PatternMatcherInstance(), oracle.L2Matcher()
    build(m)
    build(o)
    assert np.array_equal(m.dumpTable(), o.dumpTable())
    ref = cases.Reference(o, lex4, offs, seg)
    for d, code in cases.FAILING.get(name, {}).items():
        assert ref.status[d] == 0 and ref.nresults[d] > cases.COUNT_MAX
        ref.failing(d, code)
    for a in (ref.status,):
        a.setflags(write=False)
    return m, lex4, offs, seg, ref


def _context(m):
    ctx = m.createContext(result_sets=True)
    assert ctx.kernelKind() == 2
    return ctx


def _assert_reference(got, ref, what):
    ndocs = len(ref.status)
    assert np.array_equal(got.status, ref.status), (what, got.status.tolist(), ref.status.tolist())
    assert np.array_equal(got.doc_offsets, np.concatenate([[0], np.cumsum(ref.nresults)]).astype(np.uint64)), what
    for d in range(ndocs):
        a, b = results_multiset(got, d), ref.multisets[d]
        assert a == b, (what, d, list((a - b).items())[:2], list((b - a).items())[:2])
    assert len(got.items) == sum(ref.nitems), what


def _assert_counters(ctx, ref, what):
    c = ctx.batchCounters()
    assert (c["results"], c["items"], c["failed_docs"]) == (sum(ref.nresults), sum(ref.nitems), int(np.count_nonzero(ref.status))), (what, c)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_case_matches_the_oracle(name):
    m, lex4, offs, seg, ref = _built(name)
    ndocs = len(offs) - 1
    ctx = _context(m)
    got = ctx.matchDocs(lex4, offs, seg, check=not ref.status.any())
    _assert_reference(got, ref, name + " matchDocs")
    _assert_counters(ctx, ref, name + " matchDocs")
    # the device entry does not grow: it gets exactly what the oracle's output needs
    ctx = _context(m)
    ctx.reserveOutput(sum(ref.nresults), sum(ref.nitems))
    dev = _Uploaded(lex4, offs, seg)
    dev.run(ctx)
    assert np.array_equal(ctx.batchStatus(ndocs), ref.status), name
    _assert_counters(ctx, ref, name + " device")
    _assert_reference(ctx.batchFetch(), ref, name + " device")


@pytest.mark.parametrize("name", sorted(cases.FAILING))
def test_a_document_beyond_the_count_limit_fails_alone(name):
    """more than 0x7FFF matches at one lexem: SP_DOC_ERR_RANGE, nothing reserved or written; the neighbours are complete"""
    m, lex4, offs, seg, ref = _built(name)
    ctx = _context(m)
    dev = _Uploaded(lex4, offs, seg)
    dev.run(ctx)                    # (the default capacity holds the neighbours: the peak document must not ask for any)
    c = ctx.batchCounters()
    assert c["failed_docs"] == 1 and c["results"] == ref.nresults[0] + ref.nresults[2] and c["items"] == ref.nitems[0] + ref.nitems[2]
    assert ctx.batchStatus(3).tolist() == [0, cases.SP_DOC_ERR_RANGE, 0]
    got = ctx.batchFetch()
    assert results_multiset(got, 0) == ref.multisets[0] and results_multiset(got, 2) == ref.multisets[2] and len(got.doc(1)) == 0


def test_count_array_stored_recounted_and_mixed():
    """(first, count) ranges made by hand -- not ascending, unused lexems between them -- with a count array that holds
    no document, some of them, all of them: the same multisets each time"""
    import torch
    m, lex4, offs, seg, ref = _built("count_array")
    ndocs = len(offs) - 1
    buf, ranges, hints = cases.scattered(lex4, offs)
    d_lex = torch.from_numpy(np.ascontiguousarray(buf).view(np.int32).reshape(-1)).cuda()
    d_ranges = torch.from_numpy(np.ascontiguousarray(ranges).view(np.int64).reshape(-1)).cuda()
    for hint in hints:
        assert hint <= len(buf)
        ctx = _context(m)
        ctx.reserveOutput(sum(ref.nresults), sum(ref.nitems))
        ctx.matchLexedDevice(d_lex.data_ptr(), d_ranges.data_ptr(), ndocs, hint, _stream())
        assert not ctx.batchStatus(ndocs).any(), hint
        _assert_counters(ctx, ref, "hint %d" % hint)
        _assert_reference(ctx.batchFetch(), ref, "hint %d" % hint)


def _assert_partial(ctx, ref, ndocs, what):
    """a batch whose output did not fit: the failing documents have status 9 and an empty range, every other one is the
    oracle's, and the counters say what the whole batch needs"""
    st = ctx.batchStatus(ndocs)
    assert set(int(x) for x in st) == {0, SP_DOC_ERR_OUTPUT}, (what, st.tolist())
    c = ctx.batchCounters()
    assert (c["results"], c["items"], c["failed_docs"]) == (sum(ref.nresults), sum(ref.nitems), int(np.count_nonzero(st))), (what, c)
    got = ctx.batchFetch()
    assert np.array_equal(got.status, st)
    for d in range(ndocs):
        if st[d]:
            assert got.doc_offsets[d] == got.doc_offsets[d + 1], (what, d)
        else:
            assert results_multiset(got, d) == ref.multisets[d], (what, d)


def test_output_capacity_through_the_device_entry():
    m, lex4, offs, seg, ref = _built("output_capacity")
    ndocs = len(offs) - 1
    results, items = sum(ref.nresults), sum(ref.nitems)
    plan = m.launchPlan(256, ndocs, len(lex4), result_sets=True)
    assert results > int(plan["want_results"]) and items > int(plan["want_items"])
    dev = _Uploaded(lex4, offs, seg)
    # a fresh context: the result buffer is too small
    ctx = _context(m)
    dev.run(ctx)
    _assert_partial(ctx, ref, ndocs, "fresh")
    ctx.reserveOutput(results, items)
    dev.run(ctx)
    assert not ctx.batchStatus(ndocs).any()
    _assert_counters(ctx, ref, "exact sizes")
    _assert_reference(ctx.batchFetch(), ref, "exact sizes")
    # results fit, items do not
    ctx = _context(m)
    ctx.reserveOutput(results, 0)
    dev.run(ctx)
    _assert_partial(ctx, ref, ndocs, "items")
    ctx.reserveOutput(results, items)
    dev.run(ctx)
    _assert_counters(ctx, ref, "items, exact sizes")
    _assert_reference(ctx.batchFetch(), ref, "items, exact sizes")
    # the protocol of the callers, and the host entry, which grows by itself
    ctx = _context(m)
    _sized(ctx, lambda: dev.run(ctx), ndocs, "output_capacity")
    _assert_reference(ctx.batchFetch(), ref, "sized")
    _assert_reference(_context(m).matchDocs(lex4, offs, seg), ref, "matchDocs")


def test_segments_change_inside_a_match():
    m, lex4, offs, seg, ref = _built("segments")
    ctx = _context(m)
    host = ctx.matchDocs(lex4, offs, seg)
    dev = _Uploaded(lex4, offs, seg)
    dev.run(ctx)
    for got in (host, ctx.batchFetch()):
        assert int((got.results[:, 3] != got.results[:, 5]).sum()) == 4
        _assert_reference(got, ref, "segments")
    # without the segment array every segment is 0
    assert not _context(m).matchDocs(lex4, offs).results[:, [3, 5]].any()


def test_format_handles_are_the_exact_engine_s():
    m, lex4, offs, seg, ref = _built("formats")
    exact = m.createContext()
    assert exact.kernelKind() != 2
    want = exact.matchDocs(lex4, offs, seg)
    assert want.result_format is not None and want.result_format.any() and not want.result_format.all()
    ctx = _context(m)
    host = ctx.matchDocs(lex4, offs, seg)
    dev = _Uploaded(lex4, offs, seg)
    dev.run(ctx)
    for got in (host, ctx.batchFetch()):
        _assert_reference(got, ref, "formats")
        for d in range(len(offs) - 1):
            def with_formats(b):
                lo, hi = int(b.doc_offsets[d]), int(b.doc_offsets[d + 1])
                return Counter((tuple(r[:7]), int(f)) for r, f in zip(b.results[lo:hi].tolist(), b.result_format[lo:hi]))
            assert with_formats(got) == with_formats(want), d
        assert got.item_format.shape == (len(got.items), 2) and len(got.items) > 0 and not got.item_format.any()


def test_a_rule_set_without_variables_has_no_items():
    m, lex4, offs, seg, ref = _built("no_variables")
    ctx = _context(m)
    got = ctx.matchDocs(lex4, offs, seg)
    assert len(got.items) == 0 and not got.results[:, 7:].any() and len(got.results) == sum(ref.nresults) > 0
    assert ctx.batchCounters()["items"] == 0
