"""The general rule kernel (struspattern_amd/csrc/l2_kernel.hip) on its batch and capacity edges: the constructed cases
of tests/l2_general_cases.py (tests/test_l2_general_cases.py shows on the CPU which edge each one crosses) against the
oracle, bit for bit -- status, result ranges, results in firing order, statistics, captured items.  Every case runs on the
general kernel alone and in the default configuration (flat cases take the fast tier there: its expiry rows and its
hand-over get the same inputs).  The cases that exceed a default capacity of the arena also go through the device entry,
which does not grow by itself: arena status first, clean after growArena(), and the grown context stays right."""
import functools

import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from struspattern_amd import synth

from . import l2_general_cases as cases
from .finished_support import _context, _Uploaded

pytestmark = pytest.mark.gpu

SP_DOC_ERR_ARENA = 2


@functools.lru_cache(maxsize=None)
def _built(name):
    """the case, the product's instance of its rule set and the oracle's output (computed once, never changed)"""
    build, lex4, offs, seg, _ = cases.CASES[name]()
    m, o = spa.PatternMatcherInstance(), oracle.L2Matcher()
    build(m)
    build(o)
    assert np.array_equal(m.dumpTable(), o.dumpTable())
    l5 = synth.lexems5(lex4)
    l5[:, 2] = seg
    ref = o.run(l5, offs)
    for a in (ref.results, ref.items, ref.stats, ref.doc_offsets):
        a.setflags(write=False)
    return m, lex4, offs, seg, ref


def _assert_oracle(got, ref, ndocs):
    assert np.array_equal(got.status, np.zeros(ndocs, np.int32))
    assert np.array_equal(got.doc_offsets, ref.doc_offsets)
    assert np.array_equal(got.results[:, :7], ref.results[:, :7])
    assert np.array_equal(got.stats, ref.stats)
    assert np.array_equal(got.results[:, 8], ref.results[:, 8])
    assert np.array_equal(got.items, ref.items)


@pytest.mark.parametrize("config", ["general", "default"])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_case_matches_the_oracle(name, config):
    m, lex4, offs, seg, ref = _built(name)
    ctx = _context(m, config)
    got = ctx.matchDocs(lex4, offs, seg)
    if config == "general":
        assert ctx.kernelKind() == 0 and ctx.batchCounters()["handed_over"] == 0
    _assert_oracle(got, ref, len(offs) - 1)


@pytest.mark.parametrize("name", cases.CAPACITY_CASES)
def test_device_batch_reports_the_arena_status_until_the_arena_has_grown(name):
    m, lex4, offs, seg, ref = _built(name)
    ndocs = len(offs) - 1
    ctx = _context(m, "general")
    ctx.reserveOutput(len(ref.results) + 1024, len(ref.items) + 1024)      # (the output is not what is short here)
    dev = _Uploaded(lex4, offs, seg)
    dev.run(ctx)
    st = ctx.batchStatus(ndocs)
    assert (st == SP_DOC_ERR_ARENA).any() and set(int(x) for x in st if x) == {SP_DOC_ERR_ARENA}
    for _ in range(6):
        assert ctx.growArena()
        dev.run(ctx)
        st = ctx.batchStatus(ndocs)
        assert set(int(x) for x in st if x) <= {SP_DOC_ERR_ARENA}
        if not st.any():
            break
    assert not st.any() and ctx.batchCounters()["failed_docs"] == 0
    _assert_oracle(ctx.batchFetch(), ref, ndocs)
    # the grown state is used again
    _assert_oracle(ctx.matchDocs(lex4, offs, seg), ref, ndocs)
    dev.run(ctx)
    assert not ctx.batchStatus(ndocs).any()
