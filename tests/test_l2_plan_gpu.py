"""GPU test of the launch plan of the rule matcher (struspattern_amd/csrc/l2_plan.hpp): for every engine a context can run
on, the kernel it reports is the one sp_matcher_launch_plan gives for the same rule set, flags and switches, the switches
count when the context is created (and only then), and the results are the oracle's."""
import numpy as np
import pytest
import torch

import oracle
import struspattern_amd as spa
from struspattern_amd import synth
from tests import l2_plan_cases as cases

pytestmark = pytest.mark.gpu

# (switches around createContext() only, result_sets flag, kernel kind, kernel name)
ENGINES = {
    "general": ({"SPA_L2_FAST": "0"}, False, 0, "spa_l2_match_kernel"),
    "flat": ({}, False, 1, "spa_l2_fast_kernel_n"),
    "flat-t": ({"SPA_L2_FAST_SIZE": "t"}, False, 1, "spa_l2_fast_kernel_t"),
    "join": ({}, True, 2, "spa_l2_join_kernel"),
}


def _documents():
    """3 documents of 8 lexems: ids 1..11 and a delimiter, one lexem per position"""
    rng = np.random.default_rng(7)
    n = 8
    lex = np.zeros((3 * n, 4), np.uint32)
    lex[:, 0] = rng.integers(1, 12, size=3 * n)
    lex[[5, 12], 0] = synth.DELIM
    lex[:, 1] = np.tile(np.arange(1, n + 1), 3)
    lex[:, 2] = np.tile(np.arange(n) * 3, 3)
    lex[:, 3] = 2
    return lex, np.arange(4, dtype=np.uint64) * n


def _sorted_results(batch, d):
    out = []
    for r in batch.results[batch.doc_offsets[d]:batch.doc_offsets[d + 1]].tolist():
        out.append(tuple(r[:7]) + (r[8],) + tuple(batch.items[r[7]:r[7] + r[8]].reshape(-1).tolist()))
    return sorted(out)


@pytest.fixture(scope="module")
def reference():
    lex, offs = _documents()
    ref = cases.build_flat(oracle.L2Matcher()).run(synth.lexems5(lex), offs)
    assert len(ref.results) > 0 and len(ref.items) > 0
    return lex, offs, ref


@pytest.mark.parametrize("engine", list(ENGINES))
def test_context_runs_what_the_plan_says(engine, reference, monkeypatch, capfd):
    switches, result_sets, kind, kernel = ENGINES[engine]
    lex, offs, ref = reference
    for s in ("SPA_L2_FAST", "SPA_L2_FAST_SIZE", "SPA_L2_FAST_MAXRULES", "SPA_L2_FAST_MAXSTAGED", "SPA_L2_JOIN", "SPA_L2_VERBOSE"):
        monkeypatch.delenv(s, raising=False)
    m = cases.build_flat(spa.PatternMatcherInstance())
    with monkeypatch.context() as around:
        for k, v in switches.items():
            around.setenv(k, v)
        plan = m.launchPlan(torch.cuda.get_device_properties(0).multi_processor_count, 3, len(lex), result_sets=result_sets)
        ctx = m.createContext(result_sets=result_sets)
    assert (int(plan["kind"]), plan["kernel"]) == (kind, kernel)
    assert (ctx.kernelKind(), ctx.kernelName()) == (kind, kernel)
    # the verbose switch is read when the context is created: set afterwards, it leaves the run silent
    monkeypatch.setenv("SPA_L2_VERBOSE", "1")
    capfd.readouterr()
    got = ctx.matchDocs(lex, offs)
    ctx.batchCounters()
    assert "[spa]" not in capfd.readouterr().err
    assert (ctx.kernelKind(), ctx.kernelName()) == (kind, kernel)
    assert np.array_equal(got.status, np.zeros(3, np.int32))
    assert np.array_equal(got.doc_offsets, ref.doc_offsets)
    if engine == "join":                    # result-set mode: the right multiset per document, not the order inside it
        for d in range(3):
            assert _sorted_results(got, d) == _sorted_results(ref, d)
    else:
        assert np.array_equal(got.results[:, :7], ref.results[:, :7]) and np.array_equal(got.results[:, 8], ref.results[:, 8])
        assert np.array_equal(got.items, ref.items) and np.array_equal(got.stats, ref.stats)
