"""The install path of the flat-tier rule kernel (struspattern_amd/csrc/l2_fast_kernel.hip: installBatch, installCompactT,
installStaticT, installBatchT, allocRuleIds, checkBuckets) at the shapes where it can go wrong (tests/l2_fast_install_cases.py):
key lists around one batch of 64, second triggers in no lane, every lane, the first and the last, a three-trigger program among
two-term ones, a bucket filled to its LDS capacity and one beyond, the free id stack at exactly the batch's need and one short,
a dynamic batch behind a static one, results straight from the install line in lane 0 and lane 63, a hand-over between the
batches of a key list.  Every case runs on the kernel instances n and t (R = 8, T = 128: the two-place instances of the same
code) and is compared bit for bit with the CPU oracle: results in firing order, items, statistics, document status."""
import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from struspattern_amd import synth
from tests import l2_fast_install_cases as cases

SWITCHES = ("SPA_L2_FAST", "SPA_L2_FAST_SIZE", "SPA_L2_FAST_MAXRULES", "SPA_L2_FAST_MAXSTAGED", "SPA_L2_JOIN", "SPA_L2_VERBOSE")
_REFERENCE = {}


def _reference(name):
    """the oracle's batch of a case, computed once and shared by the instances"""
    if name not in _REFERENCE:
        rules, docs, compile_, _, _ = cases.CASES[name]()
        o = oracle.L2Matcher()
        synth.apply_rules(o, rules, compile=compile_)
        lex, offs = cases.batch(docs)
        ref = o.run(synth.lexems5(lex), offs)
        for a in (ref.results, ref.items, ref.stats, ref.doc_offsets):
            a.setflags(write=False)
        _REFERENCE[name] = ref
    return _REFERENCE[name]


def test_the_oracle_alone_has_results_for_every_case():
    """CPU: no comparison below is one of nothing with nothing -- every document of every case yields results, the cases with
    captured items yield items, and the dynamic case installs programs by an alternative key"""
    for name in cases.CASES:
        ref = _reference(name)
        assert (np.diff(ref.doc_offsets.astype(np.int64)) > 0).all(), name
        assert len(ref.items) > 0, name
    assert _reference("dynamic-after-static").stats[:, 1].sum() > 0
    # the fill cases: one more entry per key event, and more key events in a row than the fullest bucket of either instance has
    # entries in LDS (the device-free launch plan tells the capacities) -- so its size is once exactly the capacity, then one more
    rules, docs, _, switches, _ = cases.CASES["bucket-fill-1"]()
    assert len(rules) == 1
    for instance in ("n", "t"):
        with pytest.MonkeyPatch.context() as around:
            for s in SWITCHES:
                around.delenv(s, raising=False)
            for k, v in switches[instance].items():
                around.setenv(k, v)
            m = spa.PatternMatcherInstance()
            synth.apply_rules(m, rules, compile=False)
            plan = m.launchPlan(256, len(docs), sum(len(d) for d in docs))
        assert plan["kernel"] == "spa_l2_fast_kernel_" + instance
        assert max(int(c) for c in plan["bucket_caps"].split(",")) + 1 < int((docs[0][:, 0] == cases.K).sum()) - 1


@pytest.mark.gpu
@pytest.mark.parametrize("instance", ["n", "t"])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_install_against_the_oracle(name, instance, monkeypatch):
    rules, docs, compile_, switches, handed = cases.CASES[name]()
    ref = _reference(name)
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    m = spa.PatternMatcherInstance()
    synth.apply_rules(m, rules, compile=compile_)
    with monkeypatch.context() as around:
        for k, v in switches[instance].items():
            around.setenv(k, v)
        ctx = m.createContext()
    assert ctx.kernelKind() == 1 and ctx.kernelName() == "spa_l2_fast_kernel_" + instance
    lex, offs = cases.batch(docs)
    got = ctx.matchDocs(lex, offs)
    assert np.array_equal(got.status, np.zeros(len(docs), np.int32))
    assert ctx.batchCounters()["handed_over"] == handed[instance]
    assert np.array_equal(got.doc_offsets, ref.doc_offsets)
    assert np.array_equal(got.results[:, :7], ref.results[:, :7]) and np.array_equal(got.results[:, 8], ref.results[:, 8])
    assert np.array_equal(got.items, ref.items)
    assert np.array_equal(got.stats, ref.stats)
