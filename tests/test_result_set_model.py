"""Result-set mode on the CPU: the pure-Python restatement of the join predicate (tests/result_set_model.py) against the
oracle on COMPILED rule sets -- the optimizer moves programs keyed by frequent events onto their other term, and every case
here has such alt-keyed installs in the oracle's run -- and the eligibility query of the public interface
(PatternMatcherInstance.resultSetTier, sp_matcher_result_set_tier)."""
import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from struspattern_amd import synth

from .result_set_model import document_results, join_rules, results_multiset
from .finished_support import _docs

OPS = ["sequence", "within", "sequence_struct", "within_struct", "any", None]


def _rules(case, op):
    """a random rule set whose compiled form has alt-keyed programs.  `any` programs are never alt-keyed (the optimizer
    finds no alternative key for them), so the `any` sets carry a few sequences beside them."""
    rng = np.random.default_rng(5000 + case)
    nrules = int(rng.integers(40, 200))
    nfeat = int(rng.integers(6, 30))
    rules = synth.random_rules(nrules, nfeat, 700 + case, op=op)
    if op == "any":
        rules += synth.random_rules(nrules // 4, nfeat, 900 + case, op="sequence")
    weight_factor = 1.5 if case % 2 else 3.0            # (default 10: with few features, few programs are moved)
    return rules, nfeat, weight_factor, rng


def _compiled(m, rules, weight_factor):
    if weight_factor is not None:
        m.defineOption("weightFactor", weight_factor)
    synth.apply_rules(m, rules, compile=True)
    return m


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("chunk", range(4))
def test_model_equals_the_oracle_on_compiled_rule_sets(op, chunk):
    """10 rule sets per (operator, chunk): 240 in all; per-document multisets of (7-tuple, item count, items)"""
    for case in range(chunk * 10, chunk * 10 + 10):
        rules, nfeat, wf, rng = _rules(case, op)
        o = _compiled(oracle.L2Matcher(), rules, wf)
        jr, delimiter = join_rules(o.dumpTable())
        lex, offs = _docs(rng, 3, 110, nfeat, case % 3 != 0)
        l5 = synth.lexems5(lex)
        ref = o.run(l5, offs)
        assert ref.stats[:, 1].sum() > 0, (op, case)           # alt-keyed installs: the case exercises the replay
        for d in range(len(offs) - 1):
            doc = [tuple(x) for x in l5[int(offs[d]):int(offs[d + 1])].tolist()]
            got = document_results(jr, delimiter, doc)
            want = results_multiset(ref, d)
            assert got == want, (op, case, d, list((got - want).items())[:2], list((want - got).items())[:2])


def test_model_reads_the_same_table_from_the_product_compiler():
    rules, nfeat, wf, rng = _rules(3, None)
    o = _compiled(oracle.L2Matcher(), rules, wf)
    m = _compiled(spa.PatternMatcherInstance(), rules, wf)
    assert list(m.dumpTable()) == list(o.dumpTable())
    jr, _ = join_rules(m.dumpTable())
    assert any(r.kind != 0 and r.kind != 1 for r in jr)


def test_result_set_tier_counts_alt_keyed_programs():
    rules = synth.random_rules(400, 30, 11)
    m = spa.PatternMatcherInstance()
    synth.apply_rules(m, rules, compile=True)
    ok, why, alt = m.resultSetTier()
    assert ok and why == "" and alt > 0
    # the same rule set not optimized: eligible, nothing moved
    u = spa.PatternMatcherInstance()
    synth.apply_rules(u, rules, compile=False)
    assert u.resultSetTier() == (True, "", 0)


def _tier(build):
    m = spa.PatternMatcherInstance()
    build(m)
    m.compile()
    ok, why, alt = m.resultSetTier()
    assert not ok and why and alt == 0
    return why


def test_result_set_tier_names_what_keeps_a_rule_set_on_the_exact_engine():
    def three_terms(m):
        m.pushTerm(1); m.pushTerm(2); m.pushTerm(3)
        m.pushExpression("sequence", 3, 10, 0)
        m.definePattern("x", "", True)

    def nested(m):
        m.pushTerm(1); m.pushTerm(2)
        m.pushExpression("sequence", 2, 5, 0)
        m.definePattern("inner", "", False)
        m.pushPattern("inner"); m.pushTerm(3)
        m.pushExpression("within", 2, 5, 0)
        m.definePattern("outer", "", True)

    def and_(m):
        m.pushTerm(1); m.pushTerm(2)
        m.pushExpression("and", 2, 0, 0)
        m.definePattern("x", "", True)

    def exclusive(m):
        m.pushTerm(1); m.pushTerm(2)
        m.pushExpression("sequence", 2, 5, 0)
        m.definePattern("x", "", True)
        m.defineOption("exclusive", 1)

    assert "more than two terms" in _tier(three_terms)
    assert "listens" in _tier(nested)
    assert "neither sequence, within nor any" in _tier(and_)
    assert "exclusive" in _tier(exclusive)
