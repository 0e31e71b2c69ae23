"""The two small rule sets of the launch-plan tests of the rule matcher (tests/test_l2_plan.py, tests/test_l2_plan_gpu.py), for
any object with the PatternMatcherInstanceInterface method names."""
from struspattern_amd import synth

OPS = ["sequence", "within", "sequence_struct", "within_struct", "any"]


def build_flat(m, max_range=5):
    """two-term rules of every flat operator, position ranges 1..max_range; not optimized (no alternative keys)"""
    rules = [("r%d" % i, OPS[i % 5], 1 + i % max_range, [1 + i % 7, 1 + (3 * i) % 11]) for i in range(40)]
    synth.apply_rules(m, rules, compile=False)
    return m


def build_nested(m):
    """a rule that listens to another rule's result: the general kernel only"""
    m.pushTerm(1)
    m.pushTerm(2)
    m.attachVariable("b")
    m.pushExpression("sequence", 2, 3, 0)
    m.pushTerm(3)
    m.pushExpression("within", 2, 8, 0)
    m.definePattern("outer", "", True)
    m.compile()
    return m
