"""GPU test of the launch plan of the lexer (struspattern_amd/csrc/l1_image.hpp): for every route a batch can take, the
kernel names a context reports after the launch are the ones sp_lexer_launch_plan gives for the same table, device and
batch, and the lexems are the oracle's.  (tests/test_l1_lanes_gpu.py ties the name to the kernel that really ran.)"""
import numpy as np
import pytest
import torch

import oracle
from tests import l1_plan_cases as cases
import struspattern_amd as spa

pytestmark = pytest.mark.gpu

# (table, switches of the launch, the 70 KB document as well)
CASES = [
    ("no_exceptions", {}, False), ("no_exceptions", {"SPA_L1_NO_LANES": "1"}, False), ("no_exceptions", {"SPA_L1_WORD_WAVES": "12"}, False),
    ("no_exceptions", {}, True), ("no_exceptions", {"SPA_L1_CHUNK_BYTES": "64"}, True),
    ("exceptions", {}, False), ("shapes_behind_one_pass", {}, False), ("shapes_off", {}, False), ("literals_only", {}, False),
    ("unicode_class", {}, True), ("approx", {}, False),
]


@pytest.mark.parametrize("name,switches,long_doc", CASES, ids=["%s%s%s" % (n, "".join("-" + k[7:].lower() for k in s), "-long" if l else "") for n, s, l in CASES])
def test_reported_kernels_are_the_planned_ones(name, switches, long_doc, monkeypatch):
    lx = cases.build(spa.PatternLexerInstance(), name, monkeypatch)
    o = cases.build(oracle.L1Lexer(), name, monkeypatch)
    docs = cases.DOCS + ([cases.long_doc()] if long_doc else [])
    text = b"".join(docs)
    offs = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    plan = lx.launchPlan(torch.cuda.get_device_properties(0).multi_processor_count, len(docs), len(text))
    ctx = lx.createContext()
    assert (ctx.scanKernelName(), ctx.wordsKernelName()) == ("(none)", "(none)")
    got = ctx.matchDocs(text, offs)
    assert (ctx.scanKernelName(), ctx.wordsKernelName()) == (plan["scan_kernel"], plan["words_kernel"])
    if long_doc and name == "no_exceptions":
        assert ctx.batchCounters()["scan_units"] > len(docs) and int(plan["max_units"]) >= ctx.batchCounters()["scan_units"]
    ref, roffs = o.matchDocs(text, offs)
    assert len(ref) > 0
    assert np.array_equal(got.status, np.zeros(len(docs), np.int32))
    assert np.array_equal(got.doc_offsets, roffs)
    assert np.array_equal(got.lexems, ref)
