"""GPU tests of the loops of the words kernel's flush path (wordsFlush: literal probe, shape probes, the merge into output
rounds; confirmWalk; the waiting ends of wordsUnit) at their edges: probe depth 0, 1 and >= 3 and misses after a chain in
both hash tables, a literal longer than the 16 inline bytes, lanes with no, one and every variant, flushes of 63, 64 and
65 records on the simple and on the merging path, 63 to 128 ends in a unit, the drain under pressure, documents shorter
than four bytes and empty ones.  Every batch runs on the 16-wave and on the 12-wave instance; lexems, offsets and status are
the oracle's, the number of records the kernel queued is the one tests/l1_words_model.py predicts, no tolerance anywhere.
(What the batches contain is asserted on the CPU by tests/test_l1_words_loops_model.py, which also holds the model against
the oracle.  The kernel's records themselves are not visible to Python: they are compared through their count and through
the lexems the post kernel makes of them.)"""
import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from tests import l1_words_cases as cases
from tests import l1_words_loops_cases as lc
from tests import l1_words_model as model

pytestmark = pytest.mark.gpu

KERNEL = {"w16": "spa_l1_words_kernel_w16", "w12": "spa_l1_words_kernel"}
_REF = {}


def _reference(group):
    """the oracle's (lexems, offsets) and the model's record count of a group's batch, computed once"""
    if group not in _REF:
        name, docs = lc.GROUPS[group]
        docs = docs()
        ol = oracle.L1Lexer()
        lc.build(ol, name)
        ref, roffs = ol.matchDocs(b"".join(docs), cases.offsets(docs), nthreads=8)
        _REF[group] = (docs, ref, roffs, model.word_reports(lc.tables(name), docs, model.chunk_of(None)))
    return _REF[group]


@pytest.mark.parametrize("mode", sorted(KERNEL))
@pytest.mark.parametrize("group", sorted(lc.GROUPS))
def test_flush_loops_at_their_edges(group, mode, monkeypatch):
    for var in ("SPA_L1_SHAPES", "SPA_L1_NO_WORDS_KERNEL", "SPA_L1_WORD_WAVES", "SPA_L1_CHUNK_BYTES"):
        monkeypatch.delenv(var, raising=False)
    if mode == "w12":
        monkeypatch.setenv("SPA_L1_WORD_WAVES", "1")
    docs, ref, roffs, reports = _reference(group)
    lx = spa.PatternLexerInstance()
    lc.build(lx, lc.GROUPS[group][0])
    ctx = lx.createContext()
    got = ctx.matchDocs(b"".join(docs), cases.offsets(docs), check=False)
    assert ctx.wordsKernelName() == KERNEL[mode]
    c = ctx.batchCounters()
    print("group %s mode %s: %d documents, %d word reports (model %d), %d lexems" % (group, mode, len(docs), c["word_reports"], reports, len(got.lexems)))
    assert c["failed_docs"] == 0
    assert np.array_equal(np.array([c["word_reports"]]), np.array([reports]))
    assert np.array_equal(got.status, np.zeros(len(docs), np.int32))
    assert np.array_equal(got.doc_offsets, roffs)
    assert np.array_equal(got.lexems, ref)
