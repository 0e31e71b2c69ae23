"""CPU guards of tests/l1_words_loops_cases.py: every batch contains what tests/test_l1_words_loops_gpu.py takes it for
(probe depths in both hash tables, variants per batch, record totals around an output round, lanes on the simple and on the
merging path, waiting ends around 64 and 96, a drain under pressure, document edges), no text key collides with a
fingerprint, and the model and the oracle agree on every document: the model's live records merged with the scanned
reports are the oracle's reports.  No GPU."""
import pytest

import oracle
from tests import l1_words_loops_cases as lc
from tests import l1_words_model as model

WHOLE = model.chunk_of(None)
_ORACLE = {}


def _flushes(name, docs):
    t = lc.tables(name)
    return [f for d in docs for u in model.flush_trace(t, d, WHOLE) for f in u["flushes"]]


def test_probe_batch_reaches_every_depth():
    pw = lc.probe_words()
    for kind in ("lit_0", "lit_1", "lit_3", "lit_miss_0", "lit_miss_chain", "key_0", "key_1", "key_3", "key_miss_0", "key_miss_chain"):
        assert pw[kind], kind
    t = lc.tables("probes")
    # the tables are laid out as the kernel probes them: every key is found, at the depth the slots say
    assert all(lc.literal_depth("probes", w)[1] for w in t.literals) and all(lc.shape_depth("probes", k)[1] for k in t.shapes)
    assert max(lc.literal_depth("probes", w)[0] for w in t.literals) >= 3 and max(lc.shape_depth("probes", k)[0] for k in t.shapes) >= 3
    docs = lc.probe_docs()
    text = b" ".join(docs)
    for kind, words in pw.items():
        assert any(w in text for w in words), kind
    assert lc.LONG_LITERAL in t.literals and len(lc.LONG_LITERAL) > 16 and lc.LONG_LITERAL[:-1] + b"p" not in t.literals
    assert sorted(model.variants(t)) == [model.PREVWORD, model.PREFIX | (2 << 4), model.SUFFIX | (2 << 4)]
    assert not model.fingerprint_collisions(t, docs)


def test_variant_batch_has_lanes_of_no_one_and_every_variant():
    t = lc.tables("keys")
    docs = lc.variant_docs()
    assert len(model.variants(t)) == model.MAX_VARIANTS
    hits = [sum(1 for l in model.candidate_lists(t, docs[0], e)[1:] if l) for e in model.run_ends(t, docs[0])]
    assert 0 in hits and 1 in hits and model.MAX_VARIANTS in hits and len(docs[0]) <= model.TILE
    # one-letter words: no lane has a key of a two-byte variant
    keyed = [v for e in model.run_ends(t, docs[1]) for v in model.variants(t) if model.shape_key(docs[1], e, v)]
    assert not keyed
    assert not model.fingerprint_collisions(t, docs)


def test_merge_batch_totals_lie_around_an_output_round():
    fl = _flushes("dense", lc.merge_docs())
    totals = [f["total"] for f in fl]
    assert 63 in totals and 64 in totals and 65 in totals
    simple = [f for f in fl if f["total"] and max(f["lanes"]) == 1]
    assert any(f["total"] == 64 for f in simple)
    assert any(f["total"] == 65 and max(f["lanes"]) >= 3 for f in fl)          # a list of three on one lane carries the total over the round
    assert any(max(f["lanes"]) > 4 for f in fl)                                   # more candidates than the register network orders
    t = lc.tables("dense")
    both = [e for d in lc.merge_docs() for e in model.run_ends(t, d) if model.candidate_lists(t, d, e)[0] and any(model.candidate_lists(t, d, e)[1:])]
    assert both                                                                    # a literal list and shape lists on one end
    assert not model.fingerprint_collisions(t, lc.merge_docs())


def test_ends_batch_fills_and_drains():
    t = lc.tables("dense")
    docs = lc.ends_docs()
    for d, n in zip(docs, (63, 64, 65, 127, 128)):
        assert len(model.run_ends(t, d)) == n
    traces = [u for d in docs for u in model.flush_trace(t, d, WHOLE)]
    assert max(u["max_waiting"] for u in traces) == model.ENDS - 1
    counts = [[f["count"] for f in u["flushes"]] for u in traces]
    assert [63] in counts and [64] in counts and [64, 1] in counts and [64, 63] in counts and [64, 64] in counts and [64, 32] in counts
    assert any(f["pressure"] and f["count"] < 64 for u in traces for f in u["flushes"])
    assert not model.fingerprint_collisions(t, docs)


def test_edge_batch_has_short_and_empty_documents():
    t = lc.tables("keys_prev")
    docs = lc.edge_docs()
    assert any(len(d) < 4 and d for d in docs)
    assert any(not docs[i] and docs[i - 1] and docs[i + 1] for i in range(1, len(docs) - 1))
    assert any(e[1] < 4 for d in docs for e in model.run_ends(t, d)) and any(e[0] > len(d) - 4 and len(d) >= 8 for d in docs for e in model.run_ends(t, d))
    assert not model.fingerprint_collisions(t, docs)


@pytest.mark.parametrize("group", sorted(lc.GROUPS))
def test_model_and_oracle_agree(group):
    name, docs = lc.GROUPS[group]
    t = lc.tables(name)
    if name not in _ORACLE:
        _ORACLE[name] = oracle.L1Lexer()
        lc.build(_ORACLE[name], name)
    for d in docs():
        raw, _ = _ORACLE[name].matchDocs(d, [0, len(d)], raw=True)
        assert model.merged_reports(t, d, WHOLE) == [(int(r[0]), int(r[1]), int(r[2])) for r in raw], (group, d)
