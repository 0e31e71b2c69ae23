"""The constructed cases of tests/l2_general_cases.py, checked on the CPU: every case gives the oracle something to report,
the plain model of tests/l2_general_model.py reproduces the oracle's statistics and results on it (so the model cannot
drift), the numbers the case claims are the ones the model counts, and every claim sits on the intended side of the
kernel's thresholds.  A change to the optimizer, the event hash or a case that moves a case off its edge fails here, not
silently in tests/test_l2_general_edges_gpu.py."""
import functools

import numpy as np
import pytest

import oracle
from struspattern_amd import synth

from . import l2_general_cases as cases
from .l2_general_model import MAXT as MODEL_MAXT, Table, bucket_of, run_document

# The thresholds of the general kernel: the enums of struspattern_amd/csrc/l2_kernel.hip
# (`enum {DEACT_MAXCHAIN=4, SCRLDS_CAP=32, EXPLIST_CAP=128, REPLAY_MAX=8}` above deactivateBatch, `enum {MAXT=3}` above
# installBatch), the 64 lanes of a batch and the 64 positions of the expiry window.
EXPLIST_CAP = 128       # rules expiring at one position: LDS list up to here, the arena's dispose list above
SCRLDS_CAP = 32         # triggers of one 64-block in one bucket: partition in LDS up to here, in the arena scratch above
REPLAY_MAX = 8          # swap-removals a lane replays per round of loads
DEACT_MAXCHAIN = 4      # trigger slots of a rule block: a rule with more sends its 64-block down the serial path
MAXT = 3                # trigger templates of a program the install batch handles
BATCH = 64              # rules per deactivation block, programs per install batch
WINDOW = 64             # expiry positions kept per position; later ones wait in the far-expiry heap
# Defaults of initialArena() in struspattern_amd/csrc/capi_l2.cpp.  They are no contract: the cases only have to exceed
# them, the GPU test asserts the arena status and the growth, not the capacity at which it appears.
DEFAULT_WIN_CAP = 128
DEFAULT_BUCKET_CAP = 256
DEFAULT_HEAP_CAP = 256


@functools.lru_cache(maxsize=None)
def _case(name):
    build, lex4, offs, seg, claims = cases.CASES[name]()
    o = oracle.L2Matcher()
    build(o)
    l5 = synth.lexems5(lex4)
    l5[:, 2] = seg
    ref = o.run(l5, offs)
    table = Table(o.dumpTable())
    runs = [run_document(table, lex4[int(offs[d]):int(offs[d + 1])]) for d in range(len(offs) - 1)]
    return ref, table, runs, claims, (lex4, offs)


def _top2(per_bucket):
    return sorted(per_bucket)[-2:]


def _measure(runs):
    """the numbers a case can claim, counted by the model"""
    m = {}
    longest = [max(a.expiry_lists, default=(0, 0)) for a in runs]
    m["expiring_per_document"] = [n for n, _ in longest]
    m["max_expiring_at_one_position"] = max(m["expiring_per_document"])
    m["holes_in_the_longest_list_per_document"] = [max(h for n, h in a.expiry_lists if n == top[0]) if a.expiry_lists else 0 for a, top in zip(runs, longest)]
    blocks = [b for a in runs for b in a.blocks]
    for kind, key in (("expiry", "block_bucket_max_per_document"), ("fired", "fired_block_bucket_max_per_document")):
        m[key] = [max((max(b["per_bucket"]) for b in a.blocks if b["kind"] == kind), default=0) for a in runs]
    m["max_triggers_of_one_block_in_one_bucket"] = max(max(b["per_bucket"]) for b in blocks)
    m["two_buckets_of_one_block"] = max((_top2(b["per_bucket"]) for b in blocks), key=lambda t: t[0])
    m["fired_list_max_per_document"] = [max(a.fired_lists, default=0) for a in runs]
    m["max_fired_list"] = max(m["fired_list_max_per_document"])
    m["survivors_moved"] = sum(b["survivors_moved"] for b in blocks)
    m["duplicate_entries"] = sum(b["dups"] for b in blocks)
    m["duplicates_in_a_later_block"] = sum(1 for b in blocks for x in b["dup_blocks"] if x > 0)
    m["wide_rule_at_list_index"] = [next((b["wide_at"][0] for b in a.blocks if b["wide_at"]), None) for a in runs]
    m["wide_rules_per_list"] = max((len(b["wide_at"]) for b in blocks), default=0)
    biggest = [max(a.key_events, key=lambda k: k["programs"], default=None) for a in runs]
    m["programs_on_one_key_event"] = [k["programs"] if k else 0 for k in biggest]
    on_biggest = [k for a, big in zip(runs, biggest) if big for k in a.key_events if k["event"] == big["event"]]
    m["slow_program_slots"] = sorted(set(s for k in on_biggest for s in k["slow_slots"]))
    m["slow_program_kinds"] = sorted(set(x for k in on_biggest for v in k["slow_slots"].values() for x in v))
    m["alt_keyed_slots"] = sorted(set(s for k in on_biggest for s in k["alt_slots"]))
    m["max_expiry_positions_in_one_batch"] = max((max(k["expiry_positions_per_batch"]) for k in on_biggest), default=0)
    m["heap_peak"] = max(a.heap_peak for a in runs)
    m["positions_mod_64"] = sorted(set().union(*[a.pos_mod64 for a in runs]) & {WINDOW - 1, 0, 1})
    m["landings_at_heap_entries"] = sorted(set().union(*[a.heap_landings for a in runs]))
    m["jumps_over_64"] = sum(a.long_jumps for a in runs) > 0
    m["tie_migrations"] = sum(a.heap_tie_migrations for a in runs) > 0
    m["disposed_behind_the_window"] = sum(a.heap_disposed_directly for a in runs) > 0
    m["max_triggers_in_one_bucket"] = max(max(a.bucket_peak) for a in runs)
    m["events_in_it_per_document"] = [a.bucket_peak_events[int(np.argmax(a.bucket_peak))] for a in runs]
    return m


def _sides(values, cap):
    """the values fill the capacity exactly and go one beyond it"""
    return cap in values and cap + 1 in values


def _edges_expiry(m):
    n = m["expiring_per_document"]
    assert _sides(n, BATCH) and _sides(n, EXPLIST_CAP) and _sides(n, 3 * BATCH)                 # 64|65, 128|129, 192|193
    assert BATCH - 1 in n and EXPLIST_CAP - 1 in n and EXPLIST_CAP + 2 in n and max(n) > 4 * BATCH      # 63, 127, 130; a fifth block
    assert max(n) > DEFAULT_WIN_CAP
    assert m["survivors_moved"] > 0


def _edges_expiry_holes(m):
    _edges_expiry(m)
    assert all(0 < h < n for h, n in zip(m["holes_in_the_longest_list_per_document"], m["expiring_per_document"]))


def _edges_partition(m, key="block_bucket_max_per_document"):
    k = m[key]
    assert _sides(k, REPLAY_MAX) and _sides(k, 2 * REPLAY_MAX) and _sides(k, SCRLDS_CAP)        # 8|9, 16|17, 32|33
    assert BATCH in k
    lo, hi = m["two_buckets_of_one_block"]
    assert lo == SCRLDS_CAP - 1 and hi == SCRLDS_CAP + 1
    assert m["survivors_moved"] > 0


def _edges_fired(m):
    _edges_partition(m, "fired_block_bucket_max_per_document")
    assert m["duplicate_entries"] > 0 and m["duplicates_in_a_later_block"] > 0
    assert m["max_fired_list"] > BATCH


def _edges_chain(m):
    assert sorted(set(m["expiring_per_document"])) == [BATCH, BATCH + 1]
    at = list(zip(m["expiring_per_document"], m["wide_rule_at_list_index"]))
    assert set(at) == {(BATCH, 0), (BATCH, 31), (BATCH, 63), (BATCH + 1, 0), (BATCH + 1, 31), (BATCH + 1, 63), (BATCH + 1, 64)}
    assert m["wide_rules_per_list"] == 1


def _edges_install(m):
    assert m["programs_on_one_key_event"] == [BATCH, BATCH + 1, 2 * BATCH, 2 * BATCH + 1]
    assert m["slow_program_slots"] == [0, 1, BATCH - 2, BATCH - 1, BATCH]
    assert m["slow_program_kinds"] == ["bare_capture", "far", "wide"]
    assert m["max_expiry_positions_in_one_batch"] > 8


def _edges_install_alt(m):
    assert min(m["programs_on_one_key_event"]) > BATCH
    assert len(m["alt_keyed_slots"]) >= 3
    assert m["max_expiry_positions_in_one_batch"] > 8


def _edges_heap(m):
    assert m["heap_peak"] > DEFAULT_HEAP_CAP
    assert m["positions_mod_64"] == [0, 1, WINDOW - 1] and m["landings_at_heap_entries"] == [-1, 0, 1]
    assert m["jumps_over_64"] and m["tie_migrations"] and m["disposed_behind_the_window"]


def _edges_capacity(m):
    assert m["max_triggers_in_one_bucket"] > DEFAULT_BUCKET_CAP
    assert 1 in m["events_in_it_per_document"] and max(m["events_in_it_per_document"]) > 1
    assert m["max_fired_list"] > DEFAULT_BUCKET_CAP


EDGES = {
    "expiry_list": _edges_expiry,
    "expiry_list_holes": _edges_expiry_holes,
    "bucket_partition": _edges_partition,
    "dispose_by_firing": _edges_fired,
    "long_chain_in_block": _edges_chain,
    "install_runs": _edges_install,
    "install_runs_alt": _edges_install_alt,
    "far_heap": _edges_heap,
    "bucket_capacity": _edges_capacity,
}
WITH_ITEMS = set(cases.CASES)       # every case captures variables


def test_the_table_of_cases_is_complete():
    assert set(EDGES) == set(cases.CASES) and set(cases.CAPACITY_CASES) <= set(cases.CASES)
    assert MODEL_MAXT == MAXT


def test_event_hash_of_the_model():
    """evhash as in csrc/l2_fast_tables.cpp / l2_kernel.hip, on values worked out by hand"""
    # a = 1: a += ~(a >> 5) -> 0; a += a << 3 -> 0; a ^= a >> 4 -> 0
    assert bucket_of(1) == 0
    # a = 32: ~(1) = 0xFFFFFFFE, a = 30; a += 240 -> 270; 270 ^ 16 = 286 -> 286 & 15 = 14
    assert bucket_of(32) == 14
    for b in range(16):
        assert [bucket_of(t) for t in cases.terms_in_bucket(b, 3, 1000)] == [b] * 3


@pytest.mark.parametrize("name", list(cases.CASES))
def test_oracle_output_is_not_trivial(name):
    ref, _, runs, _, (lex4, offs) = _case(name)
    assert 4 <= len(runs) <= 12 and len(lex4) / len(runs) < 400
    assert np.array_equal(ref.status, np.zeros(len(runs), np.int32))
    assert len(ref.results) > 0 and all(len(ref.doc(d)) > 0 for d in range(len(runs)))
    if name in WITH_ITEMS:
        assert len(ref.items) > 0


@pytest.mark.parametrize("name", list(cases.CASES))
def test_model_agrees_with_the_oracle(name):
    """installed programs, alt-keyed installs, signals, open triggers and the results in their order, per document"""
    ref, _, runs, _, _ = _case(name)
    for d, a in enumerate(runs):
        assert [int(x) for x in ref.stats[d]] == a.stats, (name, d)
        got = np.array(a.results, np.uint32).reshape(-1, 3)
        assert np.array_equal(got, ref.doc(d)[:, :3]), (name, d)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_claims_sit_on_their_edges(name):
    _, _, runs, claims, _ = _case(name)
    m = _measure(runs)
    print(name, {k: m[k] for k in claims})
    for k, v in claims.items():
        assert m[k] == v, (name, k, m[k], v)
    EDGES[name](m)
