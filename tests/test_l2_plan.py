"""CPU tests (no GPU) of the host layer of a rule-matcher launch (struspattern_amd/csrc/l2_plan.hpp): which kernel serves a
rule set and why not the others, the grids, arena, spill-area and output sizes of a batch, the arena policy and the flat
tier's layout.  Expected values are worked out by hand for a device of 256 compute units; the arena size is restated here
from the record sizes documented in l2_device.h, not read from the code under test."""
import pytest

import struspattern_amd as spa
from tests import l2_plan_cases as cases

CUS = 256
WAVE_SLOTS = CUS * 12           # general kernel: 12 single-wave workgroups per CU
FAST_PER_CU = 16                # LDS-resident kernel: 10 KB of LDS per document -> 16 waves per CU
FAST_SLOTS = CUS * FAST_PER_CU
JOIN_SLOTS = CUS * 32
ARENA_LIMIT = 48 << 30          # a per-wave arena stays below 48 GiB

SWITCHES = ("SPA_L2_FAST", "SPA_L2_FAST_SIZE", "SPA_L2_FAST_MAXRULES", "SPA_L2_FAST_MAXSTAGED", "SPA_L2_JOIN", "SPA_L2_VERBOSE")


@pytest.fixture
def no_switches(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    return monkeypatch


def _flat(max_range=5):
    return cases.build_flat(spa.PatternMatcherInstance(), max_range)


def _nested():
    return cases.build_nested(spa.PatternMatcherInstance())


def _ints(p, *names):
    return tuple(int(p[n]) for n in names)


def _align(v, a):
    return (v + a - 1) // a * a


def _arena_bytes(grows, nstop=0):
    """bytes of the general kernel's per-wave arena after `grows` doublings of the initial capacities (l2_device.h: a rule
    block of 32 words = the rule record and its four trigger slots; item 12 words, follow 12, stop-log 12, staged result 8,
    data reference 2, heap entry 2; {event, trigger} pairs of 16 buckets; free lists of one word per record)"""
    g = 1 << grows
    rules, bucket, items, refs, follow, dispose, heap = 1024 * g, 256 * g, 2048 * g, 1024 * g, 256 * g, 512 * g, 256 * g
    gstack, staged, wincap, scratch = 64 * g, 1024 * g, 128 * g, 256
    w = 32 * rules + _align(2 * 16 * bucket, 32) + 16 + 64
    w += _align(2 * heap, 4) + _align(12 * follow, 4) + _align(dispose, 4) + _align(12 * max(nstop, 1), 4)
    w += _align(12 * items, 4) + _align(2 * refs, 4) + _align(gstack, 4) + _align(8 * staged, 4)
    w += _align(rules, 4) + _align(items, 4) + _align(refs, 4)
    chunk = max(16, wincap // 8)                # expiry window: lists of chunks, a pool for every live rule + 64 partly filled ones
    chunks = rules // chunk + 64
    w += _align(chunks * chunk, 4) + 64 * 8 + _align(chunks, 4)
    w += _align(16 * scratch, 4)
    return _align(w, 64) * 4


def test_general_engine_blocks_and_arena(no_switches):
    m = _nested()
    expected = {0: (1, 1), 1: (1, 1), 63: (63, 63), 64: (64, 3072), 3072: (3072, 3072), 3073: (3072, 3072)}
    for ndocs, (blocks, alloc) in expected.items():
        p = m.launchPlan(CUS, ndocs, 8 * ndocs)
        assert (p["engine"], p["kind"], p["route"], p["kernel"]) == ("general", "0", "general", "spa_l2_match_kernel"), ndocs
        assert _ints(p, "general_blocks", "arena_run", "arena_alloc_waves") == (blocks, blocks, alloc), ndocs
        assert _ints(p, "fast_blocks", "spill_alloc_waves", "list_blocks", "join_blocks") == (0, 0, 0, 0)
        assert int(p["arena_per_wave_bytes"]) == _arena_bytes(0, int(p["stop_words"]))
    assert p["flat_why_not"] == "nested expressions (a rule listens to another rule's result)"


def test_rerun_allocates_what_it_runs(no_switches):
    for m in (_nested(), _flat()):
        for n in (3, 100):
            p = m.launchPlan(CUS, 1000, 8000, rerun_docs=n)
            assert p["route"] == "rerun-list"
            assert _ints(p, "general_blocks", "arena_run", "arena_alloc_waves") == (n, n, n)        # never the full machine
            assert _ints(p, "fast_blocks", "list_blocks", "join_blocks") == (0, 0, 0)
    assert m.launchPlan(CUS, 1000, 8000, rerun_docs=100)["arena_alloc"] == str(WAVE_SLOTS)     # (what a new batch of 100 gets)


def test_arena_cap(no_switches):
    m = _nested()
    nstop = int(m.launchPlan(CUS, 1, 8)["stop_words"])
    fit = lambda g: ARENA_LIMIT // _arena_bytes(g, nstop)
    g = next(g for g in range(11) if fit(g) < WAVE_SLOTS)
    assert g > 0 and fit(g - 1) >= WAVE_SLOTS and fit(g) >= 64
    p = m.launchPlan(CUS, 5000, 40000, arena_grows=g - 1)
    assert _ints(p, "arena_run", "arena_alloc_waves") == (WAVE_SLOTS, WAVE_SLOTS)
    p = m.launchPlan(CUS, 5000, 40000, arena_grows=g)
    assert int(p["arena_per_wave_bytes"]) == _arena_bytes(g, nstop)
    assert _ints(p, "general_blocks", "arena_run", "arena_alloc", "arena_alloc_waves") == (fit(g),) * 4
    # a batch of 64 documents gets all that fits, not the full machine
    assert _ints(m.launchPlan(CUS, 64, 512, arena_grows=g), "arena_run", "arena_alloc_waves") == (64, fit(g))
    # one more grow halves it (the capacities that do not double are below 32 KB of more than 16 MB per wave)
    q = m.launchPlan(CUS, 5000, 40000, arena_grows=g + 1)
    assert _ints(q, "arena_run", "arena_alloc_waves") == (fit(g + 1),) * 2
    assert fit(g) // 2 <= int(q["arena_run"]) <= fit(g) // 2 + 2


def test_arena_grow_limit(no_switches):
    m = _nested()
    for g in range(11):
        p = m.launchPlan(CUS, 1, 8, arena_grows=g)
        assert _ints(p, "arena_max_rules", "arena_scratch_cap") == (1024 << g, 256)
    assert int(p["arena_max_rules"]) == 1 << 20
    with pytest.raises(spa.PatternError, match="arena at its maximum size"):
        m.launchPlan(CUS, 1, 8, arena_grows=11)


def test_flat_engine_blocks_and_spill_area(no_switches):
    m = _flat()
    expected = {1: (1, 1), 63: (63, 63), 64: (64, 4096), 4096: (4096, 4096), 4097: (4096, 4096)}
    for ndocs, (blocks, spill) in expected.items():
        p = m.launchPlan(CUS, ndocs, 8 * ndocs, fast_blocks_per_cu=FAST_PER_CU)
        assert (p["engine"], p["kind"], p["route"], p["kernel"], p["flat_why_not"]) == ("flat", "1", "flat+list", "spa_l2_fast_kernel_n", ""), ndocs
        assert _ints(p, "fast_blocks", "spill_alloc_waves") == (blocks, spill), ndocs
        general = min(ndocs, WAVE_SLOTS)
        assert _ints(p, "general_blocks", "list_blocks", "join_blocks") == (general, min(general, 512), 0), ndocs
        assert int(p["spill_per_wave_bytes"]) == 4 * int(p["spill_words"])
    assert p["join_why_not"] != ""


def test_join_engine_blocks(no_switches):
    m = _flat()
    for ndocs, blocks in {0: 1, 1: 1, 8192: 8192, 8193: 8192}.items():
        p = m.launchPlan(CUS, ndocs, 8 * ndocs, result_sets=True)
        assert (p["engine"], p["kind"], p["route"], p["kernel"], p["join_why_not"]) == ("join", "2", "join", "spa_l2_join_kernel", ""), ndocs
        assert _ints(p, "join_blocks", "fast_blocks", "list_blocks") == (blocks, 0, 0), ndocs
        assert int(p["arena_run"]) == max(1, min(ndocs, WAVE_SLOTS))        # (the general kernel's arena is kept for a rerun)


def test_output_sizing(no_switches):
    m = _flat()
    assert _ints(m.launchPlan(CUS, 1, 0), "want_results", "want_items") == (1024, 1024)
    assert _ints(m.launchPlan(CUS, 1, 1000), "want_results", "want_items") == (3024, 7024)
    assert _ints(m.launchPlan(CUS, 1, 1000, min_results=5000, min_items=7000), "want_results", "want_items") == (5000, 7024)
    assert _ints(m.launchPlan(CUS, 1, 1000, min_results=3000, min_items=9000), "want_results", "want_items") == (3024, 9000)
    # item indices are 32 bit: 6 x 715 827 883 + 1024 is above 2^32 - 1, 2 x 715 827 883 + 1024 is not
    assert _ints(m.launchPlan(CUS, 1, 715827883), "want_results", "want_items") == (2 * 715827883 + 1024, (1 << 32) - 1)
    assert _ints(m.launchPlan(CUS, 1, 8, min_results=1 << 40), "want_results", "want_items") == ((1 << 32) - 1, 1072)


def test_document_limit(no_switches):
    m = _flat()
    assert m.launchPlan(CUS, (1 << 32) - 2, 8)["fast_blocks"] == str(FAST_SLOTS)
    with pytest.raises(spa.PatternError, match="too many documents in one batch"):
        m.launchPlan(CUS, (1 << 32) - 1, 8)


def test_engine_choice(no_switches):
    m = _flat()
    p = m.launchPlan(CUS, 3, 24)
    assert (p["engine"], p["flat_why_not"], p["join_why_not"]) == ("flat", "", "result sets not asked for")
    assert m.fastTier() == (True, "") and m.resultSetTier()[:2] == (True, "")
    j = m.launchPlan(CUS, 3, 24, result_sets=True)
    assert (j["engine"], j["flat_why_not"], j["join_why_not"]) == ("join", "", "") and int(j["alt_programs"]) == m.resultSetTier()[2]
    no_switches.setenv("SPA_L2_JOIN", "1")
    assert m.launchPlan(CUS, 3, 24) == j                                    # the switch equals the flag
    no_switches.setenv("SPA_L2_JOIN", "0")
    assert m.launchPlan(CUS, 3, 24) == p
    no_switches.delenv("SPA_L2_JOIN")
    no_switches.setenv("SPA_L2_FAST", "0")
    q = m.launchPlan(CUS, 3, 24)
    assert (q["engine"], q["kind"], q["kernel"], q["route"], q["flat_why_not"]) == ("general", "0", "spa_l2_match_kernel", "general", "disabled by SPA_L2_FAST=0")
    assert _ints(q, "general_blocks", "fast_blocks", "list_blocks") == (3, 0, 0)
    assert m.fastTier() == (True, "") and m.resultSetTier()[:2] == (True, "")   # the tier queries ignore the environment
    no_switches.delenv("SPA_L2_FAST")
    no_switches.setenv("SPA_L2_FAST_MAXRULES", "9999")                      # trigger ids are 14 bits
    assert m.launchPlan(CUS, 3, 24)["max_rules"] == "4095"
    no_switches.setenv("SPA_L2_FAST_MAXRULES", "24")
    no_switches.setenv("SPA_L2_FAST_MAXSTAGED", "40")
    no_switches.setenv("SPA_L2_FAST_SIZE", "t")
    t = m.launchPlan(CUS, 3, 24)
    assert (t["kernel"], t["max_rules"], t["max_staged"]) == ("spa_l2_fast_kernel_t", "24", "40")


def test_engine_choice_of_rule_sets_that_are_refused(no_switches):
    m = _flat()
    m.defineOption("exclusive")
    p = m.launchPlan(CUS, 3, 24, result_sets=True)
    why = "the `exclusive` option (its outcome depends on the order of the results)"
    assert (p["engine"], p["join_why_not"], p["alt_programs"]) == ("flat", why, "0")
    assert m.resultSetTier() == (False, why, 0) and m.fastTier() == (True, "")
    n = _nested()
    p = n.launchPlan(CUS, 3, 24, result_sets=True)
    assert p["engine"] == "general" and n.fastTier() == (False, p["flat_why_not"]) and n.resultSetTier() == (False, p["join_why_not"], 0)
    assert p["flat_why_not"] != "" and p["join_why_not"] != ""


@pytest.mark.parametrize("size,R,T", [("n", 256, 448), ("t", 8, 128)])
def test_flat_layout(no_switches, size, R, T):
    """R, T: the LDS capacities of the kernel instances n and t (l2_fast_kernel.hip)"""
    no_switches.setenv("SPA_L2_FAST_SIZE", size)
    p = _flat(max_range=5).launchPlan(CUS, 3, 24)
    assert p["kernel"] == "spa_l2_fast_kernel_" + size and _ints(p, "R", "T") == (R, T)
    assert p["exp_shift"] == "3"                                            # 6 expiry rows (ranges 0..5) need 8
    caps = [int(c) for c in p["bucket_caps"].split(",")]
    assert len(caps) == 16 and min(caps) >= 8 and sum(caps) <= T
    max_rules, max_staged = _ints(p, "max_rules", "max_staged")
    assert (max_rules, max_staged) == (2048, 32768)
    a4 = lambda n: _align(n, 4)
    spill_rules = max_rules - R
    # l2_fast_tables.cpp, layoutFast: cold records of 8 words per rule id; rule word, 3 links, install line, key lexem and free
    # stack entry per spill rule; 16 spill buckets of 1024 {event, ts} entries; staged results of 8 words; the long dispose
    # list; one expiry row of max_rules per position
    words = a4(8 * max_rules) + a4(spill_rules) + a4(3 * spill_rules) + 3 * a4(spill_rules) + a4(2 * 16 * 1024)
    words += a4(8 * max_staged) + a4(max(max_rules, 64)) + a4((1 << 3) * max_rules)
    assert int(p["spill_words"]) == _align(words, 64) and int(p["spill_words"]) % 64 == 0
