"""The constructed cases of tests/l2_join_cases.py, checked on the CPU: the oracle's result multisets equal the plain model
of tests/result_set_model.py on every case (so the expected values of tests/test_l2_join_edges_gpu.py come from the
reference, not from the kernel), the product compiles the same table and takes the rule set in result-set mode, and every
number a case claims is recomputed from the model or read from the oracle's output and held to the kernel's constants: the
64 lanes of a chunk, the limit 0x7FFF of the packed count, the table size of the sizing rule, the filter bit."""
import functools
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import oracle
import struspattern_amd as spa

from . import l2_join_cases as cases
from .l2_join_cases import COUNT_MAX, JOIN_SELF, LANES
from .result_set_model import SELF, document_results, join_rules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI355X_CUS = 256


@functools.lru_cache(maxsize=None)
def _case(name):
    build, lex4, offs, seg, claims = cases.CASES[name]()
    o, m = oracle.L2Matcher(), spa.PatternMatcherInstance()
    build(o)
    build(m)
    ref = cases.Reference(o, lex4, offs, seg)
    rules, delimiter = join_rules(o.dumpTable())
    l5 = cases.lexems5(lex4, seg)
    docs = [[tuple(x) for x in l5[int(offs[d]):int(offs[d + 1])].tolist()] for d in range(len(offs) - 1)]
    return {"o": o, "m": m, "ref": ref, "rules": rules, "delimiter": delimiter, "docs": docs, "claims": claims, "lex4": lex4, "offs": offs, "seg": seg}


@functools.lru_cache(maxsize=None)
def _pairs(name):
    c = _case(name)
    return [cases.model_pairs(c["rules"], c["delimiter"], doc) if not c["ref"].status[d] else [] for d, doc in enumerate(c["docs"])]


def test_join_hash_of_the_case_module_is_the_header_s(tmp_path):
    """the Python restatement against joinHash of csrc/l2_join.h itself, compiled for the host"""
    pairs = [(1, 2), (11, 12), (JOIN_SELF, 40), (0x1FFFFFFF, 1 << 24), (123456, 0)]
    src = tmp_path / "h.cpp"
    src.write_text('#include <cstdio>\n#include "l2_join.h"\nint main(){ %s return 0; }\n' % " ".join(
        'std::printf("%%u\\n", spa::joinHash( %du, %du));' % p for p in pairs))
    exe = str(tmp_path / "h")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "struspattern_amd", "csrc"), str(src), "-o", exe])
    out = [int(x) for x in subprocess.check_output([exe]).split()]
    assert out == [cases.join_hash(*p) for p in pairs]
    assert [int(x) for x in cases.join_hash(np.array([p[0] for p in pairs[:2]], np.uint64), 2)] == [cases.join_hash(1, 2), cases.join_hash(11, 2)]
    assert cases.table_size(8) == 32 and cases.table_size(15) == 32 and cases.table_size(16) == 64 and cases.table_size(1) == 4


@pytest.mark.parametrize("name", list(cases.CASES))
def test_oracle_equals_the_model_and_the_product_compiles_the_same_table(name):
    c = _case(name)
    assert np.array_equal(c["m"].dumpTable(), c["o"].dumpTable())
    ok, why, alt = c["m"].resultSetTier()
    assert ok, why
    assert (alt > 0) == (name == "moved_keys")
    total = 0
    for d, doc in enumerate(c["docs"]):
        if c["ref"].status[d]:
            continue
        got = document_results(c["rules"], c["delimiter"], doc)
        want = c["ref"].multisets[d]
        assert got == want, (name, d, list((got - want).items())[:2], list((want - got).items())[:2])
        assert sum(m for _, _, _, m in _pairs(name)[d]) == sum(want.values())
        total += sum(want.values())
    assert total > 0


# ---------------------------------------------------------------- what the cases claim, measured
def _crossing(name):
    return [(d, i, x) for d, ps in enumerate(_pairs(name)) for i, x, _, _ in ps if i // LANES != x // LANES]


def _geometry(name):
    c = _case(name)
    sizes = [len(doc) for doc in c["docs"]]
    per_chunk = []
    for d, ps in enumerate(_pairs(name)):
        if sizes[d] == 200:
            n = [0] * 4
            for _, x, _, m in ps:
                n[x // LANES] += m
            per_chunk.append(n)
    return {"lexems_per_document": sizes, "matches_crossing_a_chunk_end": sorted(set(_crossing(name))), "matches_per_chunk_of_the_long_documents": per_chunk}


def _edges_geometry(m):
    n = m["lexems_per_document"]
    assert {0, 1, LANES - 1, LANES, LANES + 1, 2 * LANES - 1, 2 * LANES, 2 * LANES + 1, 200} <= set(n)
    assert n[0] == 0 and n[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(n, n[1:]))          # empty: first, last, neighbours
    cross = m["matches_crossing_a_chunk_end"]
    assert {(i, x) for _, i, x in cross} >= {(LANES - 1, LANES), (2 * LANES - 1, 2 * LANES), (3 * LANES - 1, 3 * LANES)}
    every, hole = m["matches_per_chunk_of_the_long_documents"]
    assert all(every) and hole[0] and not hole[1] and hole[2]


def _edges_single(m):
    assert len(m["lexems_per_document"]) == 1 and m["matches_crossing_a_chunk_end"] == [(0, LANES - 1, LANES)]


def _waves(name):
    c = _case(name)
    n = c["ref"].nresults
    plan = c["m"].launchPlan(MI355X_CUS, len(c["docs"]), len(c["lex4"]), result_sets=True)
    return {"documents": len(c["docs"]), "waves": int(plan["join_blocks"]), "matches_per_document": [min(n), max(n)]}


def _edges_waves(m):
    launched = 4 * ((m["waves"] + 3) // 4)          # launchL2Join: blocks of 4 waves
    assert m["documents"] > 2 * launched and m["matches_per_document"] == [1, 1]


def _count_limit(name):
    """read from the oracle's output: the results of the peak document by their end position"""
    c = _case(name)
    at_end, items_at_end = Counter(), Counter()
    for k, v in c["ref"].multisets[1].items():
        at_end[k[2]] += v
        items_at_end[k[2]] += v * k[7]
    per_lexem = Counter()
    for _, x, _, mult in _pairs(name)[1]:
        per_lexem[x] += mult
    assert max(per_lexem.values()) == max(at_end.values())
    return {"peak_matches_at_one_lexem": max(at_end.values()), "peak_items_at_one_lexem": max(items_at_end.values()), "lexems_of_the_peak_document": len(c["docs"][1])}


def _edges_limit_fits(m):
    assert m["peak_matches_at_one_lexem"] == COUNT_MAX and m["peak_items_at_one_lexem"] == 2 * COUNT_MAX <= 0xFFFF


def _edges_limit_one_more(m):
    assert m["peak_matches_at_one_lexem"] == COUNT_MAX + 1


def _edges_limit_wrapped(m):
    n = m["peak_matches_at_one_lexem"]
    assert n == 66000 and n > 0xFFFF and (n & 0xFFFF) <= COUNT_MAX        # the low half alone looks like a count that fits
    assert m["lexems_of_the_peak_document"] < 400


def _count_array(name):
    c = _case(name)
    buf, ranges, hints = cases.scattered(c["lex4"], c["offs"])
    ends = ranges[:, 0] + ranges[:, 1]
    for d in range(len(ranges)):            # the ranges hold the documents
        assert np.array_equal(buf[int(ranges[d, 0]):int(ends[d])], c["lex4"][int(c["offs"][d]):int(c["offs"][d + 1])])
    firsts = [int(x) for x in ranges[:, 0]]
    return {"ranges_ascending": firsts == sorted(firsts), "unused_lexems": len(buf) - len(c["lex4"]), "stored_documents_per_hint": [int((ends <= h).sum()) for h in hints],
            "hints": hints, "end": int(ends.max()), "ndocs": len(ranges), "buffer": len(buf)}


def _edges_count_array(m):
    none, some, every = m["stored_documents_per_hint"]
    assert none == 0 and 0 < some < m["ndocs"] and every == m["ndocs"]
    assert m["hints"][0] == 0 and m["hints"][2] == m["end"] < m["buffer"] and not m["ranges_ascending"]


def _capacity(name):
    c = _case(name)
    m = {"results": sum(c["ref"].nresults), "items": sum(c["ref"].nitems)}
    plan = c["m"].launchPlan(MI355X_CUS, len(c["docs"]), len(c["lex4"]), result_sets=True)
    grown = c["m"].launchPlan(MI355X_CUS, len(c["docs"]), len(c["lex4"]), result_sets=True, min_results=m["results"])
    m.update(want=(int(plan["want_results"]), int(plan["want_items"])), grown=(int(grown["want_results"]), int(grown["want_items"])), per_doc=c["ref"].nresults)
    return m


def _edges_capacity(m):
    assert m["results"] > m["want"][0] and m["items"] > m["want"][1]                # a fresh context: too small
    assert m["grown"][0] == m["results"] and m["grown"][1] < m["items"]             # results reserved: the items still do not fit
    assert min(m["per_doc"]) < m["want"][0] and max(m["per_doc"]) < m["want"][0]    # any single document fits: some succeed


def _checks(name):
    return {"status_per_document": [int(x) for x in _case(name)["ref"].status]}


def _edges_checks(m):
    st = m["status_per_document"]
    assert st.count(cases.SP_DOC_ERR_RANGE) >= 5 and st.count(cases.SP_DOC_ERR_ORDER) >= 4
    assert st[0] == 0 and st[-1] == 0 and any(a and not b for a, b in zip(st, st[1:])) and any(b and not a for a, b in zip(st, st[1:]))


def _table(name):
    c = _case(name)
    keys = cases.join_keys(c["rules"])
    slots = cases.build_table(keys)
    mask = len(slots) - 1
    home = Counter(cases.join_hash(*k) & mask for k in keys)
    wraps = any(slots[0] is not None and (cases.join_hash(*slots[0]) & mask) == mask for _ in [0])
    selfs = []
    for k in keys:
        if k[0] == JOIN_SELF:
            seen = cases.probe(slots, k)
            selfs.append(len(seen) > 1 and all(slots[s][0] != JOIN_SELF for s in seen[:-1]))
    bits = set(cases.filter_bit(*k) for k in keys)
    maxrange = max(r.range for r in c["rules"] if r.kind != SELF)
    strangers = {}
    for doc in c["docs"]:
        for x, lx in enumerate(doc):
            for i in range(x):
                li = doc[i]
                pair = (li[0], lx[0])
                if li[1] < lx[1] <= li[1] + maxrange and pair not in keys and cases.filter_bit(*pair) in bits:
                    seen = cases.probe(slots, pair)
                    assert slots[seen[-1]] is None
                    strangers[pair] = len(seen) - 1
    per_key = Counter((JOIN_SELF if r.kind == SELF else r.first, r.second) for r in c["rules"])
    multi = [r for r in c["rules"] if (r.first, r.second) == max(per_key, key=per_key.get)]
    return {"table_size": len(slots), "keys_with_one_home_slot": max(home.values()), "chain_wraps_to_slot_0": wraps,
            "self_key_behind_pair_keys_of_its_chain": any(selfs), "strangers_that_pass_the_filter": len(strangers),
            "foreign_keys_a_stranger_passes": sorted(strangers.values()), "rules_of_one_key": max(per_key.values()),
            "multi": sorted((r.range, r.struct, bool(r.vfirst), bool(r.vsecond)) for r in multi), "nkeys": len(keys)}


def _edges_table(m):
    assert m["table_size"] == cases.table_size(m["nkeys"]) and m["keys_with_one_home_slot"] >= 2
    assert m["chain_wraps_to_slot_0"] and m["self_key_behind_pair_keys_of_its_chain"]
    assert m["foreign_keys_a_stranger_passes"][0] == 0 and m["foreign_keys_a_stranger_passes"][-1] >= 2
    assert len(set(r for r, _, _, _ in m["multi"])) >= 4 and {s for _, s, _, _ in m["multi"]} == {True, False}
    assert {(f, s) for _, _, f, s in m["multi"]} == {(False, False), (True, False), (False, True), (True, True)}


def _per_document(name):
    return {"results_per_document": list(_case(name)["ref"].nresults)}


def _edges_predicate(m):
    assert m["results_per_document"][-1] == 0 and all(m["results_per_document"][:-1])


def _edges_no_struct(m):
    assert _case("delimiter_without_struct")["delimiter"] == 0
    assert any(lx[0] == cases.DEL for doc in _case("delimiter_without_struct")["docs"] for lx in doc)


def _moved(name):
    c = _case(name)
    covered, mult, crossing = {}, Counter(), 0
    for d, (doc, ps) in enumerate(zip(c["docs"], _pairs(name))):
        for i, x, r, m in ps:
            if r.kind in cases.ALT_GOALS:
                mult[m] += 1
                if m > 1 and i < LANES <= x:
                    crossing = max(crossing, m)
        for r in c["rules"]:
            if r.kind in cases.ALT_GOALS:
                for i in range(len(doc)):
                    for x in range(i + 1, len(doc)):
                        if doc[i][0] == r.first and doc[x][0] == r.second:
                            covered.setdefault(r.kind, set()).update(cases.alt_brackets(r, doc, i, x, c["delimiter"]) or ())
    claimed = c["claims"]["covered"]
    return {"covered": {k: sorted(g for g in covered[k] if g in claimed[k]) for k in covered}, "all_covered": covered,
            "multiplicities_of_moved_pairs": dict(mult), "multiplicity_across_lexem_64": crossing}


def _edges_moved(m):
    for kind, goals in cases.ALT_GOALS.items():
        assert set(goals) <= m["all_covered"][kind], (kind, goals, m["all_covered"][kind])
    assert max(m["multiplicities_of_moved_pairs"]) > 1 and m["multiplicities_of_moved_pairs"].get(1, 0) > 0
    assert m["multiplicity_across_lexem_64"] > 1
    assert _case("moved_keys")["m"].resultSetTier()[2] > 0


def _segments(name):
    ms = sum(_case(name)["ref"].multisets, Counter())
    return {"results_spanning_segments": sum(v for k, v in ms.items() if k[3] != k[5]), "results": sum(ms.values())}


def _edges_segments(m):
    assert 0 < m["results_spanning_segments"] < m["results"]


def _formats(name):
    c = _case(name)
    whole = c["o"].run(cases.lexems5(c["lex4"], c["seg"]), c["offs"])
    return {"formats": c["m"].formatCount(), "results_with_a_format": int((whole.result_format != 0).sum()), "results_without": int((whole.result_format == 0).sum())}


def _edges_formats(m):
    assert m["formats"] > 1 and m["results_with_a_format"] > 0 and m["results_without"] > 0


def _bare(name):
    c = _case(name)
    return {"items": sum(c["ref"].nitems), "results": sum(c["ref"].nresults)}


def _edges_bare(m):
    assert m["items"] == 0 and m["results"] > 0


EDGES = {
    "chunk_geometry": (_geometry, _edges_geometry),
    "single_document": (_geometry, _edges_single),
    "more_docs_than_waves": (_waves, _edges_waves),
    "count_limit_32767": (_count_limit, _edges_limit_fits),
    "count_limit_32768": (_count_limit, _edges_limit_one_more),
    "count_limit_66000": (_count_limit, _edges_limit_wrapped),
    "count_array": (_count_array, _edges_count_array),
    "output_capacity": (_capacity, _edges_capacity),
    "input_checks": (_checks, _edges_checks),
    "table_collisions": (_table, _edges_table),
    "predicate_edges": (_per_document, _edges_predicate),
    "delimiter_without_struct": (_per_document, _edges_no_struct),
    "moved_keys": (_moved, _edges_moved),
    "segments": (_segments, _edges_segments),
    "formats": (_formats, _edges_formats),
    "no_variables": (_bare, _edges_bare),
}


def test_the_table_of_cases_is_complete():
    assert set(EDGES) == set(cases.CASES) and set(cases.FAILING) <= set(cases.CASES)
    assert cases.DEFAULT_WAVES == MI355X_CUS * 32


@pytest.mark.parametrize("name", list(cases.CASES))
def test_claims_sit_on_their_edges(name):
    measure, edges = EDGES[name]
    m = measure(name)
    claims = _case(name)["claims"]
    print(name, {k: m[k] for k in claims})
    for k, v in claims.items():
        assert m[k] == v, (name, k, m[k], v)
    edges(m)


def test_documents_stay_small():
    for name in cases.CASES:
        if name != "more_docs_than_waves":
            assert max(len(doc) for doc in _case(name)["docs"]) <= 400 and len(_case(name)["docs"]) <= 20, name
