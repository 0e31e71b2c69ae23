"""CPU tests of the model of the cluster-per-lane handler route of the lexer's post-processing kernel
(tests/l1_post_model.py) on the product's compiled tables, and guards of the inputs of tests/test_l1_post_gpu.py: what every
GPU batch is meant to contain is asserted here, from the model's trace, so that a later change to the inputs cannot turn a
GPU test into a no-op.  The events the model leaves -- by its cluster route and by the reference's handler alone -- are
the oracle's lexems, document by document: what a cluster leaves is appended as it is.  No GPU."""
import functools

import pytest

import oracle
from tests import l1_post_cases as cases
from tests import l1_post_model as model
from tests import l1_words_model as words

WHOLE = words.DEFAULT_CHUNK
SWEEPS = sorted(cases.STRUCTURES)
SPLIT_DEF = [i for i, d in enumerate(cases.TABLES["merge"]) if d[0].count("|") > 3][0]     # the wide alternation


@functools.lru_cache(maxsize=None)
def _records(name, doc, chunk=WHOLE):
    return tuple(model.records(cases.tables(name), doc, chunk, cases.symbols(name)))


@functools.lru_cache(maxsize=None)
def _trace(name, doc):
    return model.trace(list(_records(name, doc)))


def _steps(name, structure=None):
    """(what, step, records of the document) of every step of the sweep documents of a table (of one structure)"""
    docs, what = cases.sweep_docs(name)
    for d, w in zip(docs, what):
        if structure is None or w[0] == structure:
            for s in _trace(name, d)["steps"]:
                yield w, s, _records(name, d)


_ORACLE = {}


def _oracle_spans(name, docs):
    """per document the (id, origpos, origsize) of the oracle's lexems"""
    if name not in _ORACLE:
        _ORACLE[name] = oracle.L1Lexer()
        cases.build(_ORACLE[name], name)
    lex, offs = _ORACLE[name].matchDocs(b"".join(docs), cases.offsets(docs), nthreads=8)
    return [[(int(r[0]), int(r[2]), int(r[3])) for r in lex[int(offs[i]):int(offs[i + 1])]] for i in range(len(docs))]


def _batches():
    """(table, documents) of every GPU batch under 48 KB"""
    out = [(name, docs) for name in SWEEPS for docs, what in cases.sweep_batches(name)]
    out.append(("survivors", tuple(cases.ending_docs()[0])))
    out.append(("merge", tuple(cases.queue_docs()[0])))
    out.append(("chain", tuple(cases.long_docs()[0])))
    return out


# ---------------------------------------------------------------- the tables
def test_tables_are_what_the_gpu_tests_take_them_for():
    for name in cases.TABLES:
        t = cases.tables(name)
        assert t.scan_passes == 1 and not t.cpBlocks and not t.nullable and not t.ucp
        assert any((p["word"] >> 6) < t.scan_passes for p in t.patterns)                   # a scanned expression: queue A exists
        assert t.literals or t.shapes                                                       # the words kernel: queue B exists
        assert all((p["levelBind"] >> 8) & 0xFF == 0 for p in t.patterns)                  # content: every event is a lexem
    assert len(cases.TABLES["capacity"]) <= 3
    # the wide alternation is cut into two patterns entries; the split word ends an alternative of either
    t = cases.tables("merge")
    assert len(t.patterns) == len(cases.TABLES["merge"]) + 1
    reps = words.automaton_reports(t, cases.SPLIT_WORD, True)
    group = [pi for pi, frm, to in reps if t.patterns[pi]["defIndex"] == SPLIT_DEF]
    assert len(group) == 2 and group[0] != group[1]
    # a symbol lookup and a sub expression selection
    t = cases.tables("bounds")
    assert sum(1 for p in t.patterns if p["levelBind"] & 1 << 16) == 1 and sum(1 for p in t.patterns if p["levelBind"] & 1 << 17) == 1


def test_views_follow_the_refill_loop():
    recs = list(range(130))
    assert [len(v) for v in model.views(recs)] == [64, 64, 2]
    assert [model.view_at(recs, wi)[1] for wi in (0, 63, 66, 67, 129)] == [False, False, False, True, True]
    assert model.view_at(recs[:64], 0) == (recs[:64], False)            # a document of exactly 64 records: not seen as ended
    assert model.view_at(recs[:63], 0) == (recs[:63], True)


def test_bounds_are_strict():
    R = lambda frm, to: model.Record(to, frm, 1, 1, 0)
    assert model.bounds([R(0, 1), R(2, 3), R(4, 5)]) == [0, 1, 2]
    assert model.bounds([R(0, 1), R(0, 3), R(4, 5)]) == [0, 2]              # same start
    assert model.bounds([R(0, 3), R(2, 3), R(4, 5)]) == [0, 2]              # same end
    # the carries are 1 + the greatest start / end so far: a start or an end equal to it is no boundary, one above is
    assert model.bounds([R(2, 3)], 3, 4) == [] and model.bounds([R(2, 3)], 3, 3) == [] and model.bounds([R(2, 3)], 2, 4) == []
    assert model.bounds([R(2, 3)], 2, 3) == [0]
    assert model.bounds([R(0, 9), R(1, 2), R(3, 4), R(10, 11)]) == [0, 3]
    assert model.carry_to([R(5, 9), R(1, 2)], 2, 0, 0) == (6, 10) and model.carry_to([R(5, 9)], 0, 3, 4) == (3, 4)


def test_lane_handler_order_of_the_checks():
    def R(frm, to, id_, level, fl=0):
        return model.Record(to, frm, id_, level | fl, 0)
    six = [R(0, 5, i, 2) for i in range(1, 7)]
    assert len(model.lane_handler(six)) == 6
    assert model.lane_handler(six + [R(0, 5, 7, 2)]) is model.HARD
    assert len(model.lane_handler(six + [R(0, 5, 7, 1)])) == 6                             # ignored: never hard
    assert model.spans(model.lane_handler(six + [R(0, 5, 7, 3)])) == [(7, 0, 5)]           # deletes all six
    assert model.lane_handler([R(0, 5, 1, 1, model.REC_SYMBOL)]) is model.HARD
    assert model.lane_handler([R(0, 5, 1, 1, model.REC_SIZEERR)]) is model.HARD
    # the twin of a symbol with the reference's element moves: one event moved is kept, of two the lower is lost
    ev = [model.Event(1, 0, 1, 1), model.Event(2, 4, 1, 1)]
    model.sequential(ev, model.Record(3, 2, 5, 1 | model.REC_SYMBOL, 900))
    assert model.spans(ev) == [(1, 0, 1), (5, 2, 1), (900, 2, 1), (2, 4, 1)]


# ---------------------------------------------------------------- the model against the oracle
@pytest.mark.parametrize("name", SWEEPS)
def test_cluster_route_and_sequential_route_leave_the_oracles_lexems(name):
    more = {"survivors": [cases.ending_docs()], "merge": [cases.queue_docs()], "chain": [cases.long_docs()]}
    for docs, what in cases.sweep_batches(name) + more.get(name, []):
        want = _oracle_spans(name, list(docs))
        for d, w, ref in zip(docs, what, want):
            tr = _trace(name, d)
            assert tr["err"] == 0 and tr["seq"]["err"] == 0
            assert model.spans(tr["events"]) == ref, (name, w)
            assert model.spans(tr["seq"]["events"]) == ref, (name, w)


def test_batches_are_small_and_mostly_not_isolated_words():
    for name, docs in _batches():
        assert sum(len(d) for d in docs) < 48 * 1024, name
        assert not words.fingerprint_collisions(cases.tables(name), docs), name
        lone = sum(1 for d in docs if model.isolated(_trace(name, d)))
        assert 4 * lone <= len(docs), (name, lone, len(docs))
    # the isolated word is one: one report, one event, one boundary -- and the preamble and the tail are of such only
    for name in SWEEPS:
        tr = _trace(name, cases.iso(10))
        assert model.isolated(tr) and len(tr["events"]) == 10 and tr["steps"][0]["lens"] == [1] * 10


# ---------------------------------------------------------------- each structure is what it is meant to be
def _cluster_lengths(name, doc):
    recs = list(_records(name, doc))
    b = model.bounds(recs)
    return [y - x for x, y in zip(b, b[1:] + [len(recs)])]


def test_survivors_five_to_eight():
    for s, n in (("five", 5), ("six", 6), ("seven", 7), ("eight", 8)):
        text = cases.STRUCTURES["survivors"][s]
        recs = list(_records("survivors", text))
        assert len(recs) == n and len(set(r.id for r in recs)) == n and len(set((r.frm, r.to, r.fl) for r in recs)) == 1
        assert len(model.sequential_run(recs)["events"]) == n
        assert (model.lane_handler(recs) is model.HARD) == (n > model.LOC_CAP)
    lv = cases.STRUCTURES["levels"]
    recs = list(_records("levels", lv["six_deleted"]))
    assert len(model.lane_handler(recs[:6])) == 6 and len(model.lane_handler(recs)) == 1 and recs[6].fl & 0xFF > recs[0].fl & 0xFF
    recs = list(_records("levels", lv["six_and_a_seventh"]))
    assert len(recs) == 7 and len(model.lane_handler(recs[:6])) == 6 and model.lane_handler(recs) is model.HARD
    recs = list(_records("levels", lv["six_and_ignored"]))
    assert len(recs) == 9 and len(model.lane_handler(recs[:6])) == 6 and model.lane_handler(recs) == model.lane_handler(recs[:6])


def test_cluster_lengths():
    for n in (62, 63, 64, 65, 127, 128, 129, 201):
        text = cases.STRUCTURES["chain"]["cluster_%d" % n]
        assert _cluster_lengths("chain", text) == [n]
        assert _cluster_lengths("chain", cases.iso(3) + text + b" " + cases.iso(2)) == [1, 1, 1, n, 1, 1]
    # a cluster of 63 at lane 0 is the longest a lane takes; 64 is as long as the view (procEnd == 0); 201 spans whole views
    at0 = [s for w, s, recs in _steps("chain", "cluster_63") if s["kind"] == "lanes" and s["heads"][:1] == [0] and s["lens"][0] == 63]
    assert at0 and all(s["first_hard"] == 0 and s["consumed"] == 63 for s in at0)
    assert any(s["reason"] == model.VIEW_LONG_CLUSTER and s["avail"] == 64 for w, s, recs in _steps("chain", "cluster_64"))
    assert any(s["first"] == 64 and s["consumed"] == 64 for w, s, recs in _steps("chain", "cluster_201"))
    assert max(s["lens"][s["heads"].index(s["first_hard"])] for w, s, recs in _steps("chain") if s["kind"] == "lanes" and s["first_hard"] < 64) == 63


def test_the_sweep_reaches_every_lane_and_every_hand_back_reason():
    """No lane above 62 can head a cluster a lane takes: a view that is not final stops at its last boundary (at most
    63), a final view holds fewer than 64 records.  So the heads are the lanes 0..62 and the first hard cluster stands
    at 0 and at 62 at the outermost."""
    heads, first_hard, first, reasons = set(), set(), set(), {}
    for name in SWEEPS:
        for w, s, recs in _steps(name):
            first.add(s["first"])
            if s["reason"]:
                reasons.setdefault(s["reason"], set()).add((name, w[0]))
            if s["kind"] == "lanes":
                assert max(s["heads"]) <= 62
                heads.update(i for i, r in zip(s["heads"], s["results"]) if i < s["first_hard"] and len(r) > 0)
                first_hard.add(s["first_hard"])
    assert heads == set(range(63))
    assert {0, 62, 64} <= first_hard and 63 not in first_hard
    assert {1, 2, 63, 64} <= first and len(first) >= 60
    assert set(reasons) == set(model.REASONS) - {model.SIZE_ERROR}                         # (the size error: test_lexem_size_documents)
    # which case reaches which reason
    assert ("chain", "cluster_64") in reasons[model.VIEW_LONG_CLUSTER]
    assert ("survivors", "seven") in reasons[model.MORE_THAN_LOC_CAP] and ("levels", "six_and_a_seventh") in reasons[model.MORE_THAN_LOC_CAP]
    assert {("bounds", "symbol"), ("bounds", "symbol_in_cluster")} <= reasons[model.SYMBOL_LOOKUP]
    assert {("bounds", "reaches_back"), ("bounds", "same_start"), ("chain", "cluster_65")} <= reasons[model.BEFORE_FIRST_BOUNDARY]
    assert not any(n == "levels" and s in ("six_deleted", "six_and_ignored") for r in reasons.values() for n, s in r)
    assert not any(n == "survivors" and s in ("five", "six") for r in reasons.values() for n, s in r)


def test_hard_clusters_at_every_place():
    def hard(s):
        return [i for i, r in zip(s["heads"], s["results"]) if r is model.HARD]
    lanes = [(w, s, recs) for w, s, recs in _steps("survivors") if s["kind"] == "lanes"]
    assert any(s["first_hard"] == 0 and not s["appended"] for w, s, recs in lanes)                              # at lane 0: nothing appended
    assert any(0 < s["heads"].index(s["first_hard"]) < len(s["heads"]) - 1 for w, s, recs in lanes if s["first_hard"] < 64)
    assert any(s["first_hard"] == s["heads"][-1] and not s["final"] for w, s, recs in lanes)                    # the last complete cluster
    by = dict(zip(cases.ending_docs()[1], cases.ending_docs()[0]))
    for n in (63, 64, 65, 127, 128, 129):
        s = _trace("survivors", by[("hard_last", n)])["steps"][-1]
        assert s["final"] and s["first_hard"] == s["heads"][-1] and s["consumed"] == s["avail"]
        s = _trace("survivors", by[("hard_first", n)])["steps"][0]
        assert s["first_hard"] == 0 and s["consumed"] == 7
    # two in one view: the second is seen again by the next view, which begins behind the first
    again = 0
    for d, w in zip(*cases.sweep_docs("survivors")):
        st = _trace("survivors", d)["steps"]
        for a, b in zip(st, st[1:]):
            if a["kind"] == "lanes" and len(hard(a)) >= 2:
                assert b["wi"] == a["wi"] + a["consumed"] <= a["wi"] + hard(a)[1] and b["kind"] == "lanes" and hard(b)
                again += 1
    assert again >= 20
    # a symbol lookup inside a cluster whose other records a lane takes
    recs = list(_records("bounds", cases.STRUCTURES["bounds"]["symbol_in_cluster"]))
    assert len(recs) == 3 and model.lane_handler(recs) is model.HARD and model.hard_reason(recs) == model.SYMBOL_LOOKUP
    assert model.lane_handler([r._replace(fl=r.fl & 0xFFFF) for r in recs]) is not model.HARD
    assert any(r.sym == 900 for r in recs)
    assert any(e.id == 900 for e in _trace("bounds", cases.sweep(cases.STRUCTURES["bounds"]["symbol"])[7])["events"])


def test_boundary_comparisons_at_the_carry():
    b = cases.STRUCTURES["bounds"]
    recs = list(_records("bounds", b["same_start"]))
    assert any(x.frm == y.frm and x.to != y.to for x in recs for y in recs)
    recs = list(_records("bounds", b["same_end"]))
    assert any(x.to == y.to and x.frm != y.frm for x in recs for y in recs)
    recs = list(_records("bounds", b["same_end_same_start"]))
    assert len(recs) == 2 and recs[0][:2] == recs[1][:2]
    for s in ("same_start", "same_end", "same_end_same_start"):
        assert max(_cluster_lengths("bounds", b[s])) == len(_records("bounds", b[s]))
    # the selection moves the end of its record left of the end of the record before it
    recs = list(_records("bounds", b["selection_moves_end"]))
    assert [(r.frm, r.to) for r in recs] == [(0, 4), (1, 3)]
    # at a view's first record: a start equal to the greatest start handled (no boundary), one above it (a boundary);
    # the same for the ends
    eqF = aboveF = eqT = aboveT = 0
    for w, s, recs in list(_steps("bounds")) + list(_steps("chain")):
        r0 = recs[s["wi"]]
        cF, cT = s["carry_in"]
        if cF and r0.frm + 1 == cF:
            assert s["first"] > 0
            eqF += 1
        if cF and r0.frm + 1 == cF + 1 and r0.to + 1 > cT:
            aboveF += s["first"] == 0
        if cT and r0.to + 1 == cT:
            assert s["first"] > 0
            eqT += 1
        if cT and r0.to + 1 == cT + 1 and r0.frm + 1 > cF:
            aboveT += s["first"] == 0
    assert eqF and aboveF and eqT and aboveT, (eqF, aboveF, eqT, aboveT)
    # a match of \\bW\\s\\w+\\b that reaches behind the carry comes as record 0, 1 and 63 of a view.  As record 0 only behind a
    # view that was consumed whole (a view begins at a boundary otherwise); as record 63 behind 63 reports of [w] inside the
    # word it ends with, in a view without any boundary: the suffix minimum of the last lane pulls every lane below the carry
    at = {}
    for name, structure, pid in (("bounds", "reaches_back", 8), ("bounds", "reaches_back_far", 8), ("chain", "cluster_129", 3), ("chain", "cluster_201", 3)):
        for w, s, recs in _steps(name, structure):
            for i in range(s["avail"]):
                if recs[s["wi"] + i].id == pid and recs[s["wi"] + i].frm + 1 <= s["carry_in"][0]:
                    at.setdefault(i, set()).add(structure)
                    assert s["first"] > i and s["kind"] == "sequential"
                    assert i < 63 or (s["first"] == 64 and not s["bounds"] and s["consumed"] == 64)
    assert {0, 1, 63} <= set(at) and "reaches_back_far" in at[63], sorted(at)
    # where its own word's report lies in the same view, the match at record 63 makes its cluster wait for the next view
    waits = 0
    for w, s, recs in _steps("chain", "cluster_201"):
        if s["avail"] == 64 and recs[s["wi"] + 63].id == 3 and s["kind"] == "lanes":
            assert s["proc_end"] <= 61 and s["consumed"] <= 61
            waits += 1
    assert waits >= 3


def test_final_views_and_waiting_clusters():
    docs, what = cases.ending_docs()
    by = dict(zip(what, docs))
    for n in (63, 64, 65, 127, 128, 129):
        for kind in ("isolated", "cluster_first", "cluster_last", "hard_first", "hard_last"):
            assert len(_records("survivors", by[(kind, n)])) == n
    st = _trace("survivors", by[("isolated", 64)])["steps"]
    assert [(s["avail"], s["final"], s["consumed"]) for s in st] == [(64, False, 63), (1, True, 1)]        # the 64th waits
    st = _trace("survivors", by[("isolated", 63)])["steps"]
    assert [(s["avail"], s["final"], s["consumed"]) for s in st] == [(63, True, 63)]
    st = _trace("survivors", by[("isolated", 128)])["steps"]
    assert [(s["avail"], s["final"], s["consumed"]) for s in st] == [(64, False, 63), (64, False, 63), (2, True, 2)]
    st = _trace("survivors", by[("cluster_last", 64)])["steps"]
    assert [(s["avail"], s["final"], s["consumed"]) for s in st] == [(64, False, 59), (5, True, 5)]        # the last cluster waits
    assert not _records("survivors", by[("empty", 0)])


def test_both_queues_and_both_merge_branches():
    docs, what = cases.queue_docs()
    t = cases.tables("merge")
    by = dict(zip(what, docs))
    q = dict((w, model.queue_records(t, by[w], WHOLE)) for w in what)
    assert q["words_only"][1] and not q["words_only"][0] and q["automaton_only"][0] and not q["automaton_only"][1]
    # (the refill model covers a document of one scan unit whose queues hold live entries only)
    passes = {}
    for w in what:
        if isinstance(w, str):
            assert words.units(len(by[w]), WHOLE) == 1 and cases.SPLIT_WORD not in by[w]
            assert not any(dead for recs in words.records(t, by[w], WHOLE) for to, pi, frm, dead in recs)
            assert len(words.automaton_reports(t, by[w], True)) == len(q[w][0])             # no report of a group is skipped
            passes[w] = model.refills(q[w][0], q[w][1], [s["consumed"] for s in _trace("merge", by[w])["steps"]])
            assert sum(a + b for a, b, lim in passes[w]) == len(_records("merge", by[w]))
    assert any(a > b > 0 for a, b, lim in passes["more_a"]) and any(b > a > 0 for a, b, lim in passes["more_b"])
    for w in ("words_first", "automaton_first"):
        assert any(lim for a, b, lim in passes[w]) and any((a == 0) != (b == 0) for a, b, lim in passes[w])
    # ties of the two queues at one end offset, the automaton's expression defined before and after the shape's
    a, b = model.queue_records(t, cases.STRUCTURES["merge"]["tie"], WHOLE)
    ends = set(x[0] for x in b)
    tied = sorted(x[1] for x in a if x[0] in ends)
    assert tied and min(tied) < b[0][1] < max(tied)
    # the group of the wide alternation lies across the entries 63 | 64 of its queue
    at = []
    for j in cases.SPLIT_AT:
        raw = words.automaton_reports(t, by[("split_group_at", j)], True)
        at.append([i for i, (pi, frm, to) in enumerate(raw) if t.patterns[pi]["defIndex"] == SPLIT_DEF])
    assert [63, 64] in at and [62, 63] in at and [64, 65] in at


@pytest.mark.parametrize("chunk", cases.CHUNKS)
def test_chunks_cut_clusters_and_leave_empty_slices(chunk):
    straddle = one_empty = last_empty = 0
    for name, docs in (("chain", cases.sweep_batches("chain")[0][0][::7]), ("merge", tuple(cases.queue_docs()[0])), ("chain", tuple(cases.long_docs()[0]))):
        t = cases.tables(name)
        for d in docs:
            assert _records(name, d, chunk) == _records(name, d)                # the stream does not depend on the cut
            recs = _records(name, d)
            b = model.bounds(list(recs))
            for x, y in zip(b, b[1:] + [len(recs)]):
                straddle += any(recs[i].to // chunk != recs[x].to // chunk for i in range(x, y))
            word = [len([1 for r in u if not r[3]]) for u in words.records(t, d, chunk)]
            auto = [0] * len(word)
            for pi, frm, to in words.automaton_reports(t, d, True):
                auto[words.owner(to, len(d), chunk)] += 1
            # an empty slice in one queue while the other has several slices left
            one_empty += any(word[i] == 0 and sum(1 for x in auto[i:] if x) >= 2 for i in range(len(word)))
            one_empty += any(auto[i] == 0 and sum(1 for x in word[i:] if x) >= 2 for i in range(len(word)))
            last_empty += len(word) > 1 and (word[-1] == 0 or auto[-1] == 0)
    assert straddle >= 2 and one_empty >= 2 and last_empty >= 2, (straddle, one_empty, last_empty)


# ---------------------------------------------------------------- capacity and lexem size
def test_capacity_documents_fail_where_the_two_conditions_say():
    """E isolated events.  The cluster route appends the last r < 64 of them at once and asks for nEvents + total + 2 <= cap
    with nEvents + total = E: it fails from E = cap - 1 on.  The sequential route asks for nEvents + 2 <= cap in front of
    every report, nEvents = E - 1 at the last: it fails from E = cap on.  They differ at E = cap - 1."""
    docs = cases.capacity_docs()
    assert len(docs) == 8 and sum(len(d) for d in docs) < 4 * 66000
    got = {}
    for e, d in zip(cases.CAPACITY_EVENTS, docs[::2]):
        tr = _trace("capacity", d)
        assert len(tr["events"]) == e == len(tr["seq"]["events"]) and model.isolated(tr)
        got[e] = [model.event_capacity(tr, cases.CAP, m) for m in ("clusters", "sequential")]
        assert [model.event_capacity(tr, 2 * cases.CAP, m) for m in ("clusters", "sequential")] == [0, 0]
    cap = cases.CAP
    assert got == {cap - 3: [0, 0], cap - 2: [0, 0], cap - 1: [model.ARENA, 0], cap: [model.ARENA, model.ARENA]}
    for d in docs[1::2]:
        assert model.event_capacity(_trace("capacity", d), cases.CAP, "clusters") == 0


def test_lexem_size_documents():
    docs = cases.lexemsize_docs()
    trs = [_trace("lexemsize", d) for d in docs]
    assert [tr["err"] for tr in trs] == [0, 0, 0, model.LEXEMSIZE, 0] == [tr["seq"]["err"] for tr in trs]
    assert max(e.size for e in trs[1]["events"]) == 65534
    assert any(s["reason"] == model.SIZE_ERROR for s in trs[3]["steps"])
    want = _oracle_spans("lexemsize", [d for i, d in enumerate(docs) if i != 3])
    assert [model.spans(tr["events"]) for i, tr in enumerate(trs) if i != 3] == want
