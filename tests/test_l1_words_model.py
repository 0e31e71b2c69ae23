"""CPU tests of the model of the words kernel (tests/l1_words_model.py) on the product's compiled tables, and guards of
the inputs of tests/test_l1_words_gpu.py: what every GPU batch is meant to contain is asserted here, by the model, so
that a later change to the inputs cannot turn a GPU test into a no-op.  The second half is the completeness of the word
shapes without a GPU: the candidates the keys yield, confirmed by the walk, are exactly the matches of the same table
compiled without shapes, and of the oracle.  No GPU."""
import functools

import pytest

import oracle
import struspattern_amd as spa
from tests import l1_words_cases as cases
from tests import l1_words_model as model

WHOLE = model.DEFAULT_CHUNK


@functools.lru_cache(maxsize=None)
def _traces(name, docs, chunk):
    t = cases.tables(name)
    return [model.flush_trace(t, d, chunk) for d in docs]


def _units(name, docs, chunk):
    return [u for tr in _traces(name, tuple(docs), chunk) for u in tr]


def _flushes(name, docs, chunk):
    return [f for u in _units(name, docs, chunk) for f in u["flushes"]]


# ---------------------------------------------------------------- the tables
def test_tables_are_what_the_gpu_tests_take_them_for():
    for name in cases.TABLES:
        t = cases.tables(name)
        assert len(cases.TABLES[name]) <= 40 and t.scan_passes == 1 and not t.cpBlocks and not t.nullable and not t.ucp
        assert any((p["word"] >> 6) < t.scan_passes for p in t.patterns)                   # the scanned number expression
        off = cases.tables(name, shapes=False)
        assert off.nof_shapes == 0 and not off.shapes and off.literals.keys() == t.literals.keys()
    # literals only: the words kernel reads its tables from global memory (wordsDocuments<false>)
    t = cases.tables("lits")
    assert t.nof_shapes == 0 and not t.shapes
    assert sorted(len(w) for w in t.literals) == sorted(cases.LIT_LENGTHS + [17, 20, 64, 3, 1])    # (+ the twins, "xyz", "y")
    assert len(t.literals[cases.SHARED_LITERAL]) == 3
    for n, at in ((17, 17), (20, 20), (64, 64)):
        a, b = cases.LITS[n], cases.LIT_TWINS[(17, 20, 64).index(n)]
        assert a[:at - 1] == b[:at - 1] and a[at - 1] != b[at - 1] and a[:16] == b[:16] and a in t.literals and b in t.literals
    # every variant the compiler can emit that fits the table of eight, lists of 3 and 2
    P, S, W = model.PREFIX, model.SUFFIX, model.PREVWORD
    t = cases.tables("keys")
    assert model.variants(t) == sorted([P | 2 << 4, P | 4 << 4, P | 1 << 2 | 2 << 4, P | 2 << 2 | 4 << 4, P | 3 << 2 | 4 << 4, S | 2 << 4, S | 3 << 4, S | 4 << 4])
    assert sorted(len(v) for v in t.shapes.values()).count(3) == 1 and sorted(len(v) for v in t.shapes.values()).count(2) == 1
    t = cases.tables("keys_prev")
    assert model.variants(t) == sorted([P | 2 << 4, P | 4 << 4, P | 1 << 2 | 2 << 4, P | 2 << 2 | 4 << 4, P | 3 << 2 | 4 << 4, S | 2 << 4, S | 3 << 4, W])
    assert len(t.shapes[(W | 2 << 8, model.word_hash(b"ab"))]) == 2
    t = cases.tables("prev")
    assert sorted(tag >> 8 for tag, _ in t.shapes if (tag & 3) == W) == [1, 1, 2] + cases.PREV_LONG
    assert len(t.shapes[(W | 2 << 8, model.word_hash(b"ab"))]) == 2 and S | 3 << 4 in model.variants(t)
    for name in ("ring", "dense"):
        assert len(model.variants(cases.tables(name))) >= 3 and cases.tables(name).literals


def test_what_the_compiler_does_not_take():
    """a literal of 65 bytes and \\bW\\sE\\b with W of 63 and 64 bytes have more byte positions than an automaton word:
    the compiler refuses them (there is nothing to cut at), so no table holds a literal longer than 64 bytes or a
    PREVWORD key longer than 62.  The text has such runs all the same (edge_docs: lit_65, prev_run_63..)."""
    def compiles(expr):
        lx = spa.PatternLexerInstance()
        lx.defineLexem(1, expr, 0, 1, "content")
        try:
            lx.compile()
        except spa.PatternError:
            return None
        from tests.l1_table_sim import Tables
        return Tables(lx.dumpTables())
    t = compiles("\\b%s\\b" % cases.LITS[64].decode())
    assert t is not None and list(t.literals) == [cases.LITS[64]]
    assert compiles("\\b%s\\b" % cases.LIT65.decode()) is None
    for n in cases.PREV_LONG:
        t = compiles("\\b%s\\s\\w+\\b" % cases.word(n).decode())
        assert t is not None and list(t.shapes) == [(model.PREVWORD | n << 8, model.word_hash(cases.word(n)))]
    for n in cases.PREV_TOO_LONG:
        assert compiles("\\b%s\\s\\w+\\b" % cases.word(n).decode()) is None


def test_more_variants_than_the_table_holds():
    t = cases.tables("variants12")
    kept = model.variants(t)
    assert len(kept) == model.MAX_VARIANTS and not set(kept) & set(cases.VARIANTS12_DROPPED)
    assert t.nof_shapes == 16 and sum(len(v) for v in t.shapes.values()) == 16
    # the four expressions of the dropped variants sit in the scanned passes
    exprs = [e for e, _, _ in cases.TABLES["variants12"]]
    for e in ("\\b[a-z][a-z]cd[a-z]*\\b", "\\b[a-z][a-z]cdef[a-z]*\\b", "\\b[a-z][a-z][a-z]defg\\w*\\b", "[a-z]+dcab\\b"):
        pi = [i for i, p in enumerate(t.patterns) if p["defIndex"] == exprs.index(e)]
        assert len(pi) == 1 and (t.patterns[pi[0]]["word"] >> 6) < t.scan_passes
        assert not any(pi[0] in v for v in t.shapes.values())


# ---------------------------------------------------------------- the model itself
def test_owner_and_back_off():
    assert [model.owner(to, 130, 64) for to in (0, 63, 64, 65, 127, 128, 129, 130)] == [0, 0, 1, 1, 1, 2, 2, 2]
    assert model.owner(128, 128, 64) == 1 and model.owner(64, 64, 64) == 0 and model.owner(0, 0, 64) == 0
    t = cases.tables("ring")
    d = b"ab " + b"k" * 400 + b" kk"
    assert model.back_off(t, d, 100) == (0, []) and model.back_off(t, d, 384) == (0, [1, 2])
    d = b"zz ab " + b"k" * 160 + b" kk"
    assert model.back_off(t, d, 166) == (3, [2])                                           # w0 = 6: the run starts there, "ab" is the word before
    assert model.back_off(t, d, 167) == (3, [1, 2])
    assert model.run_ends(t, b"a bb " + b"c" * 70 + b" d") == [(1, 0, 1, 0, False), (4, 2, 2, 1, True), (75, 5, 65, 2, True), (77, 76, 1, 65, False)]


def test_the_walk_is_the_start_of_match_of_the_table_sim():
    for name in ("keys_prev", "prev", "ring"):
        t = cases.tables(name)
        n = 0
        for d in cases.edge_docs()[0] + cases.ring_docs()[0][:6]:
            for recs in model.records(t, d, WHOLE):
                for to, pi, frm, dead in recs:
                    p = t.patterns[pi]
                    if p["word"] == 0xFFFFFFFF:
                        continue
                    w, ln = divmod(p["word"], 64)
                    R = p["mask"] & t.acceptMask[(w * 4 + t.ctx(d, to)) * 64 + ln] & t.charMask[(w * t.nofClasses + t.cls(d, to - 1)) * 64 + ln]
                    assert (not R and dead and frm == to) or (R and t.som(d, pi, to, R) == frm and dead == (frm == to))
                    n += 1
        assert n > 50


# ---------------------------------------------------------------- what the batches contain
def _batches():
    """(table, documents, chunk) of every GPU batch"""
    out = []
    e = tuple(cases.edge_docs()[0])
    for name in ("lits", "keys", "keys_prev", "variants12", "prev"):
        out.append((name, e, WHOLE))
    for name in ("keys", "lits", "prev"):
        for c in cases.CHUNKS:
            out.append((name, tuple(cases.edge_docs(c)[0]), c))
    out.append(("dense", tuple(cases.dense_docs()[0]), WHOLE))
    out.append(("ring", tuple(cases.ring_docs()[0]), WHOLE))
    out.append(("ring", tuple(cases.ring_docs()[0]), 1024))
    for c in cases.CHUNKS:
        for name in ("prev", "keys", "ring"):
            out.append((name, tuple(cases.chunk_docs(c)[0]), c))
    out.append(("dense", tuple(cases.overflow_docs()[0]), WHOLE))
    return out


def test_batches_are_small_and_no_fingerprint_collides():
    """no key the text yields has the fingerprint of a table key it is not: word_reports of the model is exact"""
    for name, docs, chunk in _batches():
        assert sum(len(d) for d in docs) < 48 * 1024, name
        assert not model.fingerprint_collisions(cases.tables(name), docs), name
    # the salt is the compiler's: the fingerprints of the keys are the ones of the words kernel's image
    for name in ("keys", "prev", "variants12"):
        lx = spa.PatternLexerInstance()
        cases.build(lx, name)
        t = cases.tables(name)
        offs, words = lx.dumpImage(2)
        salt = model.shape_salt(t)
        fps = set(int(w) & 0xFFFFFFFF for w in words[offs[7]:]) - {0}
        assert fps == set(model.shape_fingerprint(tag, key, salt) for tag, key in t.shapes)


def test_edge_batch_reaches_the_run_key_and_literal_edges():
    docs, what = cases.edge_docs()
    lits, keys, kp, prev = (cases.tables(n) for n in ("lits", "keys", "keys_prev", "prev"))
    # runs that start at, end at and straddle every tile offset; runs of the lengths around the cap
    for p in cases.TILE_OFFSETS:
        rs = [r for d in docs for r in model.runs(keys, d)]
        assert any(f == p for f, to in rs) and (p == 0 or (any(to == p for f, to in rs) and any(f < p < to for f, to in rs)))
    ends = [(d, e) for d in docs for e in model.run_ends(lits, d)]
    assert set(cases.RUN_LENGTHS) <= set(e[0] - e[1] for d, e in ends)
    assert {63, 64, 65} <= set(e[2] for d, e in ends) and {62, 65} <= set(e[3] for d, e in ends)
    assert any(e[3] == 64 and e[4] for d, e in ends) and any(e[3] == 65 and not e[4] for d, e in ends)
    # documents that end in a word and in a separator, at every edge length
    for n in cases.DOC_LENGTHS:
        ds = [d for d in docs if len(d) == n]
        assert any(not d or not model.is_word(lits, d[-1]) for d in ds)
        if n:
            assert any(model.is_word(lits, d[-1]) for d in ds)
            assert any(e[0] == n and (model.candidates(keys, d, e) or model.candidates(lits, d, e)) for d in ds for e in model.run_ends(keys, d))
    # literals of every length, the compare beyond the 16 inline bytes with a rest of 1, 2 and 3, the byte-wise loads
    probes = [model.literal_probe(lits, d, e) for d, e in ends]
    hits = [p for p in probes if p and p["hit"]]
    assert set(len(w) for w in lits.literals) == set(e[2] for (d, e), p in zip(ends, probes) if p and p["hit"])
    assert {1, 2, 3} <= set(p["rems"][-1] for p in hits if p["rems"]) and any(p["rems"] and p["rems"][-1] == 4 for p in hits)
    assert any(p["first16_bytewise"] and p["hit"] for p in hits) and any(p["tail_bytewise"] for p in hits)
    assert any(p["rems"] and not p["tail_bytewise"] for p in hits)
    for back in (15, 16, 17, 3):
        assert any(e[1] == len(d) - back and p and p["hit"] for (d, e), p in zip(ends, probes))
    assert any(len(model.candidates(lits, d, e)) == 3 for d, e in ends)
    # shape keys: the run as long as the key's place and one byte short, keys from single bytes (o + k > 4), ends below 4
    kends = [(d, e) for d in docs for e in model.run_ends(keys, d)]
    for var in model.variants(keys):
        kind, o, k = model.variant_fields(var)
        need = o + k if kind == model.PREFIX else k
        assert any(e[2] == need and model.shape_key(d, e, var) in keys.shapes for d, e in kends), hex(var)
        assert any(e[2] == need - 1 for d, e in kends)
    assert any(e[0] < 4 and model.shape_key(d, e, model.SUFFIX | 2 << 4) in keys.shapes for d, e in kends)
    assert any(e[0] == 3 and model.shape_key(d, e, model.SUFFIX | 3 << 4) in keys.shapes for d, e in kends)
    # an end that hits all nine lists
    for t in (keys, kp):
        assert any(all(model.candidate_lists(t, d, e)) and len(model.candidate_lists(t, d, e)) == 9 for d in docs for e in model.run_ends(t, d))
    # the word before at offsets 0 and 1, in an earlier tile, of 61 and 62 bytes
    pends = [(d, e) for d in docs for e in model.run_ends(prev, d)]
    hit = [(d, e) for d, e in pends if e[4] and model.shape_key(d, e, model.PREVWORD) in prev.shapes]
    assert {0, 1} <= set(e[1] - 1 - e[3] for d, e in hit) and set(cases.PREV_LONG) | {1, 2} <= set(e[3] for d, e in hit)
    assert any((e[1] - 1) // 64 < e[0] // 64 for d, e in hit)
    # dead candidates: a key of the table whose walk does not confirm
    for name in ("keys", "prev"):
        assert any(dead for d in docs for recs in model.records(cases.tables(name), d, WHOLE) for _, _, _, dead in recs)
    assert any(any(b >= 0x80 for b in d) for d in docs)


def test_dense_batch_fills_the_ends_and_mixes_the_merges():
    docs, what = cases.dense_docs()
    t = cases.tables("dense")
    us = _units("dense", docs, WHOLE)
    assert max(u["max_waiting"] for u in us) == 95 == model.ENDS - 1                        # 63 wait, 32 more come
    fl = _flushes("dense", docs, WHOLE)
    assert any(f["total"] > 64 for f in fl) and any(f["total"] > 128 for f in fl)           # two rounds of walks and more
    assert any(max(f["lanes"]) > 4 and 0 < min(x for x in f["lanes"] if x) <= 4 for f in fl)
    assert any(all(x >= 5 for x in f["lanes"]) and f["count"] == 64 for f in fl)           # ends every second byte, 5 candidates each
    # lanes that take the sorting network next to lanes that merge lists, in one flush
    d = docs[what.index("mixed")]
    kinds = set()
    for e in model.run_ends(t, d)[:64]:
        ls = [l for l in model.candidate_lists(t, d, e) if l]
        if ls:
            kinds.add(sum(len(l) for l in ls) <= 4 and all(len(l) == 1 for l in ls))
    assert kinds == {True, False}


def test_ring_batch_walks_on_both_sides_of_the_ring():
    docs, what = cases.ring_docs()
    t = cases.tables("ring")
    assert [w[1] for w in what if w[0] == "word"] == [L for L in cases.RING_LENGTHS for _ in cases.RING_ALIGN]
    left = {}
    for d, w, tr in zip(docs, what, _traces("ring", tuple(docs), WHOLE)):
        if w[0] == "word":
            walks = [x for f in tr[0]["flushes"] for x in f["walks"] if x[0] == len(d)]
            assert len(walks) >= 3
            left[(w[1], w[2])] = any(x[2] for x in walks)
    # the document ends with the word at a tile offset a: the last flush has the 512 bytes before the next tile
    for a in cases.RING_ALIGN:
        stay = [L for L in cases.RING_LENGTHS if not left[(L, a)]]
        leave = [L for L in cases.RING_LENGTHS if left[(L, a)]]
        assert stay == [L for L in cases.RING_LENGTHS if L < 448 + a] and leave == [L for L in cases.RING_LENGTHS if L >= 448 + a], (a, stay, leave)
    assert not left[(510, 63)] and left[(511, 63)] and not left[(384, 0)] and left[(448, 0)]
    # pressure: a flush for one waiting end, and for two; an end at a tile offset of 0 that waits until the flush
    fl = _flushes("ring", docs, WHOLE)
    assert any(f["pressure"] and f["count"] == 1 for f in fl) and any(f["pressure"] and f["count"] == 2 for f in fl)
    assert any(f["pressure"] and f["count"] == 1 and f["walks"] and f["walks"][0][0] % 64 == 0 for f in fl)
    assert sum(1 for f in fl if f["pressure"]) >= 10
    # in chunks of 1024 the words cross chunk boundaries
    assert any(len(tr) > 1 for tr in _traces("ring", tuple(docs), 1024))


@pytest.mark.parametrize("chunk", cases.CHUNKS)
def test_chunk_batch_reaches_ownership_and_back_off(chunk):
    docs, what = cases.chunk_docs(chunk)
    t = cases.tables("keys")
    B = 1024 if chunk == 1024 else 384
    assert B % chunk == 0
    by = dict(zip(what, docs))
    ends = dict((k, [e for e in model.run_ends(t, by[k])]) for k in by)
    for k, to in (("end_at_B-1", B - 1), ("end_at_B+0", B), ("end_at_B+1", B + 1)):
        assert any(e[0] == to and model.candidates(t, by[k], e) for e in ends[k])
    # an end at to == segBeg is owned there; an end at to == segEnd < len by the next unit
    u = B // chunk
    assert model.owner(B, len(by["end_at_B+0"]), chunk) == u and model.segments(len(by["end_at_B+0"]), chunk)[u][0] == B
    tr = model.flush_trace(t, by["end_at_B+0"], chunk)
    assert B in [e[0] for e in tr[u]["ends"]] and B not in [e[0] for e in tr[u - 1]["ends"]]
    for ln in (1, 2, 159, 160, 161, 300):
        assert any(e[0] == B + 1 and e[0] - e[1] == ln for e in ends["run_%d" % ln])
    assert any(e[0] - e[1] >= chunk + 20 for e in ends["run_over_chunk"])
    # the back-off: both steps, the second one alone (the word before lies wholly before the back-off)
    steps = dict((k, model.flush_trace(t, by[k], chunk)[u]["steps"]) for k in by if len(by[k]) > B)
    assert 1 not in steps["run_161"] and steps["run_162"][0] == 1 and steps["run_300"][0] == 1
    assert model.flush_trace(t, by["run_161"], chunk)[u]["w0"] <= B - 160 == B + 1 - 161                       # (the run starts where the back-off lands)
    assert steps["prev_ends_at_B-161"] == [2] and steps["prev_before_back_off"] == [1, 2]
    p = cases.tables("prev")
    for k in ("sep_at_B-1", "sep_at_B", "sep_at_B_dash", "prev_ends_at_B-161", "prev_before_back_off"):
        hit = [e for e in model.run_ends(p, by[k]) if e[4] and model.shape_key(by[k], e, model.PREVWORD) in p.shapes]
        assert hit and all(e[0] > B for e in hit), k
        # ... seen from the unit's own start as well
        assert any(e in model.flush_trace(p, by[k], chunk)[u]["ends"] for e in hit), k
    assert by["sep_at_B-1"][B - 1:B] == b" " and by["sep_at_B"][B:B + 1] == b" " and by["prev_ends_at_B-161"][B - 161:B - 160] == b" "
    # to == segEnd == len; whole chunks
    d = by["last_chunk_ends_in_word"]
    assert model.is_word(t, d[-1]) and len(d) % chunk and model.flush_trace(t, d, chunk)[-1]["ends"][-1][0] == len(d)
    for k in ("whole_chunks_word", "whole_chunks_pair", "whole_chunks_sep", "one_chunk"):
        assert len(by[k]) % chunk == 0 and model.units(len(by[k]), chunk) == len(by[k]) // chunk
    assert model.flush_trace(t, by["whole_chunks_word"], chunk)[-1]["ends"][-1][0] == len(by["whole_chunks_word"])


def test_overflow_batch_is_short_once_and_twice():
    docs, what = cases.overflow_docs()
    t = cases.tables("dense")
    over = [set(di for di, u in model.overflowing(t, docs, WHOLE, m)) for m in (8, 16, 32)]
    assert over == [{what.index("dense"), what.index("very_dense")}, {what.index("very_dense")}, set()]
    assert all(model.units(len(d), WHOLE) == 1 for d in docs)
    # (nothing for the scan kernel's queue, or a lane's part of it, to be short of)
    assert all(not model.automaton_reports(t, d, True) for d in docs)


# ---------------------------------------------------------------- completeness of the shapes
_ORACLE = {}


def _oracle_raw(name, doc):
    if name not in _ORACLE:
        _ORACLE[name] = oracle.L1Lexer()
        cases.build(_ORACLE[name], name)
    raw, _ = _ORACLE[name].matchDocs(doc, [0, len(doc)], raw=True)
    return [(int(r[0]), int(r[1]), int(r[2])) for r in raw]


def _completeness_docs(name):
    if name == "dense":
        return [d[:300] for d in cases.dense_docs()[0]], [WHOLE]
    if name == "ring":
        return [d for d, w in zip(*cases.ring_docs()) if w[0] == "word" and w[1] in (190, 511, 600) and w[2] == 63] + cases.chunk_docs(64)[0], [WHOLE, 64]
    docs = list(cases.edge_docs()[0])
    if name in ("prev", "keys"):
        docs += cases.chunk_docs(64)[0]
    return docs, [WHOLE, 64]


@pytest.mark.parametrize("name", sorted(cases.TABLES))
def test_shapes_are_complete(name):
    """every match of a shape expression is among the candidates its key yields and is confirmed with its leftmost
    start: the model's live records merged with the reports of the scanned passes are, document by document, the reports
    of the table compiled without shapes, and the oracle's -- whole and in chunks of 64 bytes"""
    t, off = cases.tables(name), cases.tables(name, shapes=False)
    docs, chunks = _completeness_docs(name)
    some = 0
    for d in docs:
        want = model.by_definition(off, model.automaton_reports(off, d, False))
        for c in chunks:
            assert model.merged_reports(t, d, c) == want, (name, c, d)
        if len(d) <= 200:
            assert want == off.raw_reports(d) == _oracle_raw(name, d), (name, d)
        else:
            assert want == _oracle_raw(name, d), (name, d)
        some += len(want)
    assert some > 50
