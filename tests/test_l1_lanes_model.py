"""CPU tests of the model of the lane-per-stream scan kernel (tests/l1_lanes_model.py) on the product's compiled tables,
and guards of the inputs of tests/test_l1_lanes_gpu.py: what every GPU batch is meant to contain is asserted here, by
the model, so that a later change to the inputs cannot turn a GPU test into a no-op.  No GPU."""
import random

import pytest

from tests import l1_lanes_cases as cases
from tests import l1_lanes_model as model


@pytest.mark.parametrize("name", sorted(cases.TABLES))
def test_tables_are_what_the_gpu_tests_take_them_for(name):
    """one scanned pass, whole-word literals and word shapes for the words kernel, the number of automaton words the
    case is named after, no classes by code point; exception rows and the bytes of the multi-byte class where meant"""
    t = cases.tables(name)
    exprs, words, lanes = cases.TABLES[name]
    assert t.scan_passes == 1 and t.nof_shapes >= 1 and len(t.literals) >= 2 and not t.cpBlocks and not t.nullable and not t.ucp
    n = model.scan_words(t)
    if lanes:
        assert n == words and 1 <= n <= model.MAX_LANE_WORDS
    else:
        assert n > model.MAX_LANE_WORDS
    if name == "ex":
        assert t.exCount[0] > 0
    if name == "utf":
        others = set(t.byteClass[b] for b in (0xC4, 0xA5, 0x80, 0x61))
        assert t.byteClass[0xC3] not in others and not others & set(t.byteClass[b] for b in (0xA4, 0xB6, 0xBC))


def test_scan_words_counts_scanned_passes_only():
    t = cases.tables("w1")
    assert any((p["word"] >> 6) >= t.scan_passes for p in t.patterns)      # (literals and word shapes lie behind the scanned pass)
    assert model.scan_words(t) == 1


SPANS = list(range(0, 2101)) + [4096, 4097, 32768]


def test_pieces_tile_the_unit():
    for span in SPANS:
        for seg_beg in (0, 1024, 32768 * 3):
            seg_end = seg_beg + span
            pcs = model.pieces(seg_beg, seg_end)
            assert len(pcs) == 64
            at = seg_beg
            empty = False
            for b0, b1 in pcs:
                assert b0 == at and b0 <= b1 <= seg_end             # no gap, no overlap, nothing behind the unit
                assert (b0 - seg_beg) % 16 == 0 or b0 == seg_end
                if b0 == b1:
                    empty = True
                else:
                    assert not empty                                # empty pieces come only at the end
                at = b1
            assert at == seg_end
            if span:
                assert pcs[0][1] > pcs[0][0]


def test_piece_size_steps():
    assert [model.piece_bytes(s) for s in (0, 1, 16, 17, 1024, 1025, 2048, 2049, 4096, 4097, 32768)] == [0, 16, 16, 16, 16, 32, 32, 48, 64, 80, 512]
    assert sum(1 for b0, b1 in model.pieces(0, 17) if b0 < b1) == 2
    assert sum(1 for b0, b1 in model.pieces(0, 1025) if b0 < b1) == 33
    assert sum(1 for b0, b1 in model.pieces(0, 64) if b0 < b1) == 4        # 64-byte chunks: four live lanes


def test_units():
    assert [model.units(n, 64) for n in (0, 1, 64, 65, 128, 129)] == [1, 1, 1, 2, 2, 3]
    assert model.segments(130, 64) == [(0, 64), (64, 128), (128, 130)]
    assert model.chunk_of(None) == 32768 and model.chunk_of(100) == 64


@pytest.mark.parametrize("name", [n for n in sorted(cases.TABLES) if cases.TABLES[n][2]])
def test_a_proven_state_is_the_true_state(name):
    """soundness of the warm-up proof on compiled tables: whenever F lies inside S, S is the state reached from the
    document's first byte.  (A proof that lied would be a wrong lexem no parity test is guaranteed to hit.)"""
    t = cases.tables(name)
    rng = random.Random(77)
    docs = [d for c in cases.EDGE_CHUNKS for d in cases.edge_docs(c)[0] if len(d) > 300] + cases.proof_docs(None)[0] + cases.proof_docs(1024)[0]
    if name == "dense":
        docs += list(cases.overflow_docs()[0]) + [cases.very_dense_doc(), cases.full_unit_doc()]
    docs = [d for d in docs if len(d) > 300]
    proven = unproven = 0
    for _ in range(300):
        d = rng.choice(docs)
        b0 = rng.randrange(1, len(d) + 1) if rng.random() < 0.5 else min(len(d), 16 * rng.randrange(1, len(d) // 16 + 1))
        ok, S = model.proof(t, d, b0)
        assert model.proven(t, d, b0) == ok
        if ok:
            proven += 1
            assert S == model.exact_state(t, d, b0), (name, len(d), b0)
        else:
            unproven += 1
    assert proven > 20
    assert unproven >= 1


@pytest.mark.parametrize("chunk", cases.EDGE_CHUNKS)
def test_edge_batch_reaches_the_piece_edges(chunk):
    docs, planted = cases.edge_docs(chunk)
    assert [len(d) for d in docs] == cases.EDGE_LENGTHS and len(docs) <= 200 and sum(len(d) for d in docs) < 1 << 20
    kinds = set(k for _, _, k in planted)
    assert kinds == set(cases.FEATURES)
    for di, b, kind in planted:
        feat, at = cases.FEATURES[kind]
        d = docs[di]
        assert b in cases.boundaries(len(d), chunk) and d[b - at:b - at + len(feat)] == feat
    # a match that ends with the document, on a document whose last piece is cut short (the bytewise tail load)
    assert any(d.endswith(e) and len(d) % 16 for d in docs for e in cases.ENDINGS)
    # features on the boundary between two chunks: lane 0 of a later chunk warms up from the chunk before it
    if chunk is not None:
        assert any(b % model.chunk_of(chunk) == 0 for _, b, _ in planted)
    t = cases.tables("w1")
    reps = {}
    for di, b, kind in planted:
        if di not in reps:
            reps[di] = set(to for to, _ in model.scan_reports(t, docs[di]))
    # ... and the scanned automaton reports where the features say: at the boundary, and right behind it
    assert any(kind == "ends_at" and b in reps[di] for di, b, kind in planted)
    assert any(kind == "straddle" and b + 3 in reps[di] for di, b, kind in planted)
    assert any(len(d) in set(to for to, _ in model.scan_reports(t, d)) for d in docs if d)


@pytest.mark.parametrize("chunk", [None, 1024])
def test_proof_batch_has_both_kinds_of_documents(chunk):
    t = cases.tables("w1")
    docs, what = cases.proof_docs(chunk)
    assert len(docs) <= 200 and sum(len(d) for d in docs) < 1 << 20
    c = model.chunk_of(chunk)
    if chunk is None:
        assert all(model.units(len(d), c) == 1 for d in docs)              # an unchunked batch
    else:
        assert any(model.units(len(d), c) > 1 for d in docs)
    again = model.rescanned(t, docs, c)
    kinds = dict((k, i in again) for i, k in enumerate(what))
    assert 1 <= len(again) < len(docs)
    assert all(v for k, v in kinds.items() if k.endswith("over_piece_boundary"))
    # (256 digits fill the warm-up: nothing in it says whether a '.' came before them)
    assert kinds["run256_ends_at_boundary"] and kinds["run257_ends_at_boundary"] and kinds["run257_ends_behind_boundary"]
    assert not kinds["run255_ends_at_boundary"] and not kinds["run_inside_first_256_bytes"] and not kinds["plain"] and not kinds["empty"]
    # every unproven piece lies more than 256 bytes into its document
    for di in again:
        for u, lane in model.unproven_pieces(t, docs[di], c):
            sb, se = model.segments(len(docs[di]), c)[u]
            assert model.pieces(sb, se)[lane][0] > model.WARM
    if chunk is not None:
        by_chunks = model.rescanned_by_chunks(t, docs, c)
        assert kinds["run_over_chunk_boundary"] and what.index("run_over_chunk_boundary") in by_chunks
        assert by_chunks < again                                           # a run over a piece boundary only
    # the document with a lexem that is too long fails its proof as well
    assert model.unproven_pieces(t, cases.too_long_doc(), c)


def test_overflow_batch_overflows_one_lane_and_no_unit():
    t = cases.tables("dense")
    docs, what = cases.overflow_docs()
    c = model.chunk_of(None)
    assert not model.rescanned(t, docs, c)
    over8, over16 = model.overflowing(t, docs, c, 8), model.overflowing(t, docs, c, 16)
    assert over8 == set(i for i, k in enumerate(what) if k.startswith("dense")) and len(over8) == 2 and not over16
    beg = 0
    for di, d in enumerate(docs):
        counts = model.lane_counts(t, d, c)
        # (the wave-per-unit kernel has the whole slice for the unit: never short)
        assert sum(counts.values()) <= 64 * model.region_cap(beg, 0, len(d), 8)
        if di in over8:
            full = [lane for (u, lane), n in counts.items() if n > model.region_cap(beg, 0, len(d), 8)]
            assert len(full) == 1
            live = [lane for lane, (b0, b1) in enumerate(model.pieces(0, len(d))) if b0 < b1]
            if what[di] == "dense_last_live_lane":
                assert full == [live[-1]] and live[-1] < 63
        beg += len(d)
    # a unit short as a whole (and not for a failed proof)
    f = cases.full_unit_doc()
    assert not model.unproven_pieces(t, f, c) and sum(model.lane_counts(t, f, c).values()) > model.unit_cap(0, 0, len(f), 8)
    # 200 dense bytes: short at 8, 16 and 32, fits at 64 (three doublings of the queue)
    v = [cases.very_dense_doc()]
    assert [bool(model.overflowing(t, v, c, m)) for m in (8, 16, 32, 64)] == [True, True, True, False]
