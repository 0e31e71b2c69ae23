"""The numpy statement of the stitch (tests/segments_model.py) against a literal per-lexem loop over the rule of DESIGN.md 4
on random inputs, and against one hand-written case (tests/golden/segments_stitch_case.json).  No GPU."""
import json
import os

import numpy as np
import pytest

from tests import segments_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX32 = 0xFFFFFFFF


def literal_stitch(lexems, seg_offsets, seg_status, doc_seg_offsets):
    """the rule, one lexem at a time, in Python integers"""
    nseg = len(seg_offsets) - 1
    out, origseg, doc_offsets, status = [], [], [0], []
    for d in range(len(doc_seg_offsets) - 1):
        a, b = int(doc_seg_offsets[d]), int(doc_seg_offsets[d + 1])
        st, doc, segs = 0, [], []
        if a > b or b > nseg:
            st = 5
        else:
            base = 0
            for s in range(a, b):
                if seg_status[s] != 0:
                    st = int(seg_status[s])
                    break
                seg = [[int(x) for x in lx] for lx in lexems[int(seg_offsets[s]):int(seg_offsets[s + 1])]]
                for lid, ordpos, origpos, origsize in seg:
                    doc.append([lid, ordpos + base, origpos, origsize])
                    segs.append(s - a)
                if seg:
                    base = doc[-1][1]
            if st == 0 and (len(doc) > MAX32 or any(lx[1] > MAX32 for lx in doc)):
                st = 5
        if st != 0:
            doc, segs = [], []
        out += doc
        origseg += segs
        doc_offsets.append(len(out))
        status.append(st)
    return (np.array(out, np.uint32).reshape(-1, 4), np.array(origseg, np.uint32), np.array(doc_offsets, np.uint64),
            np.array(status, np.int32))


def random_case(rng, big_ordpos=False):
    nseg = int(rng.integers(0, 40))
    counts = rng.integers(0, 6, nseg) * (rng.random(nseg) < 0.7)
    seg_status = np.where(rng.random(nseg) < 0.08, rng.choice([2, 7, 9], nseg), 0).astype(np.int32)
    counts[seg_status != 0] = 0
    seg_offsets = np.zeros(nseg + 1, np.uint64)
    seg_offsets[1:] = np.cumsum(counts)
    n = int(seg_offsets[-1])
    lexems = np.zeros((n, 4), np.uint32)
    lexems[:, 0] = rng.integers(1, 9, n)
    for s in range(nseg):
        a, b = int(seg_offsets[s]), int(seg_offsets[s + 1])
        top = MAX32 // 2 if big_ordpos and rng.random() < 0.3 else 5
        lexems[a:b, 1] = np.cumsum(rng.integers(0, top, b - a)) % (MAX32 + 1) if b - a < 2 or not big_ordpos else np.sort(rng.integers(0, top, b - a))
    lexems[:, 2] = rng.integers(0, 1000, n)
    lexems[:, 3] = rng.integers(1, 9, n)
    # mostly ascending cuts; sometimes a descending pair, a range beyond the batch, ranges that share segments
    ndocs = int(rng.integers(0, 8))
    cuts = np.sort(rng.integers(0, nseg + 1, ndocs + 1)).astype(np.uint64)
    for i in range(len(cuts)):
        r = rng.random()
        if r < 0.06:
            cuts[i] = nseg + int(rng.integers(1, 4))
        elif r < 0.14:
            cuts[i] = int(rng.integers(0, nseg + 1))
    return lexems, seg_offsets, seg_status, cuts


def assert_same(got, want):
    for g, w, name in zip(got, want, ("lexems", "origseg", "doc_offsets", "status")):
        assert g.dtype == w.dtype and np.array_equal(g, w), name


@pytest.mark.parametrize("seed", range(40))
def test_model_equals_the_literal_loop(seed):
    rng = np.random.default_rng(seed)
    for _ in range(25):
        case = random_case(rng)
        assert_same(segments_model.stitch(*case), literal_stitch(*case))


def test_an_ordpos_beyond_32_bits_fails_its_document_only():
    rng = np.random.default_rng(7)
    failed = 0
    for _ in range(300):
        case = random_case(rng, big_ordpos=True)
        got, want = segments_model.stitch(*case), literal_stitch(*case)
        assert_same(got, want)
        failed += int(np.count_nonzero(want[3] == 5))
    assert failed > 20
    # the smallest case: two segments whose last positions add up to 2^32, between two good documents
    lexems = np.array([[1, 1, 0, 1], [1, MAX32, 0, 1], [2, 1, 0, 1], [1, MAX32 - 1, 0, 1], [2, 1, 0, 1]], np.uint32)
    got = segments_model.stitch(lexems, [0, 1, 2, 3, 4, 5], [0] * 5, [0, 1, 3, 5])
    assert got[3].tolist() == [0, 5, 0] and got[2].tolist() == [0, 1, 1, 3]
    assert got[0].tolist() == [[1, 1, 0, 1], [1, MAX32 - 1, 0, 1], [2, MAX32, 0, 1]] and got[1].tolist() == [0, 0, 1]


def test_the_hand_written_case():
    with open(os.path.join(GOLDEN, "segments_stitch_case.json")) as f:
        case = json.load(f)
    segs = case["segments"]
    lexems = np.array([lx for s in segs for lx in s], np.uint32).reshape(-1, 4)
    seg_offsets = np.cumsum([0] + [len(s) for s in segs]).astype(np.uint64)
    assert len(case["doc_seg_offsets"]) - 1 == 3 and len(segs) == 7 and sum(1 for s in segs if not s) == 2
    lex, origseg, offs, status = segments_model.stitch(lexems, seg_offsets, np.zeros(len(segs), np.int32), case["doc_seg_offsets"])
    want = case["expected"]
    assert lex.tolist() == want["lexems"] and origseg.tolist() == want["origseg"]
    assert offs.tolist() == want["doc_offsets"] and status.tolist() == want["status"]
    assert_same((lex, origseg, offs, status), literal_stitch(lexems, seg_offsets, np.zeros(len(segs), np.int32), case["doc_seg_offsets"]))


def test_empty_inputs():
    lex, origseg, offs, status = segments_model.stitch(np.zeros((0, 4), np.uint32), [0], [], [0])
    assert len(lex) == 0 and len(origseg) == 0 and offs.tolist() == [0] and len(status) == 0
    lex, origseg, offs, status = segments_model.stitch(np.zeros((0, 4), np.uint32), [0, 0], [0], [0, 0, 1, 1])
    assert len(lex) == 0 and offs.tolist() == [0, 0, 0, 0] and status.tolist() == [0, 0, 0]
