"""Segmented documents on the device (csrc/l1_stitch.h): the lexer's segments stitched to documents in HBM, bit for bit
what tests/segments_model.py makes of the same lexer batch; the failure paths; lexer -> stitch -> matcher against the
oracle chain (oracle lexer per segment -> segments_model -> oracle matcher with the origseg column) on all three rule
kernels; matchSegmentedDocs and `match.py --paragraphs`."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from struspattern_amd import match, rulelang, segments, synth
from tests import segments_model
from tests.result_set_model import results_multiset

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SP_DOC_ERR_RANGE, SP_DOC_ERR_OUTPUT = 5, 9

# a small lexer: words and numbers count positions, the full stop is bound to the word before it (so that the last
# ordinal position of a segment is not its lexem count)
PATTERNS = [(1, "[a-z]+", 0, 1, "content"), (2, "[0-9]+", 0, 1, "content"), (3, "[.]", 0, 2, "predecessor")]


def _lexer(cls=None):
    lx = (cls or spa.PatternLexerInstance)()
    synth.apply_lexer_patterns(lx, PATTERNS)
    return lx


def _segment_text(rng, nlexems):
    """a segment that lexes to exactly `nlexems` lexems"""
    out, n = [], 0
    while n < nlexems:
        r = rng.random()
        if r < 0.15 and n + 2 <= nlexems:
            out.append("".join(rng.choice(list("abc"), int(rng.integers(1, 4)))) + ".")
            n += 2
        elif r < 0.3:
            out.append(str(int(rng.integers(0, 100))))
            n += 1
        else:
            out.append("".join(rng.choice(list("abcde"), int(rng.integers(1, 5)))))
            n += 1
    return (" ".join(out) + (" " if rng.random() < 0.5 else "")).encode()


class _Batch:
    """segments on the device and the lexer's batch of them"""

    def __init__(self, lctx, pieces):
        import torch
        self.torch = torch
        self.text = b"".join(pieces)
        self.seg_offsets = np.zeros(len(pieces) + 1, np.uint64)
        self.seg_offsets[1:] = np.cumsum([len(p) for p in pieces])
        self.nseg = len(pieces)
        self.d_text = torch.frombuffer(bytearray(self.text + b"\0" * 16), dtype=torch.uint8).cuda()
        self.d_offs = torch.from_numpy(self.seg_offsets.view(np.int64)).cuda()
        self.stream = torch.cuda.current_stream().cuda_stream
        self.lctx = lctx

    def lex(self, grow_output=True):
        """the device protocol: a batch with segments that had no room in the working set (status 2) or, with grow_output,
        in the lexem buffer (status 9) is grown and rerun"""
        for _ in range(12):
            out = self.lctx.matchDocsDevice(self.d_text.data_ptr(), self.d_offs.data_ptr(), self.nseg, len(self.text), self.stream)
            codes = set(int(x) for x in self.lctx.batchStatus(self.nseg))
            assert codes <= {0, 2, 9}
            if 2 not in codes and not (grow_output and 9 in codes):
                return out
            if grow_output:
                self.lctx.reserveOutput(int(self.lctx.batchCounters()["lexems"] * 1.2) + 1024)
            if 2 in codes:
                assert self.lctx.growArena()
        raise AssertionError("segments still failing after resizing")

    def stitch(self, doc_seg_offsets):
        dso = np.ascontiguousarray(doc_seg_offsets, dtype=np.uint64)
        self.d_dso = self.torch.from_numpy(dso.view(np.int64)).cuda()
        return self.lctx.stitchSegmentsDevice(self.d_dso.data_ptr(), len(dso) - 1, self.stream)

    def model(self, doc_seg_offsets):
        raw = self.lctx.batchFetch(0, self.nseg)
        return raw, segments_model.stitch(raw.lexems, raw.doc_offsets, raw.status, doc_seg_offsets)


def _assert_stitched(lctx, want):
    lb, origseg = lctx.stitchedFetch()
    lex, seg, offs, status = want
    assert np.array_equal(lb.status, status)
    assert np.array_equal(lb.doc_offsets, offs)
    assert np.array_equal(lb.lexems, lex)
    assert np.array_equal(origseg, seg)
    assert np.array_equal(lctx.stitchedStatus(), status)
    return lb, origseg


# ---- 1. stitch parity, bit-exact
def _shapes(rng):
    """documents as lists of lexem counts per segment"""
    small = lambda n: [int(x) for x in rng.integers(0, 4, n)]
    return [
        [5], [], [3, 0], small(63), small(64), small(65), small(130),
        [0, 0, 4], [2, 0, 0, 3], [3, 0], [0, 0, 0],
        [1, 63, 64, 65, 1000],
        [1] * 70,                                   # a carry of one per segment over a round boundary
    ]


def test_stitch_parity_all_shapes():
    rng = np.random.default_rng(11)
    docs = _shapes(rng)
    lead, trail = [2, 0], [4, 1, 0]                 # lexer documents in front of and behind the ranges, in no document
    counts = lead + [c for d in docs for c in d] + trail
    pieces = [_segment_text(rng, c) for c in counts]
    dso = len(lead) + np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    lctx = _lexer().createContext()
    b = _Batch(lctx, pieces)
    b.lex()
    out = b.stitch(dso)
    raw, want = b.model(dso)
    assert np.array_equal(np.diff(raw.doc_offsets.astype(np.int64)), counts) and not raw.status.any()
    assert out.ndocs == len(docs)
    lb, origseg = _assert_stitched(lctx, want)
    # what the shapes are there for
    assert np.array_equal(np.diff(lb.doc_offsets.astype(np.int64)), [sum(d) for d in docs])
    assert int(origseg.max()) == 129 and len(lb.lexems) == sum(counts) - sum(lead) - sum(trail)
    assert lctx.lastStitchMs() >= 0.0
    # the raw batch stays as it is, and a second stitch of it (other documents: every segment its own) is as exact
    again = lctx.batchFetch(0, b.nseg)
    assert np.array_equal(again.lexems, raw.lexems) and np.array_equal(again.doc_offsets, raw.doc_offsets)
    each = np.arange(b.nseg + 1, dtype=np.uint64)
    b.stitch(each)
    lb, origseg = _assert_stitched(lctx, b.model(each)[1])
    assert np.array_equal(lb.lexems, raw.lexems) and not origseg.any()


def test_stitch_parity_one_document():
    rng = np.random.default_rng(12)
    counts = [7, 0, 66]
    lctx = _lexer().createContext()
    b = _Batch(lctx, [_segment_text(rng, c) for c in counts])
    b.lex()
    assert b.stitch([0, 3]).ndocs == 1
    lb, origseg = _assert_stitched(lctx, b.model([0, 3])[1])
    assert len(lb.lexems) == 73 and origseg.tolist() == [0] * 7 + [2] * 66
    # no documents at all
    assert b.stitch([0]).ndocs == 0
    lb, origseg = _assert_stitched(lctx, b.model([0])[1])
    assert len(lb.lexems) == 0 and lb.doc_offsets.tolist() == [0]


def test_stitch_on_another_stream_than_the_batch():
    import torch
    rng = np.random.default_rng(13)
    counts = [int(x) for x in rng.integers(0, 40, 50)]
    lctx = _lexer().createContext()
    b = _Batch(lctx, [_segment_text(rng, c) for c in counts])
    b.lex()
    dso = np.arange(0, 51, 5, dtype=np.uint64)
    other = torch.cuda.Stream()
    d_dso = torch.from_numpy(dso.view(np.int64)).cuda()
    torch.cuda.current_stream().synchronize()      # (the upload of the offsets; the batch itself is ordered by the call)
    lctx.stitchSegmentsDevice(d_dso.data_ptr(), 10, other.cuda_stream)
    _assert_stitched(lctx, b.model(dso)[1])


# the offsets pass scans the documents in tiles of 1024: batches around the tile boundary and into a third tile
_TILE = []


def _tile_batch():
    """the lexer's batch of the segments of 2049 documents of 0..2 segments of 0..3 lexems each; document 1024, the first of
    the second tile, has two segments with lexems between documents without segments"""
    if not _TILE:
        rng = np.random.default_rng(14)
        nsegs = rng.integers(0, 3, 2049)
        nsegs[[0, 1022, 1023, 1025, 2047]] = 0
        nsegs[[1021, 1024, 2048]] = 2
        counts = [int(x) for x in rng.integers(0, 4, int(nsegs.sum()))]
        dso = np.concatenate([[0], np.cumsum(nsegs)]).astype(np.uint64)
        counts[int(dso[1024])] = counts[int(dso[1024]) + 1] = 2
        b = _Batch(_lexer().createContext(), [_segment_text(rng, c) for c in counts])
        b.lex()
        _TILE.append((b, dso, counts))
    return _TILE[0]


@pytest.mark.parametrize("ndocs", [1023, 1024, 1025, 2049])
def test_stitch_parity_around_the_tile_of_the_offsets_pass(ndocs):
    b, dso, counts = _tile_batch()
    dso = dso[:ndocs + 1]                           # (the segments behind are in no document)
    out = b.stitch(dso)
    raw, want = b.model(dso)
    assert np.array_equal(np.diff(raw.doc_offsets.astype(np.int64)), counts) and not raw.status.any()
    assert out.ndocs == ndocs and not want[3].any()
    lb, origseg = _assert_stitched(b.lctx, want)
    sizes = np.diff(lb.doc_offsets.astype(np.int64))
    assert sizes.tolist() == [sum(counts[int(dso[d]):int(dso[d + 1])]) for d in range(ndocs)]
    assert sizes[1022] == 0 and (ndocs <= 1024 or sizes[1024] == 4) and (ndocs <= 1025 or sizes[1025:].sum() > 0)


def test_documents_beyond_the_capacity_in_the_second_tile_of_the_offsets_pass():
    """2100 documents over the same four segments, 3 lexems per document on average: the running sum passes the lexer's lexem
    capacity (for a small text 4096 + a third of its bytes, see test_a_segment_failed_by_the_lexer_fails_its_document) at a
    document of the second tile.  Documents can share segments only where the segment offsets descend, and the document
    across the descent fails with SP_DOC_ERR_RANGE and has no lexems: here every fifth one."""
    rng = np.random.default_rng(15)
    counts = [5, 5, 5, 0]
    ndocs = 2100
    lctx = _lexer().createContext()
    b = _Batch(lctx, [_segment_text(rng, c) for c in counts])
    b.lex()
    dso = np.array([d % 5 for d in range(ndocs + 1)], np.uint64)    # [0,1) [1,2) [2,3) [3,4): no lexems, [4,0): descends
    assert b.stitch(dso).ndocs == ndocs
    raw, (lex, seg, offs, status) = b.model(dso)                    # (the model knows no capacity)
    assert np.array_equal(np.diff(raw.doc_offsets.astype(np.int64)), counts)
    sizes = np.diff(offs.astype(np.int64))
    assert sizes.tolist() == [(5, 5, 5, 0, 0)[d % 5] for d in range(ndocs)]
    assert status.tolist() == [(0, 0, 0, 0, SP_DOC_ERR_RANGE)[d % 5] for d in range(ndocs)]
    lb, origseg = lctx.stitchedFetch()
    assert np.array_equal(lctx.stitchedStatus(), lb.status)
    # the statuses: the model's up to the first document that does not fit; from there on SP_DOC_ERR_OUTPUT for every
    # document with lexems, the model's for the others
    failed = np.flatnonzero(lb.status == SP_DOC_ERR_OUTPUT)
    first = int(failed[0])
    assert 1024 < first < ndocs                     # (behind the first tile: what the test is there for)
    assert np.array_equal(lb.status[:first], status[:first])
    assert np.array_equal(lb.status[first:], np.where(sizes[first:] > 0, SP_DOC_ERR_OUTPUT, status[first:]))
    # every document of the prefix is the model's
    end = int(offs[first])
    assert np.array_equal(lb.doc_offsets[:first + 1], offs[:first + 1])
    assert np.array_equal(lb.lexems, lex[:end]) and np.array_equal(origseg, seg[:end])
    # every document from there on is empty, at the end of what fits
    assert np.all(lb.doc_offsets[first:] == end)


# ---- 2. failure paths
def test_bad_segment_ranges_fail_their_documents_only():
    rng = np.random.default_rng(21)
    counts = [3, 2, 5, 1, 4, 6, 2, 3, 1, 2]
    lctx = _lexer().createContext()
    b = _Batch(lctx, [_segment_text(rng, c) for c in counts])
    b.lex()
    # document 1 ends beyond the batch, document 2 descends; 0 and 3 are their neighbours, 4 is empty at the end of the batch
    dso = [0, 3, 12, 5, 8, 8]
    b.stitch(dso)
    want = b.model(dso)[1]
    assert want[3].tolist() == [0, SP_DOC_ERR_RANGE, SP_DOC_ERR_RANGE, 0, 0]
    lb, origseg = _assert_stitched(lctx, want)
    assert np.diff(lb.doc_offsets.astype(np.int64)).tolist() == [10, 0, 0, 11, 0]
    # an index far beyond anything
    dso = [0, 2, 1 << 40, 1 << 41]
    b.stitch(dso)
    want = b.model(dso)[1]
    assert want[3].tolist() == [0, SP_DOC_ERR_RANGE, SP_DOC_ERR_RANGE]
    _assert_stitched(lctx, want)


def test_a_segment_failed_by_the_lexer_fails_its_document():
    # 20 segments of 1000 one-letter words: 20 000 lexems in 40 000 bytes, more than a fresh context's lexem buffer
    # (a third of the bytes + 4096) holds; the batch is not rerun for that, so the segments that came last have SP_DOC_ERR_OUTPUT
    pieces = [b"a " * 1000] * 20
    lctx = _lexer().createContext()
    b = _Batch(lctx, pieces)
    b.lex(grow_output=False)
    dso = np.arange(0, 21, 2, dtype=np.uint64)
    b.stitch(dso)
    raw, want = b.model(dso)
    assert set(raw.status.tolist()) == {0, SP_DOC_ERR_OUTPUT}
    failed_docs = sorted(set(int(s) // 2 for s in np.flatnonzero(raw.status)))
    assert 0 < len(failed_docs) < 10
    assert np.flatnonzero(want[3]).tolist() == failed_docs and set(want[3][failed_docs].tolist()) == {SP_DOC_ERR_OUTPUT}
    lb, origseg = _assert_stitched(lctx, want)
    sizes = np.diff(lb.doc_offsets.astype(np.int64))
    assert all(sizes[d] == (0 if d in failed_docs else 2000) for d in range(10))


def test_call_order():
    rng = np.random.default_rng(23)
    lctx = _lexer().createContext()
    b = _Batch(lctx, [_segment_text(rng, 4), _segment_text(rng, 5)])
    d = b.torch.from_numpy(np.array([0, 2], np.int64)).cuda()
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):         # SP_ERR_INVALID: no batch yet
        lctx.stitchSegmentsDevice(d.data_ptr(), 1, b.stream)
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        lctx.stitchedFetch()
    b.lex()
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):         # a batch, not stitched
        lctx.stitchedFetch()
    b.stitch([0, 2])
    assert len(lctx.stitchedFetch()[0].lexems) == 9
    b.lex()                                                        # the next batch invalidates the stitched state
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        lctx.stitchedFetch()
    b.stitch([0, 1, 2])
    assert np.diff(lctx.stitchedFetch()[0].doc_offsets.astype(np.int64)).tolist() == [4, 5]


# ---- 3. end to end against the oracle
E2E = (3, 400, 30)          # seed, rules, features


def _e2e_inputs():
    """(lexer patterns, documents as lists of segments): Zipf words of a 30-word vocabulary, cut at blanks"""
    seed, _, nfeat = E2E
    vocab = synth.vocabulary(nfeat, seed)
    pats = [(i + 1, "\\b%s\\b" % w, 0, 1, "content") for i, w in enumerate(vocab)] + [(synth.DELIM, "[.]", 0, 5, "content")]
    text, offs = synth.text_documents(12, 1500, vocab, 40 + seed)
    rng = np.random.default_rng(seed)
    docs = []
    for d in range(len(offs) - 1):
        doc = text[int(offs[d]):int(offs[d + 1])]
        blanks = [i + 1 for i, c in enumerate(doc) if c == 32]
        cuts = sorted(set(int(x) for x in rng.choice(blanks, int(rng.integers(0, 9)), replace=False))) if d else []
        bounds = [0] + cuts + [len(doc)]
        segs = [doc[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
        if d == 5:
            segs = [b"", b"  "] + segs + [b""]          # empty segments around
        docs.append(segs)
    return pats, docs


_ORACLE = {}


def _e2e_oracle(with_and):
    """the oracle chain, computed once per rule set: oracle lexer per segment -> segments_model -> oracle matcher"""
    if with_and not in _ORACLE:
        pats, docs = _e2e_inputs()
        pieces = [s for d in docs for s in d]
        seg_offsets = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.uint64)
        dso = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
        ol = oracle.L1Lexer()
        synth.apply_lexer_patterns(ol, pats)
        lex, loffs = ol.matchDocs(b"".join(pieces), seg_offsets, nthreads=4)
        slex, sseg, soffs, sstatus = segments_model.stitch(lex, loffs, np.zeros(len(pieces), np.int32), dso)
        assert not sstatus.any()
        om = oracle.L2Matcher()
        synth.apply_rules(om, _e2e_rules(with_and))
        ref = om.run(segments_model.lexems5(slex, sseg), soffs, nthreads=4)
        # the case shows something: results that span segments, results wholly inside a later segment
        r = ref.results
        assert np.count_nonzero(r[:, 3] != r[:, 5]) > 0
        assert np.count_nonzero((r[:, 3] == r[:, 5]) & (r[:, 3] > 0)) > 0
        _ORACLE[with_and] = (pats, pieces, dso, (slex, sseg, soffs, sstatus), ref)
    return _ORACLE[with_and]


def _e2e_rules(with_and):
    seed, nrules, nfeat = E2E
    rules = synth.random_rules(nrules, nfeat, seed)
    if with_and:
        rules.append(("and_%d" % nrules, "and", 3, [1, 2]))     # (not a flat rule set: the general kernel)
    return rules


def _device_chain(kind):
    pats, pieces, dso, stitched, ref = _e2e_oracle(kind == 0)
    lx = spa.PatternLexerInstance()
    synth.apply_lexer_patterns(lx, pats)
    m = spa.PatternMatcherInstance()
    synth.apply_rules(m, _e2e_rules(kind == 0))
    lctx, mctx = lx.createContext(), m.createContext(result_sets=(kind == 2))
    assert mctx.kernelKind() == kind
    b = _Batch(lctx, pieces)
    b.lex()
    assert lctx.batchCounters()["failed_docs"] == 0
    st = b.stitch(dso)
    _assert_stitched(lctx, stitched)
    ndocs, nlex = len(dso) - 1, len(stitched[0])
    for _ in range(8):
        mctx.matchDocsDevice(st.d_lexems, st.d_doc_offsets, ndocs, nlex, b.stream, d_origseg=st.d_origseg)
        mc = mctx.batchCounters()
        if mc["failed_docs"] == 0:
            break
        assert set(int(x) for x in mctx.batchStatus(ndocs)) <= {0, 2, 9}
        mctx.reserveOutput(int(mc["results"] * 1.2) + 1024, int(mc["items"] * 1.2) + 1024)
        mctx.growArena()
    assert mc["failed_docs"] == 0
    return mctx.batchFetch(), ref


@pytest.mark.parametrize("kind", [1, 0])
def test_end_to_end_exact_engines(kind):
    gpu, ref = _device_chain(kind)
    assert np.array_equal(gpu.doc_offsets, ref.doc_offsets)
    assert np.array_equal(gpu.results[:, :7], ref.results[:, :7])       # firing order; item_begin is the engine's own
    assert np.array_equal(gpu.results[:, 8], ref.results[:, 8])
    assert np.array_equal(gpu.items, ref.items)
    assert np.array_equal(gpu.stats, ref.stats)
    assert not gpu.status.any()
    r = gpu.results
    assert np.count_nonzero(r[:, 3] != r[:, 5]) > 0 and np.count_nonzero((r[:, 3] == r[:, 5]) & (r[:, 3] > 0)) > 0


def test_end_to_end_result_sets():
    gpu, ref = _device_chain(2)
    assert np.array_equal(gpu.doc_offsets, ref.doc_offsets) and not gpu.status.any()
    for d in range(len(ref.doc_offsets) - 1):
        assert results_multiset(gpu, d) == results_multiset(ref, d)
    r = gpu.results
    assert np.count_nonzero(r[:, 3] != r[:, 5]) > 0 and np.count_nonzero((r[:, 3] == r[:, 5]) & (r[:, 3] > 0)) > 0


# ---- 4. matchSegmentedDocs and match.py --paragraphs
def _two_paragraphs():
    with open(os.path.join(HERE, "golden", "doc_example.json")) as f:
        case = json.load(f)
    first, second = case["text"].splitlines(keepends=True)
    # the second line in front, an empty and a blank line, then the line with the names: its results lie in segment 1
    return case, (second + "\n  \n" + first).encode()


def _oracle_listing(case, doc, tokens):
    lx, mt = oracle.L1Lexer(), oracle.L2Matcher()
    prg = rulelang.load(case["program"], lx, mt)
    text, seg_offsets, dso, posmaps = segments.segmented_batch([doc])
    assert len(seg_offsets) == 3 and posmaps[0].tolist() == [0, doc.index(b"This")]
    lex, loffs = lx.matchDocs(text, seg_offsets)
    slex, sseg, soffs, sstatus = segments_model.stitch(lex, loffs, [0, 0], dso)
    res = mt.run(segments_model.lexems5(slex, sseg), soffs)
    assert len(res.results) and np.all(res.results[:, 3] == 1)
    pn, vn = rulelang.name_tables(prg, mt)
    lines = rulelang.format_tokens(prg, doc, segments.absolute_lexems(slex, sseg, posmaps[0])) if tokens else []
    return lines + rulelang.format_results(doc, segments.absolute_records(res.results, posmaps[0]),
                                           segments.absolute_records(res.items, posmaps[0]), pn, vn, origin=case["origin"]), res


def test_match_segmented_docs_and_the_paragraphs_listing(tmp_path):
    case, doc = _two_paragraphs()
    want, ref = _oracle_listing(case, doc, tokens=True)
    # the function
    lx, mt = spa.PatternLexerInstance(), spa.PatternMatcherInstance()
    rulelang.load(case["program"], lx, mt)
    text, seg_offsets, dso, _ = segments.segmented_batch([doc, b"", doc])
    mb = spa.matchSegmentedDocs(lx.createContext(), mt.createContext(), text, seg_offsets, dso)
    assert mb.status.tolist() == [0, 0, 0] and mb.doc_offsets.tolist() == [0, len(ref.results), len(ref.results), 2 * len(ref.results)]
    for d in (0, 2):
        assert np.array_equal(mb.doc(d)[:, :7], ref.results[:, :7]) and np.array_equal(mb.doc(d)[:, 8], ref.results[:, 8])
    # a bad range comes back in the combined status
    mb = spa.matchSegmentedDocs(lx.createContext(), mt.createContext(), text, seg_offsets, [0, 2, 9])
    assert mb.status.tolist() == [0, SP_DOC_ERR_RANGE] and mb.doc_offsets.tolist() == [0, len(ref.results), len(ref.results)]
    # the command line
    prog, fn = tmp_path / "example.rul", tmp_path / "example.txt"
    prog.write_text(case["program"], encoding="utf-8")
    fn.write_bytes(doc)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert match.main(["-p", str(prog), "-K", "-o", str(case["origin"]), "--paragraphs", str(fn)]) == 0
    assert out.getvalue().splitlines() == ["%s:" % fn] + want + ["OK done"]
    # without the option nothing changes: the file is one segment
    lx, mt = oracle.L1Lexer(), oracle.L2Matcher()
    prg = rulelang.load(case["program"], lx, mt)
    lex, offs = lx.matchDocs(doc, np.array([0, len(doc)], np.uint64))
    res = mt.run(synth.lexems5(lex), offs)
    pn, vn = rulelang.name_tables(prg, mt)
    whole = rulelang.format_results(doc, res.results, res.items, pn, vn, origin=case["origin"])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert match.main(["-p", str(prog), "-o", str(case["origin"]), str(fn)]) == 0
    assert out.getvalue().splitlines() == ["%s:" % fn] + whole + ["OK done"]
