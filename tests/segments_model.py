"""Numpy statement of the stitch of segmented documents ("Segmented documents"; the definition the device
passes of csrc/l1_stitch.h are checked against).

Input: the lexer's output for the segments, as PatternLexerContext.batchFetch returns it -- lexems (n,4) u32
[id, ordpos, origpos, origsize] grouped by segment, seg_offsets (nseg+1,) u64, seg_status (nseg,) i32 (a failed segment has
an empty range) -- and doc_seg_offsets (ndocs+1,) u64: document d consists of the segments
[doc_seg_offsets[d], doc_seg_offsets[d+1]).

The rule, for the s-th segment of a document (s counts every segment from 0, empty ones included):
    (id, ordpos, origpos, origsize) -> (id, ordpos + base_s, origpos, origsize), origseg = s
    base_0 = 0;  base_{s+1} = stitched ordpos of the last lexem of segment s, or base_s if segment s has no lexems
A document fails (status != 0, no lexems) when a segment of it failed in the lexer (status of its first failing segment),
when its segment range ends beyond the batch or descends (RANGE), or when a stitched ordpos or its lexem count does not fit
32 bits (RANGE); in that order.  This is the caller loop of the reference's command-line tool
(`ordposOffset = lexems.back().ordpos()`), which lives outside the reference repository: unpinned by a reference vector."""
import numpy as np

SP_DOC_ERR_RANGE = 5
MAX32 = 0xFFFFFFFF


def _ranges(starts, counts):
    """concatenation of arange(starts[i], starts[i] + counts[i])"""
    starts = np.asarray(starts, np.int64)
    counts = np.asarray(counts, np.int64)
    total = int(counts.sum())
    if total == 0:
        return np.zeros(0, np.int64)
    owner = np.repeat(np.arange(len(counts)), counts)
    first = np.cumsum(counts) - counts
    return starts[owner] + (np.arange(total, dtype=np.int64) - first[owner])


def stitch(lexems, seg_offsets, seg_status, doc_seg_offsets):
    """-> (lexems (m,4) u32, origseg (m,) u32, doc_offsets (ndocs+1,) u64, status (ndocs,) i32)"""
    lexems = np.ascontiguousarray(lexems, dtype=np.uint32).reshape(-1, 4)
    seg_offsets = np.asarray(seg_offsets, np.uint64)
    seg_status = np.asarray(seg_status, np.int32)
    dso = np.asarray(doc_seg_offsets, np.uint64)
    nseg, ndocs = len(seg_offsets) - 1, len(dso) - 1
    s0, s1 = dso[:-1], dso[1:]
    status = np.zeros(ndocs, np.int32)
    in_range = (s0 <= s1) & (s1 <= np.uint64(nseg))
    status[~in_range] = SP_DOC_ERR_RANGE
    a = np.where(in_range, s0, 0).astype(np.int64)
    b = np.where(in_range, s1, 0).astype(np.int64)
    # the first failing segment of every document
    bad = np.flatnonzero(seg_status != 0)
    if len(bad):
        at = np.searchsorted(bad, a)
        first_bad = bad[np.minimum(at, len(bad) - 1)]
        failed = in_range & (at < len(bad)) & (first_bad < b)
        status[failed] = seg_status[first_bad[failed]]
    # lexem counts and last ordinal positions of the segments, and their running sums over the batch, in 64 bits
    cnt = (seg_offsets[1:] - seg_offsets[:-1]).astype(np.int64)
    cnt[seg_status != 0] = 0
    last = np.zeros(nseg, np.uint64)
    nonempty = cnt > 0
    last[nonempty] = lexems[(seg_offsets[1:].astype(np.int64) - 1)[nonempty], 1]
    ccnt = np.concatenate([[0], np.cumsum(cnt.astype(np.uint64))]).astype(np.uint64)
    cord = np.concatenate([[0], np.cumsum(last)]).astype(np.uint64)
    # candidates: the documents that have not failed so far; their segments, in order
    cand = np.flatnonzero(status == 0)
    segs = _ranges(a[cand], b[cand] - a[cand])
    seg_doc = np.repeat(cand, b[cand] - a[cand])
    seg_base = cord[segs] - cord[a[seg_doc]]
    seg_local = segs - a[seg_doc]
    idx = _ranges(seg_offsets[:-1].astype(np.int64)[segs], cnt[segs])
    lex_seg = np.repeat(np.arange(len(segs)), cnt[segs])
    ordpos = lexems[idx, 1].astype(np.uint64) + seg_base[lex_seg]
    count = ccnt[b] - ccnt[a]
    over = np.zeros(ndocs, bool)
    np.logical_or.at(over, seg_doc[lex_seg], ordpos > np.uint64(MAX32))
    over |= count > np.uint64(MAX32)
    status[(status == 0) & over] = SP_DOC_ERR_RANGE
    keep = status[seg_doc[lex_seg]] == 0
    out = lexems[idx[keep]].copy()
    out[:, 1] = ordpos[keep].astype(np.uint32)
    origseg = seg_local[lex_seg][keep].astype(np.uint32)
    doc_offsets = np.zeros(ndocs + 1, np.uint64)
    doc_offsets[1:] = np.cumsum(np.where(status == 0, count, 0).astype(np.uint64))
    return out, origseg, doc_offsets, status


def lexems5(lexems, origseg):
    """(n,4) + origseg -> (n,5) [id, ordpos, origseg, origpos, origsize], the input of oracle.L2Matcher.run"""
    out = np.zeros((len(lexems), 5), np.uint32)
    out[:, 0] = lexems[:, 0]
    out[:, 1] = lexems[:, 1]
    out[:, 2] = origseg
    out[:, 3] = lexems[:, 2]
    out[:, 4] = lexems[:, 3]
    return out
