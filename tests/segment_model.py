"""The lookup rule of include/strus_pattern_amd.h ("segment lookups") in plain Python: the yardstick of the device-free twin
(sp_match_segment_lookup) and, through it, of the device passes.  Written from the header text, not from the C++: answers queries
from the decoded segment -- MatchTermBlocks.entries() and MatchPostingBlocks.lists() -- by going through all of it.  And what
the CPU tests and the GPU tests of the lookups share: hand-made segments and the comparison of two lookups."""
import numpy as np

import struspattern_amd as spa
from struspattern_amd import products as P
from tests import postingblocks_model, termblocks_model

ARRAYS = tuple(a.attr for a in P.SegmentLookup._ARRAYS)


def runs(entries, queries, prefix=False):
    """per query (first, count): `first` the number of entries below (handle, value) -- bytes compare as memcmp does, a prefix
    before what it is a prefix of, which is Python's order --, the run from there on whose handle is the query's and whose value
    equals its bytes, or starts with them"""
    out = []
    for h, q in queries:
        h, q = int(h), bytes(q)
        first = sum(1 for e in entries if (int(e[0]), bytes(e[1])) < (h, q))
        k = first
        while k < len(entries) and int(entries[k][0]) == h and (bytes(entries[k][1]).startswith(q) if prefix else bytes(entries[k][1]) == q):
            k += 1
        out.append((first, k - first))
    return out


def lookup(entries, lists, queries, prefix=False):
    """per query [(handle, value, doc_freq, count, [(doc, count, [positions])])]: what SegmentLookup.query(i) must give"""
    return [[(int(entries[k][0]), bytes(entries[k][1]), int(entries[k][2]), int(entries[k][3]), [(d, c, list(p)) for d, c, p in lists[k]])
             for k in range(first, first + count)] for first, count in runs(entries, queries, prefix)]


def check(got, entries, lists, queries, prefix=False):
    """the SegmentLookup `got` is what the model says, and its arrays are laid out as the header says"""
    queries = list(queries)
    want_runs, want = runs(entries, queries, prefix), lookup(entries, lists, queries, prefix)
    nq, nsel = len(queries), sum(c for _, c in want_runs)
    assert got.q_first.tolist() == [f for f, _ in want_runs] and got.q_count.tolist() == [c for _, c in want_runs]
    assert got.q_status.tolist() == [0] * nq and got.flags == (P.SP_LOOKUP_PREFIX if prefix else 0)
    assert got.q_sel_offsets.tolist() == np.concatenate(([0], np.cumsum([c for _, c in want_runs], dtype=np.int64))).astype(np.int64).tolist()
    assert [got.query(i) for i in range(nq)] == want
    flat = [sel for found in want for sel in found]
    postings = [p for sel in flat for p in sel[4]]
    assert len(got.selections) == nsel == len(flat)
    assert got.selections[:, 0].tolist() == [k for f, c in want_runs for k in range(f, f + c)]
    assert got.selections[:, 3].tolist() == [len(sel[1]) for sel in flat]
    assert got.sel_value_offsets.tolist() == np.concatenate(([0], np.cumsum([len(sel[1]) for sel in flat], dtype=np.int64))).astype(np.int64).tolist()
    assert got.sel_posting_offsets.tolist() == np.concatenate(([0], np.cumsum([len(sel[4]) for sel in flat], dtype=np.int64))).astype(np.int64).tolist()
    assert got.values.tobytes() == b"".join(sel[1] for sel in flat)
    assert got.postings.tolist() == [[d, c, len(p), 0] for d, c, p in postings]
    assert got.posting_position_offsets.tolist() == np.concatenate(([0], np.cumsum([len(p) for _, _, p in postings], dtype=np.int64))).astype(np.int64).tolist()
    assert got.positions.tolist() == [x for _, _, p in postings for x in p]
    assert got.totals.tolist() == [nsel, len(postings), len(got.positions), len(got.values)]
    return got


def assert_same(a, b):
    """two lookups are the same arrays, byte by byte"""
    for name in ARRAYS:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, x, y)
    assert a.flags == b.flags


def segment_of(entries, lists, B=16):
    """the MatchTermBlocks and the MatchPostingBlocks of a sorted dictionary made by hand, coded by the two models.  entries: per
    sorted position (handle, value bytes, doc_freq, count); lists: per sorted position [(doc, count, [distinct positions])]"""
    assert len(entries) == len(lists)
    t, p = termblocks_model.term_blocks(entries, B), postingblocks_model.posting_blocks(lists, B)
    return (spa.MatchTermBlocks(t.bytes, t.block_offsets, t.block_handles, t.totals, t.ndict, B),
            spa.MatchPostingBlocks(p.bytes, p.block_offsets, p.totals, p.ndict, B))


def numbered(n, handles=(1, 2, 5)):
    """a sorted dictionary of n entries over `handles` with values that share prefixes, and a list per entry: entry k lies in
    1 + k % 3 documents"""
    pairs = sorted({(handles[k % len(handles)], b"t%02d" % (k // 7) + b"x" * (k % 4) + (b"%d" % k if k % 5 else b"")) for k in range(n)})
    entries = [(h, v, 1 + k % 3, 2 + k) for k, (h, v) in enumerate(pairs)]
    lists = [[(4 * d + k % 3, 1 + (k + d) % 3, [1 + k + 2 * i for i in range(1 + (k + d) % 3)]) for d in range(1 + k % 3)] for k in range(len(pairs))]
    return entries, lists


def probes(entries):
    """queries around a sorted dictionary: every entry, and per entry a proper prefix, an extension, a neighbour below and above,
    a handle without entries; the same query twice"""
    out = []
    for h, v, _, _ in entries:
        out += [(h, v), (h, v[:-1]), (h, v + b"\0"), (h, v + b"\xff"), (h, v[:1])]
        if v:
            out.append((h, v[:-1] + bytes([max(v[-1] - 1, 0)])))
    handles = sorted({e[0] for e in entries})
    out += [(0, b""), (0, b"a"), (handles[-1] + 1, b""), (handles[-1] + 7, b"zz"), (handles[0], b""), (handles[-1], b"\xff\xff\xff")]
    out += [(h + 1, b"t") for h in handles if h + 1 not in handles]
    return out + out[:2]
