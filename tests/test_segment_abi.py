"""Segment lookups without a device (sp_match_segment_lookup, csrc/match_segment.hpp; the refusals of sp_segment_open, which checks
the tables on the host before it touches a device): the twin equals the model (tests/segment_model.py) on hand-made segments --
every block size, hits and misses at every place of a block, prefix runs --, every refusal with its message, and a status for
every malformed code with nothing written beyond what was counted.  The walks are csrc/segment_walk.h for the twin and the
device alike, so these tests speak for the device's bounds: no GPU test feeds malformed bytes."""
import ctypes
import os

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from struspattern_amd import products as P
from tests import segment_model as model
from tests import termblocks_model

M32 = (1 << 32) - 1


def test_symbols_and_signatures():
    vp, Ptr = ctypes.c_void_p, ctypes.POINTER
    for name in ("sp_segment_open", "sp_segment_from_ctx", "sp_segment_free", "sp_segment_last_error", "sp_segment_lookup_device", "sp_segment_lookup_fetch",
                 "sp_segment_lookup_free", "sp_segment_last_lookup_ms", "sp_match_segment_lookup"):
        assert name in capi.SIGNATURES and hasattr(capi.lib(), name)
    assert capi.SIGNATURES["sp_segment_open"] == (ctypes.c_int, [Ptr(capi.SpMatchTermBlocks), Ptr(capi.SpMatchPostingBlocks), Ptr(vp), ctypes.c_char_p, ctypes.c_size_t])
    assert capi.SIGNATURES["sp_segment_lookup_device"] == (ctypes.c_int, [vp, vp, vp, vp, ctypes.c_size_t, ctypes.c_uint32, vp, Ptr(capi.SpSegmentLookupDevice)])
    assert ctypes.sizeof(capi.SpSegmentSelection) == 24 and [n for n, _ in capi.SpSegmentSelection._fields_] == ["position", "handle", "doc_freq", "value_bytes", "count"]
    assert ctypes.sizeof(capi.SpSegmentPosting) == 16 and [n for n, _ in capi.SpSegmentPosting._fields_] == ["doc", "count", "npos", "reserved"]
    assert [n for n, _ in capi.SpSegmentLookup._fields_] == ["nq", "nsel", "npostings", "npositions", "nvalue_bytes", "flags", "q_first", "q_count", "q_status",
                                                             "q_sel_offsets", "selections", "sel_value_offsets", "sel_posting_offsets", "values", "postings",
                                                             "posting_position_offsets", "positions", "totals"]
    assert [n for n, _ in capi.SpSegmentLookupDevice._fields_][6:] == ["d_" + n for n, _ in capi.SpSegmentLookup._fields_[6:]]
    for name in ("open", "fromContext", "lookupDevice", "lookupFetch", "close"):
        assert hasattr(spa.Segment, name)
    for name in ("Segment", "SegmentLookup", "segmentLookup"):
        assert name in spa.__all__
    assert P.SP_LOOKUP_PREFIX == 1


def test_the_header_states_the_rule():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "strus_pattern_amd.h")) as f:
        header = f.read()
    assert "---- segment lookups:" in header and "unpinned by a reference vector" in header.split("---- segment lookups:")[1].split("THE ORDER")[0]


# ---- the twin against the model
def _both(entries, lists, queries, B=16):
    t, p = model.segment_of(entries, lists, B)
    assert t.entries() == [tuple(e) for e in entries] and p.lists() == lists          # (the library's readers give the model's input back)
    exact = model.check(spa.segmentLookup(t, p, queries), entries, lists, queries)
    prefix = model.check(spa.segmentLookup(t, p, queries, prefix=True), entries, lists, queries, prefix=True)
    return exact, prefix


def test_one_term_and_the_empty_segment():
    exact, prefix = _both([(3, b"ab", 1, 4)], [[(0, 4, [1, 9])]], [(3, b"ab"), (3, b"a"), (3, b"abc"), (3, b""), (2, b"ab"), (4, b"")])
    assert exact.q_count.tolist() == [1, 0, 0, 0, 0, 0] and exact.q_first.tolist() == [0, 0, 1, 0, 0, 1]
    assert prefix.q_count.tolist() == [1, 1, 0, 1, 0, 0] and prefix.query(3) == [(3, b"ab", 1, 4, [(0, 4, [1, 9])])]
    exact, prefix = _both([], [], [(1, b"a"), (0, b"")])
    assert exact.q_first.tolist() == [0, 0] and prefix.totals.tolist() == [0, 0, 0, 0] and prefix.posting_position_offsets.tolist() == [0]
    exact, prefix = _both([(3, b"ab", 1, 4)], [[(0, 4, [1, 9])]], [])
    assert exact.q_sel_offsets.tolist() == [0] and len(exact.selections) == 0


@pytest.mark.parametrize("B", termblocks_model.SIZES)
def test_every_block_size_every_place(B):
    entries, lists = model.numbered(70)
    exact, prefix = _both(entries, lists, model.probes(entries), B)
    assert int(exact.q_count.sum()) >= len(entries) and int(prefix.q_count.max()) >= 3


def test_value_shapes():
    long = b"b" + bytes(range(256))[56:]                # 201 bytes: a suffix varint of two bytes
    entries = [(1, b"", 1, 1), (1, b"\0", 1, 1), (1, b"\0\0", 1, 1), (1, b"\0\xff", 1, 1), (1, b"a", 1, 1), (1, b"ab", 1, 1), (1, long, 1, 1),
               (1, b"\xff", 1, 1), (1, b"\xff\xff", 1, 1), (4, b"", 1, 1), (4, b"\xff", 1, 1)]
    lists = [[(k, 1, [k + 1])] for k in range(len(entries))]
    queries = [(h, v) for h, v, _, _ in entries] + [(1, long[:200]), (1, long + b"!"), (1, b"\0\1"), (1, b"\xfe"), (1, b"\xff\xff\xff"), (2, b""), (3, b"\xff"), (4, b"\0")]
    for B in (2, 16):
        exact, prefix = _both(entries, lists, queries, B)
        assert exact.q_count.tolist()[:len(entries)] == [1] * len(entries) and exact.q_count.tolist()[len(entries):] == [0] * 8
        assert prefix.q_count.tolist()[0] == 9 and prefix.q_count.tolist()[9] == 2          # the empty query selects the whole handle
        assert prefix.query(len(entries))[0][1] == long                                     # a proper prefix of 200 bytes finds it


def test_prefix_runs_across_blocks_and_wide_lists():
    entries = [(1, b"a%02d" % k, 1, 1) for k in range(5)] + [(2, b"run%03d" % k, 1, 1) for k in range(40)] + [(7, b"z", 200, 200)]
    lists = [[(k, 1, [k])] for k in range(45)] + [[(300 * d, 130 if d == 5 else 1, [7, 7 + 16384] if d == 5 else [d]) for d in range(200)]]
    queries = [(2, b"run"), (2, b""), (2, b"run01"), (7, b""), (7, b"z"), (1, b"a0"), (2, b"rux"), (3, b"")] * 2
    exact, prefix = _both(entries, lists, queries, 16)
    assert prefix.q_count.tolist()[:8] == [40, 40, 10, 1, 1, 5, 0, 0] and prefix.q_first.tolist()[3] + 1 == len(entries)
    assert len(prefix.query(3)[0][4]) == 200 and prefix.query(4)[0][4][5] == (1500, 130, [7, 16391])


# ---- refusals
def _raw_open(t, p, damage=None):
    keep = []
    t = spa.MatchTermBlocks(t.bytes.copy(), t.block_offsets.copy(), t.block_handles.copy(), t.totals, t.ndict, t.block_entries)    # (a damage writes into the arrays)
    p = spa.MatchPostingBlocks(p.bytes.copy(), p.block_offsets.copy(), p.totals, p.ndict, p.block_entries)
    ct, cp = P._to_c(t, keep), P._to_c(p, keep)
    if damage:
        damage(ct, cp)
    h, err = ctypes.c_void_p(0x77), ctypes.create_string_buffer(256)
    rc = capi.lib().sp_segment_open(ctypes.byref(ct), ctypes.byref(cp), ctypes.byref(h), err, 256)
    out, err2 = capi.SpSegmentLookup(), ctypes.create_string_buffer(256)
    handles, offsets = (ctypes.c_uint32 * 1)(1), (ctypes.c_uint64 * 2)(0, 0)
    rc2 = capi.lib().sp_match_segment_lookup(ctypes.byref(ct), ctypes.byref(cp), handles, offsets, None, 1, 0, ctypes.byref(out), err2, 256)
    assert not out.q_first and not out.selections and out.nq == 0
    assert rc2 == rc and err2.value == err.value and not h.value        # (the twin refuses what open refuses, with the same words)
    return rc, err.value.decode()


def test_open_refuses_tables_that_are_not_one_segment():
    entries, lists = model.numbered(40)
    t, p = model.segment_of(entries, lists, 16)
    n = len(entries)

    def put(which, field, value, at=None):
        def damage(ct, cp):
            target = ct if which == "t" else cp
            if at is None:
                setattr(target, field, value)
            else:
                getattr(target, field)[at] = value
        return damage

    refusals = [
        (put("p", "ndict", n - 1), "another ndict"), (put("p", "nblocks", 2), "another ndict, nblocks"), (put("p", "block_entries", 8), "block size"),
        (lambda ct, cp: (setattr(ct, "block_entries", 3), setattr(cp, "block_entries", 3)), "not 1, 2, 4, 8, 16, 32 or 64"),
        (lambda ct, cp: (setattr(ct, "block_entries", 128), setattr(cp, "block_entries", 128)), "not 1, 2, 4, 8, 16, 32 or 64"),
        (lambda ct, cp: (setattr(ct, "ndict", 16), setattr(cp, "ndict", 16)), "not ceil"),
        (put("t", "block_offsets", int(t.block_offsets[2]) + 1, 1), "descend"), (put("p", "block_offsets", int(p.block_offsets[2]) + 1, 1), "descend"),
        (put("t", "block_offsets", int(t.block_offsets[2]), 1), "an empty block"), (put("p", "block_offsets", int(p.block_offsets[1]), 2), "an empty block"),
        (put("t", "nbytes", len(t.bytes) - 1), "do not end at nbytes"), (put("p", "nbytes", len(p.bytes) + 1), "do not end at nbytes"),
        (put("t", "block_offsets", 1, 0), "do not start at 0"),
        (put("t", "block_handles", int(t.block_handles[2]) + 1, 1), "block handles that descend"),
    ]
    for damage, words in refusals:
        rc, message = _raw_open(t, p, damage)
        assert rc == -1 and words in message, (words, message)
    with pytest.raises(spa.PatternError, match="another ndict"):
        spa.Segment.open(t, spa.MatchPostingBlocks(p.bytes, p.block_offsets, p.totals, p.ndict - 1, 16))


def test_the_twin_refuses_bad_queries():
    t, p = model.segment_of(*model.numbered(5))
    keep = []
    ct, cp = P._to_c(t, keep), P._to_c(p, keep)
    out, err = capi.SpSegmentLookup(), ctypes.create_string_buffer(256)
    handles, data = (ctypes.c_uint32 * 2)(1, 1), ctypes.create_string_buffer(b"abcd")
    call = capi.lib().sp_match_segment_lookup
    assert call(ctypes.byref(ct), ctypes.byref(cp), handles, (ctypes.c_uint64 * 3)(0, 3, 2), ctypes.addressof(data), 2, 0, ctypes.byref(out), err, 256) == -1 and b"descend" in err.value
    assert call(ctypes.byref(ct), ctypes.byref(cp), handles, (ctypes.c_uint64 * 3)(0, 1, 2), ctypes.addressof(data), 2, 2, ctypes.byref(out), err, 256) == -1 and b"flags" in err.value
    assert call(ctypes.byref(ct), ctypes.byref(cp), handles, (ctypes.c_uint64 * 3)(0, 1, 2), None, 2, 0, ctypes.byref(out), err, 256) == -1 and b"bytes" in err.value
    assert call(None, ctypes.byref(cp), handles, (ctypes.c_uint64 * 3)(0, 1, 2), ctypes.addressof(data), 2, 0, ctypes.byref(out), err, 8) == -1 and err.value == b"no term"
    # offsets that do not start at 0 are offsets into the caller's bytes
    assert call(ctypes.byref(ct), ctypes.byref(cp), handles, (ctypes.c_uint64 * 3)(1, 2, 4), ctypes.addressof(data), 2, 0, ctypes.byref(out), err, 256) == 0 and out.nq == 2
    capi.lib().sp_segment_lookup_free(ctypes.byref(out))


# ---- malformed bytes: a status, and nothing beyond what was counted
def _hand(term_blocks, posting_blocks, handles, ndict, B):
    """a segment of blocks given as bytes"""
    t_off, p_off = np.cumsum([0] + [len(b) for b in term_blocks]), np.cumsum([0] + [len(b) for b in posting_blocks])
    tb, pb = b"".join(term_blocks), b"".join(posting_blocks)
    t = spa.MatchTermBlocks(np.frombuffer(tb, np.uint8).copy(), t_off.astype(np.uint64), np.array(handles, np.uint32), np.array([len(handles), len(tb), B, 0], np.uint64), ndict, B)
    p = spa.MatchPostingBlocks(np.frombuffer(pb, np.uint8).copy(), p_off.astype(np.uint64), np.array([len(handles), len(pb), B, 0], np.uint64), ndict, B)
    return t, p


GOOD_TERMS = b"\0\0\2\1\1ab" + b"\0\1\1\1\1c"        # (1, "ab"), (1, "ac")
GOOD_LISTS = b"\4\0\1\1\1" + b"\x09\2\3\2\5\4\2\1\1\1"


def _consistent(got):
    """the arrays are as long as the totals say, and the offsets end there"""
    nsel, npostings, npositions, nvalues = got.totals.tolist()
    assert len(got.selections) == nsel == int(got.q_sel_offsets[-1]) == int(got.q_count.sum())
    assert len(got.postings) == npostings == int(got.sel_posting_offsets[-1]) and len(got.values) == nvalues == int(got.sel_value_offsets[-1])
    assert len(got.positions) == npositions == int(got.posting_position_offsets[-1])
    assert (np.diff(got.sel_value_offsets.astype(np.int64)) >= 0).all() and (np.diff(got.sel_posting_offsets.astype(np.int64)) >= 0).all()


def test_the_good_hand_made_block():
    t, p = _hand([GOOD_TERMS], [GOOD_LISTS], [1], 2, 16)
    got = spa.segmentLookup(t, p, [(1, b"ac"), (1, b"ab")])
    assert got.q_status.tolist() == [0, 0] and got.query(0) == [(1, b"ac", 1, 1, [(2, 3, [5, 9]), (4, 1, [1])])] and got.query(1) == [(1, b"ab", 1, 1, [(0, 1, [1])])]


MALFORMED_TERMS = [
    (b"\0\0\2\1\1ab" + b"\0\1\1\1\x80", 1), (b"\0\0\2\1", 1),                                   # a varint past the block
    (b"\0\0\2\1" + b"\x80" * 10 + b"\1ab", 1), (b"\0\0\2\1" + b"\xff" * 9 + b"\2ab", 1),        # longer than ten bytes, more than 64 bits
    (b"\0\1\1\1\1b", 2), (b"\1\0\1\1\1b", 2),                                                   # a head that is not in full
    (b"\0\0\2\1\1ab" + b"\0\3\1\1\1c", 3),                                                      # shared above the length before
    (b"\0\0\2\1\1ab" + b"\0\1\5\1\1c", 4), (b"\0\0\7\1\1ab", 4),                                # a suffix past the block
    (b"\0\0\2\1\1ab" + b"\xff\xff\xff\xff\x0f\1\1\1\1c", 8),                                    # a handle that leaves 32 bits
    (b"\0\0\2\1\1ab" + b"\xff" * 9 + b"\1\1\1\1\1c", 8),                                           # ... and 64
    (b"\0\0\2\xff\xff\xff\xff\x1f\1ab" + b"\0\1\1\1\1c", 8),                                    # a doc_freq that does
]


@pytest.mark.parametrize("terms,status", MALFORMED_TERMS)
@pytest.mark.parametrize("prefix", [False, True])
def test_a_malformed_term_code_ends_the_query(terms, status, prefix):
    t, p = _hand([terms], [GOOD_LISTS], [1], 2, 16)
    got = spa.segmentLookup(t, p, [(1, b"ac"), (1, b"zz")], prefix=prefix)
    assert got.q_status.tolist() == [status, status] and got.q_count.tolist() == [0, 0] and got.q_first.tolist() == [0, 0]
    assert got.totals.tolist() == [0, 0, 0, 0]
    _consistent(got)


MALFORMED_LISTS = [
    (b"\4\0\1\1\x80", 1), (b"\x80", 1), (b"\x80" * 10 + b"\1\0\1\1\1", 1), (b"\xff" * 9 + b"\2\0\1\1\1", 1),
    (b"\5\0\1\1\1", 5), (b"\0", 5), (b"\3\0\1\1\1", 5), (b"\2\0\1\1\1", 1),                   # a body past the block, of 0, a posting beyond it
    (b"\x08\2\1\1\5\0\1\1\1", 6), (b"\5\0\2\2\5\0", 6),                                       # a ddelta of 0, a gap of 0
    (b"\3\0\1\0", 7), (b"\5\0\1\2\5\1", 7),                                                   # npos 0, npos above the count
    (b"\x08\xff\xff\xff\xff\x1f\1\1\1", 8), (b"\x08\0\xff\xff\xff\xff\x1f\1\1", 8), (b"\x08\0\1\1\xff\xff\xff\xff\x1f", 8),
    (b"\x09\0\2\2\xff\xff\xff\xff\x0f\1", 8),
]


@pytest.mark.parametrize("code,status", MALFORMED_LISTS)
def test_a_malformed_list_empties_its_selection(code, status):
    """block 1 is sound, the lists of block 0 are malformed: as the list looked for, and as the list to skip in front of it"""
    for bad_first in (True, False):
        lists0 = code + b"\4\0\1\1\1" if bad_first else b"\4\0\1\1\1" + code
        t, p = _hand([GOOD_TERMS, b"\0\0\1\1\1b"], [lists0, b"\4\7\2\1\3"], [1, 1], 3, 2)
        for prefix in (False, True):
            got = spa.segmentLookup(t, p, [(1, b"b"), (1, b"ac"), (1, b"ab"), (1, b"")], prefix=prefix)
            _consistent(got)
            assert got.q_status[0] == 0 and got.query(0) == [(1, b"b", 1, 1, [(7, 2, [3])])]
            assert got.q_count.tolist() == [1, 1, 1, 3 if prefix else 0]
            if bad_first:
                # looked for with a sound list behind it: a status, whichever; "ac" skips it by its `body` where that holds
                assert int(got.q_status[2]) != 0 and got.query(2) == [(0, b"", 0, 0, [])] and got.selections[2].tolist() == [0, 0, 0, 0, 0, 0]
                assert got.query(1) in ([(0, b"", 0, 0, [])], [(1, b"ac", 1, 1, [(0, 1, [1])])]) and (int(got.q_status[1]) != 0) == (got.query(1)[0][2] == 0)
            else:
                assert int(got.q_status[1]) == status and got.query(1) == [(0, b"", 0, 0, [])] and got.selections[1].tolist() == [1, 0, 0, 0, 0, 0]
                assert int(got.q_status[2]) == 0 and got.query(2) == [(1, b"ab", 1, 1, [(0, 1, [1])])]
            if prefix:
                assert int(got.q_status[3]) == max(int(got.q_status[1]), int(got.q_status[2])) != 0 and got.query(3)[2] == (1, b"b", 1, 1, [(7, 2, [3])])
                assert got.query(3)[:2] == got.query(2) + got.query(1)


def test_blocks_that_leave_the_bytes_are_refused_not_read():
    t, p = _hand([GOOD_TERMS], [GOOD_LISTS], [1], 2, 16)
    short = spa.MatchTermBlocks(t.bytes[:-1], t.block_offsets, t.block_handles, t.totals, 2, 16)
    with pytest.raises(spa.PatternError, match="do not end at nbytes"):
        spa.segmentLookup(short, p, [(1, b"ab")])
