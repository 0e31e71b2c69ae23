"""Posting blocks without a device (sp_match_batch_posting_blocks, sp_match_posting_blocks_decode_block,
csrc/match_postingblocks.hpp): the twin equals the model (tests/postingblocks_model.py) and decodes to the lists on hand-made
dictionaries, orders, postings and positions -- every block size of the switch, varints at their edges --, every refusal of the
twin and of the reader with its message, and the struct round trip of MatchPostingBlocks.  What an occurrence adds to a code is
composed by csrc/posting_block_code.h for the twin and the device alike, so these tests speak for the device's encoder on values
that no small batch reaches on a GPU."""
import ctypes
import os

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from struspattern_amd import products as P
from tests import postingblocks_cases as cases
from tests import postingblocks_model as model
from tests.postingblocks_cases import Hand

M32 = (1 << 32) - 1


def test_symbols_and_signatures():
    vp, Ptr = ctypes.c_void_p, ctypes.POINTER
    for name in ("sp_matcher_ctx_finished_posting_blocks_device", "sp_matcher_ctx_finished_posting_blocks_fetch", "sp_match_posting_blocks_free",
                 "sp_matcher_ctx_last_posting_blocks_ms", "sp_match_batch_posting_blocks", "sp_match_posting_blocks_decode_block"):
        assert name in capi.SIGNATURES and hasattr(capi.lib(), name)
    assert capi.SIGNATURES["sp_matcher_ctx_finished_posting_blocks_device"] == (ctypes.c_int, [vp, vp, Ptr(capi.SpMatchPostingBlocksDevice)])
    assert capi.SIGNATURES["sp_match_batch_posting_blocks"][1][:5] == [Ptr(capi.SpMatchDictionary), Ptr(capi.SpMatchDictionaryOrder), Ptr(capi.SpMatchPostings),
                                                                       Ptr(capi.SpMatchPositions), Ptr(capi.SpMatchPostingBlocks)]
    assert [n for n, _ in capi.SpMatchPostingBlocksDevice._fields_] == ["ndict", "nblocks", "nbytes", "block_entries", "d_bytes", "d_block_offsets", "d_totals"]
    assert [n for n, _ in capi.SpMatchPostingBlocks._fields_] == ["ndict", "nblocks", "nbytes", "block_entries", "bytes", "block_offsets", "totals"]
    assert [n for n, _ in capi.SpBlockPosting._fields_] == ["doc", "count", "npos", "reserved", "position_offset"] and ctypes.sizeof(capi.SpBlockPosting) == 24
    for name in ("finishedPostingBlocksDevice", "finishedPostingBlocksFetch", "lastPostingBlocksMs"):
        assert hasattr(spa.PatternMatcherContext, name)
    for name in ("MatchPostingBlocks", "batchPostingBlocks"):
        assert name in spa.__all__
    assert ("PostingBlocks", ("DictionaryOrder", "Positions")) in spa._SEGMENT_PRODUCTS


def test_the_header_states_the_rule():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "strus_pattern_amd.h")) as f:
        header = f.read()
    assert "---- posting blocks:" in header and "unpinned by a reference vector" in header.split("---- posting blocks:")[1].split("INPUT:")[0]


# ---- the twin against the model, the reader and postings(k)
def test_one_term_once_and_its_literal_bytes():
    got = Hand([[(0, 1, [1])]]).check()
    assert bytes(got.bytes) == b"\4\0\1\1\1" and got.block_offsets.tolist() == [0, 5] and got.totals.tolist() == [1, 5, 16, 1]
    assert got.postings(0) == [(0, 1, [1])]
    got = Hand([]).check()
    assert got.block_offsets.tolist() == [0] and len(got.bytes) == 0 and got.totals.tolist() == [0, 0, 16, 0]
    with pytest.raises(spa.PatternError):
        got.postings(0)


def test_lists_in_sorted_order_with_repeated_positions():
    x = Hand([[(2, 3, [5, 5, 9]), (4, 1, [1])], [(0, 2, [7, 7])], [(1, 1, [0]), (200, 2, [3, 300])]], order=[2, 0, 1])
    got = x.check()
    assert bytes(got.bytes) == (b"\x0b\1\1\1\0" + b"\xc7\1\2\2\3\xa9\2") + (b"\x09\2\3\2\5\4" + b"\2\1\1\1") + b"\4\0\2\1\7"
    assert [got.postings(k) for k in range(3)] == x.want() == [[(1, 1, [0]), (200, 2, [3, 300])], [(2, 3, [5, 9]), (4, 1, [1])], [(0, 2, [7])]]
    assert int(got.totals[3]) == int(x.positions.totals[1]) == 7


@pytest.mark.parametrize("B", model.SIZES)
def test_every_block_size(B):
    x = Hand(cases.numbered(150))
    got = x.check(B)
    assert got.block_entries == B and int(got.totals[2]) == B and len(got.block_offsets) - 1 == (150 + B - 1) // B
    for k in (0, B - 1, B, 149):
        assert got.postings(k) == x.want()[k]


@pytest.mark.parametrize("B", [4, 16])
def test_ndict_at_the_block_edges(B):
    for n in (1, B - 1, B, B + 1, 3 * B + 1):
        got = Hand(cases.numbered(n)).check(B)
        assert got.ndict == n and len(model.decode_block(got, (n - 1) // B)) == (n - 1) % B + 1


def test_wide_varints():
    """values that no batch on a GPU reaches: a count of 2^32 - 1 with a small npos, documents and positions near 2^32 - 1, gaps
    at the varint edges"""
    gaps = [127, 128, 16383, 16384, 1 << 21, 1 << 28]
    pos = np.cumsum([5] + gaps).tolist()
    x = Hand([[(M32 - 1, M32, [M32 - 1, M32 - 1, M32]), (M32, 2, [M32])], [(3, len(pos), pos)], [(126, 1, [127]), (254, 1, [128]), (254 + 16384, 1, [16383])]])
    got = x.check()
    assert got.lists() == [[(126, 1, [127]), (254, 1, [128]), (16638, 1, [16383])], [(3, 7, pos)], [(M32 - 1, M32, [M32 - 1, M32]), (M32, 2, [M32])]]
    code = model.list_code(x.want()[1])
    assert code[1:5] == b"\3\7\7\5" and code[5:] == b"\x7f" + b"\x80\1" + b"\xff\x7f" + b"\x80\x80\1" + b"\x80\x80\x80\1" + b"\x80\x80\x80\x80\1"
    assert model.list_code(x.want()[2])[:11] == b"\x19" + b"\xfe\xff\xff\xff\x0f" + b"\xff\xff\xff\xff\x0f"
    assert [len(model.varint(n)) for n in (127, 128, 16383, 16384, 1 << 21, 1 << 28, M32)] == [1, 2, 2, 3, 4, 5, 5]


@pytest.mark.parametrize("body", [127, 128, 16383, 16384])
def test_a_body_at_the_varint_edges(body):
    """postings of four bytes each (ddelta, count, npos and a position below 128) and one that fills the rest"""
    n, rest = divmod(body - 4, 4)
    entry = [(d, 1, [9]) for d in range(1, n + 1)]
    last = {0: [(n + 1, 1, [9])], 1: [(n + 1, 1, [128])], 2: [(n + 1, 1, [16384])], 3: [(n + 1, 1, [1 << 21])]}[rest]
    x = Hand([entry + last, [(5, 1, [1])]])
    got = x.check()
    assert int(got.block_offsets[1]) == 5 + body + len(model.varint(body)) and bytes(got.bytes[5:5 + len(model.varint(body))]) == model.varint(body)


# ---- the twin's refusals
def _raw(x, damage=None, null=()):
    """sp_match_batch_posting_blocks over C structs made of the Hand x; damage(d, o, q, p) may change them, `null` names the
    arguments passed as NULL.  Returns (rc, message)."""
    keep = []
    d = P._to_c(spa.MatchDictionary(x.d.records.copy(), x.d.term_dict, x.d.doc_offsets, x.d.handle_terms), keep)
    o = P._to_c(spa.MatchDictionaryOrder(x.order.order.copy(), x.order.rank, x.order.prefix_bytes, x.order.handle_offsets), keep)
    q = P._to_c(spa.MatchPostings(x.postings.records.copy(), x.postings.entry_offsets.copy(), x.postings.record_posting), keep)
    p = P._to_c(spa.MatchPositions(x.positions.occurrences.copy(), x.positions.posting_offsets.copy(), x.positions.posting_positions.copy(), x.positions.totals), keep)
    if damage:
        damage(d, o, q, p)
    args = {"dict": d, "order": o, "postings": q, "positions": p}
    out = capi.SpMatchPostingBlocks()
    out.ndict = 77                                      # (the call clears `out` first)
    err = ctypes.create_string_buffer(256)
    rc = capi.lib().sp_match_batch_posting_blocks(*[None if k in null else ctypes.byref(a) for k, a in args.items()], ctypes.byref(out), err, 256)
    if rc == 0:
        assert out.ndict == len(x.d.records) and out.nblocks == out.totals[0] and out.nbytes == out.totals[1] and out.bytes and out.block_offsets
        capi.lib().sp_match_posting_blocks_free(ctypes.byref(out))
    assert not out.bytes and not out.block_offsets and out.ndict == out.nblocks == out.nbytes == 0 and out.totals[1] == 0
    return rc, err.value.decode()


def _put(which, field, value, at=None):
    def damage(d, o, q, p):
        target = {"d": d, "o": o, "q": q, "p": p}[which]
        if at is None:
            setattr(target, field, value)
        elif isinstance(at, tuple):
            setattr(getattr(target, field)[at[0]], at[1], value)
        else:
            getattr(target, field)[at] = value
    return damage


# the refusal input: entry 0 = [(2, 3, [5, 5, 9]), (4, 1, [1])], entry 1 = [(0, 2, [7, 7])]: postings 0 1 2, occurrences 0..5
REFUSED = [
    ("the order is not that of the dictionary", _put("o", "ndict", 1)),
    ("the postings are not those of the dictionary", _put("q", "ndict", 1)),
    ("the positions are not those of the postings", _put("p", "nterms", 2)),
    ("not a permutation", _put("o", "order", 0, at=0)),
    ("not a permutation", _put("o", "order", 2, at=0)),
    ("entry offsets that do not cover the postings", _put("q", "entry_offsets", 2, at=2)),
    ("entry offsets that do not ascend", _put("q", "entry_offsets", 4, at=1)),
    ("a doc_freq that is not the length of its list", _put("d", "records", 1, at=(0, "doc_freq"))),
    ("posting offsets that do not cover the occurrences", _put("p", "posting_offsets", 5, at=3)),
    ("posting offsets that do not ascend", _put("p", "posting_offsets", 7, at=1)),
    ("a posting with a count of 0", _put("q", "postings", 0, at=(1, "count"))),
    ("a posting without an occurrence", _put("p", "posting_offsets", 3, at=2)),
    ("documents that do not ascend inside a list", _put("q", "postings", 2, at=(1, "doc"))),
    ("documents that do not ascend inside a list", _put("q", "postings", 1, at=(1, "doc"))),
    ("positions that do not ascend inside a posting", _put("p", "occurrences", 4, at=(2, "ordpos"))),
    ("a posting_positions that is 0 or above the count", _put("p", "posting_positions", 0, at=0)),
    ("a posting_positions that is 0 or above the count", _put("p", "posting_positions", 4, at=0)),
    ("a posting_positions that is 0 or above the count", _put("p", "posting_positions", 2, at=1)),
    ("not the number of distinct positions", _put("p", "posting_positions", 3, at=0)),
    ("not the number of distinct positions", _put("p", "posting_positions", 2, at=2)),
]


def _refusal_inputs():
    return Hand([[(2, 3, [5, 5, 9]), (4, 1, [1])], [(0, 2, [7, 7])]])


@pytest.mark.parametrize("message,damage", REFUSED, ids=["%02d %s" % (k, m[:40]) for k, (m, _) in enumerate(REFUSED)])
def test_refusals_with_their_message(message, damage):
    x = _refusal_inputs()
    assert _raw(x) == (0, "")
    rc, msg = _raw(x, damage)
    assert rc == -1 and message in msg, msg
    assert _raw(x) == (0, "")                           # the same objects then serve a good call


def test_refused_arguments():
    x = _refusal_inputs()
    for name, message in (("dict", "no dictionary"), ("order", "no order"), ("postings", "no postings"), ("positions", "no positions")):
        rc, msg = _raw(x, null=(name,))
        assert rc == -1 and message in msg, name
    with block_entries_of(16):
        bad = Hand([[(2, 1, [5])]])
        bad.positions.posting_positions[0] = 2
        with pytest.raises(spa.PatternError, match=r"no posting blocks of the batch \(-1\): a posting_positions that is 0 or above"):
            bad.blocks()


block_entries_of = cases.block_entries


# ---- the reader
def _decode(pb, j, caps=None, query=False):
    """sp_match_posting_blocks_decode_block on block j of the MatchPostingBlocks pb: (rc, message, nlists, npostings, npositions, lists)"""
    keep = []
    s = P._to_c(pb, keep)
    nl, npo, nq, err = ctypes.c_size_t(77), ctypes.c_size_t(77), ctypes.c_size_t(77), ctypes.create_string_buffer(256)
    lcap, pcap, qcap = caps or (int(pb.block_entries), 4096, 4096)
    lists, postings, positions = (ctypes.c_uint32 * max(lcap, 1))(), (capi.SpBlockPosting * max(pcap, 1))(), (ctypes.c_uint32 * max(qcap, 1))()
    rc = capi.lib().sp_match_posting_blocks_decode_block(ctypes.byref(s), j, None if query else lists, lcap, None if query else postings, pcap,
                                                          None if query else positions, qcap, ctypes.byref(nl), ctypes.byref(npo), ctypes.byref(nq), err, 256)
    found = None
    if rc == 0 and not query:
        found, at = [], 0
        for n in lists[:nl.value]:
            found.append([(p.doc, p.count, list(positions[p.position_offset:p.position_offset + p.npos])) for p in postings[at:at + n]])
            at += n
    return rc, err.value.decode(), nl.value, npo.value, nq.value, found


def _blocks_of(data, offsets=None, B=16):
    data = bytes(data)
    offsets = [0, len(data)] if offsets is None else offsets
    return spa.MatchPostingBlocks(np.frombuffer(data, np.uint8).copy(), np.array(offsets, np.uint64), np.array([len(offsets) - 1, len(data), B, 0], np.uint64),
                                  ndict=0, block_entries=B)


def test_the_reader_decodes_a_block_from_its_own_bytes():
    x = Hand(cases.numbered(40))
    got = x.check()
    want = x.want()
    for j in range(3):
        rc, msg, nl, npo, nq, found = _decode(got, j)
        assert (rc, msg) == (0, "") and found == want[16 * j:16 * j + 16] and nl == len(found)
        assert npo == sum(len(e) for e in found) and nq == sum(len(p[2]) for e in found for p in e)
        assert _decode(got, j, query=True)[:5] == (0, "", nl, npo, nq)          # only counts
        assert got.block(j) == found
    # room that does not suffice: the counts all the same
    nl, npo, nq = _decode(got, 0, query=True)[2:5]
    for caps in ((15, npo, nq), (16, npo - 1, nq), (16, npo, nq - 1)):
        rc, msg, l, p, q, _ = _decode(got, 0, caps=caps)
        assert rc == -1 and "room" in msg and (l, p, q) == (nl, npo, nq)
    rc, msg = _decode(got, 3)[:2]
    assert rc == -1 and "no such block" in msg
    with pytest.raises(spa.PatternError, match=r"no block 3 of the posting blocks of the batch \(-1\): no such block"):
        got.block(3)


GOOD = b"\x09\2\3\2\5\4" + b"\2\1\1\1"      # [(2, 3, [5, 9]), (4, 1, [1])]
MALFORMED = [
    ("a varint that runs past the block", b"\4\0\1\1\x80"),                             # the position never ends
    ("a varint that runs past the block", b"\x80"),                                     # the body never ends
    ("longer than ten bytes", b"\x80" * 10 + b"\1\0\1\1\1"),
    ("longer than ten bytes", b"\xff" * 9 + b"\2\0\1\1\1"),                             # ten bytes, more than 64 bits
    ("a body that runs past the block", b"\5\0\1\1\1"),
    ("a body that runs past the block", b"\xff\xff\xff\xff\xff\xff\xff\xff\xff\1\0\1\1\1"),   # ... and does not wrap
    ("a body of 0", b"\0"),
    ("a posting that ends beyond its body", b"\3\0\1\1\1"),                              # the position lies behind the body
    ("a posting that ends beyond its body", b"\4\0\2\2\1" + b"\4\0\1\1\1"),              # the second position is the next list's
    ("a posting that ends beyond its body", b"\2\0\1\1\1"),                              # npos lies behind the body
    ("a ddelta of 0 behind the first posting", b"\x08\2\1\1\5" + b"\0\1\1\1"),
    ("a position gap of 0 behind the first position", b"\5\0\2\2\5\0"),
    ("an npos of 0 or above the count", b"\3\0\1\0"),
    ("an npos of 0 or above the count", b"\5\0\1\2\5\1"),
    ("leaves 32 bits", b"\x08\xff\xff\xff\xff\x1f\1\1\1"),                               # the document
    ("leaves 32 bits", b"\x0c\xff\xff\xff\xff\x0f\1\1\1" + b"\1\1\1\1"),                 # ... by its delta
    ("leaves 32 bits", b"\x08\0\xff\xff\xff\xff\x1f\1\1"),                               # the count
    ("a position that leaves 32 bits", b"\x08\0\1\1\xff\xff\xff\xff\x1f"),
    ("a position that leaves 32 bits", b"\x09\0\2\2\xff\xff\xff\xff\x0f\1"),             # ... by its gap
    ("more lists than a block holds", b"\4\0\1\1\1" * 17),
]


@pytest.mark.parametrize("message,data", MALFORMED, ids=["%02d %s" % (k, m[:40]) for k, (m, _) in enumerate(MALFORMED)])
def test_the_reader_refuses_a_malformed_block(message, data):
    rc, msg = _decode(_blocks_of(data), 0)[:2]
    assert rc == -1 and message in msg, msg


def test_the_reader_refuses_offsets_outside_the_bytes():
    assert _decode(_blocks_of(GOOD), 0)[5] == [[(2, 3, [5, 9]), (4, 1, [1])]]
    assert _decode(_blocks_of(b"\x10" + b"\xff\xff\xff\xff\x0f" * 2 + b"\1" + b"\xff\xff\xff\xff\x0f"), 0)[5] == [[(M32, M32, [M32])]]
    for offsets, message in (([0, 11], "descend or leave the bytes"), ([7, 0], "descend or leave the bytes"), ([3, 3], "an empty block")):
        rc, msg = _decode(_blocks_of(GOOD, offsets=offsets), 0)[:2]
        assert rc == -1 and message in msg
    rc, msg = _decode(_blocks_of(GOOD, B=3), 0)[:2]
    assert rc == -1 and "block size" in msg


# ---- the Python class
@pytest.mark.parametrize("n,nblocks", [(0, 0), (5, 1), (40, 3)])
def test_struct_round_trip_in_both_directions(n, nblocks):
    want = spa.MatchPostingBlocks((np.arange(n * 7, dtype=np.uint32) % 251).astype(np.uint8), np.arange(nblocks + 1, dtype=np.uint64) + (1 << 33),
                                  np.array([nblocks, n * 7, 16, 1 << 40], np.uint64), ndict=n, block_entries=16)
    keep = []
    s = P._to_c(want, keep)
    assert (s.ndict, s.nblocks, s.nbytes, s.block_entries) == (n, nblocks, n * 7, 16) and list(s.totals) == want.totals.tolist()
    got = P._from_c(spa.MatchPostingBlocks, s)
    for a in spa.MatchPostingBlocks._ARRAYS:
        g, w = getattr(got, a.attr), getattr(want, a.attr)
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), a.attr
    assert (got.ndict, got.block_entries) == (n, 16)
    assert [a.attr for a in spa.MatchPostingBlocks._ARRAYS] == list(model.FIELDS)
    assert spa.MatchPostingBlocks._FREE == "sp_match_posting_blocks_free" and spa.MatchPostingBlocks._FETCH == "sp_matcher_ctx_finished_posting_blocks_fetch"
