"""Term blocks without a device (sp_match_batch_term_blocks, sp_match_term_blocks_decode_block, csrc/match_termblocks.hpp): the
twin equals the model (tests/termblocks_model.py) and decodes to the sorted entries on hand-made batches -- every varint length
of every field, every block size of the switch, ndict at the block edges --, every refusal of the twin and of the reader with its
message, find() on the product alone, and the struct round trip of MatchTermBlocks in both directions.  The header of a code is
composed by csrc/term_block_code.h for the twin and the device alike, so these tests speak for the device's encoder on values
that no small batch reaches on a GPU."""
import ctypes

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from struspattern_amd import products as P
from tests import dictorder_cases
from tests import termblocks_cases as cases
from tests import termblocks_model as model
from tests.termblocks_cases import Inputs

BOUND = 8


def test_symbols_and_signatures():
    vp, Ptr = ctypes.c_void_p, ctypes.POINTER
    for name in ("sp_matcher_ctx_finished_term_blocks_device", "sp_matcher_ctx_finished_term_blocks_fetch", "sp_match_term_blocks_free",
                 "sp_matcher_ctx_last_term_blocks_ms", "sp_match_batch_term_blocks", "sp_match_term_blocks_decode_block",
                 "sp_matcher_term_block_entries", "sp_test_term_block_entries"):
        assert name in capi.SIGNATURES and hasattr(capi.lib(), name)
    assert capi.SIGNATURES["sp_matcher_ctx_finished_term_blocks_device"] == (ctypes.c_int, [vp, vp, Ptr(capi.SpMatchTermBlocksDevice)])
    assert capi.SIGNATURES["sp_match_batch_term_blocks"][1][:7] == [Ptr(capi.SpMatchBatch), Ptr(capi.SpMatchValues), Ptr(capi.SpMatchText), Ptr(capi.SpMatchTerms),
                                                                    Ptr(capi.SpMatchDictionary), Ptr(capi.SpMatchDictionaryOrder), Ptr(capi.SpMatchTermBlocks)]
    assert [n for n, _ in capi.SpMatchTermBlocksDevice._fields_] == ["ndict", "nblocks", "nbytes", "block_entries", "d_bytes", "d_block_offsets", "d_block_handles", "d_totals"]
    assert [n for n, _ in capi.SpMatchTermBlocks._fields_] == ["ndict", "nblocks", "nbytes", "block_entries", "bytes", "block_offsets", "block_handles", "totals"]
    assert [n for n, _ in capi.SpTermBlockEntry._fields_] == ["handle", "value_bytes", "value_offset", "doc_freq", "reserved", "count"]
    assert ctypes.sizeof(capi.SpTermBlockEntry) == 32
    for name in ("finishedTermBlocksDevice", "finishedTermBlocksFetch", "lastTermBlocksMs"):
        assert hasattr(spa.PatternMatcherContext, name)
    for name in ("MatchTermBlocks", "batchTermBlocks"):
        assert name in spa.__all__
    assert spa._SEGMENT_PRODUCTS[-1] == ("TermBlocks", ("DictionaryOrder",))
    assert capi.lib().sp_matcher_term_block_entries() == 16


def test_the_header_states_the_rule():
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "strus_pattern_amd.h")) as f:
        header = f.read()
    assert "---- term blocks:" in header and "unpinned by a reference vector" in header.split("---- term blocks:")[1].split("INPUT:")[0]


def test_the_switch_takes_its_seven_sizes_and_nothing_else():
    L = capi.lib()
    try:
        for n in model.SIZES:
            L.sp_test_term_block_entries(n)
            assert L.sp_matcher_term_block_entries() == n
        for n in (3, 128, 0):
            L.sp_test_term_block_entries(n)
            assert L.sp_matcher_term_block_entries() == 16
    finally:
        L.sp_test_term_block_entries(0)


# ---- the twin against the model
def test_comparator_edges_and_a_long_shared_prefix():
    pairs = dictorder_cases.comparator_values() + dictorder_cases.long_prefix_group()
    x = Inputs(dictorder_cases.in_documents(pairs, 11))
    got = x.check()
    fields = [f for j in range(len(got.block_handles)) for f in model.decode_block(got, j)[1]]
    assert [s for _, s, _ in fields].count(300) >= 60 and model.varint(300) == b"\xac\x02"          # a shared prefix of two bytes


def test_a_handle_per_entry_and_two_handles_far_apart():
    x = Inputs([cases.handle_per_entry()[:35], cases.handle_per_entry()[35:]], bound=71)
    got = x.check()
    fields = [f for j in range(len(got.block_handles)) for f in model.decode_block(got, j)[1]]
    assert [h for h, _, _ in fields] == [0 if k % 16 == 0 else 1 for k in range(70)] and not any(s for _, s, _ in fields)
    assert got.block_handles.tolist() == [1, 17, 33, 49, 65]
    y = Inputs([cases.far_handles()], bound=300)
    got = y.check()
    assert model.decode_block(got, 0)[1] == [(0, 0, 4), (199, 0, 5), (0, 5, 1)] and model.varint(199) == b"\xc7\x01"
    assert bytes(got.bytes) == b"\0\0\4\1\1left" + b"\xc7\1\0\5\1\1right" + b"\0\5\1\1\1s"


def test_value_lengths_and_shared_lengths_at_the_varint_edges():
    x = Inputs([cases.value_lengths() + cases.shared_lengths()])
    got = x.check()
    fields = model.decode_block(got, 0)[1]
    assert [f[2] for f in fields[:6]] == [0, 1, 127, 128, 16383, 16384]
    assert [f[1] for f in fields[6:]] == [0, 127, 0, 128] and [f[2] for f in fields[6:]] == [128, 1, 129, 1]
    assert [len(model.varint(n)) for n in (0, 127, 128, 16383, 16384)] == [1, 1, 2, 2, 3]


COUNTS = [127, 128, (1 << 32) - 1, 1 << 32, 1 << 35, 1 << 63, (1 << 64) - 1]


def test_frequencies_at_the_varint_edges_set_by_hand():
    pairs = [(1, b"v%02d" % k) for k in range(9)]
    x = Inputs([pairs]).set_frequencies(doc_freq=[127, 128, 16383, 16384, (1 << 32) - 1], count=COUNTS)
    got = x.check()
    assert [e[3] for e in got.entries()[:7]] == COUNTS and [e[2] for e in got.entries()[:5]] == [127, 128, 16383, 16384, (1 << 32) - 1]
    assert [len(model.varint(c)) for c in COUNTS] == [1, 2, 5, 5, 6, 10, 10]
    assert model.varint((1 << 64) - 1) == b"\xff" * 9 + b"\x01"


@pytest.mark.parametrize("B", model.SIZES)
def test_every_block_size(B):
    pairs = dictorder_cases.numbered(150) + dictorder_cases.comparator_values()
    x = Inputs(dictorder_cases.in_documents(pairs, 37))
    got = x.check(B)
    assert got.block_entries == B and int(got.totals[2]) == B and len(got.block_handles) == (len(x.entries) + B - 1) // B
    if B == 1:
        fields = [model.decode_block(got, j)[1] for j in range(len(got.block_handles))]
        assert all(f == [(0, 0, len(e[1]))] for f, e in zip(fields, x.sorted()))
        assert len(got.bytes) == sum(len(model.code(True, None, e)) for e in x.sorted())


@pytest.mark.parametrize("B", [4, 16])
def test_ndict_at_the_block_edges(B):
    for n in (0, 1, B - 1, B, B + 1, 3 * B + 1):
        x = Inputs([dictorder_cases.numbered(n)] if n else [])
        got = x.check(B)
        assert got.ndict == n and len(got.block_handles) == (n + B - 1) // B
        if n == 0:
            assert got.block_offsets.tolist() == [0] and len(got.bytes) == 0 and got.totals.tolist() == [0, 0, B, 0]
        if n == 3 * B + 1:
            assert len(model.decode_block(got, 3)[0]) == 1          # a partial last block


def test_values_and_text_in_one_batch():
    formatted = {(1, b"eur"), (2, b"b"), (2, b"")}
    docs = [[(1, b"usd"), (1, b"eur"), (2, b"c")], [(2, b"b"), (2, b"a"), (2, b"")], [(1, b"chf"), (1, b"eur")]]
    x = Inputs(docs, flags=cases.V | cases.T, formatted=formatted)
    got = x.check()
    assert got.entries() == [(1, b"chf", 1, 1), (1, b"eur", 2, 2), (1, b"usd", 1, 1), (2, b"", 1, 1), (2, b"a", 1, 1), (2, b"b", 1, 1), (2, b"c", 1, 1)]


# ---- the twin's refusals
def _raw(x, damage=None, null=()):
    """sp_match_batch_term_blocks over C structs made of the Inputs x; damage(b, t, q, o) may change them, `null` names the
    arguments passed as NULL.  Returns (rc, message)."""
    keep = []
    b, keep_b = P._host_batch(x.mb, formats="results", status=True)
    v, t_ = P._host_source(x.values, keep), P._host_source(x.text, keep)
    t = P._to_c(spa.MatchTerms(x.terms.records.copy(), x.terms.doc_offsets.copy(), x.terms.result_term, x.terms.status, x.terms.flags, x.terms.handle_bound), keep)
    q = P._to_c(spa.MatchDictionary(x.d.records.copy(), x.d.term_dict, x.d.doc_offsets, x.d.handle_terms.copy()), keep, flags=x.terms.flags)
    o = P._to_c(spa.MatchDictionaryOrder(x.order.order.copy(), x.order.rank.copy(), x.order.prefix_bytes.copy(), x.order.handle_offsets.copy()), keep)
    if damage:
        damage(b, t, q, o)
    args = {"mb": b, "values": v, "text": t_, "terms": t, "dict": q, "order": o}
    out = capi.SpMatchTermBlocks()
    out.ndict = 77                                      # (the call clears `out` first)
    err = ctypes.create_string_buffer(256)
    rc = capi.lib().sp_match_batch_term_blocks(*[None if k in null or a is None else ctypes.byref(a) for k, a in args.items()], ctypes.byref(out), err, 256)
    if rc == 0:
        assert out.ndict == len(x.d.records) and out.nblocks == out.totals[0] and out.nbytes == out.totals[1] and out.bytes and out.block_offsets
        capi.lib().sp_match_term_blocks_free(ctypes.byref(out))
    assert not out.bytes and not out.block_offsets and not out.block_handles and out.ndict == out.nblocks == out.nbytes == 0 and out.totals[1] == 0
    return rc, err.value.decode()


def _swap(array, i, j):
    def damage(b, t, q, o):
        a = getattr(o, array)
        a[i], a[j] = a[j], a[i]
    return damage


def _put(which, field, value, at=None):
    def damage(b, t, q, o):
        target = {"b": b, "t": t, "q": q, "o": o}[which]
        if at is None:
            setattr(target, field, value)
        elif isinstance(at, tuple):
            setattr(getattr(target, field)[at[0]], at[1], value)
        else:
            getattr(target, field)[at] = value
    return damage


# the refusal batch sorts to (1, "a"), (1, "ab"), (1, "abc"), (1, "c"), (2, "a"), (2, "d"): prefix_bytes 0 1 2 0 0 0
REFUSED = [
    # what sp_match_batch_dictionary_order refuses
    ("other counts of documents or results", _put("t", "nresults", 99)),
    ("term offsets do not ascend", _put("t", "doc_term_offsets", 99, at=1)),
    ("other counts of documents or term records", _put("q", "nterms", 1)),
    ("another handle bound or other flags", _put("q", "flags", cases.V)),
    ("a handle outside the bound", _put("q", "records", 0, at=(1, "handle"))),
    ("first_doc lies outside the documents", _put("q", "records", 2, at=(0, "first_doc"))),
    ("first_term lies outside its document's records", _put("q", "records", 4, at=(0, "first_term"))),
    ("first_result lies outside its document", _put("t", "records", 4, at=(0, "first_result"))),
    ("dictionary entry whose value_bytes is not the length", _put("q", "records", 9, at=(0, "value_bytes"))),
    ("handle_terms that are not the number of entries", _put("q", "handle_terms", 1, at=2)),
    ("two dictionary entries with the same handle and bytes", lambda b, t, q, o: (setattr(q.records[int(o.order[1])], "first_doc", q.records[int(o.order[0])].first_doc),
                                                                                  setattr(q.records[int(o.order[1])], "first_term", q.records[int(o.order[0])].first_term),
                                                                                  setattr(q.records[int(o.order[1])], "value_bytes", 1))),
    # the order against its dictionary
    ("another number of entries or another handle bound", _put("o", "ndict", 5)),
    ("another number of entries or another handle bound", _put("o", "handle_bound", BOUND + 1)),
    ("not a permutation", lambda b, t, q, o: o.order.__setitem__(2, o.order[1])),
    ("not a permutation", _put("o", "order", 6, at=0)),
    ("handles descend", _swap("order", 3, 4)),
    ("above the length of a neighbour's value", _put("o", "prefix_bytes", 2, at=1)),
    ("above the length of a neighbour's value", _put("o", "prefix_bytes", 3, at=2)),
    ("not what the two values share", _put("o", "prefix_bytes", 1, at=2)),
    ("not what the two values share", _put("o", "prefix_bytes", 0, at=1)),
    ("not what the two values share", _put("o", "prefix_bytes", 1, at=4)),        # the first position of a handle shares nothing
]


def _refusal_inputs():
    return Inputs([[(1, b"c"), (1, b"ab"), (2, b"a")], [(1, b"abc"), (1, b"a"), (1, b"ab"), (2, b"d")]])


@pytest.mark.parametrize("message,damage", REFUSED, ids=["%02d %s" % (k, m[:40]) for k, (m, _) in enumerate(REFUSED)])
def test_refusals_with_their_message(message, damage):
    x = _refusal_inputs()
    assert [e[:2] for e in x.sorted()] == [(1, b"a"), (1, b"ab"), (1, b"abc"), (1, b"c"), (2, b"a"), (2, b"d")] and x.order.prefix_bytes.tolist() == [0, 1, 2, 0, 0, 0]
    assert _raw(x) == (0, "")
    rc, msg = _raw(x, damage)
    assert rc == -1 and message in msg, msg
    assert _raw(x) == (0, "")                           # the same objects then serve a good call


def test_refused_arguments_and_sources():
    x = _refusal_inputs()
    for name, message in (("mb", "no batch"), ("terms", "no terms"), ("dict", "no dictionary"), ("order", "no order"), ("text", "no text of the results")):
        rc, msg = _raw(x, null=(name,))
        assert rc == -1 and message in msg, name
    # a source range outside the source's bytes, which the device codes as the empty value: the twin refuses it
    x.text = spa.MatchText(x.text.result_text[:-1], x.text.result_offsets, None, None, x.text.status)
    rc, msg = _raw(x)
    assert rc == -1 and "outside the bytes of its source" in msg
    with pytest.raises(spa.PatternError, match=r"no term blocks of the batch \(-1\): a term value outside"):
        x.blocks()


# ---- the reader
def _decode(tb, j, entries_cap=None, values_cap=None, query=False):
    """sp_match_term_blocks_decode_block on block j of the MatchTermBlocks tb: (rc, message, nentries, nvalues, entries)"""
    keep = []
    s = P._to_c(tb, keep)
    n, nv, err = ctypes.c_size_t(77), ctypes.c_size_t(77), ctypes.create_string_buffer(256)
    ecap = tb.block_entries if entries_cap is None else entries_cap
    vcap = 1 << 16 if values_cap is None else values_cap
    entries, values = (capi.SpTermBlockEntry * max(ecap, 1))(), (ctypes.c_uint8 * max(vcap, 1))()
    rc = capi.lib().sp_match_term_blocks_decode_block(ctypes.byref(s), j, None if query else entries, ecap, None if query else values, vcap,
                                                       ctypes.byref(n), ctypes.byref(nv), err, 256)
    data = bytes(values)
    found = [(e.handle, data[e.value_offset:e.value_offset + e.value_bytes], e.doc_freq, e.count) for e in entries[:n.value]] if rc == 0 and not query else None
    return rc, err.value.decode(), n.value, nv.value, found


def _blocks_of(data, handles=(1,), offsets=None, B=16):
    data = bytes(data)
    offsets = [0, len(data)] if offsets is None else offsets
    return spa.MatchTermBlocks(np.frombuffer(data, np.uint8).copy(), np.array(offsets, np.uint64), np.array(handles, np.uint32),
                               np.array([len(handles), len(data), B, 0], np.uint64), ndict=0, block_entries=B)


def test_the_reader_decodes_a_block_from_its_own_bytes():
    x = Inputs(dictorder_cases.in_documents(dictorder_cases.numbered(40) + cases.far_handles(), 9), bound=300)
    got = x.check()
    want = x.sorted()
    for j in range(3):
        rc, msg, n, nv, found = _decode(got, j)
        assert (rc, msg) == (0, "") and found == want[16 * j:16 * j + 16] and n == len(found) and nv == sum(len(e[1]) for e in found)
        assert _decode(got, j, query=True)[:4] == (0, "", n, nv)                # only counts
        assert got.block(j) == found
    # room that does not suffice: the counts all the same
    rc, msg, n, nv, _ = _decode(got, 0, entries_cap=15)
    assert rc == -1 and "room" in msg and n == 16 and nv == sum(len(e[1]) for e in want[:16])
    rc, msg, n, nv, _ = _decode(got, 0, values_cap=nv - 1)
    assert rc == -1 and "room" in msg and n == 16
    rc, msg = _decode(got, 3)[:2]
    assert rc == -1 and "no such block" in msg
    with pytest.raises(spa.PatternError, match=r"no block 3 of the term blocks of the batch \(-1\): no such block"):
        got.block(3)


MALFORMED = [
    ("a varint that runs past the block", b"\0\0\2\1\1ab" + b"\0\1\1\1\x80"),                             # the count of the second code never ends
    ("a varint that runs past the block", b"\0\0\2\1"),                                                   # a header cut off
    ("longer than ten bytes", b"\0\0\2\1" + b"\x80" * 10 + b"\1ab"),
    ("longer than ten bytes", b"\0\0\2\1" + b"\xff" * 9 + b"\2ab"),                                       # ten bytes, more than 64 bits
    ("a shared prefix above the length of the value before", b"\0\0\2\1\1ab" + b"\0\3\1\1\1c"),
    ("a head that does not carry", b"\0\1\1\1\1b"),
    ("a head that does not carry", b"\1\0\1\1\1b"),
    ("a suffix that runs past the block", b"\0\0\2\1\1ab" + b"\0\1\3\1\1cd"),
    ("a suffix that runs past the block", b"\0\0\xff\xff\xff\xff\xff\xff\xff\xff\xff\1\1\1ab"),             # ... and does not wrap
    ("leaves 32 bits", b"\0\0\1\1\1a" + b"\xff\xff\xff\xff\x0f\0\1\1\1b"),                                # the handle
    ("leaves 32 bits", b"\0\0\1\xff\xff\xff\xff\x1f\1a"),                                                 # the doc_freq
    ("more codes than a block holds", b"\0\0\0\1\1" * 17),
]


@pytest.mark.parametrize("message,data", MALFORMED, ids=["%02d %s" % (k, m[:40]) for k, (m, _) in enumerate(MALFORMED)])
def test_the_reader_refuses_a_malformed_block(message, data):
    rc, msg, n, nv, _ = _decode(_blocks_of(data), 0)
    assert rc == -1 and message in msg, msg


def test_the_reader_refuses_offsets_outside_the_bytes():
    good = b"\0\0\2\1\1ab"
    assert _decode(_blocks_of(good), 0)[4] == [(1, b"ab", 1, 1)]
    assert _decode(_blocks_of(good + b"\0\2\0\xff\xff\xff\xff\x0f" + b"\xff" * 9 + b"\1"), 0)[4] == [(1, b"ab", 1, 1), (1, b"ab", 0xFFFFFFFF, (1 << 64) - 1)]
    for offsets, message in (([0, 8], "descend or leave the bytes"), ([7, 0], "descend or leave the bytes"), ([3, 3], "an empty block")):
        rc, msg = _decode(_blocks_of(good, offsets=offsets), 0)[:2]
        assert rc == -1 and message in msg
    rc, msg = _decode(_blocks_of(good, B=3), 0)[:2]
    assert rc == -1 and "block size" in msg


# ---- find, on the product alone
def test_find_hits_and_misses():
    pairs = dictorder_cases.comparator_values() + dictorder_cases.numbered(60) + cases.handle_per_entry(6)
    x = Inputs(dictorder_cases.in_documents(pairs, 13))
    for B in (1, 4, 16):
        got = x.check(B)
        want = x.sorted()
        where = {e[:2]: k for k, e in enumerate(want)}
        handles = sorted(set(h for h, _ in where))
        for k, (h, v, df, count) in enumerate(want):
            assert got.find(h, v) == k
            # the last byte changed, the value extended by one byte, the same value under another handle: found only where the
            # batch happens to hold that term too
            changed = [v[:-1] + bytes([v[-1] ^ 1])] if v else []
            for other in changed + [v + b"\0", v + b"\xff"]:
                assert got.find(h, other) == where.get((h, other)), (h, other)
            for o in handles + [BOUND - 1]:
                assert o == h or got.find(o, v) == where.get((o, v)), (o, v)
        assert got.find(2, b"abcdef") is None and got.find(2, b"abcdd") is None and got.find(3, b"abc") is None
        for h, v in [(0, b""), (BOUND, b"abc"), (99, b""), (2, b"\xff\xff"), (1, b"")]:
            assert got.find(h, v) is None, (h, v)
    assert Inputs([]).check().find(1, b"") is None


# ---- the Python class
@pytest.mark.parametrize("n,nblocks", [(0, 0), (5, 1), (40, 3)])
def test_struct_round_trip_in_both_directions(n, nblocks):
    want = spa.MatchTermBlocks((np.arange(n * 7, dtype=np.uint32) % 251).astype(np.uint8), np.arange(nblocks + 1, dtype=np.uint64) + (1 << 33),
                               np.arange(nblocks, dtype=np.uint32) + 7, np.array([nblocks, n * 7, 16, 1 << 40], np.uint64), ndict=n, block_entries=16)
    keep = []
    s = P._to_c(want, keep)
    assert (s.ndict, s.nblocks, s.nbytes, s.block_entries) == (n, nblocks, n * 7, 16) and list(s.totals) == want.totals.tolist()
    assert (bool(s.bytes) or n == 0) and s.block_offsets
    got = P._from_c(spa.MatchTermBlocks, s)
    for a in spa.MatchTermBlocks._ARRAYS:
        g, w = getattr(got, a.attr), getattr(want, a.attr)
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), a.attr
    assert (got.ndict, got.block_entries) == (n, 16)
    assert [a.attr for a in spa.MatchTermBlocks._ARRAYS] == list(model.FIELDS)
    assert spa.MatchTermBlocks._FREE == "sp_match_term_blocks_free" and spa.MatchTermBlocks._FETCH == "sp_matcher_ctx_finished_term_blocks_fetch"
    assert spa.MatchTermBlocks._TOTAL is None and spa.MatchTermBlocks._C is capi.SpMatchTermBlocks
