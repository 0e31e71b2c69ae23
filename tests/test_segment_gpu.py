"""Segment lookups on the device (sp_segment_open, sp_segment_from_ctx, sp_segment_lookup_device, csrc/l2_segment.h): what the
launches leave must EQUAL what the device-free twin (sp_match_segment_lookup) makes of the fetched term blocks and posting blocks,
and the model (tests/segment_model.py) on their decoded entries and lists; the device pointers of `out` hold the fetched bytes.
Bare-term matchers over hand-made lexems as in tests/test_postingblocks_gpu.py: a test sets every handle, value and position
itself.  (A text on the device ends in 0xFF sentinels, so a value cannot hold that byte there: the one test of values with 0xFF
and of the empty value opens a segment coded by the two models.)  No test here feeds malformed bytes: the walks are one copy, and
tests/test_segment_abi.py and tests/micro/match_segment_san.cpp speak for the bounds."""
import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from tests import postingblocks_cases as cases
from tests import segment_model as model
from tests.finished_support import _bare, _from_device, Run, Source, _stream

pytestmark = pytest.mark.gpu

T = spa.SP_TERM_TEXT


def _blocks(docs, nhandles=8):
    """the term blocks and the posting blocks of the text terms of hand-made documents of (handle, value, ordpos), built on the
    device: (context, run)"""
    pieces, lex, seg, offs = cases.build_at(docs)
    ctx = _bare(nhandles).createContext()
    src = Source(pieces)
    run = Run(ctx, lex, seg, offs)
    src.gather(ctx, items=False)
    ctx.finishedTermsDevice(T, _stream())
    ctx.finishedDictionaryDevice(_stream())
    ctx.finishedDictionaryOrderDevice(_stream())
    ctx.finishedPostingsDevice(_stream())
    ctx.finishedPositionsDevice(_stream())
    ctx.finishedTermBlocksDevice(_stream())
    ctx.finishedPostingBlocksDevice(_stream())
    return ctx, run


def _lookup(seg, t, p, queries, prefix=False, decoded=None):
    """device == twin == model for one lookup on the segment `seg` of the products t, p; the bytes behind the device pointers are
    the fetched ones; returns the SegmentLookup"""
    queries = list(queries)
    entries, lists = decoded or (t.entries(), p.lists())
    out = seg.lookupDevice(queries, prefix=prefix, stream=_stream())
    got = seg.lookupFetch()
    model.check(got, entries, lists, queries, prefix)
    model.assert_same(got, spa.segmentLookup(t, p, queries, prefix=prefix))
    nq, nsel, npostings, npositions, nvalues = len(queries), len(got.selections), len(got.postings), len(got.positions), len(got.values)
    assert (out.nq, out.nsel, out.npostings, out.npositions, out.nvalue_bytes, out.flags) == (nq, nsel, npostings, npositions, nvalues, got.flags)
    for ptr, n, dtype, want in ((out.d_q_first, nq, np.uint32, got.q_first), (out.d_q_count, nq, np.uint32, got.q_count), (out.d_q_status, nq, np.uint32, got.q_status),
                                (out.d_q_sel_offsets, nq + 1, np.uint64, got.q_sel_offsets), (out.d_selections, 6 * nsel, np.uint32, got.selections.reshape(-1)),
                                (out.d_sel_value_offsets, nsel + 1, np.uint64, got.sel_value_offsets), (out.d_sel_posting_offsets, nsel + 1, np.uint64, got.sel_posting_offsets),
                                (out.d_values, nvalues, np.uint8, got.values), (out.d_postings, 4 * npostings, np.uint32, got.postings.reshape(-1)),
                                (out.d_posting_position_offsets, npostings + 1, np.uint64, got.posting_position_offsets),
                                (out.d_positions, npositions, np.uint32, got.positions), (out.d_totals, 4, np.uint64, got.totals)):
        assert np.array_equal(_from_device(ptr, n, dtype), want)
    return got


def _both(seg, t, p, queries, decoded=None):
    return _lookup(seg, t, p, queries, False, decoded), _lookup(seg, t, p, queries, True, decoded)


def _go(docs, queries=None, nhandles=8, B=0):
    """the segment of hand-made documents, from the context and opened from the fetches: both answer `queries` (those around
    its entries unless given), exact and by prefix, with the same bytes; returns (entries, exact, prefix)"""
    with cases.block_entries(B):
        ctx, run = _blocks(docs, nhandles)
        t, p = ctx.finishedTermBlocksFetch(), ctx.finishedPostingBlocksFetch()
        a, b = spa.Segment.fromContext(ctx, _stream()), spa.Segment.open(t, p)
    decoded = (t.entries(), p.lists())
    queries = model.probes(decoded[0]) if queries is None else queries
    exact, prefix = _both(a, t, p, queries, decoded)
    model.assert_same(_lookup(b, t, p, queries, False, decoded), exact)
    model.assert_same(_lookup(b, t, p, queries, True, decoded), prefix)
    a.close()
    b.close()
    return decoded[0], exact, prefix


# ---- 1. trivial inputs
def test_no_queries_the_empty_segment_and_one_term():
    entries, exact, prefix = _go([[], [(3, b"only", 7)]], [])
    assert entries == [(3, b"only", 1, 1)] and exact.q_sel_offsets.tolist() == [0] and exact.totals.tolist() == [0, 0, 0, 0]
    entries, exact, prefix = _go([[], [(3, b"only", 7)]], [(3, b"only"), (3, b"on"), (3, b"only!"), (2, b"only"), (3, b"")])
    assert exact.q_count.tolist() == [1, 0, 0, 0, 0] and prefix.q_count.tolist() == [1, 1, 0, 0, 1] and prefix.query(1) == [(3, b"only", 1, 1, [(1, 1, [7])])]
    entries, exact, prefix = _go([[], []], [(1, b"a"), (0, b"")])
    assert entries == [] and exact.q_first.tolist() == [0, 0] and prefix.totals.tolist() == [0, 0, 0, 0]
    _go([[], []], [])


# ---- 2. every place of a hit and of a miss, at three block sizes
def _spread(n):
    """n distinct terms over the handles 1, 2 and 5 (a handle delta above 1 inside a block) whose values share prefixes"""
    terms = sorted({((1, 2, 5)[k % 3], b"t%02d" % (k // 7) + b"x" * (k % 4) + (b"%d" % k if k % 5 else b"")) for k in range(n)})
    return [[(h, v, 1 + i + 3 * d) for i, (h, v) in enumerate(terms[at:at + 6])] for d, at in enumerate(range(0, len(terms), 6))] + [[(h, v, 2) for h, v in terms[::4]]]


@pytest.mark.parametrize("B", [1, 2, 16])
def test_hits_and_misses_at_every_place_of_a_block(B):
    """the probes query every entry -- block heads, the last position of a full block, the partial last block --, and per entry
    a proper prefix, two extensions and a neighbour: below the first, above the last, between two entries of a block, between
    two blocks; handles without entries below, between (inside a block) and above"""
    entries, exact, prefix = _go(_spread(37), nhandles=8, B=B)
    assert len(entries) % max(B, 2) != 0 or B == 1
    assert int(exact.q_count.sum()) >= len(entries) and int(exact.totals[0]) < len(exact.q_count) and 0 in exact.q_count.tolist()
    assert capi.lib().sp_matcher_term_block_entries() == 16           # (restored)


# ---- 3. value shapes
def test_value_shapes_from_the_device():
    long = b"b" + bytes(range(56, 255)) + b"z"             # 201 bytes: a suffix varint of two bytes
    docs = [[(1, b"\0", 1), (1, b"\0\0", 2), (1, b"\0\x7f", 3), (1, b"a", 4), (1, b"ab", 5), (1, long, 6), (4, b"\0", 7)], [(1, long, 3), (1, b"ab", 9)]]
    queries = [(1, b"\0"), (1, b"\0\0"), (1, b"\0\x7f"), (1, b"a"), (1, b"ab"), (1, long), (4, b"\0"), (1, long[:200]), (1, long + b"\xff"), (1, b"\0\1"), (1, b"\xff"),
               (1, b"\xff\xff"), (1, b""), (4, b""), (2, b"\xff"), (4, b"\0\0"), (1, b"abc")]
    entries, exact, prefix = _go(docs, queries)
    assert exact.q_count.tolist() == [1] * 7 + [0] * 10 and prefix.q_count.tolist() == [3, 1, 1, 2, 1, 1, 1, 1, 0, 0, 0, 0, 6, 1, 0, 0, 0]
    assert prefix.query(7) == [(1, long, 2, 2, [(0, 1, [6]), (1, 1, [3])])]


def test_the_empty_value_and_0xff_in_an_opened_segment():
    entries = [(1, b"", 1, 1), (1, b"\0", 1, 1), (1, b"\0\xff", 1, 1), (1, b"\xfe\xff", 2, 3), (1, b"\xff", 1, 1), (1, b"\xff\xff", 1, 1), (4, b"", 1, 1), (4, b"\xff", 1, 1)]
    lists = [[(k, 1, [k + 1])] for k in range(len(entries))]
    lists[3] = [(0, 2, [1, 2]), (9, 1, [4])]
    queries = [(h, v) for h, v, _, _ in entries] + [(1, b"\xff\xff\xff"), (1, b"\xfe"), (0, b""), (2, b""), (4, b"\xfe"), (5, b"")]
    for B in (2, 16):
        t, p = model.segment_of(entries, lists, B)
        seg = spa.Segment.open(t, p)
        exact, prefix = _both(seg, t, p, queries)
        seg.close()
        assert exact.q_count.tolist() == [1] * 8 + [0] * 6 and prefix.q_count.tolist() == [6, 2, 1, 1, 2, 1, 2, 1, 0, 1, 0, 0, 0, 0]


# ---- 4. prefix runs
def test_prefix_runs():
    """a run that spans three blocks, a run that is a whole handle, a run that ends at the end of the segment, no hit at all"""
    docs = [[(1, b"a%02d" % k, k + 1) for k in range(5)], [(2, b"run%03d" % k, k + 1) for k in range(40)], [(7, b"za", 1), (7, b"zb", 2)]]
    entries, exact, prefix = _go(docs, [(2, b"run"), (2, b""), (2, b"run01"), (7, b"z"), (7, b""), (1, b"a0"), (2, b"rux"), (3, b""), (7, b"zb")])
    assert prefix.q_count.tolist() == [40, 40, 10, 2, 2, 5, 0, 0, 1] and prefix.q_first.tolist()[3] + 2 == len(entries) == 47
    assert prefix.q_first.tolist()[0] // 16 + 2 == (prefix.q_first.tolist()[0] + 39) // 16        # blocks 0, 1 and 2
    entries, exact, prefix = _go(docs, [(2, b"rux"), (3, b""), (9, b"z"), (1, b"b")])
    assert prefix.totals.tolist() == [0, 0, 0, 0] and exact.totals.tolist() == [0, 0, 0, 0]      # nsel == 0 after the first wait


# ---- 5. query counts
@pytest.mark.parametrize("nq", [63, 64, 65])
def test_query_counts_at_the_wave_edge(nq):
    docs = [[(1 + k % 3, b"w%03d" % k, k + 1) for k in range(at, min(at + 9, 50))] for at in range(0, 50, 9)]
    queries = [(1 + k % 3, b"w%03d" % (k % 55)) for k in range(nq - 2)] + [(1, b"w000")] * 2       # the same query twice
    entries, exact, prefix = _go(docs, queries)
    assert exact.query(nq - 1) == exact.query(nq - 2) == [(1, b"w000", 1, 1, [(0, 1, [1])])] and exact.q_count.tolist().count(1) == 52    # (the 50 terms once each, and the two)


# ---- 6. varint widths in the lists, a long list
def test_wide_varints_and_a_long_list():
    """a document delta of 130, a count of 130 with repeated positions (npos 65), a position gap of 20000; one list of 200
    postings among lists of one"""
    docs = [[(1, b"n%03d" % d, 1), (2, b"often", 2 + d % 3)] for d in range(200)]
    docs[3] = docs[3] + [(3, b"gap", 5), (3, b"gap", 20005)]
    docs[140] = docs[140] + [(3, b"gap", 9)] + [(4, b"many", 10 + i // 2) for i in range(130)]
    entries, exact, prefix = _go(docs, [(2, b"often"), (3, b"gap"), (4, b"many"), (1, b"n1"), (1, b"n140"), (2, b"")])
    assert len(exact.query(0)[0][4]) == 200 and exact.query(1) == [(3, b"gap", 2, 3, [(3, 2, [5, 20005]), (140, 1, [9])])]
    assert exact.query(2) == [(4, b"many", 1, 130, [(140, 130, list(range(10, 75)))])] and prefix.q_count.tolist() == [1, 1, 1, 100, 1, 1]


# ---- 7. lifetime, reuse
def test_a_segment_outlives_its_context_and_reuses_its_buffers():
    docs = [[(1, b"a%02d" % k, k + 1) for k in range(20)], [(2, b"b%02d" % k, k + 1) for k in range(30)] + [(1, b"a03", 40)]]
    ctx, run = _blocks(docs)
    t, p = ctx.finishedTermBlocksFetch(), ctx.finishedPostingBlocksFetch()
    opened, copied = spa.Segment.open(t, p), spa.Segment.fromContext(ctx, _stream())
    decoded = (t.entries(), p.lists())
    many, few = model.probes(decoded[0]), [(1, b"a03"), (2, b"b")]
    first = _lookup(opened, t, p, many, True, decoded)
    model.assert_same(_lookup(copied, t, p, many, True, decoded), first)
    # another batch on the context, then the context goes: both segments answer as before
    other, _ = _blocks([[(3, b"other", 1)]])
    pieces, lex, seg, offs = cases.build_at([[(5, b"next", 1), (5, b"batch", 2)]])
    Run(ctx, lex, seg, offs)
    del ctx, run
    before = capi.SpSegmentLookupDevice()
    for s in (opened, copied):
        out = s.lookupDevice(many, prefix=True, stream=_stream())
        model.assert_same(s.lookupFetch(), first)
        # a second lookup with fewer queries: the buffers are the same ones
        again = s.lookupDevice(few, stream=_stream())
        assert (again.d_q_first, again.d_selections, again.d_values, again.d_postings, again.d_positions) == (out.d_q_first, out.d_selections, out.d_values, out.d_postings, out.d_positions)
        got = _lookup(s, t, p, few, False, decoded)
        assert got.query(0) == [(1, b"a03", 2, 2, [(0, 1, [4]), (1, 1, [40])])] and got.q_count.tolist() == [1, 0]
        assert s.lastLookupMs() >= 0.0
    del before
    opened.close()
    copied.close()
    with pytest.raises(spa.PatternError):
        spa.Segment.fromContext(_bare(8).createContext(), _stream())       # no blocks on that context


# ---- 8. the command line
def _listing(capsys, argv):
    from struspattern_amd import match
    assert match.main(argv) == 0
    return capsys.readouterr().out.splitlines()


def test_match_lookup_listing(capsys, tmp_path):
    """--lookup implies --blocks and --posting-blocks; its `post` lines, decoded from the segment, are those of the listing"""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    prog = os.path.join(here, "golden", "doc_example.rul")
    a, b = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    with open(os.path.join(here, "golden", "doc_example.txt"), "rb") as f:
        example = f.read().replace(b"\n", b" ")
    with open(a, "wb") as f:
        f.write(example)
    with open(b, "wb") as f:
        f.write(b"Prof. Anna B. Smith wrote to anna@etc.com. " + example[:len(example) // 2])
    common = ["-p", prog, "--device-values"]
    for paragraphs in ([], ["--paragraphs"]):
        plain = _listing(capsys, common + paragraphs + ["--posting-blocks", a, b])
        posts = [line for line in plain if line.startswith("post ") and line.count("'") == 2 and "=" not in line]
        assert len(posts) >= 2
        name, value = posts[-1].split(" ")[1], posts[-1].split("'")[1]
        other, missing = posts[0].split(" ")[1], posts[0].split("'")[1] + "~"
        out = _listing(capsys, common + paragraphs + ["--lookup", "%s=%s" % (name, value), "--lookup", "%s=%s" % (other, missing), a, b])
        assert out[-1] == "OK done" and out[:len(plain) - 1] == plain[:-1]
        assert out[len(plain) - 1:-1] == ["lookup %s '%s': terms 1" % (name, value), posts[-1], "lookup %s '%s': terms 0" % (other, missing)]
        out = _listing(capsys, common + paragraphs + ["--lookup", "%s=%s" % (name, value[:1]), "--lookup-prefix", a, b])
        found = out[len(plain) - 1:-1]
        want = [line for line in plain if line.startswith("post %s '%s" % (name, value[:1]))]
        assert found == ["lookup %s '%s': terms %d" % (name, value[:1], len(want))] + want and posts[-1] in want
    with pytest.raises(spa.PatternError):
        _listing(capsys, common + ["--lookup", "NoSuchPattern=x", a])
