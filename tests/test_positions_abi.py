"""Posting positions without a device (sp_match_batch_positions, csrc/match_positions.hpp): the twin equals the model
(tests/positions_model.py) on hand-made batches -- lists out of position order, ties, a failed document in the middle, empty
shapes -- with every expected occurrence written out by hand; every invariant of the header; and every error return of the
header over hand-filled C structs, after which `out` is empty and the same objects serve a good call."""
import ctypes

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from tests import positions_model as model
from tests.finished_support import _batch, _family

T = spa.SP_TERM_TEXT
BOUND = 4

# per document the results (handle, ordpos, ordend) in finished order, and the text of every result
DOCS = [
    [(1, 9, 10), (2, 4, 5), (1, 3, 4), (1, 3, 6), (1, 0, 1)],          # (1,"eur") fires late for early positions; a tie at 3
    [(1, 5, 6)],
    [(2, 2, 3), (1, 7, 8), (1, 1, 2), (2, 2, 9)],                       # (2,"x") twice at position 2 with two ends
]
TEXT = [b"eur", b"x", b"eur", b"eur", b"eur", b"usd", b"x", b"eur", b"eur", b"x"]
# the postings: (1,"eur") in the documents 0 and 2, (2,"x") in 0 and 2, (1,"usd") in 1
POSTINGS = [[0, 0, 4, 0], [2, 0, 2, 1], [0, 1, 1, 4], [2, 1, 2, 2], [1, 0, 1, 5]]
LISTS = [[[0, 4], [3, 2], [3, 3], [9, 0]], [[1, 2], [7, 1]], [[4, 1]], [[2, 0], [2, 3]], [[5, 0]]]
DISTINCT = [3, 2, 1, 1, 1]


def _inputs(docs=DOCS, text=TEXT, text_status=None):
    """(batch, terms, dictionary, postings) of hand-made documents by the twins, text terms"""
    mb = _batch(docs)
    mt = _family(spa.MatchText, text, len(docs), status=text_status)
    terms = spa.batchTerms(mb, text=mt, handle_bound=BOUND, flags=T)
    d = spa.batchDictionary(mb, terms, text=mt)
    return mb, terms, d, spa.batchPostings(terms, d)


def _check(mb, terms, postings):
    got = spa.batchPositions(mb, terms, postings)
    model.assert_same(got, model.of_batch(mb, terms, postings))
    model.check_invariants(got, mb, terms, postings)
    return got


def test_symbols_and_signatures():
    vp, P = ctypes.c_void_p, ctypes.POINTER
    for name in ("sp_matcher_ctx_finished_positions_device", "sp_matcher_ctx_finished_positions_fetch", "sp_match_positions_free",
                 "sp_matcher_ctx_last_positions_ms", "sp_match_batch_positions", "sp_matcher_positions_tile",
                 "sp_test_positions_launch_events", "sp_matcher_ctx_last_positions_launch_ms"):
        assert name in capi.SIGNATURES and hasattr(capi.lib(), name)
    assert capi.SIGNATURES["sp_matcher_ctx_finished_positions_device"] == (ctypes.c_int, [vp, vp, P(capi.SpMatchPositionsDevice)])
    assert capi.SIGNATURES["sp_matcher_ctx_finished_positions_fetch"] == (ctypes.c_int, [vp, P(capi.SpMatchPositions)])
    assert capi.SIGNATURES["sp_match_batch_positions"][1][:4] == [P(capi.SpMatchBatch), P(capi.SpMatchTerms), P(capi.SpMatchPostings), P(capi.SpMatchPositions)]
    assert ctypes.sizeof(capi.SpOccurrence) == 8 and capi.SpOccurrence.ordpos.offset == 0 and capi.SpOccurrence.result.offset == 4
    assert [n for n, _ in capi.SpMatchPositionsDevice._fields_] == ["ndocs", "nterms", "nocc", "d_occurrences", "d_posting_offsets", "d_posting_positions", "d_totals"]
    assert [n for n, _ in capi.SpMatchPositions._fields_] == ["ndocs", "nterms", "nocc", "occurrences", "posting_offsets", "posting_positions", "totals"]
    assert capi.SpMatchPositions.totals.size == 16
    for name in ("finishedPositionsDevice", "finishedPositionsFetch", "lastPositionsMs"):
        assert hasattr(spa.PatternMatcherContext, name)
    for name in ("MatchPositions", "batchPositions"):
        assert name in spa.__all__
    tile = capi.lib().sp_matcher_positions_tile()
    assert tile >= 64 and tile % 64 == 0


def test_lists_out_of_position_order_and_ties_equal_the_occurrences_written_out():
    mb, terms, d, postings = _inputs()
    assert postings.records.tolist() == POSTINGS
    got = _check(mb, terms, postings)
    assert got.occurrences.tolist() == [row for rows in LISTS for row in rows]
    assert got.posting_offsets.tolist() == [0, 4, 6, 7, 9, 10] and got.posting_positions.tolist() == DISTINCT
    assert got.totals.tolist() == [10, 8]
    assert got.occurrences.dtype == np.uint32 and got.posting_offsets.dtype == np.uint64 and got.posting_positions.dtype == np.uint32
    for p, rows in enumerate(LISTS):
        assert got.posting(p).tolist() == rows and got.positions(p).tolist() == sorted(set(row[0] for row in rows))
    assert int(got.posting_positions[3]) < int(postings.records[3, 2])             # one position, two ends


def test_a_failed_document_in_the_middle_has_no_occurrences():
    mb, terms, d, postings = _inputs(text_status=[0, 5, 0])
    assert terms.status.tolist() == [0, 5, 0] and terms.result_term.tolist()[5] == 0xFFFFFFFF
    assert postings.records.tolist() == POSTINGS[:4]
    got = _check(mb, terms, postings)
    assert got.occurrences.tolist() == [row for rows in LISTS[:4] for row in rows]
    assert got.posting_offsets.tolist() == [0, 4, 6, 7, 9] and got.posting_positions.tolist() == DISTINCT[:4] and got.totals.tolist() == [9, 7]


def test_no_documents_and_no_results():
    for ndocs in (0, 2):
        mb, terms, d, postings = _inputs([[]] * ndocs, [])
        got = _check(mb, terms, postings)
        assert got.occurrences.shape == (0, 2) and got.posting_offsets.tolist() == [0] and len(got.posting_positions) == 0
        assert got.totals.tolist() == [0, 0]


def test_position_zero_everywhere_is_one_position_per_list():
    docs = [[(1, 0, 1), (1, 0, 2), (2, 0, 1)], [(1, 0, 3)]]
    mb, terms, d, postings = _inputs(docs, [b"a", b"a", b"a", b"a"])
    got = _check(mb, terms, postings)
    assert got.posting_positions.tolist() == [1, 1, 1] and got.occurrences.tolist() == [[0, 0], [0, 1], [0, 0], [0, 2]]


def _raw(mb, terms, postings, break_=None, null=()):
    """sp_match_batch_positions over hand-filled C structs; break_( b, t, q) may damage them, `null` names the arguments passed
    as NULL.  Returns (rc, message)."""
    L = capi.lib()
    res, offs = np.array(mb.results, np.uint32), np.array(mb.doc_offsets, np.uint64)               # (copies: break_ writes into them)
    b = capi.SpMatchBatch()
    b.ndocs, b.nresults = len(offs) - 1, len(res)
    b.results = ctypes.cast(res.ctypes.data, ctypes.POINTER(capi.SpResult))
    b.doc_result_offsets = ctypes.cast(offs.ctypes.data, ctypes.POINTER(ctypes.c_uint64))
    rec, toffs = np.array(terms.records, np.uint32), np.array(terms.doc_offsets, np.uint64)
    rt, st = np.array(terms.result_term, np.uint32), np.array(terms.status, np.int32)
    t = capi.SpMatchTerms()
    t.ndocs, t.nresults, t.nrecords, t.handle_bound, t.flags = len(toffs) - 1, len(rt), len(rec), terms.handle_bound, terms.flags
    t.records = ctypes.cast(rec.ctypes.data, ctypes.POINTER(capi.SpMatchTerm))
    t.doc_term_offsets = ctypes.cast(toffs.ctypes.data, ctypes.POINTER(ctypes.c_uint64))
    t.result_term = ctypes.cast(rt.ctypes.data, ctypes.POINTER(ctypes.c_uint32))
    t.doc_term_status = ctypes.cast(st.ctypes.data, ctypes.POINTER(ctypes.c_int32))
    t.totals[0] = len(rec)
    prec, eoffs, rp = np.array(postings.records, np.uint32), np.array(postings.entry_offsets, np.uint64), np.array(postings.record_posting, np.uint32)
    q = capi.SpMatchPostings()
    q.ndocs, q.nterms, q.ndict = len(toffs) - 1, len(prec), len(eoffs) - 1
    q.postings = ctypes.cast(prec.ctypes.data, ctypes.POINTER(capi.SpPosting))
    q.entry_offsets = ctypes.cast(eoffs.ctypes.data, ctypes.POINTER(ctypes.c_uint64))
    q.record_posting = ctypes.cast(rp.ctypes.data, ctypes.POINTER(ctypes.c_uint32))
    q.totals[0] = len(prec)
    if break_:
        break_(b, t, q)
    args = {"mb": b, "terms": t, "postings": q}
    out = capi.SpMatchPositions()
    out.nocc = 77                                       # (the call clears `out` first)
    err = ctypes.create_string_buffer(256)
    rc = L.sp_match_batch_positions(*[None if k in null else ctypes.byref(a) for k, a in args.items()], ctypes.byref(out), err, 256)
    if rc == 0:
        assert out.nocc == 10 and out.nterms == len(prec) and out.ndocs == len(offs) - 1 and list(out.totals) == [10, 8]
        assert np.ctypeslib.as_array(ctypes.cast(out.occurrences, ctypes.POINTER(ctypes.c_uint32)), shape=(10, 2)).tolist() == [row for rows in LISTS for row in rows]
        L.sp_match_positions_free(ctypes.byref(out))
        assert not out.occurrences and out.nocc == 0
    else:
        assert not out.occurrences and not out.posting_offsets and not out.posting_positions
        assert out.nocc == 0 and out.nterms == 0 and out.ndocs == 0 and list(out.totals) == [0, 0]
    return rc, err.value.decode()


def test_error_returns_leave_out_empty_and_the_same_objects_serve_a_good_call():
    mb, terms, d, postings = _inputs()
    assert _raw(mb, terms, postings) == (0, "")
    # a NULL argument
    for name, word in (("mb", "batch"), ("terms", "terms"), ("postings", "postings")):
        rc, msg = _raw(mb, terms, postings, null=(name,))
        assert rc == -1 and word in msg, name

    # ndocs, nresults or nterms that disagree
    def count(which, field, by):
        def damage(b, t, q):
            target = {"b": b, "t": t, "q": q}[which]
            setattr(target, field, getattr(target, field) + by)
        return damage
    for which, field in (("b", "ndocs"), ("t", "ndocs"), ("q", "ndocs"), ("b", "nresults"), ("t", "nresults"), ("t", "nrecords"), ("q", "nterms")):
        rc, msg = _raw(mb, terms, postings, count(which, field, -1))
        assert rc == -1 and "counts" in msg, (which, field)

    # offsets that do not ascend or do not cover their total: those of the documents, those of the terms
    def doc_descending(b, t, q):
        b.doc_result_offsets[1], b.doc_result_offsets[2] = 6, 5

    def doc_uncovered(b, t, q):
        b.doc_result_offsets[3] -= 1

    def doc_beyond(b, t, q):
        b.doc_result_offsets[3] += 1

    def doc_late_start(b, t, q):
        b.doc_result_offsets[0] = 1

    def term_descending(b, t, q):
        t.doc_term_offsets[1], t.doc_term_offsets[2] = 3, 2

    def term_uncovered(b, t, q):
        t.doc_term_offsets[3] -= 1

    def term_beyond(b, t, q):
        t.doc_term_offsets[3] += 1

    def term_late_start(b, t, q):
        t.doc_term_offsets[0] = 1

    def fewer_results(b, t, q):
        b.nresults -= 1
        t.nresults -= 1

    def fewer_records(b, t, q):
        t.nrecords -= 1
        q.nterms -= 1
    for damage in (doc_descending, doc_uncovered, doc_beyond, doc_late_start, term_descending, term_uncovered, term_beyond, term_late_start,
                   fewer_results, fewer_records):
        rc, msg = _raw(mb, terms, postings, damage)
        assert rc == -1 and "offsets" in msg, damage.__name__

    # a result_term at or beyond its document's records
    def term_at_count(b, t, q):
        t.result_term[5] = 1                            # document 1 has one record

    def term_far(b, t, q):
        t.result_term[0] = 0xFFFFFFFE
    for damage in (term_at_count, term_far):
        rc, msg = _raw(mb, terms, postings, damage)
        assert rc == -1 and "result_term" in msg, damage.__name__

    # a record_posting at or beyond N
    def posting_at_n(b, t, q):
        q.record_posting[2] = q.nterms

    def no_posting(b, t, q):
        q.record_posting[0] = 0xFFFFFFFF
    for damage in (posting_at_n, no_posting):
        rc, msg = _raw(mb, terms, postings, damage)
        assert rc == -1 and "record_posting" in msg, damage.__name__

    # a posting whose count is not the number of its results
    def one_more(b, t, q):
        q.postings[0].count += 1

    def moved(b, t, q):
        t.result_term[0] = 1                            # a result of (1,"eur") counted for (2,"x") of the same document

    def left_out(b, t, q):
        t.result_term[9] = 0xFFFFFFFF                   # a result that does not participate: its posting misses one
    for damage in (one_more, moved, left_out):
        rc, msg = _raw(mb, terms, postings, damage)
        assert rc == -1 and "count" in msg and "counts" not in msg, damage.__name__

    # the same objects then serve a good call; the Python call raises
    assert _raw(mb, terms, postings) == (0, "")
    bad = spa.MatchPostings(postings.records, postings.entry_offsets, np.where(postings.record_posting == 4, 5, postings.record_posting).astype(np.uint32))
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        spa.batchPositions(mb, terms, bad)
    _check(mb, terms, postings)
