"""Batch postings without a device (sp_match_batch_postings, csrc/match_postings.hpp): the twin equals the model
(tests/postings_model.py) on the four-document batch of tests/test_dictionary_abi.py, with every expected posting written out
by hand; every error return of the header, after which the same objects serve a good call; empty shapes; and the malformed
offsets of tests/test_host_twins_abi.py, here those of the terms."""
import ctypes

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi
from tests import postings_model as model
from tests.finished_support import (_batch, DICT_EXPECTED, _dict_inputs, _family, T, TWIN_BAD_OFFSETS, _twin_batch, TWIN_BOUND, TWIN_RESULT_TEXT,
                                    TWIN_TERMS, TWIN_VALUES, V)

# flags -> (postings per entry [doc, term, count, first_ordpos], entry_offsets, record_posting)
EXPECTED = {
    # the text: (1,"eur") in the documents 0, 2 and 3; (2,"x") in 0 and 3; (3,"") in 0 and 2
    T: ([[[0, 0, 2, 1], [2, 0, 3, 1], [3, 0, 1, 1]], [[0, 1, 1, 7]], [[0, 2, 1, 5], [3, 1, 1, 3]], [[0, 3, 1, 9], [2, 1, 1, 3]], [[1, 0, 1, 3]], [[1, 1, 1, 1]]],
        [0, 3, 4, 6, 8, 9, 10], [0, 3, 4, 6, 8, 9, 1, 7, 2, 5]),
    # the values: the empty value of the unformatted results of handle 1 in the documents 0, 2 and 3
    V: ([[[0, 0, 2, 1], [2, 1, 1, 5]], [[0, 1, 1, 7], [2, 0, 2, 1], [3, 0, 1, 1]], [[0, 2, 1, 5], [1, 1, 1, 1]], [[0, 3, 1, 9], [2, 2, 1, 3]], [[1, 0, 1, 3]], [[3, 1, 1, 3]]],
        [0, 2, 5, 7, 9, 10, 11], [0, 2, 5, 7, 9, 6, 3, 1, 8, 4, 10]),
    # both: the formatted "eur" of document 1 heads the list of the text "eur" of the documents 2 and 3
    V | T: ([[[0, 0, 2, 1], [2, 1, 1, 5]], [[0, 1, 1, 7]], [[0, 2, 1, 5], [3, 1, 1, 3]], [[0, 3, 1, 9], [2, 2, 1, 3]], [[1, 0, 1, 3], [2, 0, 2, 1], [3, 0, 1, 1]], [[1, 1, 1, 1]]],
            [0, 2, 3, 5, 7, 10, 11], [0, 2, 3, 5, 7, 10, 8, 1, 6, 9, 4]),
}


def _dictionary(flags, **kw):
    mb, mv, mt, terms = _dict_inputs(flags, **kw)
    return terms, spa.batchDictionary(mb, terms, values=mv, text=mt)


def _check(terms, d):
    got = spa.batchPostings(terms, d)
    model.assert_same(got, model.of_batch(terms, d))
    model.check_invariants(got, terms, d)
    return got


def test_symbols_and_signatures():
    vp, P = ctypes.c_void_p, ctypes.POINTER
    for name in ("sp_matcher_ctx_finished_postings_device", "sp_matcher_ctx_finished_postings_fetch", "sp_match_postings_free",
                 "sp_matcher_ctx_last_postings_ms", "sp_match_batch_postings", "sp_matcher_postings_tile", "sp_test_postings_digit_bits"):
        assert name in capi.SIGNATURES and hasattr(capi.lib(), name)
    assert capi.SIGNATURES["sp_matcher_ctx_finished_postings_device"] == (ctypes.c_int, [vp, vp, P(capi.SpMatchPostingsDevice)])
    assert capi.SIGNATURES["sp_match_batch_postings"][1][:3] == [P(capi.SpMatchTerms), P(capi.SpMatchDictionary), P(capi.SpMatchPostings)]
    assert ctypes.sizeof(capi.SpPosting) == 16 and capi.SpPosting.first_ordpos.offset == 12
    assert [n for n, _ in capi.SpMatchPostingsDevice._fields_] == ["ndocs", "nterms", "ndict", "d_postings", "d_entry_offsets", "d_record_posting", "d_totals"]
    for name in ("finishedPostingsDevice", "finishedPostingsFetch", "lastPostingsMs"):
        assert hasattr(spa.PatternMatcherContext, name)
    for name in ("MatchPostings", "batchPostings"):
        assert name in spa.__all__
    tile = capi.lib().sp_matcher_postings_tile()
    assert tile >= 64 and tile % 64 == 0


@pytest.mark.parametrize("flags", [V, T, V | T])
def test_three_flag_combinations_equal_the_model_and_the_postings_written_out(flags):
    terms, d = _dictionary(flags)
    assert d.term_dict.tolist() == DICT_EXPECTED[flags][1]
    got = _check(terms, d)
    lists, offsets, record_posting = EXPECTED[flags]
    assert got.records.tolist() == [row for rows in lists for row in rows]
    assert got.entry_offsets.tolist() == offsets and got.record_posting.tolist() == record_posting
    assert got.records.dtype == np.uint32 and got.entry_offsets.dtype == np.uint64 and got.record_posting.dtype == np.uint32
    for e, rows in enumerate(lists):
        assert got.entry(e).tolist() == rows and got.docs(e).tolist() == [row[0] for row in rows]


def test_a_document_without_term_records_has_no_posting():
    terms, d = _dictionary(T, text_status=[0, 5, 0, 0])
    assert terms.doc_offsets.tolist() == [0, 4, 4, 6, 8]
    got = _check(terms, d)
    assert not np.any(got.records[:, 0] == 1) and got.entry_offsets.tolist() == [0, 3, 4, 6, 8]
    assert got.docs(0).tolist() == [0, 2, 3] and got.docs(3).tolist() == [0, 2]


def test_no_documents_and_no_records():
    for ndocs in (0, 2):
        mb = _batch([[]] * ndocs)
        mt = _family(spa.MatchText, [], ndocs)
        terms = spa.batchTerms(mb, text=mt, handle_bound=3, flags=T)
        d = spa.batchDictionary(mb, terms, text=mt)
        got = _check(terms, d)
        assert got.records.shape == (0, 4) and got.entry_offsets.tolist() == [0] and len(got.record_posting) == 0


def _raw(terms, d, break_=None, null=()):
    """sp_match_batch_postings over hand-filled C structs; break_( t, q) may damage them, `null` names the arguments passed
    as NULL.  Returns (rc, message)."""
    L = capi.lib()
    rec, toffs = np.array(terms.records, np.uint32), np.array(terms.doc_offsets, np.uint64)       # (copies: break_ writes into them)
    rt, st = np.array(terms.result_term, np.uint32), np.array(terms.status, np.int32)
    t = capi.SpMatchTerms()
    t.ndocs, t.nresults, t.nrecords, t.handle_bound, t.flags = len(toffs) - 1, len(rt), len(rec), terms.handle_bound, terms.flags
    t.records = ctypes.cast(rec.ctypes.data, ctypes.POINTER(capi.SpMatchTerm))
    t.doc_term_offsets = ctypes.cast(toffs.ctypes.data, ctypes.POINTER(ctypes.c_uint64))
    t.result_term = ctypes.cast(rt.ctypes.data, ctypes.POINTER(ctypes.c_uint32))
    t.doc_term_status = ctypes.cast(st.ctypes.data, ctypes.POINTER(ctypes.c_int32))
    t.totals[0] = len(rec)
    drec, td = np.array(d.records, np.uint32), np.array(d.term_dict, np.uint32)
    doffs, ht = np.array(d.doc_offsets, np.uint64), np.array(d.handle_terms, np.uint32)
    q = capi.SpMatchDictionary()
    q.ndocs, q.nterms, q.ndict, q.handle_bound, q.flags = len(doffs) - 1, len(td), len(drec), len(ht), terms.flags
    q.records = ctypes.cast(drec.ctypes.data, ctypes.POINTER(capi.SpDictTerm))
    q.term_dict = ctypes.cast(td.ctypes.data, ctypes.POINTER(ctypes.c_uint32))
    q.doc_dict_offsets = ctypes.cast(doffs.ctypes.data, ctypes.POINTER(ctypes.c_uint64))
    q.handle_terms = ctypes.cast(ht.ctypes.data, ctypes.POINTER(ctypes.c_uint32))
    q.totals[0] = len(drec)
    if break_:
        break_(t, q)
    args = {"terms": t, "dict": q}
    p = capi.SpMatchPostings()
    p.nterms = 77                                       # (the call clears `out` first)
    err = ctypes.create_string_buffer(256)
    rc = L.sp_match_batch_postings(*[None if k in null else ctypes.byref(a) for k, a in args.items()], ctypes.byref(p), err, 256)
    if rc == 0:
        assert p.nterms == len(rec) and p.ndict == len(drec) and p.ndocs == len(toffs) - 1 and p.totals[0] == len(rec)
        assert [list(row) for row in np.ctypeslib.as_array(ctypes.cast(p.postings, ctypes.POINTER(ctypes.c_uint32)), shape=(len(rec), 4)).tolist()] \
            == [row for rows in EXPECTED[terms.flags][0] for row in rows]
        L.sp_match_postings_free(ctypes.byref(p))
        assert not p.postings and p.nterms == 0
    else:
        assert not p.postings and not p.entry_offsets and not p.record_posting and p.nterms == 0 and p.ndict == 0 and p.totals[0] == 0
    return rc, err.value.decode()


def test_error_returns_and_the_same_objects_serve_a_good_call():
    terms, d = _dictionary(V | T)
    assert _raw(terms, d) == (0, "")
    # a NULL argument
    rc, msg = _raw(terms, d, null=("terms",))
    assert rc == -1 and "terms" in msg
    rc, msg = _raw(terms, d, null=("dict",))
    assert rc == -1 and "dictionary" in msg

    # ndocs or nterms that disagree between the two inputs
    def count(which, field, by):
        def damage(t, q):
            target = t if which == "t" else q
            setattr(target, field, getattr(target, field) + by)
        return damage
    for which, field in (("t", "ndocs"), ("q", "ndocs"), ("q", "nterms")):
        rc, msg = _raw(terms, d, count(which, field, -1))
        assert rc == -1 and "counts" in msg, (which, field)

    # term offsets that do not ascend or do not cover nrecords
    def descending(t, q):
        t.doc_term_offsets[1], t.doc_term_offsets[2] = 6, 4

    def uncovered(t, q):
        t.doc_term_offsets[4] -= 1

    def beyond(t, q):
        t.doc_term_offsets[4] += 1

    def late_start(t, q):
        t.doc_term_offsets[0] = 1

    def fewer_records(t, q):
        t.nrecords -= 1
        q.nterms -= 1
    for damage in (descending, uncovered, beyond, late_start, fewer_records):
        rc, msg = _raw(terms, d, damage)
        assert rc == -1 and "offsets" in msg, damage.__name__

    # a term_dict[i] at or beyond ndict
    def entry_at_ndict(t, q):
        q.term_dict[3] = q.ndict

    def no_entry(t, q):
        q.term_dict[10] = 0xFFFFFFFF
    for damage in (entry_at_ndict, no_entry):
        rc, msg = _raw(terms, d, damage)
        assert rc == -1 and "term_dict" in msg, damage.__name__

    # a doc_freq that is not the number of records of its entry
    def one_more(t, q):
        q.records[4].doc_freq += 1

    def moved(t, q):
        q.term_dict[1] = 0                              # entry 0 gets a record of entry 1: both counts are wrong
    for damage in (one_more, moved):
        rc, msg = _raw(terms, d, damage)
        assert rc == -1 and "doc_freq" in msg, damage.__name__

    # the same objects then serve a good call; the Python call raises
    assert _raw(terms, d) == (0, "")
    bad = spa.MatchDictionary(d.records, np.where(d.term_dict == 5, 6, d.term_dict).astype(np.uint32), d.doc_offsets, d.handle_terms)
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        spa.batchPostings(terms, bad)
    _check(terms, d)


@pytest.mark.parametrize("offsets", sorted(TWIN_BAD_OFFSETS))
def test_malformed_term_offsets_are_refused_and_the_same_objects_serve_a_good_call(offsets):
    mb = _twin_batch()
    d = spa.batchDictionary(mb, TWIN_TERMS, values=TWIN_VALUES, text=TWIN_RESULT_TEXT)
    terms = spa.MatchTerms(TWIN_TERMS.records, np.array(TWIN_BAD_OFFSETS[offsets], np.uint64), TWIN_TERMS.result_term, TWIN_TERMS.status,
                           TWIN_TERMS.flags, TWIN_BOUND)
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        spa.batchPostings(terms, d)
    terms.doc_offsets = np.array([0, 2], np.uint64)
    got = _check(terms, d)
    # (1, "cd") of result 1 at ordinal position 1, (2, "<ab>") of result 0 at 0: one document, every list a single posting
    assert got.records.tolist() == [[0, 0, 1, 1], [0, 1, 1, 0]] and got.entry_offsets.tolist() == [0, 1, 2] and got.record_posting.tolist() == [0, 1]
