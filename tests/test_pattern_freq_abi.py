"""sp_match_batch_pattern_freq (csrc/pattern_freq.hpp), the device-free twin of the frequency passes: the C++ statement of
the rule against the numpy one (tests/pattern_freq_model.py) over hand-made batches -- the trip sizes, one handle and all
handles distinct, minima and maxima away from the first and last record, a failed document, the range rule, the arguments
that are refused -- and against counts taken from the oracle's results.  Needs no device."""
import ctypes

import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from struspattern_amd import capi, synth
from tests import pattern_freq_model as model

SP_ERR_INVALID = -1


def make_batch(docs, failed=()):
    """docs: per document a list of (handle, ordpos, ordend) -> MatchBatch in the finished layout; a failed document has
    status 2 and no results"""
    results, offs = [], [0]
    for d, doc in enumerate(docs):
        assert not (d in failed and doc)
        results += [[h, p, e, 0, 0, 0, 0, 0, 0] for h, p, e in doc]
        offs.append(len(results))
    status = np.zeros(len(docs), np.int32)
    status[list(failed)] = 2
    return spa.MatchBatch(np.array(results, np.uint32).reshape(-1, 9), np.zeros((0, 7), np.uint32), np.array(offs, np.uint64),
                          np.zeros((len(docs), 4), np.uint64), status)


def check(mb, bound):
    got = spa.batchPatternFreq(mb, bound)
    model.assert_same(got, model.batch_pattern_freq(mb.results, mb.doc_offsets, bound, mb.status))
    return got


def test_symbols_and_signatures():
    names = ("sp_matcher_handle_bound", "sp_matcher_ctx_finished_pattern_freq_device", "sp_matcher_ctx_finished_pattern_freq_fetch",
             "sp_pattern_freq_batch_free", "sp_matcher_ctx_last_pattern_freq_ms", "sp_matcher_pattern_freq_window", "sp_match_batch_pattern_freq")
    for name in names:
        assert name in capi.SIGNATURES and hasattr(capi.lib(), name)
    vp, P, u32 = ctypes.c_void_p, ctypes.POINTER, ctypes.c_uint32
    assert capi.SIGNATURES["sp_matcher_handle_bound"] == (u32, [vp])
    assert capi.SIGNATURES["sp_matcher_ctx_finished_pattern_freq_device"] == (ctypes.c_int, [vp, vp, P(capi.SpPatternFreqDevice)])
    assert capi.SIGNATURES["sp_matcher_ctx_finished_pattern_freq_fetch"] == (ctypes.c_int, [vp, P(capi.SpPatternFreqBatch)])
    assert capi.SIGNATURES["sp_matcher_ctx_last_pattern_freq_ms"] == (ctypes.c_int, [vp, P(ctypes.c_double)])
    assert capi.SIGNATURES["sp_match_batch_pattern_freq"] == (ctypes.c_int, [P(capi.SpMatchBatch), u32, P(capi.SpPatternFreqBatch), ctypes.c_char_p, ctypes.c_size_t])
    assert [n for n, _ in capi.SpPatternFreq._fields_] == ["handle", "count", "first_ordpos", "last_ordend"] and ctypes.sizeof(capi.SpPatternFreq) == 16
    assert [n for n, _ in capi.SpPatternFreqDevice._fields_] == ["ndocs", "handle_bound", "d_records", "d_doc_offsets", "d_doc_freq_status",
                                                                 "d_handle_results", "d_handle_docs", "d_totals"]
    window = capi.lib().sp_matcher_pattern_freq_window()
    assert window >= 2048 and window % 2048 == 0


def test_handle_bound_is_one_more_than_the_pattern_names():
    m = spa.PatternMatcherInstance()
    assert m.handleBound() == 1
    for k in range(5):
        m.pushTerm(k + 1)
        m.definePattern("p%d" % (k % 3), "", True)           # three names, two of them twice
    m.compile()
    assert m.handleBound() == 4 and m.patternName(m.handleBound() - 1) and not m.patternName(m.handleBound())


def test_document_sizes_one_handle_and_all_distinct():
    docs = []
    for n in (0, 1, 2, 65):
        docs.append([(250, 3 * k, 3 * k + 2) for k in range(n)])                # one handle
        docs.append([(1 + (k * 37) % 200, 5 + k, 9 + k) for k in range(n)])     # all handles distinct, not ascending
    got = check(make_batch(docs), 251)
    assert np.diff(got.doc_offsets.astype(np.int64)).tolist() == [0, 0, 1, 1, 1, 2, 1, 65]
    assert got.doc(6).tolist() == [[250, 65, 0, 3 * 64 + 2]]
    last = got.doc(7)
    assert np.all(np.diff(last[:, 0].astype(np.int64)) > 0) and np.all(last[:, 1] == 1)
    assert int(got.handle_results[250]) == 1 + 2 + 65 and int(got.handle_docs[250]) == 3
    assert int(got.handle_results.sum()) == 2 * (1 + 2 + 65) and int(got.handle_docs.sum()) == len(got.records)
    assert got.handle_results[0] == 0 and got.handle_docs[0] == 0


def test_minimum_and_maximum_are_not_the_first_and_last_record():
    doc = [(4, 50, 51), (9, 7, 8), (4, 10, 90), (4, 30, 31), (9, 6, 7), (9, 8, 9)]
    got = check(make_batch([doc]), 10)
    assert got.records.tolist() == [[4, 3, 10, 90], [9, 3, 6, 9]]
    # the same multiset in another order: the same bytes
    again = check(make_batch([doc[::-1]]), 10)
    assert np.array_equal(got.records, again.records)
    # unsigned values: positions above 2^31
    big = [(2, 0xFFFFFFF0, 0xFFFFFFFE), (2, 0x80000000, 0x80000001), (2, 5, 6)]
    assert check(make_batch([big]), 3).records.tolist() == [[2, 3, 5, 0xFFFFFFFE]]


def test_failed_document_is_empty_with_status_0():
    docs = [[(1, 0, 1)], [], [(2, 4, 5), (1, 1, 2)], []]
    got = check(make_batch(docs, failed=[1]), 3)
    assert got.status.tolist() == [0, 0, 0, 0] and got.doc_offsets.tolist() == [0, 1, 1, 3, 3]
    assert got.handle_docs.tolist() == [0, 2, 1] and got.handle_results.tolist() == [0, 2, 1]
    # a document with a status has no records whatever its range holds
    mb = make_batch([[(1, 0, 1)], [(2, 0, 1)]])
    mb.status[1] = 1
    got = check(mb, 3)
    assert got.doc_offsets.tolist() == [0, 1, 1] and got.status.tolist() == [0, 0]


@pytest.mark.parametrize("bad", [0, 6, 7, 0xFFFFFFFF], ids=["handle 0", "handle = bound", "handle > bound", "handle 2^32-1"])
def test_range_rule(bad):
    bound = 6
    first = [(5, 1, 2), (1, 0, 9)]
    middle = [(2, 0, 1), (bad, 3, 4), (2, 5, 6)]
    last = [(5, 7, 8)]
    got = check(make_batch([first, middle, last]), bound)
    assert got.status.tolist() == [0, model.SP_DOC_ERR_RANGE, 0]
    assert got.doc_offsets.tolist() == [0, 2, 2, 3]
    # the neighbours are what they are without the middle document, which is absent from the sums
    without = check(make_batch([first, [], last]), bound)
    assert np.array_equal(got.records, without.records)
    assert np.array_equal(got.handle_results, without.handle_results) and np.array_equal(got.handle_docs, without.handle_docs)
    assert got.handle_docs[2] == 0 and got.handle_results[2] == 0
    # the largest valid handle is bound - 1
    assert check(make_batch([[(bound - 1, 0, 1)]]), bound).status.tolist() == [0]


def test_refused_arguments_return_a_message():
    L = capi.lib()
    mb = make_batch([[(1, 0, 1), (1, 2, 3)], [(1, 4, 5)]])
    with pytest.raises(spa.PatternError, match=r"\(-1\).*bound"):
        spa.batchPatternFreq(mb, 0)
    for offs in ([0, 3, 2], [0, 1, 2], [0, 2, 4], [1, 2, 3]):       # descending, not covering, beyond, not from 0
        mb.doc_offsets = np.array(offs, np.uint64)
        with pytest.raises(spa.PatternError, match=r"\(-1\).*offsets"):
            spa.batchPatternFreq(mb, 4)
    f = capi.SpPatternFreqBatch()
    err = ctypes.create_string_buffer(128)
    assert L.sp_match_batch_pattern_freq(None, 4, ctypes.byref(f), err, 128) == SP_ERR_INVALID and err.value
    assert not f.records and not f.doc_offsets
    # no documents: valid and empty
    got = check(make_batch([]), 2)
    assert got.doc_offsets.tolist() == [0] and len(got.records) == 0 and got.handle_docs.tolist() == [0, 0]


def test_random_batches_against_the_model():
    rng = np.random.default_rng(11)
    for _ in range(20):
        bound = int(rng.integers(2, 40))
        docs = []
        for _ in range(int(rng.integers(0, 8))):
            n = int(rng.integers(0, 90))
            slack = 1 if rng.random() < 0.2 else 0              # now and then a handle of 0 or of the bound
            docs.append([(int(rng.integers(1 - slack, bound + slack)), int(rng.integers(0, 1000)), int(rng.integers(0, 1000))) for _ in range(n)])
        check(make_batch(docs), bound)


def test_counts_of_the_oracles_results():
    """the expectation comes from the oracle's results, counted here result by result"""
    rules = synth.random_rules(30, 12, 3)
    lex, offs = synth.random_documents(12, 120, 12, 4)
    om = oracle.L2Matcher()
    synth.apply_rules(om, rules)
    ref = om.run(synth.lexems5(lex), offs)
    assert len(ref.results) > 100 and not ref.status.any()
    bound = 1 + len({name for name, _, _, _ in rules})
    assert int(ref.results[:, 0].max()) < bound
    got = spa.batchPatternFreq(spa.MatchBatch(ref.results, ref.items, ref.doc_offsets, ref.stats, ref.status), bound)
    assert not got.status.any()
    collection, documents = {}, {}
    for d in range(len(offs) - 1):
        want = {}
        for r in ref.doc(d):
            h, p, e = int(r[0]), int(r[1]), int(r[2])
            n, lo, hi = want.get(h, (0, p, e))
            want[h] = (n + 1, min(lo, p), max(hi, e))
        assert [tuple(int(x) for x in rec) for rec in got.doc(d)] == [(h, *want[h]) for h in sorted(want)]
        for h, (n, _, _) in want.items():
            collection[h] = collection.get(h, 0) + n
            documents[h] = documents.get(h, 0) + 1
    assert {h: int(n) for h, n in enumerate(got.handle_results) if n} == collection
    assert {h: int(n) for h, n in enumerate(got.handle_docs) if n} == documents
    assert len({len(got.doc(d)) for d in range(len(offs) - 1)}) > 1 and max(collection.values()) > 1
