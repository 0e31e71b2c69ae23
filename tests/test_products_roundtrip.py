"""The one description of the arrays of a finished-batch product (struspattern_amd/products.py, `_ARRAYS`) is read in both
directions: a hand-made product sent object -> C struct (the marshaller of the host twins) -> object (the converter of the
fetches) comes back with the same arrays, dtypes, shapes and scalars, with records and without.  Needs no device and no
library call."""
import ctypes

import numpy as np
import pytest

from struspattern_amd import products as P

u32, u64, i32 = np.uint32, np.uint64, np.int32


def _a(rows, dtype, cols=0):
    return np.array(rows, dtype).reshape((-1, cols) if cols else -1)


def _offsets(ndocs, n):
    """ndocs + 1 offsets whose last document holds the n records"""
    return _a([0] * ndocs + [n], u64)


def batch(ndocs, n):
    m = 2 * n
    return P.MatchBatch(_a(np.arange(9 * n), u32, 9), _a(np.arange(7 * m) + 100, u32, 7), _offsets(ndocs, n), _a(np.arange(4 * ndocs), u64, 4),
                        _a(np.arange(ndocs) % 2 * 5, i32), _a(np.arange(n) % 2, u32), _a(np.arange(2 * m), u32, 2))


def terms(ndocs, n):
    return P.MatchTerms(_a(np.arange(6 * n), u32, 6), _offsets(ndocs, n), _a(np.arange(n + 1), u32), _a(np.arange(ndocs) % 2 * 5, i32), flags=P.SP_TERM_TEXT,
                        handle_bound=7)


def dictionary(ndocs, n):
    records = _a(np.arange(8 * n), u32, 8)
    if n:
        records[0, 6:8] = [5, 1]            # a collection frequency above 2^32
    return P.MatchDictionary(records, _a(np.arange(n + 2), u32), _offsets(ndocs, n), _a(np.arange(4), u32))


def postings(ndocs, n):
    return P.MatchPostings(_a(np.arange(4 * n), u32, 4), _offsets(ndocs, n), _a(np.arange(n)[::-1], u32))


def positions(ndocs, n):
    return P.MatchPositions(_a(np.arange(2 * n), u32, 2), _offsets(ndocs, n), _a(np.arange(ndocs), u32), _a([n, ndocs], u64))


def pattern_freq(ndocs, n):
    return P.PatternFreq(_a(np.arange(4 * n), u32, 4), _offsets(ndocs, n), _a(np.arange(ndocs) % 2 * 5, i32), _a([0, 1 << 40, 2], u64), _a([0, 1, 1], u32))


def _assert_same(got, want, names=None):
    for a in type(want)._ARRAYS:
        if names is not None and a.attr not in names:
            continue
        g, w = getattr(got, a.attr), getattr(want, a.attr)
        if g is None and a.given and not len(w):    # (an optional array of no elements: whether it has an address is numpy's business)
            continue
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), a.attr
    for n in type(want)._SCALARS:
        assert getattr(got, n) == getattr(want, n), n


SHAPES = [(0, 0), (2, 0), (2, 3)]      # (documents, records): no documents, documents without records, records


@pytest.mark.parametrize("ndocs,n", SHAPES)
@pytest.mark.parametrize("make", [batch, terms, dictionary, postings, positions, pattern_freq], ids=lambda f: f.__name__)
def test_every_array_and_scalar_comes_back(make, ndocs, n):
    want, keep = make(ndocs, n), []
    s = P._to_c(want, keep)
    for a in type(want)._ARRAYS:            # the struct itself: the counts and, for the marshaller's own arrays, the pointers
        if a.count:
            assert getattr(s, a.count) + a.plus == len(getattr(want, a.attr)), a.attr
            assert getattr(s, a.field) or len(getattr(want, a.attr)) == 0, a.attr
    if type(want)._TOTAL:
        assert s.totals[0] == getattr(s, type(want)._TOTAL) == len(want.records)
    got = P._from_c(type(want), s)
    _assert_same(got, want)
    if make is dictionary:
        assert got.counts.dtype == np.uint64 and np.array_equal(got.counts, want.counts) and (n == 0 or int(got.counts[0]) == (1 << 32) + 5)
    if make is positions:
        assert got.totals.tolist() == [n, ndocs]


@pytest.mark.parametrize("ndocs,n", SHAPES)
def test_scalars_given_to_the_marshaller_win_over_those_of_the_object(ndocs, n):
    keep = []
    t = P._to_c(terms(ndocs, n), keep, handle_bound=11)
    assert (t.handle_bound, t.flags, t.ndocs, t.nrecords, t.nresults) == (11, P.SP_TERM_TEXT, ndocs, n, n + 1)
    d = P._to_c(dictionary(ndocs, n), keep, flags=3)
    assert (d.flags, d.handle_bound, d.ndict, d.nterms, d.ndocs) == (3, 4, n, n + 2, ndocs)     # (the bound: the length of handle_terms)
    p = P._to_c(postings(ndocs, n), keep, ndocs=9)
    assert (p.ndocs, p.nterms, p.ndict) == (9, n, ndocs)


@pytest.mark.parametrize("ndocs,n", SHAPES)
def test_batch_modes_of_the_twins(ndocs, n):
    want = batch(ndocs, n)
    b, keep = P._host_batch(want)                                  # results and offsets alone
    got = P._from_c(P.MatchBatch, b)
    _assert_same(got, want, ("results", "doc_offsets"))
    assert (b.ndocs, b.nresults, b.nitems) == (ndocs, n, 0) and not b.items and not b.doc_status and not b.result_format and not b.item_format
    assert got.items.shape == (0, 7) and got.status.shape == (ndocs,) and got.stats.shape == (ndocs, 4) and got.result_format is None and got.item_format is None
    b, keep = P._host_batch(want, items=True, formats="all", status=True)
    assert b.nitems == 2 * n
    got = P._from_c(P.MatchBatch, b)
    _assert_same(got, want, ("results", "items", "doc_offsets", "status") + (("result_format", "item_format") if n else ()))
    if not n:   # (whether an array of no elements has an address is numpy's business: no formats, or none of them)
        assert got.result_format is None or (got.result_format.shape == (0,) and got.item_format.shape == (0, 2))
    b, keep = P._host_batch(want, formats="results")
    assert (b.result_format or not n) and not b.item_format and not b.doc_status
    want.result_format = want.result_format[:-1] if n else _a([1], u32)
    with pytest.raises(P.PatternError, match="format array of the batch is not parallel to its results"):
        P._host_batch(want, formats="results")
    with pytest.raises(P.PatternError, match="format arrays of the batch are not parallel to its results and items"):
        P._host_batch(want, items=True, formats="all")
    want.result_format = None
    b, keep = P._host_batch(want, items=True, formats="all")
    assert not b.result_format and not b.item_format


@pytest.mark.parametrize("cls", [P.MatchValues, P.MatchText], ids=lambda c: c.__name__)
@pytest.mark.parametrize("ndocs,strings", [(0, []), (2, []), (2, [b"ab", b"", b"cde"]), (1, [b""])])
def test_byte_families(cls, ndocs, strings):
    offs = np.cumsum([0] + [len(s) for s in strings]).astype(u64)
    want, keep = cls(b"".join(strings), offs, None, None, _a(np.arange(ndocs) % 2 * 5, i32)), []
    c = P._host_source(want, keep)
    assert (c.ndocs, c.nresults, c.nitems, c.totals[0], c.totals[1]) == (ndocs, len(strings), 0, len(b"".join(strings)), 0)
    assert getattr(c, cls._results[0]) and getattr(c, cls._results[1])        # a pointer that is not null, also for no bytes
    assert ctypes.string_at(getattr(c, cls._results[0]), c.totals[0] + 1)[-1:] == b"\0"
    got = P._from_c(cls, c)
    assert type(got) is cls
    assert getattr(got, cls._results[0]) == b"".join(strings) and [got.result(r) for r in range(len(strings))] == strings
    assert got.result_offsets.dtype == u64 and got.result_offsets.shape == offs.shape and np.array_equal(got.result_offsets, offs)
    assert got.status.dtype == i32 and got.status.shape == (ndocs,) and np.array_equal(got.status, want.status)
    assert getattr(got, cls._items[0]) is None and got.item_offsets is None
    # without the results family the struct has the status alone
    c = P._host_source(cls(None, None, None, None, want.status), keep)
    assert (c.ndocs, c.nresults) == (ndocs, 0) and not getattr(c, cls._results[0]) and not getattr(c, cls._results[1])
    got = P._from_c(cls, c)
    assert getattr(got, cls._results[0]) is None and got.result_offsets is None and np.array_equal(got.status, want.status)
    assert P._host_source(None, keep) is None
