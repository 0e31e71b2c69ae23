"""CPU tests (no GPU) of the host fetch layer (struspattern_amd/csrc/batch_fetch.hpp) through the test entry
sp_match_batch_regroup: what batchFetch(first_doc, ndocs) makes of the arrays the rule kernels leave on the device -- whole
documents appended in completion order, a (first, count) range and a status per document -- with memcpy in the place of
the device copies.  The `exclusive` elimination is pinned against the oracle."""
import ctypes
import random

import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from struspattern_amd import capi, synth
from .finished_support import _apply, _random_program

MAX_RESULT_SIZE = 30


class DeviceLayout:
    """a batch as the kernels leave it: the documents' result and item blocks in the order `order` (completion order)"""

    def __init__(self, ref, order):
        ndocs = len(ref.doc_offsets) - 1
        offs = ref.doc_offsets.astype(np.int64)
        res, items, rfmt, ifmt = [], [], [], []
        self.ranges = np.zeros((ndocs, 2), np.uint64)
        self.status = np.zeros(ndocs, np.int32)
        nres = nitems = 0
        for d in order:
            r = ref.results[offs[d]:offs[d + 1]].copy()
            ib, ie = self._item_block(r)
            r[:, 7] = r[:, 7] - ib + nitems                 # the device's item_begin: an index into ITS item array
            res.append(r)
            items.append(ref.items[ib:ie])
            if ref.result_format is not None:
                rfmt.append(ref.result_format[offs[d]:offs[d + 1]])
                ifmt.append(ref.item_format[ib:ie])
            self.ranges[d] = (nres, len(r))
            nres += len(r)
            nitems += ie - ib
        self.results = np.ascontiguousarray(np.concatenate(res))
        self.items = np.ascontiguousarray(np.concatenate(items))
        self.result_format = np.ascontiguousarray(np.concatenate(rfmt)) if rfmt else None
        self.item_format = np.ascontiguousarray(np.concatenate(ifmt)) if ifmt else None
        self.nresults, self.nitems = len(self.results), len(self.items)     # what lies inside the device buffers

    @staticmethod
    def _item_block(r):
        with_items = r[r[:, 8] > 0]
        if not len(with_items):
            return 0, 0
        return int(with_items[0, 7]), int(with_items[0, 7]) + int(r[:, 8].sum())

    def regroup(self, first_doc=None, ndocs=None, exclusive=False, formats=True):
        if first_doc is None:
            first_doc, ndocs = 0, len(self.ranges)
        formats = formats and self.result_format is not None
        b = capi.SpMatchBatch()
        err = ctypes.create_string_buffer(256)
        L = capi.lib()
        rc = L.sp_match_batch_regroup(self.results.ctypes.data, self.nresults, self.items.ctypes.data, self.nitems,
                                      self.result_format.ctypes.data if formats else None, self.item_format.ctypes.data if formats else None,
                                      self.ranges.ctypes.data, self.status.ctypes.data, len(self.ranges), first_doc, ndocs,
                                      int(exclusive), MAX_RESULT_SIZE, ctypes.byref(b), err, 256)
        try:
            if rc != 0:
                raise spa.PatternError(err.value.decode())
            return spa._match_batch_of(b)
        finally:
            L.sp_match_batch_free(ctypes.byref(b))


def _assert_gap_free(b):
    """item_begin is the running sum of item_count"""
    assert np.array_equal(b.results[:, 7], np.cumsum(b.results[:, 8], dtype=np.uint64) - b.results[:, 8])
    assert len(b.items) == int(b.results[:, 8].sum())


@pytest.fixture(scope="module")
def exclusive_case():
    """the shape of test_exclusive_option: (oracle without options, oracle with `exclusive`, the device layout of the first)"""
    rules = synth.random_rules(300, 20, 3)
    lex, offs = synth.random_documents(60, 200, 20, 4)
    raw, excl = oracle.L2Matcher(), oracle.L2Matcher()
    excl.defineOption("exclusive")
    excl.defineOption("maxResultSize", MAX_RESULT_SIZE)
    synth.apply_rules(raw, rules)
    synth.apply_rules(excl, rules)
    raw, excl = raw.run(synth.lexems5(lex), offs), excl.run(synth.lexems5(lex), offs)
    order = list(range(len(offs) - 1))
    random.Random(7).shuffle(order)
    return raw, excl, DeviceLayout(raw, order)


@pytest.fixture(scope="module")
def format_case():
    """documents of a program with format strings (tests/test_formats.py) in a permuted device layout"""
    omt = oracle.L2Matcher()
    _apply(omt, _random_program(random.Random(9102), 6))      # (a seed with item-less results between results with items)
    lex, offs = synth.random_documents(12, 60, 6, seed=52)
    ref = omt.run(synth.lexems5(lex), offs)
    assert ref.result_format is not None and len(ref.results) > 50
    assert (ref.results[:, 8] == 0).any() and (ref.results[:, 8] > 0).any()
    order = list(range(12))
    random.Random(3).shuffle(order)
    return ref, DeviceLayout(ref, order)


def test_exclusive_regroup_equals_the_oracle(exclusive_case):
    raw, excl, dev = exclusive_case
    ndocs = len(raw.doc_offsets) - 1
    assert len(excl.results) < len(raw.results)
    changed = sum(1 for d in range(ndocs) if len(excl.doc(d)) != len(raw.doc(d)))
    assert changed > ndocs // 2                             # (the elimination is at work in most documents)
    got = dev.regroup(exclusive=True)
    assert len(got.results) < dev.nresults
    assert np.array_equal(got.doc_offsets, excl.doc_offsets)
    assert np.array_equal(got.results[:, :7], excl.results[:, :7])
    assert np.array_equal(got.results[:, 8], excl.results[:, 8])
    assert np.array_equal(got.items, excl.items)
    _assert_gap_free(got)
    assert got.result_format is None and not got.status.any() and not got.stats.any()


def test_plain_regroup_is_the_raw_results_in_document_order(exclusive_case):
    raw, _, dev = exclusive_case
    got = dev.regroup(exclusive=False)
    assert np.array_equal(got.doc_offsets, raw.doc_offsets)
    assert np.array_equal(got.results[:, :7], raw.results[:, :7])
    assert np.array_equal(got.results[:, 8], raw.results[:, 8])
    assert np.array_equal(got.items, raw.items)
    _assert_gap_free(got)


def _assert_slice(sub, whole, first, n):
    lo, hi = int(whole.doc_offsets[first]), int(whole.doc_offsets[first + n])
    ilo = int(whole.results[:lo, 8].sum())
    ihi = ilo + int(whole.results[lo:hi, 8].sum())
    assert np.array_equal(sub.doc_offsets, whole.doc_offsets[first:first + n + 1] - whole.doc_offsets[first])
    assert np.array_equal(sub.status, whole.status[first:first + n])
    assert np.array_equal(sub.results[:, :7], whole.results[lo:hi, :7])
    assert np.array_equal(sub.results[:, 8], whole.results[lo:hi, 8])
    assert np.array_equal(sub.items, whole.items[ilo:ihi])
    _assert_gap_free(sub)
    if whole.result_format is None:
        assert sub.result_format is None and sub.item_format is None
    else:
        assert np.array_equal(sub.result_format, whole.result_format[lo:hi])
        assert np.array_equal(sub.item_format, whole.item_format[ilo:ihi])


def _ranges(ndocs):
    return [(0, 0), (0, 1), (5, 3), (ndocs - 1, 1), (ndocs, 0)]


@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("formats", [False, True])
def test_sub_range_equals_the_slice_of_the_whole_batch(format_case, exclusive, formats):
    ref, dev = format_case
    ndocs = len(dev.ranges)
    whole = dev.regroup(exclusive=exclusive, formats=formats)
    assert (whole.result_format is not None) == formats
    if not exclusive:
        assert np.array_equal(whole.results[:, :7], ref.results[:, :7]) and np.array_equal(whole.items, ref.items)
        if formats:
            assert np.array_equal(whole.result_format, ref.result_format) and np.array_equal(whole.item_format, ref.item_format)
    for first, n in _ranges(ndocs):
        _assert_slice(dev.regroup(first, n, exclusive=exclusive, formats=formats), whole, first, n)
    with pytest.raises(spa.PatternError, match="document range outside the last batch"):
        dev.regroup(ndocs + 1, 0)
    with pytest.raises(spa.PatternError, match="document range outside the last batch"):
        dev.regroup(ndocs - 1, 2)


def test_sub_range_of_the_exclusive_case(exclusive_case):
    _, _, dev = exclusive_case
    whole = dev.regroup(exclusive=True)
    for first, n in _ranges(len(dev.ranges)):
        _assert_slice(dev.regroup(first, n, exclusive=True), whole, first, n)


def test_failed_and_out_of_buffer_documents_come_out_empty(format_case):
    ref, dev = format_case
    ndocs = len(dev.ranges)
    good = dev.regroup()
    failed = 6                                              # in the middle of (5, 3)
    last = max(range(ndocs), key=lambda d: int(dev.ranges[d, 0]))     # the document at the end of the device buffer
    assert last != failed and dev.ranges[last, 1] > 0 and dev.ranges[failed, 1] > 0
    bad = DeviceLayout.__new__(DeviceLayout)
    bad.__dict__.update(dev.__dict__)
    bad.status = dev.status.copy()
    bad.status[failed] = 1
    bad.nresults = dev.nresults - 1                         # the range of `last` ends one record past the buffer count
    for first, n in [(0, ndocs)] + [r for r in _ranges(ndocs)] + [(last, 1), (failed, 1)]:
        got = bad.regroup(first, n)
        for d in range(first, first + n):
            mine = got.doc(d - first)
            if d in (failed, last):
                assert len(mine) == 0
            else:
                assert np.array_equal(mine[:, :7], good.doc(d)[:, :7]) and np.array_equal(mine[:, 8], good.doc(d)[:, 8])
        assert np.array_equal(got.status, bad.status[first:first + n])
        _assert_gap_free(got)
        kept = [d for d in range(first, first + n) if d not in (failed, last)]
        want = [good.items[int(r[7]) + k] for d in kept for r in good.doc(d) for k in range(int(r[8]))]
        assert np.array_equal(got.items, np.array(want, np.uint32).reshape(-1, 7))


def test_item_block_outside_the_buffer_is_an_error(format_case):
    _, dev = format_case
    ndocs = len(dev.ranges)
    # the document whose item block ends the device item array
    ends = {d: DeviceLayout._item_block(dev.results[int(dev.ranges[d, 0]):int(dev.ranges[d, 0] + dev.ranges[d, 1])])[1] for d in range(ndocs)}
    last = max(ends, key=ends.get)
    assert ends[last] == dev.nitems
    bad = DeviceLayout.__new__(DeviceLayout)
    bad.__dict__.update(dev.__dict__)
    bad.nitems = dev.nitems - 1
    for first, n in ((0, ndocs), (last, 1)):
        with pytest.raises(spa.PatternError, match="item block of a document lies outside the device buffer"):
            bad.regroup(first, n)
    other = (last + 1) % ndocs
    assert len(bad.regroup(other, 1).results) == dev.ranges[other, 1]
