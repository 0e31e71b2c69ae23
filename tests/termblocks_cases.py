"""What the CPU tests (tests/test_termblocks_abi.py) and the GPU tests (tests/test_termblocks_gpu.py) of the term blocks share: the
value cases that reach every varint length a batch can produce, the hand-made batch of the twins with its dictionary and order,
and the block size switch.  Needs no device."""
import contextlib

import numpy as np

import struspattern_amd as spa
from struspattern_amd import capi
from tests import dictorder_cases
from tests import dictorder_model
from tests import termblocks_model as model
from tests.finished_support import _batch, _family, T, V

LONG = dictorder_cases.LONG


def value_lengths(handle=2):
    """values of 0, 1, 127, 128, 16 383 and 16 384 bytes that share nothing: the suffix as a varint of one, two and three bytes"""
    return [(handle, bytes([66 + i]) * n) for i, n in enumerate((0, 1, 127, 128, 16383, 16384))]


def shared_lengths(handle=3):
    """two pairs of neighbours that share 127 and 128 bytes: `shared` as a varint of one and of two bytes"""
    a, b = (LONG * 4)[:127], (LONG[::-1] * 4)[:128]
    return [(handle, a + b"b"), (handle, b + b"y"), (handle, a + b"a"), (handle, b + b"x")]


def handle_per_entry(n=70):
    """every entry under its own handle: every hdelta behind a head is 1"""
    return [(1 + (k * 37) % n, b"same") for k in range(n)]


def far_handles():
    """the handles 1 and 200 next to each other: an hdelta of two bytes"""
    return [(200, b"right"), (1, b"left"), (200, b"rights")]


def lengths_in_turn(nhandles=14):
    """per handle ten values of the lengths 0..9 whose first bytes ascend with the length: along the order the lengths come
    0..9 in turn, so the codes of consecutive positions, and the spans of consecutive waves, start at every alignment"""
    return [(h, bytes([97 + n]) * n) for h in range(1, nhandles + 1) for n in range(10)]


@contextlib.contextmanager
def block_entries(n):
    """B = n for the calls inside (sp_test_term_block_entries), the default after them"""
    capi.lib().sp_test_term_block_entries(n)
    try:
        yield
    finally:
        capi.lib().sp_test_term_block_entries(0)


class Inputs:
    """documents of (handle, value) terms as a finished batch on the host with its terms, dictionary and order by the twins: every
    term is one result whose text is the value; formatted: the (handle, value) pairs whose result has a format, its value in the
    values and another text"""

    def __init__(self, docs, flags=T, formatted=(), bound=8):
        rows = [[(h, k + 1, k + 2) for k, (h, _) in enumerate(doc)] for doc in docs]
        flat = [t for doc in docs for t in doc]
        formats = [1 if t in formatted else 0 for t in flat]
        self.mb = _batch(rows, formats if flags & V else None)
        self.text = _family(spa.MatchText, [b"?" if f else v for (_, v), f in zip(flat, formats)], len(docs)) if flags & T else None
        self.values = _family(spa.MatchValues, [v if f or flags == V else b"" for (_, v), f in zip(flat, formats)], len(docs)) if flags & V else None
        self.terms = spa.batchTerms(self.mb, values=self.values, text=self.text, handle_bound=bound, flags=flags)
        self.d = spa.batchDictionary(self.mb, self.terms, values=self.values, text=self.text)
        self.entries = dictorder_model.entries_of(self.mb, self.terms, self.d, self.values, self.text)
        self.order = spa.batchDictionaryOrder(self.mb, self.terms, self.d, values=self.values, text=self.text)

    def set_frequencies(self, doc_freq=None, count=None):
        """the doc_freq and the count of the entries at the sorted positions 0.. set by hand: the twin takes host arrays, so no
        batch has to produce them"""
        records = self.d.records.copy()
        for k, df in enumerate(doc_freq or ()):
            records[int(self.order.order[k]), 4] = df
        for k, c in enumerate(count or ()):
            records[int(self.order.order[k]), 6:8] = [c & 0xFFFFFFFF, c >> 32]
        self.d = spa.MatchDictionary(records, self.d.term_dict, self.d.doc_offsets, self.d.handle_terms)
        return self

    def sorted(self):
        return model.sorted_entries(self.d, self.entries, self.order)

    def blocks(self):
        return spa.batchTermBlocks(self.mb, self.terms, self.d, self.order, values=self.values, text=self.text)

    def check(self, B=16):
        """the twin's blocks equal the model's and decode to the sorted entries, by the model's reader and the library's"""
        with block_entries(B):
            got = self.blocks()
        want = self.sorted()
        model.assert_same(got, model.term_blocks(want, B))
        model.check_invariants(got, want)
        assert got.entries() == want
        return got
