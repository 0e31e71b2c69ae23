"""What the CPU tests (tests/test_postingblocks_abi.py) and the GPU tests (tests/test_postingblocks_gpu.py) of the posting blocks
share: hand-made dictionaries, orders, postings and positions for the twin, documents of (handle, value, position) terms for
the device, and the block size switch.  Needs no device."""
import contextlib

import numpy as np

import struspattern_amd as spa
from struspattern_amd import capi
from tests import postingblocks_model as model


@contextlib.contextmanager
def block_entries(n):
    """B = n for the calls inside (sp_test_term_block_entries), the default after them"""
    capi.lib().sp_test_term_block_entries(n)
    try:
        yield
    finally:
        capi.lib().sp_test_term_block_entries(0)


class Hand:
    """A dictionary, its order, its postings and their positions made by hand.  lists: per dictionary entry its postings
    [(doc, count, [the ordpos of every occurrence, ascending, repeats allowed])] -- `count` is the word as given, the twin codes
    it as it is --; order: the entry at every sorted position (the entries in reverse unless given)."""

    def __init__(self, lists, order=None):
        ndict = len(lists)
        order = list(range(ndict))[::-1] if order is None else list(order)
        records = np.zeros((ndict, 8), np.uint32)
        rows, occ, entry_offsets, posting_offsets, npos = [], [], [0], [0], []
        for e, entry in enumerate(lists):
            records[e, 0], records[e, 4] = 1, len(entry)
            for doc, count, positions in entry:
                rows.append([doc, 0, count, positions[0] if positions else 0])
                occ += [[x, i] for i, x in enumerate(positions)]
                posting_offsets.append(len(occ))
                npos.append(len(set(positions)))
            entry_offsets.append(len(rows))
        n = len(rows)
        self.lists = lists
        self.d = spa.MatchDictionary(records, np.zeros(n, np.uint32), np.zeros(1, np.uint64), np.array([0, ndict], np.uint32))
        self.order = spa.MatchDictionaryOrder(np.array(order, np.uint32), np.argsort(np.array(order, np.int64)).astype(np.uint32), np.zeros(ndict, np.uint32),
                                              np.array([0, 0, ndict], np.uint64))
        self.postings = spa.MatchPostings(np.array(rows, np.uint32).reshape(-1, 4), np.array(entry_offsets, np.uint64), np.arange(n, dtype=np.uint32))
        self.positions = spa.MatchPositions(np.array(occ, np.uint32).reshape(-1, 2), np.array(posting_offsets, np.uint64), np.array(npos, np.uint32),
                                            np.array([len(occ), sum(npos)], np.uint64))

    def want(self):
        """per sorted position [(doc, count, [distinct positions])]"""
        return [[(doc, count, sorted(set(pos))) for doc, count, pos in self.lists[e]] for e in self.order.order.tolist()]

    def blocks(self):
        return spa.batchPostingBlocks(self.d, self.order, self.postings, self.positions)

    def check(self, B=16):
        """the twin's blocks equal the model's and decode to the lists, by the model's reader and the library's"""
        with block_entries(B):
            got = self.blocks()
        want = self.want()
        assert model.lists_of(self.order, self.postings, self.positions) == want
        model.assert_same(got, model.posting_blocks(want, B))
        model.check_invariants(got, want)
        assert got.lists() == want
        return got


def numbered(n, docs=3):
    """n entries: entry e lies in 1 + e % docs documents, e % 4 + 1 times in each, every second occurrence at the position before"""
    return [[(7 * d + e % 5, e % 4 + 1, [3 + e + (i // 2) * (e % 9 + 1) for i in range(e % 4 + 1)]) for d in range(1 + e % docs)] for e in range(n)]


def build_at(docs):
    """docs: per document a list of (handle, value bytes, ordpos), the positions not descending: every occurrence gets its own
    copy of the value in the document's text -> pieces, lexems (n, 4), origseg, document offsets"""
    pieces, lex, offs = [], [], [0]
    for doc in docs:
        text = b""
        for h, value, pos in doc:
            lex.append([h, pos, len(text), len(value)])
            text += value
        pieces.append(text)
        offs.append(len(lex))
    return pieces, np.array(lex, np.uint32).reshape(-1, 4), np.zeros(len(lex), np.uint32), np.array(offs, np.uint64)


def counted(docs):
    """(handle, value) documents at the positions 1, 2, .."""
    return [[(h, v, k + 1) for k, (h, v) in enumerate(doc)] for doc in docs]


def postings_in(n, arrival="shuffle", per_doc=7):
    """documents that make exactly n postings: n distinct terms, one occurrence each, per_doc a document; arrival: the order in
    which the values come"""
    values = [b"w%05d" % k for k in range(n)]
    if arrival == "descending":
        values = values[::-1]
    else:
        values = [values[int(i)] for i in np.random.default_rng(n).permutation(n)]
    return counted([[(1 + k % 3, v) for k, v in enumerate(values[at:at + per_doc])] for at in range(0, n, per_doc)])
