"""The batch-postings rule as include/strus_pattern_amd.h ("batch postings") states it, in plain Python and numpy: the
yardstick of the device-free twin (sp_match_batch_postings) and, through it, of the device passes.  Written from the header
text, not from the C++: per dictionary entry a list that is appended to while walking the documents in order."""
import numpy as np

FIELDS = ("records", "entry_offsets", "record_posting")


class Postings:
    def __init__(self, records, entry_offsets, record_posting):
        self.records = records                  # (N, 4) u32: doc, term, count, first_ordpos
        self.entry_offsets = entry_offsets      # (ndict+1,) u64
        self.record_posting = record_posting    # (N,) u32


def batch_postings(term_records, doc_term_offsets, term_dict, ndict):
    """term_records (N, 6), doc_term_offsets (ndocs+1,), term_dict (N,): the postings of the terms batch and its dictionary"""
    term_records = np.asarray(term_records, np.uint32).reshape(-1, 6)
    lists = [[] for _ in range(ndict)]          # per entry: (record index, [doc, term, count, first_ordpos])
    for d in range(len(doc_term_offsets) - 1):
        t0, t1 = int(doc_term_offsets[d]), int(doc_term_offsets[d + 1])
        for i in range(t0, t1):
            lists[int(term_dict[i])].append((i, [d, i - t0, int(term_records[i][1]), int(term_records[i][2])]))
    offsets = np.zeros(ndict + 1, np.uint64)
    offsets[1:] = np.cumsum([len(x) for x in lists])
    records = np.array([row for x in lists for _, row in x], np.uint32).reshape(-1, 4)
    record_posting = np.full(len(term_records), 0xFFFFFFFF, np.uint32)
    for p, (i, _) in enumerate(pair for x in lists for pair in x):
        record_posting[i] = p
    return Postings(records, offsets, record_posting)


def of_batch(terms, d):
    """the model's postings of a MatchTerms and the MatchDictionary built from it"""
    return batch_postings(terms.records, terms.doc_offsets, d.term_dict, len(d.records))


def assert_same(got, want):
    for name in FIELDS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (name, a, b)
        assert a.tobytes() == b.tobytes(), name


def check_invariants(p, terms, d):
    """the invariants of the header, from the postings, their terms and their dictionary"""
    n, ndict = len(terms.records), len(d.records)
    assert p.records.shape == (n, 4) and len(p.entry_offsets) == ndict + 1 and len(p.record_posting) == n
    offs = p.entry_offsets.astype(np.int64)
    assert int(offs[0]) == 0 and int(offs[-1]) == n
    # the list of e has doc_freq postings: the offsets are the exclusive prefix sums of doc_freq
    assert np.array_equal(np.diff(offs), d.records[:, 4].astype(np.int64))
    # record_posting is a permutation, and postings[record_posting[i]] is {d(i), t(i), count, first_ordpos}
    assert np.array_equal(np.sort(p.record_posting), np.arange(n, dtype=np.uint32))
    ndocs = len(terms.doc_offsets) - 1
    doc_of = np.repeat(np.arange(ndocs, dtype=np.int64), np.diff(terms.doc_offsets.astype(np.int64)))
    local = np.arange(n, dtype=np.int64) - terms.doc_offsets.astype(np.int64)[doc_of]
    want = np.stack([doc_of, local, terms.records[:, 1].astype(np.int64), terms.records[:, 2].astype(np.int64)], axis=1).astype(np.uint32).reshape(-1, 4)
    assert np.array_equal(p.records[p.record_posting], want)
    # record_posting[i] lies in the range of entry term_dict[i]
    e = d.term_dict.astype(np.int64)
    assert np.all(offs[e] <= p.record_posting) and np.all(p.record_posting < offs[e + 1])
    for e in range(ndict):
        rows = p.records[int(offs[e]):int(offs[e + 1])]
        assert len(rows) == int(d.records[e, 4]) > 0
        assert rows[0, 0] == d.records[e, 2] and rows[0, 1] == d.records[e, 3]         # the first posting is {first_doc, first_term, ..}
        assert np.all(np.diff(rows[:, 0].astype(np.int64)) > 0)                       # strictly ascending by document
        assert int(rows[:, 2].astype(np.uint64).sum()) == int(d.counts[e]) and int(rows[:, 2].max()) == int(d.records[e, 5])
