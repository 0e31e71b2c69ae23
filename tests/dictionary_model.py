"""The batch-dictionary rule as include/strus_pattern_amd.h ("batch dictionary") states it, in plain Python and numpy: the
yardstick of the device-free twin (sp_match_batch_dictionary) and, through it, of the device passes.  Written from the
header text, not from the C++: one dict keyed by (handle, bytes) over the documents in order, no hash of its own."""
import numpy as np

from tests import terms_model

NO_ENTRY = 0xFFFFFFFF
FIELDS = ("records", "counts", "term_dict", "doc_offsets", "handle_terms")


class Dictionary:
    def __init__(self, records, term_dict, doc_offsets, handle_terms):
        self.records = records              # (ndict, 8) u32: handle, value_bytes, first_doc, first_term, doc_freq, max_count, count low, count high
        self.counts = np.ascontiguousarray(records[:, 6:8]).view(np.uint64).reshape(-1)
        self.term_dict, self.doc_offsets, self.handle_terms = term_dict, doc_offsets, handle_terms


def batch_dictionary(term_records, doc_term_offsets, doc_offsets, handle_bound, flags, values=None, text=None, result_format=None):
    """term_records (N, 6), doc_term_offsets and doc_offsets (ndocs+1,): the dictionary of the terms batch"""
    term_records = np.asarray(term_records, np.uint32).reshape(-1, 6)
    ndocs = len(doc_term_offsets) - 1
    entries, index = [], {}                         # entry: [handle, value_bytes, first_doc, first_term, doc_freq, max_count, count]
    term_dict = np.full(len(term_records), NO_ENTRY, np.uint32)
    offsets = []
    handle_terms = np.zeros(handle_bound, np.uint32)
    for d in range(ndocs):
        offsets.append(len(entries))
        t0, t1 = int(doc_term_offsets[d]), int(doc_term_offsets[d + 1])
        for i in range(t0, t1):
            h, count, _, _, first, size = (int(x) for x in term_records[i])
            value = terms_model.term_value(int(doc_offsets[d]) + first, flags, values, text, result_format)
            assert len(value) == size
            if (h, value) not in index:
                index[(h, value)] = len(entries)
                entries.append([h, size, d, i - t0, 0, 0, 0])
                handle_terms[h] += 1
            e = entries[index[(h, value)]]
            e[4] += 1
            e[5] = max(e[5], count)
            e[6] += count
            term_dict[i] = index[(h, value)]
    offsets.append(len(entries))
    records = np.array([e[:6] + [e[6] & 0xFFFFFFFF, e[6] >> 32] for e in entries], np.uint32).reshape(-1, 8)
    return Dictionary(records, term_dict, np.array(offsets, np.uint64), handle_terms)


def assert_same(got, want):
    assert np.array_equal(got.doc_offsets, want.doc_offsets), (got.doc_offsets, want.doc_offsets)
    assert got.records.shape == want.records.shape and np.array_equal(got.records, want.records), (got.records, want.records)
    assert np.array_equal(got.term_dict, want.term_dict), (got.term_dict, want.term_dict)
    assert np.array_equal(got.handle_terms, want.handle_terms), (got.handle_terms, want.handle_terms)
    for name in FIELDS:
        assert getattr(got, name).dtype == getattr(want, name).dtype and getattr(got, name).tobytes() == getattr(want, name).tobytes(), name


def of_batch(mb, terms, bound, mv=None, mt=None):
    """the model's dictionary of a MatchTerms with the batch and the MatchValues / MatchText it was built from"""
    values, text = terms_model.sources_of(mv, mt)
    return batch_dictionary(terms.records, terms.doc_offsets, mb.doc_offsets, bound, terms.flags, values, text, mb.result_format)


def check_invariants(d, terms, mb):
    """the invariants of the header that need nothing but the dictionary, its terms and the batch"""
    n = len(terms.records)
    assert int(d.records[:, 4].sum()) == n and int(d.handle_terms.sum()) == len(d.records)
    assert n == 0 or int(d.term_dict.max()) < len(d.records)
    with_records = np.diff(terms.doc_offsets.astype(np.int64)) > 0
    results = np.diff(mb.doc_offsets.astype(np.int64))
    assert int(d.counts.sum()) == int(results[with_records].sum())
    assert int(d.doc_offsets[-1]) == len(d.records) and np.all(np.diff(d.doc_offsets.astype(np.int64)) >= 0)
    # first occurrence order: (first_doc, first_term) ascends strictly, and an entry's own record points back at it
    first = d.records[:, 2].astype(np.int64) * (1 << 32) + d.records[:, 3]
    assert np.all(np.diff(first) > 0)
    own = terms.doc_offsets[d.records[:, 2]].astype(np.int64) + d.records[:, 3]
    assert np.array_equal(d.term_dict[own], np.arange(len(d.records), dtype=np.uint32))
