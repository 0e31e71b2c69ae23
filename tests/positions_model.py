"""The posting-positions rule as include/strus_pattern_amd.h ("posting positions") states it, in plain Python: the yardstick of
the device-free twin (sp_match_batch_positions) and, through it, of the device passes.  Written from the header text, not from
the C++: every participating result becomes a tuple (posting, ordpos, result) and the tuples are sorted."""
import numpy as np

FIELDS = ("occurrences", "posting_offsets", "posting_positions", "totals")
NONE = 0xFFFFFFFF


class Positions:
    def __init__(self, occurrences, posting_offsets, posting_positions, totals):
        self.occurrences = occurrences              # (nocc, 2) u32: ordpos, result
        self.posting_offsets = posting_offsets      # (N+1,) u64
        self.posting_positions = posting_positions  # (N,) u32
        self.totals = totals                        # (2,) u64


def batch_positions(results, doc_offsets, result_term, doc_term_offsets, record_posting, nterms):
    """results (R, 9), doc_offsets (ndocs+1,), result_term (R,), doc_term_offsets (ndocs+1,), record_posting (N,)"""
    results = np.asarray(results, np.uint32).reshape(-1, 9)
    found = []
    for d in range(len(doc_offsets) - 1):
        r0, t0 = int(doc_offsets[d]), int(doc_term_offsets[d])
        for r in range(r0, int(doc_offsets[d + 1])):
            if int(result_term[r]) != NONE:
                found.append((int(record_posting[t0 + int(result_term[r])]), int(results[r][1]), r - r0))
    found = sorted(found)
    counts = [0] * nterms
    distinct = [set() for _ in range(nterms)]
    for p, pos, _ in found:
        counts[p] += 1
        distinct[p].add(pos)
    offsets = np.zeros(nterms + 1, np.uint64)
    offsets[1:] = np.cumsum(counts)
    occurrences = np.array([[pos, r] for _, pos, r in found], np.uint32).reshape(-1, 2)
    positions = np.array([len(x) for x in distinct], np.uint32)
    return Positions(occurrences, offsets, positions, np.array([len(found), int(positions.sum())], np.uint64))


def of_batch(mb, terms, postings):
    """the model's positions of a finished MatchBatch, its MatchTerms and their MatchPostings"""
    return batch_positions(mb.results, mb.doc_offsets, terms.result_term, terms.doc_offsets, postings.record_posting, len(postings.records))


def assert_same(got, want):
    for name in FIELDS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (name, a, b)
        assert a.tobytes() == b.tobytes(), name


def check_invariants(q, mb, terms, postings):
    """the invariants of the header, from the positions, the batch, its terms and their postings"""
    n = len(postings.records)
    offs = q.posting_offsets.astype(np.int64)
    assert q.occurrences.shape == (int(offs[-1]), 2) and len(offs) == n + 1 and len(q.posting_positions) == n
    # the list of p has postings[p].count records: the offsets are the exclusive prefix sums of count
    assert int(offs[0]) == 0 and np.array_equal(np.diff(offs), postings.records[:, 2].astype(np.int64))
    participating = int(np.count_nonzero(terms.result_term != NONE))
    assert int(q.totals[0]) == int(offs[-1]) == participating and int(q.totals[1]) == int(q.posting_positions.astype(np.uint64).sum())
    seen = set()
    for p in range(n):
        doc, term, count, first = (int(x) for x in postings.records[p])
        rows = q.occurrences[int(offs[p]):int(offs[p + 1])]
        assert len(rows) == count >= 1
        assert int(rows[0, 0]) == first                                                  # its first ordpos is first_ordpos
        keys = [(int(pos), int(r)) for pos, r in rows.tolist()]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)                    # ascending by ordpos, ties by result
        r0 = int(mb.doc_offsets[doc])
        for pos, r in keys:
            assert r0 + r < int(mb.doc_offsets[doc + 1])
            assert int(terms.result_term[r0 + r]) == term and int(mb.results[r0 + r][1]) == pos
            assert (doc, r) not in seen
            seen.add((doc, r))
        assert min(r for _, r in keys) == int(terms.doc(doc)[term][4])                   # the term record's first_result
        assert 1 <= int(q.posting_positions[p]) == len(set(pos for pos, _ in keys)) <= count
    assert len(seen) == participating                                                    # every participating result exactly once
