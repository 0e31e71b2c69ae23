"""The index-term rule as include/strus_pattern_amd.h ("index terms") states it, in plain Python and numpy: the yardstick of
the device-free twin (sp_match_batch_terms) and, through it, of the device passes.  Written from the header text, not from
the C++: a dictionary per document, no sort of occurrences, no hash of its own."""
import numpy as np

SP_TERM_VALUES, SP_TERM_TEXT = 1, 2
ERR_RANGE = 5
NO_TERM = 0xFFFFFFFF


class Terms:
    def __init__(self, records, doc_offsets, result_term, status):
        self.records, self.doc_offsets, self.result_term, self.status = records, doc_offsets, result_term, status


class Source:
    """bytes plus nresults+1 offsets parallel to the results, and a status per document"""

    def __init__(self, data, offsets, status):
        self.data, self.offsets, self.status = bytes(data), np.asarray(offsets, np.uint64), np.asarray(status, np.int32)

    def value(self, r):
        return self.data[int(self.offsets[r]):int(self.offsets[r + 1])]


def term_value(r, flags, values, text, result_format):
    if flags == SP_TERM_VALUES:
        return values.value(r)
    if flags == SP_TERM_TEXT:
        return text.value(r)
    formatted = result_format is not None and int(result_format[r]) != 0
    return values.value(r) if formatted else text.value(r)


def batch_terms(results, doc_offsets, handle_bound, flags, values=None, text=None, result_format=None, status=None):
    """results (n, 9), doc_offsets (ndocs+1,): the terms of every document"""
    results = np.asarray(results, np.uint32).reshape(-1, 9)
    ndocs = len(doc_offsets) - 1
    records, offsets = [], [0]
    term_status = np.zeros(ndocs, np.int32)
    result_term = np.full(len(results), NO_TERM, np.uint32)
    selected = [s for bit, s in ((SP_TERM_VALUES, values), (SP_TERM_TEXT, text)) if flags & bit]
    for d in range(ndocs):
        r0, r1 = int(doc_offsets[d]), int(doc_offsets[d + 1])
        if (status is not None and int(status[d]) != 0) or r0 == r1:
            offsets.append(len(records))
            continue
        failed = any(int(s.status[d]) != 0 for s in selected)
        failed = failed or any(not (1 <= int(h) < handle_bound) for h in results[r0:r1, 0])
        if failed:
            term_status[d] = ERR_RANGE
            offsets.append(len(records))
            continue
        found = {}                                      # (handle, value) -> [handle, count, first_ordpos, last_ordend, first_result, value_bytes]
        for r in range(r0, r1):
            h, pos, end = (int(x) for x in results[r, :3])
            value = term_value(r, flags, values, text, result_format)
            rec = found.setdefault((h, value), [h, 0, 0xFFFFFFFF, 0, r - r0, len(value)])
            rec[1] += 1
            rec[2] = min(rec[2], pos)
            rec[3] = max(rec[3], end)
        ordered = sorted(found.items(), key=lambda kv: (kv[1][0], kv[1][4]))
        index = {key: k for k, (key, _) in enumerate(ordered)}
        for r in range(r0, r1):
            result_term[r] = index[(int(results[r, 0]), term_value(r, flags, values, text, result_format))]
        records += [rec for _, rec in ordered]
        offsets.append(len(records))
    return Terms(np.array(records, np.uint32).reshape(-1, 6), np.array(offsets, np.uint64), result_term, term_status)


def assert_same(got, want):
    assert np.array_equal(got.doc_offsets, want.doc_offsets), (got.doc_offsets, want.doc_offsets)
    assert np.array_equal(got.status, want.status), (got.status, want.status)
    assert got.records.shape == want.records.shape and np.array_equal(got.records, want.records), (got.records, want.records)
    assert np.array_equal(got.result_term, want.result_term)
    for name in ("records", "doc_offsets", "result_term", "status"):
        assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name


def sources_of(mv, mt):
    """the model's sources of a MatchValues / MatchText (either may be None)"""
    values = None if mv is None or mv.result_offsets is None else Source(mv.result_values, mv.result_offsets, mv.status)
    text = None if mt is None or mt.result_offsets is None else Source(mt.result_text, mt.result_offsets, mt.status)
    return values, text


def of_batch(mb, bound, flags, mv=None, mt=None):
    values, text = sources_of(mv, mt)
    return batch_terms(mb.results, mb.doc_offsets, bound, flags, values, text, mb.result_format, mb.status)
