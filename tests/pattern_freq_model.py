"""The pattern frequencies of a finished batch, stated independently in numpy (include/strus_pattern_amd.h "pattern
frequencies"): the yardstick of the C++ twin (csrc/pattern_freq.hpp) and, through it and directly, of the device passes.
Shares no code with the product."""
import numpy as np

SP_DOC_ERR_RANGE = 5


def batch_pattern_freq(results, doc_offsets, handle_bound, status=None):
    """results: (n, 9) u32 records of a finished batch, doc_offsets: (ndocs+1,) -> dict of records (m, 4) u32
    [handle, count, first_ordpos, last_ordend], doc_offsets (ndocs+1,) u64, status (ndocs,) i32, handle_results
    (handle_bound,) u64, handle_docs (handle_bound,) u32, total"""
    results = np.asarray(results, np.uint32).reshape(-1, 9)
    offs = np.asarray(doc_offsets, np.uint64).astype(np.int64)
    ndocs = len(offs) - 1
    blocks, out_offs, out_status = [], np.zeros(ndocs + 1, np.uint64), np.zeros(ndocs, np.int32)
    handle_results, handle_docs = np.zeros(handle_bound, np.uint64), np.zeros(handle_bound, np.uint32)
    for d in range(ndocs):
        doc = results[offs[d]:offs[d + 1]]
        if status is not None and status[d] != 0:
            doc = doc[:0]
        handles = doc[:, 0].astype(np.int64)
        if len(doc) and (handles.min() < 1 or handles.max() >= handle_bound):
            out_status[d] = SP_DOC_ERR_RANGE
        elif len(doc):
            order = np.argsort(handles, kind="stable")
            distinct, first, counts = np.unique(handles[order], return_index=True, return_counts=True)
            block = np.zeros((len(distinct), 4), np.uint32)
            block[:, 0], block[:, 1] = distinct, counts
            block[:, 2] = np.minimum.reduceat(doc[order, 1], first)
            block[:, 3] = np.maximum.reduceat(doc[order, 2], first)
            blocks.append(block)
            np.add.at(handle_results, distinct, counts.astype(np.uint64))
            np.add.at(handle_docs, distinct, 1)
        out_offs[d + 1] = out_offs[d] + (len(blocks[-1]) if len(doc) and not out_status[d] else 0)
    records = np.concatenate(blocks) if blocks else np.zeros((0, 4), np.uint32)
    return dict(records=records, doc_offsets=out_offs, status=out_status, handle_results=handle_results, handle_docs=handle_docs,
                total=len(records))


def assert_same(got, want):
    """a struspattern_amd.PatternFreq against the model's dict, field for field"""
    assert np.array_equal(got.status, want["status"])
    assert np.array_equal(got.doc_offsets, want["doc_offsets"])
    assert got.records.shape == want["records"].shape and np.array_equal(got.records, want["records"])
    assert np.array_equal(got.handle_results, want["handle_results"]) and got.handle_results.dtype == np.uint64
    assert np.array_equal(got.handle_docs, want["handle_docs"])
    assert int(got.doc_offsets[-1]) == want["total"] == len(got.records)
