"""The canonical order inside a document of a finished batch (include/strus_pattern_amd.h, SP_FINISH_CANONICAL) as plain
Python: the expectation of the canonical device finish.  It is computed from a batch in ANY order inside the documents
(batchFetch(), the oracle) and never from the canonical finish itself."""
import numpy as np

from struspattern_amd import MatchBatch


def canonical_key(batch, r):
    """T(r) of result r of `batch` (struspattern_amd.MatchBatch or oracle.L2Results) as a tuple of ints"""
    rec = batch.results[r]
    ib, ic = int(rec[7]), int(rec[8])
    formats = getattr(batch, "result_format", None) is not None
    key = [int(rec[w]) for w in (1, 2, 3, 4, 5, 6)] + [int(rec[0]), ic]
    if formats:
        key.append(int(batch.result_format[r]))
    key.extend(int(x) for x in batch.items[ib:ib + ic].reshape(-1))
    if formats:
        key.extend(int(x) for x in batch.item_format[ib:ib + ic].reshape(-1))
    return tuple(key)


def sorted_batch(batch):
    """`batch` with the results of every document sorted by canonical_key, the items (and format words) regathered in the
    new result order and item_begin reassigned: the running sum of the item counts"""
    formats = getattr(batch, "result_format", None) is not None
    order = []
    for d in range(len(batch.doc_offsets) - 1):
        b, e = int(batch.doc_offsets[d]), int(batch.doc_offsets[d + 1])
        order.extend(sorted(range(b, e), key=lambda r: canonical_key(batch, r)))
    order = np.asarray(order, np.int64)
    results = batch.results[order].copy() if len(order) else batch.results[:0].copy()
    gather = [np.arange(int(batch.results[r, 7]), int(batch.results[r, 7]) + int(batch.results[r, 8]), dtype=np.int64) for r in order]
    gather = np.concatenate(gather) if gather else np.zeros(0, np.int64)
    counts = results[:, 8].astype(np.int64)
    results[:, 7] = (np.cumsum(counts) - counts).astype(np.uint32)
    return MatchBatch(results, batch.items[gather].copy(), batch.doc_offsets.copy(), batch.stats, batch.status,
                      batch.result_format[order].copy() if formats else None, batch.item_format[gather].copy() if formats else None)


def in_canonical_order(batch, d):
    """whether document d of `batch` is sorted by canonical_key already"""
    keys = [canonical_key(batch, r) for r in range(int(batch.doc_offsets[d]), int(batch.doc_offsets[d + 1]))]
    return all(a <= b for a, b in zip(keys, keys[1:]))
