"""The matched text of a finished batch, restated over numpy arrays and Python integers (include/strus_pattern_amd.h
"matched text"; csrc/span_text.hpp is the C++ statement, csrc/l2_text.h the device's).  The rule is the project's own,
unpinned by a reference vector."""
import numpy as np

SP_TEXT_RESULTS, SP_TEXT_ITEMS = 1, 2
SP_DOC_ERR_RANGE = 5


def span_range(w, d, seg_offsets, doc_seg_offsets, nbytes):
    """(begin, length) of the span with the words w = (origseg, origpos, origendseg, origend) of document d, None for an
    invalid one"""
    origseg, origpos, origendseg, origend = (int(x) for x in w)
    nseg = len(seg_offsets) - 1
    d0, d1 = (d, d + 1) if doc_seg_offsets is None else (int(doc_seg_offsets[d]), int(doc_seg_offsets[d + 1]))
    if not d0 <= d1 <= nseg:
        return None
    if not origseg <= origendseg < d1 - d0:
        return None
    s0, s1 = d0 + origseg, d0 + origendseg
    a, b, c, e = int(seg_offsets[s0]), int(seg_offsets[s0 + 1]), int(seg_offsets[s1]), int(seg_offsets[s1 + 1])
    if a > b or c > e or (s0 != s1 and b > c):
        return None
    if origpos > b - a or origend > e - c:
        return None
    begin, end = a + origpos, c + origend
    if not begin <= end <= nbytes:
        return None
    return begin, end - begin


def item_offsets(results, doc_offsets):
    """the items of a finished batch follow each other without gaps in result order: (ndocs+1,) offsets"""
    results = np.asarray(results, np.int64).reshape(-1, 9)
    out = [0]
    for d in range(len(doc_offsets) - 1):
        out.append(out[-1] + int(results[int(doc_offsets[d]):int(doc_offsets[d + 1]), 8].sum()))
    return out


def batch_text(results, items, doc_offsets, text, seg_offsets, doc_seg_offsets=None, flags=SP_TEXT_RESULTS | SP_TEXT_ITEMS):
    """-> dict: result_text, result_offsets, item_text, item_offsets (None for a family that `flags` leaves out), status"""
    text = bytes(text)
    ndocs = len(doc_offsets) - 1
    families = []
    if flags & SP_TEXT_RESULTS:
        families.append(("result", np.asarray(results).reshape(-1, 9), [int(x) for x in doc_offsets]))
    if flags & SP_TEXT_ITEMS:
        families.append(("item", np.asarray(items).reshape(-1, 7), item_offsets(results, doc_offsets)))
    status = np.zeros(ndocs, np.int32)
    ranges = {}
    for name, rec, offs in families:
        for d in range(ndocs):
            got = [span_range(rec[i, 3:7], d, seg_offsets, doc_seg_offsets, len(text)) for i in range(offs[d], offs[d + 1])]
            if any(g is None for g in got) or sum(g[1] for g in got) >= 2 ** 32:
                status[d] = SP_DOC_ERR_RANGE
            ranges[name, d] = got
    out = {"result_text": None, "result_offsets": None, "item_text": None, "item_offsets": None, "status": status}
    for name, rec, offs in families:
        chunks, span_offsets, at = [], [], 0
        for d in range(ndocs):
            for begin, length in ([(0, 0)] * len(ranges[name, d]) if status[d] else ranges[name, d]):
                span_offsets.append(at)
                chunks.append(text[begin:begin + length])
                at += length
        out[name + "_text"] = b"".join(chunks)
        out[name + "_offsets"] = np.array(span_offsets + [at], np.uint64)
    return out
