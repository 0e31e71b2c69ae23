"""The products of a finished batch as host copies, and their device-free twins (include/strus_pattern_amd.h, the sp_match_batch_*
calls).  A product class states its arrays once (`_ARRAYS`); the converter (C struct -> object, `_from_c`) and the marshaller
(object -> C struct for a twin, `_to_c`) both read that one statement."""
import ctypes
from typing import NamedTuple, Optional

import numpy as np

from . import capi

SP_TEXT_RESULTS, SP_TEXT_ITEMS = 1, 2   # include/strus_pattern_amd.h: the families of spans of a text call
SP_VALUE_RESULTS, SP_VALUE_ITEMS = 1, 2  # include/strus_pattern_amd.h: the families of records of a values call
SP_TERM_VALUES, SP_TERM_TEXT = 1, 2    # include/strus_pattern_amd.h: the sources of the term values of a terms call

u32, u64, i32 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32


class PatternError(RuntimeError):
    pass


class Arr(NamedTuple):
    """One array of a product: attribute `attr` of the Python object, field `field` of its C struct (a pointer), of
    struct.count + plus rows (count None: a fixed array of `plus` elements inside the struct) of `cols` columns (0: one
    dimension) of `ctype`.  given: the field whose null pointer says that the product has no such array (the attribute is None)."""
    attr: str
    field: str
    count: Optional[str]
    plus: int
    cols: int
    ctype: type
    given: Optional[str] = None


# What a product class states beside _ARRAYS: _C, the struct of its host copy; _SCALARS, the fields that are attributes of the
# same name; _TOTAL, the count that goes to totals[0] (None: no such slot); _WHAT, its name in an error message; _FREE and _FETCH,
# the library calls that free the struct and that fetch it from a context.

def _rows(ptr, n, k, ctype=u32):
    """n rows of k columns of `ctype` behind the ctypes pointer `ptr` (to records of any type), copied: shape (n, k), or (n,) for k = 0"""
    if not n or not ptr:
        return np.zeros((n, k) if k else n, ctype)
    a = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=(n * max(k, 1),)).copy()
    return a.reshape(n, k) if k else a


def _from_c(cls, s):
    """the product `cls` of its C struct `s` (copies)"""
    if issubclass(cls, _ByteFamilies):
        return _byte_families_of(cls, s)
    arrays = {a.attr: _rows(getattr(s, a.field), (getattr(s, a.count) if a.count else 0) + a.plus, a.cols, a.ctype)
              if not a.given or getattr(s, a.given) else None for a in cls._ARRAYS}
    return cls(**arrays, **{n: getattr(s, n) for n in cls._SCALARS})


def _to_c(obj, keep, arrays=None, **scalars):
    """The C struct of a product for a host twin, with all its arrays or those named in `arrays`; an array that is None stays a
    null pointer.  A count is the length of the first array that has it.  scalars: fields set after those of the object.  What
    the struct points into is appended to `keep`: the caller holds it until its C call has returned."""
    s, counted = obj._C(), set()
    pointer = dict(s._fields_)
    for a in obj._ARRAYS:
        v = getattr(obj, a.attr)
        if v is None or (arrays is not None and a.attr not in arrays):
            continue
        v = np.ascontiguousarray(v, dtype=a.ctype).reshape((-1, a.cols) if a.cols else -1)
        if a.count is None:
            getattr(s, a.field)[:] = v.tolist()
            continue
        keep.append(v)
        setattr(s, a.field, ctypes.cast(v.ctypes.data, pointer[a.field]))
        if a.count not in counted:
            counted.add(a.count)
            setattr(s, a.count, len(v) - a.plus)
    for n in obj._SCALARS:
        setattr(s, n, getattr(obj, n))
    for n, value in scalars.items():
        setattr(s, n, value)
    if obj._TOTAL:
        s.totals[0] = getattr(s, obj._TOTAL)
    return s


def _product(cls, call, failed):
    """One C call that fills a struct the library allocates for: call(struct) is the return code, failed(rc) the message of
    the PatternError for one that is not 0; returns the product `cls` of the struct.  The struct is freed whatever happens."""
    s = cls._C()
    rc = call(s)
    try:
        if rc != 0:
            raise PatternError(failed(rc))
        return _from_c(cls, s)
    finally:
        getattr(capi.lib(), cls._FREE)(ctypes.byref(s))


def _twin(cls, fn, *args, errsize=256, errors="strict"):
    """The host twin `fn` of the library that makes the product `cls`: fn(*args, struct pointer, error buffer, its size)"""
    err = ctypes.create_string_buffer(errsize)
    return _product(cls, lambda s: getattr(capi.lib(), fn)(*args, ctypes.byref(s), err, errsize),
                    lambda rc: "no %s (%d): %s" % (cls._WHAT, rc, err.value.decode(errors=errors)))


def _ref(s):
    return ctypes.byref(s) if s is not None else None


class MatchBatch:
    """Results of a batch of documents (host copies)."""
    _C, _SCALARS, _TOTAL, _WHAT, _FREE = capi.SpMatchBatch, (), None, "batch", "sp_match_batch_free"
    _ARRAYS = (
        Arr("results", "results", "nresults", 0, 9, u32),     # handle, ordpos, ordend, origseg, origpos, origendseg, origend, item_begin, item_count
        Arr("items", "items", "nitems", 0, 7, u32),           # variable, ordpos, ordend, origseg, origpos, origendseg, origend
        Arr("doc_offsets", "doc_result_offsets", "ndocs", 1, 0, u64),
        Arr("stats", "doc_stats", "ndocs", 0, 4, u64),
        Arr("status", "doc_status", "ndocs", 0, 0, i32),
        Arr("result_format", "result_format", "nresults", 0, 0, u32, given="result_format"),   # format handle per result, None without format strings
        Arr("item_format", "item_format", "nitems", 0, 2, u32, given="result_format"),         # {format handle, nsub} per item (see resultformat.py)
    )

    def __init__(self, results, items, doc_offsets, stats, status, result_format=None, item_format=None):
        self.result_format, self.item_format = result_format, item_format
        self.results, self.items, self.doc_offsets, self.stats, self.status = results, items, doc_offsets, stats, status

    def doc(self, i):
        return self.results[self.doc_offsets[i]:self.doc_offsets[i + 1]]


def _match_batch_of(b):
    """the MatchBatch of a capi.SpMatchBatch (copies)"""
    return _from_c(MatchBatch, b)


def _host_batch(mb, items=False, formats=None, status=False):
    """The capi.SpMatchBatch of a MatchBatch for a host twin, and the arrays it points into: the caller holds them until its
    C call has returned.  items: with the items; formats: "results" with the format handles of the results, "all" with those
    of the items too (where the batch has them); status: with the document status (where the batch has one)."""
    keep = []
    b = _to_c(mb, keep, ["results", "doc_offsets"] + ["items"] * bool(items) + ["status"] * bool(status))
    want = {"results": ["result_format"], "all": ["result_format", "item_format"]}.get(formats, [])
    if want and all(getattr(mb, n) is not None for n in want):
        f = _to_c(mb, keep, want)       # (its counts are the lengths of the format arrays)
        if formats == "results" and f.nresults != b.nresults:
            raise PatternError("format array of the batch is not parallel to its results")
        if formats == "all" and (f.nresults != b.nresults or f.nitems != b.nitems):
            raise PatternError("format arrays of the batch are not parallel to its results and items")
        b.result_format, b.item_format = f.result_format, f.item_format
    return b, keep


def _host_text(text, seg_offsets, doc_seg_offsets):
    """The text source arguments of a host twin (text, nbytes, seg_offsets, nseg, doc_seg_offsets), and what they point into"""
    text = bytes(text)
    so = np.ascontiguousarray(seg_offsets, dtype=np.uint64)
    dso = None if doc_seg_offsets is None else np.ascontiguousarray(doc_seg_offsets, dtype=np.uint64)
    return (text, len(text), so.ctypes.data, len(so) - 1, dso.ctypes.data if dso is not None else None), [text, so, dso]


class _ByteFamilies:
    """Bytes per result and per item of a batch (host copies): those of record i of a family are bytes[offsets[i]:offsets[i+1]],
    parallel to the results / items of the batch.  A family that was not asked for is None.  A product states _results and
    _items, the fields (bytes, offsets) of the two families in its C struct, the first of which is also the attribute with the
    bytes, and _status, its status field."""

    def result(self, i):
        return getattr(self, self._results[0])[int(self.result_offsets[i]):int(self.result_offsets[i + 1])]

    def item(self, i):
        return getattr(self, self._items[0])[int(self.item_offsets[i]):int(self.item_offsets[i + 1])]


def _byte_families_of(cls, s):
    """the MatchText / MatchValues (`cls`) of its C struct `s` (copies)"""
    def family(fields, n, total):
        data, offsets = getattr(s, fields[0]), getattr(s, fields[1])
        if not offsets:
            return None, None
        return (ctypes.string_at(data, total) if total else b""), _rows(offsets, n + 1, 0, u64)
    return cls(*family(cls._results, s.nresults, s.totals[0]), *family(cls._items, s.nitems, s.totals[1]), _rows(getattr(s, cls._status), s.ndocs, 0, i32))


def _host_source(family, keep):
    """the C struct of a MatchValues / MatchText for a host twin, its results family only; None for None.  What it points into
    is appended to `keep`."""
    if family is None:
        return None
    c = family._C()
    c.ndocs, c.nresults = len(family.status), (len(family.result_offsets) - 1 if family.result_offsets is not None else 0)
    st = np.ascontiguousarray(family.status, dtype=np.int32)
    keep.append(st)
    setattr(c, family._status, ctypes.cast(st.ctypes.data, ctypes.POINTER(i32)))
    if family.result_offsets is not None:
        data = bytes(getattr(family, family._results[0]))
        ro = np.ascontiguousarray(family.result_offsets, dtype=np.uint64)
        buf = ctypes.create_string_buffer(data, len(data) + 1)      # (a pointer that is not null for no bytes)
        keep.extend([ro, buf])
        setattr(c, family._results[0], ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint8)))
        setattr(c, family._results[1], ctypes.cast(ro.ctypes.data, ctypes.POINTER(u64)))
        c.totals[0] = len(data)
    return c


class MatchText(_ByteFamilies):
    """The text that the results and items of a finished batch cover (host copies): the bytes of span i of a family are
    text[offsets[i]:offsets[i+1]], parallel to the results / items of the batch.  A family that was not asked for is None."""
    _C, _WHAT, _FREE, _FETCH = capi.SpMatchText, "text of the batch", "sp_match_text_free", "sp_matcher_ctx_finished_text_fetch"
    _results, _items, _status = ("result_text", "result_text_offsets"), ("item_text", "item_text_offsets"), "doc_text_status"

    def __init__(self, result_text, result_offsets, item_text, item_offsets, status):
        self.result_text = result_text        # bytes
        self.result_offsets = result_offsets  # (nresults+1,) u64
        self.item_text = item_text
        self.item_offsets = item_offsets      # (nitems+1,) u64
        self.status = status                  # (ndocs,) i32: 0, or 5 for a document with a span outside the text (all its spans empty)


def batchText(mb, text, seg_offsets, doc_seg_offsets=None, results=True, items=True):
    """The text of a batch already on the host (a MatchBatch in document order with items without gaps: finishedFetch,
    batchFetch, matchDocs), by the rule of the device call (include/strus_pattern_amd.h "matched text"), without a device:
    `text` holds the segments back to back (seg_offsets: nseg+1 byte offsets), document d is the segments
    [doc_seg_offsets[d], doc_seg_offsets[d+1]), or segment d without doc_seg_offsets.  Returns a MatchText."""
    b, keep = _host_batch(mb, items=True)
    source, keep_text = _host_text(text, seg_offsets, doc_seg_offsets)      # (keep, keep_text: until the call has returned)
    flags = (SP_TEXT_RESULTS if results else 0) | (SP_TEXT_ITEMS if items else 0)
    return _twin(MatchText, "sp_match_batch_text", ctypes.byref(b), *source, flags)


class MatchValues(_ByteFamilies):
    """The values of the format strings of a finished batch (host copies): the value of record i of a family is
    values[offsets[i]:offsets[i+1]], parallel to the results / items of the batch; a record without a format has an empty
    range (the format arrays of the batch tell an empty value from no value).  A family that was not asked for is None."""
    _C, _WHAT, _FREE, _FETCH = capi.SpMatchValues, "values of the batch", "sp_match_values_free", "sp_matcher_ctx_finished_values_fetch"
    _results, _items, _status = ("result_values", "result_value_offsets"), ("item_values", "item_value_offsets"), "doc_value_status"

    def __init__(self, result_values, result_offsets, item_values, item_offsets, status):
        self.result_values = result_values    # bytes
        self.result_offsets = result_offsets  # (nresults+1,) u64
        self.item_values = item_values
        self.item_offsets = item_offsets
        self.status = status                  # (ndocs,) i32: 0, or 5 for a document whose values cannot be built (all of them empty)


def batchValues(matcher, mb, text, seg_offsets, doc_seg_offsets=None, flags=SP_VALUE_RESULTS | SP_VALUE_ITEMS):
    """The values of the format strings of a batch already on the host (a MatchBatch of `matcher`, a PatternMatcherInstance,
    in document order with items without gaps: finishedFetch, batchFetch, matchDocs), by the rule of the device call
    (include/strus_pattern_amd.h "result values"), without a device.  The text source is that of batchText.  Returns a
    MatchValues."""
    b, keep = _host_batch(mb, items=True, formats="all")
    source, keep_text = _host_text(text, seg_offsets, doc_seg_offsets)      # (keep, keep_text: until the call has returned)
    return _twin(MatchValues, "sp_match_batch_values", matcher._h, ctypes.byref(b), *source, flags, errsize=512, errors="replace")


class PatternFreq:
    """The pattern frequencies of a finished batch (host copies): per document one record per distinct handle, ascending by
    handle, and per handle the sums over the batch (include/strus_pattern_amd.h "pattern frequencies")."""
    _C, _SCALARS, _TOTAL, _WHAT = capi.SpPatternFreqBatch, (), "nrecords", "pattern frequencies of the batch"
    _FREE, _FETCH = "sp_pattern_freq_batch_free", "sp_matcher_ctx_finished_pattern_freq_fetch"
    _ARRAYS = (
        Arr("records", "records", "nrecords", 0, 4, u32),                   # handle, count, first_ordpos, last_ordend
        Arr("doc_offsets", "doc_offsets", "ndocs", 1, 0, u64),
        Arr("status", "doc_freq_status", "ndocs", 0, 0, i32),               # 0, or 5 for a document with a handle outside the bound (no records)
        Arr("handle_results", "handle_results", "handle_bound", 0, 0, u64),  # results per handle over the batch (collection frequency)
        Arr("handle_docs", "handle_docs", "handle_bound", 0, 0, u32),       # documents per handle (document frequency)
    )

    def __init__(self, records, doc_offsets, status, handle_results, handle_docs):
        self.records, self.doc_offsets, self.status, self.handle_results, self.handle_docs = records, doc_offsets, status, handle_results, handle_docs

    def doc(self, i):
        return self.records[int(self.doc_offsets[i]):int(self.doc_offsets[i + 1])]


def batchPatternFreq(mb, handle_bound):
    """The pattern frequencies of a batch already on the host (a MatchBatch in document order: finishedFetch, batchFetch,
    matchDocs), by the rule of the device call, without a device.  handle_bound: PatternMatcherInstance.handleBound().
    Returns a PatternFreq."""
    b, keep = _host_batch(mb, status=True)      # (keep: until the call has returned)
    return _twin(PatternFreq, "sp_match_batch_pattern_freq", ctypes.byref(b), handle_bound)


def _term_value(flags, mb, values, text, r):
    """the value bytes of result r of the finished batch mb: those of `values` (a MatchValues) unless the flags say `text` (a
    MatchText); with both flags the text of a result without a format"""
    use_text = not (flags & SP_TERM_VALUES)
    if flags == (SP_TERM_VALUES | SP_TERM_TEXT):
        use_text = mb.result_format is None or int(mb.result_format[r]) == 0
    return text.result(r) if use_text else values.result(r)


class MatchTerms:
    """The index terms of a finished batch (host copies): per document one record per distinct pair (handle, value bytes),
    ascending by handle, then by first_result, and per result the index of its term inside its document's block
    (include/strus_pattern_amd.h "index terms").  A term owns no bytes: its value is the range of its first result in the
    values or the text it was built from."""
    _C, _SCALARS, _TOTAL, _WHAT = capi.SpMatchTerms, ("flags", "handle_bound"), "nrecords", "terms of the batch"
    _FREE, _FETCH = "sp_match_terms_free", "sp_matcher_ctx_finished_terms_fetch"
    _ARRAYS = (
        Arr("records", "records", "nrecords", 0, 6, u32),          # handle, count, first_ordpos, last_ordend, first_result, value_bytes
        Arr("doc_offsets", "doc_term_offsets", "ndocs", 1, 0, u64),
        Arr("result_term", "result_term", "nresults", 0, 0, u32),  # 0xFFFFFFFF throughout a failed document
        Arr("status", "doc_term_status", "ndocs", 0, 0, i32),      # 0, or 5 for a failed document (no records)
    )

    def __init__(self, records, doc_offsets, result_term, status, flags=SP_TERM_VALUES | SP_TERM_TEXT, handle_bound=0):
        self.handle_bound = handle_bound    # the bound the terms were built with (0: not known; batchDictionary then needs it as an argument)
        self.records, self.doc_offsets, self.result_term, self.status, self.flags = records, doc_offsets, result_term, status, flags

    def doc(self, i):
        return self.records[int(self.doc_offsets[i]):int(self.doc_offsets[i + 1])]

    def terms(self, d, mb, values=None, text=None):
        """yields (handle, value bytes, count, first_ordpos, last_ordend) per term of document d; mb: the finished batch,
        values / text: the MatchValues / MatchText the terms were built from"""
        first = int(mb.doc_offsets[d])
        for h, count, pos, end, fr, size in self.doc(d).tolist():
            value = _term_value(self.flags, mb, values, text, first + fr)
            assert len(value) == size
            yield h, value, count, pos, end


def batchTerms(mb, values=None, text=None, handle_bound=0, flags=SP_TERM_VALUES | SP_TERM_TEXT):
    """The index terms of a batch already on the host (a MatchBatch in document order: finishedFetch, batchFetch, matchDocs)
    with its MatchValues and / or MatchText (their results family), by the rule of the device call, without a device.
    handle_bound: PatternMatcherInstance.handleBound().  Returns a MatchTerms."""
    b, keep = _host_batch(mb, formats="results", status=True)       # (keep: until the call has returned)
    v, x = _host_source(values, keep), _host_source(text, keep)
    return _twin(MatchTerms, "sp_match_batch_terms", ctypes.byref(b), _ref(v), _ref(x), handle_bound, flags)


class MatchDictionary:
    """The dictionary of a terms batch (host copies): one entry per distinct pair (handle, value bytes) over all documents, in
    the order of first occurrence, and per term record the index of its entry (include/strus_pattern_amd.h "batch
    dictionary").  An entry owns no bytes: its value is that of term record first_term of document first_doc."""
    _C, _SCALARS, _TOTAL, _WHAT = capi.SpMatchDictionary, (), "ndict", "dictionary of the batch"
    _FREE, _FETCH = "sp_match_dictionary_free", "sp_matcher_ctx_finished_dictionary_fetch"
    _ARRAYS = (
        Arr("records", "records", "ndict", 0, 8, u32),        # handle, value_bytes, first_doc, first_term, doc_freq, max_count, count (low, high)
        Arr("term_dict", "term_dict", "nterms", 0, 0, u32),   # parallel to the term records
        Arr("doc_offsets", "doc_dict_offsets", "ndocs", 1, 0, u64),   # the entries first seen in every document
        Arr("handle_terms", "handle_terms", "handle_bound", 0, 0, u32),   # distinct terms per handle
    )

    def __init__(self, records, term_dict, doc_offsets, handle_terms):
        self.records, self.term_dict, self.doc_offsets, self.handle_terms = records, term_dict, doc_offsets, handle_terms
        self.counts = np.ascontiguousarray(records[:, 6:8]).view(np.uint64).reshape(-1)   # (ndict,) u64: the collection frequencies

    def entries(self, mb, terms, values=None, text=None):
        """yields (handle, value bytes, doc_freq, count, max_count) per entry, in dictionary order; mb: the finished batch,
        terms: the MatchTerms the dictionary was built from, values / text: the MatchValues / MatchText of those"""
        for (h, size, d, t, df, mx, _, _), count in zip(self.records.tolist(), self.counts.tolist()):
            value = _term_value(terms.flags, mb, values, text, int(mb.doc_offsets[d]) + int(terms.doc(d)[t][4]))
            assert len(value) == size
            yield h, value, df, count, mx


def batchDictionary(mb, terms, values=None, text=None, handle_bound=0):
    """The dictionary of the terms of a batch already on the host (terms: the MatchTerms of finishedTermsFetch or batchTerms,
    mb, values, text: what they were built from), by the rule of the device call, without a device.  The handle bound, which
    is the length of handle_terms, is that of `terms`; a MatchTerms made by hand without one needs `handle_bound`
    (PatternMatcherInstance.handleBound()): it is not guessed from the records.  Returns a MatchDictionary."""
    bound = handle_bound or terms.handle_bound
    if not bound:
        raise PatternError("no dictionary of the batch: the terms carry no handle bound and none was given")
    b, keep = _host_batch(mb, formats="results", status=True)       # (keep: until the call has returned)
    v, x = _host_source(values, keep), _host_source(text, keep)
    t = _to_c(terms, keep, handle_bound=bound)
    return _twin(MatchDictionary, "sp_match_batch_dictionary", ctypes.byref(b), _ref(v), _ref(x), ctypes.byref(t))


class MatchDictionaryOrder:
    """The order of a dictionary (host copies): its entries ranked by (handle, value bytes), the inverse permutation, per sorted
    position the leading bytes its value shares with the one before it inside a handle, and where the entries of every handle
    start (include/strus_pattern_amd.h "dictionary order")."""
    _C, _SCALARS, _TOTAL, _WHAT = capi.SpMatchDictionaryOrder, (), "ndict", "order of the dictionary"
    _FREE, _FETCH = "sp_match_dictionary_order_free", "sp_matcher_ctx_finished_dictionary_order_fetch"
    _ARRAYS = (
        Arr("order", "order", "ndict", 0, 0, u32),                  # the entry at every sorted position
        Arr("rank", "rank", "ndict", 0, 0, u32),                    # the sorted position of every entry
        Arr("prefix_bytes", "prefix_bytes", "ndict", 0, 0, u32),    # parallel to order: bytes shared with the position before, 0 at the first of a handle
        Arr("handle_offsets", "handle_offsets", "handle_bound", 1, 0, u64),   # the entries of handle h are order[handle_offsets[h]:handle_offsets[h+1]]
    )

    def __init__(self, order, rank, prefix_bytes, handle_offsets):
        self.order, self.rank, self.prefix_bytes, self.handle_offsets = order, rank, prefix_bytes, handle_offsets

    def handle(self, h):
        """the entries of handle h, ascending by value"""
        return self.order[int(self.handle_offsets[h]):int(self.handle_offsets[h + 1])]

    def find(self, handle, value, mb, terms, dictionary, values=None, text=None):
        """the entry (handle, value bytes) by bisection over the entries of the handle, or None; mb: the finished batch, terms,
        dictionary: the MatchTerms and the MatchDictionary the order was built from, values / text: the sources of the terms"""
        if not 0 <= handle < len(self.handle_offsets) - 1:
            return None
        value, lo, hi = bytes(value), int(self.handle_offsets[handle]), int(self.handle_offsets[handle + 1])
        while lo < hi:
            mid = (lo + hi) // 2
            _, _, d, t = dictionary.records[int(self.order[mid])][:4].tolist()
            other = bytes(_term_value(terms.flags, mb, values, text, int(mb.doc_offsets[d]) + int(terms.doc(d)[t][4])))
            if other == value:
                return int(self.order[mid])
            lo, hi = (mid + 1, hi) if other < value else (lo, mid)
        return None


def batchDictionaryOrder(mb, terms, dictionary, values=None, text=None):
    """The order of a dictionary already on the host (terms: the MatchTerms, dictionary: the MatchDictionary built from them,
    mb, values, text: what the terms were built from: the fetches of a context, or the twins), by the rule of the device call,
    without a device.  Returns a MatchDictionaryOrder."""
    b, keep = _host_batch(mb, formats="results", status=True)       # (keep: until the call has returned)
    v, x = _host_source(values, keep), _host_source(text, keep)
    bound = terms.handle_bound or len(dictionary.handle_terms)      # (terms made by hand may carry none: that of the dictionary then)
    t, d = _to_c(terms, keep, handle_bound=bound), _to_c(dictionary, keep, flags=terms.flags)
    return _twin(MatchDictionaryOrder, "sp_match_batch_dictionary_order", ctypes.byref(b), _ref(v), _ref(x), ctypes.byref(t), ctypes.byref(d))


def _bytes_of(array, n):
    """the first n bytes of a ctypes array of uint8"""
    return ctypes.string_at(array, n) if n else b""


class MatchTermBlocks:
    """The term blocks of a dictionary order (host copies): the sorted dictionary front-coded in blocks of block_entries
    positions, each block decodable from its own bytes and its handle (include/strus_pattern_amd.h "term blocks").  The first
    product that owns its bytes: neither the batch nor its text or values are needed to read it."""
    _C, _SCALARS, _TOTAL, _WHAT = capi.SpMatchTermBlocks, ("ndict", "block_entries"), None, "term blocks of the batch"
    _FREE, _FETCH = "sp_match_term_blocks_free", "sp_matcher_ctx_finished_term_blocks_fetch"
    _ARRAYS = (
        Arr("bytes", "bytes", "nbytes", 0, 0, ctypes.c_uint8),             # the codes of all sorted positions, without gaps
        Arr("block_offsets", "block_offsets", "nblocks", 1, 0, u64),       # block j is bytes[block_offsets[j]:block_offsets[j+1]]
        Arr("block_handles", "block_handles", "nblocks", 0, 0, u32),       # the handle of the head of every block
        Arr("totals", "totals", None, 4, 0, u64),                          # nblocks, nbytes, block_entries, the sum of value_bytes
    )

    def __init__(self, bytes, block_offsets, block_handles, totals, ndict=0, block_entries=16):
        self.bytes, self.block_offsets, self.block_handles, self.totals = bytes, block_offsets, block_handles, totals
        self.ndict, self.block_entries = ndict, block_entries

    def block(self, j):
        """the entries of block j, decoded by the library's reader from the block alone: a list of (handle, value bytes,
        doc_freq, count) in sorted order"""
        keep = []
        s = _to_c(self, keep)                                          # (keep: until the calls have returned)
        n, nv, err = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.create_string_buffer(256)
        call = capi.lib().sp_match_term_blocks_decode_block
        rc = call(ctypes.byref(s), j, None, 0, None, 0, ctypes.byref(n), ctypes.byref(nv), err, 256)
        if rc == 0:
            entries, values = (capi.SpTermBlockEntry * max(n.value, 1))(), (ctypes.c_uint8 * max(nv.value, 1))()
            rc = call(ctypes.byref(s), j, entries, n.value, values, nv.value, ctypes.byref(n), ctypes.byref(nv), err, 256)
        if rc != 0:
            raise PatternError("no block %d of the %s (%d): %s" % (j, self._WHAT, rc, err.value.decode()))
        data = _bytes_of(values, nv.value)
        return [(e.handle, data[e.value_offset:e.value_offset + e.value_bytes], e.doc_freq, e.count) for e in entries[:n.value]]

    def entries(self):
        """all entries in sorted order: (handle, value bytes, doc_freq, count)"""
        return [entry for j in range(len(self.block_handles)) for entry in self.block(j)]

    def find(self, handle, value):
        """the sorted position of the entry (handle, value bytes), or None, from the product alone: bisects the block heads by
        (block_handles[j], head value), then decodes one block"""
        key, lo, hi = (int(handle), bytes(value)), 0, len(self.block_handles)
        while lo < hi:                                                  # the last block whose head is not behind the key
            mid = (lo + hi) // 2
            head = self.block(mid)[0]
            lo, hi = (mid + 1, hi) if (head[0], head[1]) <= key else (lo, mid)
        if not lo:
            return None
        for k, (h, v, _, _) in enumerate(self.block(lo - 1)):
            if (h, v) == key:
                return (lo - 1) * int(self.block_entries) + k
        return None


def batchTermBlocks(mb, terms, dictionary, order, values=None, text=None):
    """The term blocks of a dictionary order already on the host (terms: the MatchTerms, dictionary: the MatchDictionary built
    from them, order: its MatchDictionaryOrder, mb, values, text: what the terms were built from: the fetches of a context, or
    the twins), by the rule of the device call, without a device.  Returns a MatchTermBlocks."""
    b, keep = _host_batch(mb, formats="results", status=True)       # (keep: until the call has returned)
    v, x = _host_source(values, keep), _host_source(text, keep)
    bound = terms.handle_bound or len(dictionary.handle_terms)      # (terms made by hand may carry none: that of the dictionary then)
    t, d, o = _to_c(terms, keep, handle_bound=bound), _to_c(dictionary, keep, flags=terms.flags), _to_c(order, keep)
    return _twin(MatchTermBlocks, "sp_match_batch_term_blocks", ctypes.byref(b), _ref(v), _ref(x), ctypes.byref(t), ctypes.byref(d), ctypes.byref(o))


class MatchPostings:
    """The postings of a dictionary (host copies): per term record one posting (doc, term, count, first_ordpos), the postings
    of dictionary entry e together and ascending by document, and per term record the index of its posting
    (include/strus_pattern_amd.h "batch postings")."""
    _C, _SCALARS, _TOTAL, _WHAT = capi.SpMatchPostings, (), "nterms", "postings of the batch"
    _FREE, _FETCH = "sp_match_postings_free", "sp_matcher_ctx_finished_postings_fetch"
    _ARRAYS = (
        Arr("records", "postings", "nterms", 0, 4, u32),            # doc, term, count, first_ordpos
        Arr("entry_offsets", "entry_offsets", "ndict", 1, 0, u64),  # the postings of entry e are records[entry_offsets[e]:entry_offsets[e+1]]
        Arr("record_posting", "record_posting", "nterms", 0, 0, u32),   # parallel to the term records
    )

    def __init__(self, records, entry_offsets, record_posting):
        self.records, self.entry_offsets, self.record_posting = records, entry_offsets, record_posting

    def entry(self, e):
        """the postings of dictionary entry e, in document order: rows (doc, term, count, first_ordpos)"""
        return self.records[int(self.entry_offsets[e]):int(self.entry_offsets[e + 1])]

    def docs(self, e):
        """the documents that hold dictionary entry e, ascending"""
        return self.entry(e)[:, 0]


def batchPostings(terms, dictionary):
    """The postings of a dictionary already on the host (terms: the MatchTerms, dictionary: the MatchDictionary built from
    them: the fetches of a context, or batchTerms and batchDictionary), by the rule of the device call, without a device.
    Returns a MatchPostings."""
    keep = []                                                        # (until the call has returned)
    t, d = _to_c(terms, keep), _to_c(dictionary, keep, flags=terms.flags)
    return _twin(MatchPostings, "sp_match_batch_postings", ctypes.byref(t), ctypes.byref(d))


class MatchPositions:
    """The positions of the postings of a batch (host copies): per participating result one occurrence (ordpos, result), the
    occurrences of posting p together, ascending by ordpos and then by result, and per posting the number of distinct
    positions (include/strus_pattern_amd.h "posting positions")."""
    _C, _SCALARS, _TOTAL, _WHAT = capi.SpMatchPositions, (), None, "positions of the batch"
    _FREE, _FETCH = "sp_match_positions_free", "sp_matcher_ctx_finished_positions_fetch"
    _ARRAYS = (
        Arr("occurrences", "occurrences", "nocc", 0, 2, u32),               # ordpos, result (index inside the document's finished block)
        Arr("posting_offsets", "posting_offsets", "nterms", 1, 0, u64),     # the occurrences of posting p are occurrences[posting_offsets[p]:posting_offsets[p+1]]
        Arr("posting_positions", "posting_positions", "nterms", 0, 0, u32),  # distinct ordpos per posting
        Arr("totals", "totals", None, 2, 0, u64),                           # nocc, the sum of posting_positions
    )

    def __init__(self, occurrences, posting_offsets, posting_positions, totals):
        self.occurrences, self.posting_offsets, self.posting_positions, self.totals = occurrences, posting_offsets, posting_positions, totals

    def posting(self, p):
        """the occurrences of posting p, by position: rows (ordpos, result)"""
        return self.occurrences[int(self.posting_offsets[p]):int(self.posting_offsets[p + 1])]

    def positions(self, p):
        """the distinct ordinal positions of posting p, ascending: what an index stores"""
        pos = self.posting(p)[:, 0]
        return pos[np.concatenate(([True], pos[1:] != pos[:-1]))] if len(pos) else pos


def batchPositions(mb, terms, postings):
    """The positions of the postings of a batch already on the host (mb: the finished MatchBatch, terms: its MatchTerms,
    postings: the MatchPostings built from their dictionary: the fetches of a context, or the twins), by the rule of the device
    call, without a device.  Returns a MatchPositions."""
    b, keep = _host_batch(mb)                                        # (keep: until the call has returned)
    t, q = _to_c(terms, keep), _to_c(postings, keep, ndocs=len(terms.doc_offsets) - 1)
    return _twin(MatchPositions, "sp_match_batch_positions", ctypes.byref(b), ctypes.byref(t), ctypes.byref(q))


class MatchPostingBlocks:
    """The posting blocks of a batch (host copies): the posting lists with their positions in the sorted order of the dictionary,
    cut into the blocks of the term blocks and delta-coded, each block decodable from its own bytes
    (include/strus_pattern_amd.h "posting blocks").  List k is the term at position k of the MatchTermBlocks of the same batch:
    the two together are the index segment of the batch."""
    _C, _SCALARS, _TOTAL, _WHAT = capi.SpMatchPostingBlocks, ("ndict", "block_entries"), None, "posting blocks of the batch"
    _FREE, _FETCH = "sp_match_posting_blocks_free", "sp_matcher_ctx_finished_posting_blocks_fetch"
    _ARRAYS = (
        Arr("bytes", "bytes", "nbytes", 0, 0, ctypes.c_uint8),             # the codes of all sorted positions, without gaps
        Arr("block_offsets", "block_offsets", "nblocks", 1, 0, u64),       # block j is bytes[block_offsets[j]:block_offsets[j+1]]
        Arr("totals", "totals", None, 4, 0, u64),                          # nblocks, nbytes, block_entries, the position varints written
    )

    def __init__(self, bytes, block_offsets, totals, ndict=0, block_entries=16):
        self.bytes, self.block_offsets, self.totals = bytes, block_offsets, totals
        self.ndict, self.block_entries = ndict, block_entries

    def block(self, j):
        """the lists of block j, decoded by the library's reader from the block alone: per sorted position a list of
        (doc, count, [positions]) in document order"""
        keep = []
        s = _to_c(self, keep)                                          # (keep: until the calls have returned)
        nl, np_, nq, err = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.create_string_buffer(256)
        counts = (ctypes.byref(nl), ctypes.byref(np_), ctypes.byref(nq), err, 256)
        call = capi.lib().sp_match_posting_blocks_decode_block
        rc = call(ctypes.byref(s), j, None, 0, None, 0, None, 0, *counts)
        if rc == 0:
            lists, postings, positions = (u32 * max(nl.value, 1))(), (capi.SpBlockPosting * max(np_.value, 1))(), (u32 * max(nq.value, 1))()
            rc = call(ctypes.byref(s), j, lists, nl.value, postings, np_.value, positions, nq.value, *counts)
        if rc != 0:
            raise PatternError("no block %d of the %s (%d): %s" % (j, self._WHAT, rc, err.value.decode()))
        out, at = [], 0
        for n in lists[:nl.value]:
            out.append([(p.doc, p.count, list(positions[p.position_offset:p.position_offset + p.npos])) for p in postings[at:at + n]])
            at += n
        return out

    def lists(self):
        """all lists in sorted order: per sorted position [(doc, count, [positions])]"""
        return [entry for j in range(len(self.block_offsets) - 1) for entry in self.block(j)]

    def postings(self, k):
        """the list of sorted position k -- MatchTermBlocks.find(handle, value) gives the k -- as [(doc, count, [positions])],
        decoding only its block"""
        B = int(self.block_entries)
        if not 0 <= k < self.ndict:
            raise PatternError("no sorted position %d in the %s" % (k, self._WHAT))
        return self.block(k // B)[k % B]


def batchPostingBlocks(dictionary, order, postings, positions):
    """The posting blocks of a dictionary already on the host (dictionary: the MatchDictionary, order: its MatchDictionaryOrder,
    postings: its MatchPostings, positions: their MatchPositions: the fetches of a context, or the twins), by the rule of the
    device call, without a device, a batch or a source.  Returns a MatchPostingBlocks."""
    keep = []                                                        # (until the call has returned)
    d, o, q, x = _to_c(dictionary, keep), _to_c(order, keep), _to_c(postings, keep), _to_c(positions, keep)
    return _twin(MatchPostingBlocks, "sp_match_batch_posting_blocks", ctypes.byref(d), ctypes.byref(o), ctypes.byref(q), ctypes.byref(x))


SP_LOOKUP_PREFIX = 1    # include/strus_pattern_amd.h: the flag of a lookup by prefix


class SegmentLookup:
    """The answer to the queries of one lookup in an index segment (host copies): per query its run of sorted positions, the
    runs one behind the other being the selection, and per selected position its record, its full value and its decoded posting
    list (include/strus_pattern_amd.h "segment lookups")."""
    _C, _SCALARS, _TOTAL, _WHAT = capi.SpSegmentLookup, ("flags",), None, "lookup in the segment"
    _FREE, _FETCH = "sp_segment_lookup_free", "sp_segment_lookup_fetch"
    _ARRAYS = (
        Arr("q_first", "q_first", "nq", 0, 0, u32),                        # the first sorted position not below the query
        Arr("q_count", "q_count", "nq", 0, 0, u32),                        # the length of its run
        Arr("q_status", "q_status", "nq", 0, 0, u32),                      # 0, or an SP_LOOKUP_ERR_* for a walk that met a malformed code
        Arr("q_sel_offsets", "q_sel_offsets", "nq", 1, 0, u64),            # the run of query i is the selection [q_sel_offsets[i], q_sel_offsets[i+1])
        Arr("selections", "selections", "nsel", 0, 6, u32),                # position, handle, doc_freq, value_bytes, count (low, high)
        Arr("sel_value_offsets", "sel_value_offsets", "nsel", 1, 0, u64),  # into values
        Arr("sel_posting_offsets", "sel_posting_offsets", "nsel", 1, 0, u64),   # into postings
        Arr("values", "values", "nvalue_bytes", 0, 0, ctypes.c_uint8),     # the full values of the selected positions
        Arr("postings", "postings", "npostings", 0, 4, u32),               # doc, count, npos, 0
        Arr("posting_position_offsets", "posting_position_offsets", "npostings", 1, 0, u64),   # into positions
        Arr("positions", "positions", "npositions", 0, 0, u32),            # the distinct ordinal positions, absolute and ascending
        Arr("totals", "totals", None, 4, 0, u64),                          # nsel, npostings, npositions, the bytes of values
    )

    def __init__(self, q_first, q_count, q_status, q_sel_offsets, selections, sel_value_offsets, sel_posting_offsets, values, postings,
                 posting_position_offsets, positions, totals, flags=0):
        self.q_first, self.q_count, self.q_status, self.q_sel_offsets = q_first, q_count, q_status, q_sel_offsets
        self.selections, self.sel_value_offsets, self.sel_posting_offsets = selections, sel_value_offsets, sel_posting_offsets
        self.values, self.postings, self.posting_position_offsets, self.positions = values, postings, posting_position_offsets, positions
        self.totals, self.flags = totals, flags
        self.counts = np.ascontiguousarray(selections[:, 4:6]).view(np.uint64).reshape(-1)    # (nsel,) u64: the collection frequencies

    def selection(self, s):
        """selected position s: (handle, value bytes, doc_freq, count, [(doc, count, [positions])])"""
        _, handle, doc_freq, _, _, _ = self.selections[s].tolist()
        value = self.values[int(self.sel_value_offsets[s]):int(self.sel_value_offsets[s + 1])].tobytes()
        postings = []
        for p in range(int(self.sel_posting_offsets[s]), int(self.sel_posting_offsets[s + 1])):
            doc, count, _, _ = self.postings[p].tolist()
            postings.append((doc, count, self.positions[int(self.posting_position_offsets[p]):int(self.posting_position_offsets[p + 1])].tolist()))
        return handle, value, doc_freq, int(self.counts[s]), postings

    def query(self, i):
        """what query i found, in sorted order: [(handle, value bytes, doc_freq, count, [(doc, count, [positions])])]"""
        return [self.selection(s) for s in range(int(self.q_sel_offsets[i]), int(self.q_sel_offsets[i + 1]))]


def _host_queries(queries):
    """The query arguments of a lookup call (handles, offsets, bytes, nq) for an iterable of (handle, value bytes), and the arrays
    they point into: the caller holds them until its C call has returned"""
    queries = [(int(h), bytes(v)) for h, v in queries]
    handles = np.ascontiguousarray([h for h, _ in queries], dtype=np.uint32)
    offsets = np.zeros(len(queries) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(v) for _, v in queries], dtype=np.uint64)
    data = ctypes.create_string_buffer(b"".join(v for _, v in queries), int(offsets[-1]) + 1)   # (a pointer that is not null for no bytes)
    return (handles.ctypes.data, offsets.ctypes.data, ctypes.addressof(data), len(queries)), [handles, offsets, data]


def segmentLookup(term_blocks, posting_blocks, queries, prefix=False):
    """The lookup of `queries` -- an iterable of (handle, value bytes) -- in the segment made of a MatchTermBlocks and the
    MatchPostingBlocks of the same batch, exact or by prefix, by the rule of Segment.lookupDevice, without a device.  Returns a
    SegmentLookup."""
    keep = []                                                        # (until the call has returned)
    t, p = _to_c(term_blocks, keep), _to_c(posting_blocks, keep)
    args, held = _host_queries(queries)
    return _twin(SegmentLookup, "sp_match_segment_lookup", ctypes.byref(t), ctypes.byref(p), *args, SP_LOOKUP_PREFIX if prefix else 0)


class Segment:
    """An index segment on the device: copies of the term blocks and the posting blocks of one batch that live without the
    context that built them, and the buffers of the lookups in it (include/strus_pattern_amd.h "segment lookups")."""

    def __init__(self, handle):
        self._L, self._h = capi.lib(), handle

    @classmethod
    def open(cls, term_blocks, posting_blocks):
        """the segment of a MatchTermBlocks and the MatchPostingBlocks of the same batch: fetches, twin output, or what was read
        back from a file; only the tables are checked"""
        keep, h, err = [], ctypes.c_void_p(), ctypes.create_string_buffer(256)
        t, p = _to_c(term_blocks, keep), _to_c(posting_blocks, keep)
        rc = capi.lib().sp_segment_open(ctypes.byref(t), ctypes.byref(p), ctypes.byref(h), err, 256)
        if rc != 0:
            raise PatternError("no segment (%d): %s" % (rc, err.value.decode()))
        return cls(h)

    @classmethod
    def fromContext(cls, ctx, stream=0):
        """the segment of the term blocks and the posting blocks built last on the PatternMatcherContext `ctx`, copied on the
        device; it outlives the context and its next batch"""
        h = ctypes.c_void_p()
        rc = capi.lib().sp_segment_from_ctx(ctx._h, stream or None, ctypes.byref(h))
        if rc != 0:
            raise PatternError("no segment of the context (%d): %s" % (rc, ctx._err()))
        return cls(h)

    def _err(self):
        return self._L.sp_segment_last_error(self._h).decode(errors="replace")

    def lookupDevice(self, queries, prefix=False, stream=0):
        """look `queries` -- an iterable of (handle, value bytes) -- up on the device, exact or by prefix: their runs, and the
        records, values and decoded posting lists of what they select (the call waits once for the sizes, under prefix=True
        twice; the emitting launch is asynchronous on `stream`).  Returns the device pointers (capi.SpSegmentLookupDevice), valid
        until the next lookup on this segment."""
        args, held = _host_queries(queries)                          # (held: until the call has returned)
        out = capi.SpSegmentLookupDevice()
        rc = self._L.sp_segment_lookup_device(self._h, *args, SP_LOOKUP_PREFIX if prefix else 0, stream or None, ctypes.byref(out))
        if rc != 0:
            raise PatternError("lookup in the segment failed (%d): %s" % (rc, self._err()))
        return out

    def lookupFetch(self):
        """plain host copy of the last lookupDevice: a SegmentLookup"""
        return _product(SegmentLookup, lambda s: self._L.sp_segment_lookup_fetch(self._h, ctypes.byref(s)),
                        lambda rc: "fetching the %s failed (%d): %s" % (SegmentLookup._WHAT, rc, self._err()))

    def lastLookupMs(self):
        """duration of the last lookupDevice in milliseconds"""
        ms = ctypes.c_double(-1.0)
        if self._L.sp_segment_last_lookup_ms(self._h, ctypes.byref(ms)) != 0:
            raise PatternError("no timed lookup")
        return ms.value

    def close(self):
        if self._h:
            self._L.sp_segment_free(self._h)
            self._h = None

    def __del__(self):
        self.close()
