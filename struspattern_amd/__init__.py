"""struspattern_amd -- MI355X-native two-level pattern engine behind the strus pattern API.

Python mirror of the reference's plugin interfaces for the hot path (same method names and
argument meaning as src/patternMatcher.cpp / src/patternLexer.cpp of strusPattern), layered on
the C-ABI of libstruspattern_amd.so (include/strus_pattern_amd.h).  The native library is the
product; there is no Python/CPU fallback for matching.
"""
import ctypes

import numpy as np

from . import capi
from .capi import SpLexem, SpResult, SpResultItem

__all__ = ["PatternMatcher", "PatternMatcherInstance", "PatternMatcherContext", "PatternLexer", "PatternLexerInstance",
           "PatternLexerContext", "PatternError", "JOIN_OP", "POSITION_BIND", "matchSegmentedDocs", "MatchText", "batchText", "MatchValues", "batchValues", "PatternFreq", "batchPatternFreq", "MatchTerms", "batchTerms", "MatchDictionary", "batchDictionary", "MatchPostings", "batchPostings", "MatchPositions", "batchPositions"]

SP_CTX_RESULT_SETS = 1      # include/strus_pattern_amd.h: context flag of result-set mode
SP_FINISH_CANONICAL = 1     # include/strus_pattern_amd.h: finish flag of the canonical order inside a document
SP_TEXT_RESULTS, SP_TEXT_ITEMS = 1, 2   # include/strus_pattern_amd.h: the families of spans of a text call
SP_VALUE_RESULTS, SP_VALUE_ITEMS = 1, 2  # include/strus_pattern_amd.h: the families of records of a values call
SP_TERM_VALUES, SP_TERM_TEXT = 1, 2    # include/strus_pattern_amd.h: the sources of the term values of a terms call
SP_ERR_UNAVAILABLE = -6     # include/strus_pattern_amd.h: a value that does not exist for the context

JOIN_OP = {"sequence": 0, "sequence_imm": 1, "sequence_struct": 2, "within": 3, "within_struct": 4, "any": 5, "and": 6}

DOC_STATUS = {
    0: "ok", 1: "term events not fed in ascending order", 2: "working set of the document exceeds the arena",
    3: "pattern with too many identical key events defined", 4: "internal: encountered past trigger with follow",
    5: "term event out of range", 6: "illegal free of event data reference",
}


class PatternError(RuntimeError):
    pass


class MatchBatch:
    """Results of a batch of documents (host copies)."""

    def __init__(self, results, items, doc_offsets, stats, status, result_format=None, item_format=None):
        self.result_format = result_format  # (n,) u32 format handle per result, None without format strings
        self.item_format = item_format      # (m, 2) u32 {format handle, nsub} per item (see resultformat.py)
        self.results = results          # (n, 9) u32: handle, ordpos, ordend, origseg, origpos, origendseg, origend, item_begin, item_count
        self.items = items              # (m, 7) u32: variable, ordpos, ordend, origseg, origpos, origendseg, origend
        self.doc_offsets = doc_offsets  # (ndocs+1,) u64
        self.stats = stats              # (ndocs, 4) u64
        self.status = status            # (ndocs,) i32

    def doc(self, i):
        return self.results[self.doc_offsets[i]:self.doc_offsets[i + 1]]


def _rows(ptr, n, k, ctype=ctypes.c_uint32):
    """n rows of k columns of `ctype` behind the ctypes pointer `ptr` (to records of any type), copied: shape (n, k), or (n,) for k = 0"""
    if not n or not ptr:
        return np.zeros((n, k) if k else n, ctype)
    a = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=(n * max(k, 1),)).copy()
    return a.reshape(n, k) if k else a


def _formats_of(b):
    if not b.result_format:
        return None, None
    return _rows(b.result_format, b.nresults, 0), _rows(b.item_format, b.nitems, 2)


def _match_batch_of(b):
    """the MatchBatch of a capi.SpMatchBatch (copies)"""
    return MatchBatch(_rows(b.results, b.nresults, 9), _rows(b.items, b.nitems, 7), _rows(b.doc_result_offsets, b.ndocs + 1, 0, ctypes.c_uint64),
                      _rows(b.doc_stats, b.ndocs, 4, ctypes.c_uint64), _rows(b.doc_status, b.ndocs, 0, ctypes.c_int32), *_formats_of(b))


def _product(struct_type, call, free, convert, failed):
    """One C call that fills a struct the library allocates for: call(struct) is the return code, failed(rc) the message of
    the PatternError for one that is not 0, convert(struct) the Python copy.  The struct is freed whatever happens."""
    s = struct_type()
    rc = call(s)
    try:
        if rc != 0:
            raise PatternError(failed(rc))
        return convert(s)
    finally:
        free(ctypes.byref(s))


def _host_batch(mb, items=False, formats=None, status=False):
    """The capi.SpMatchBatch of a MatchBatch for a host twin, and the arrays it points into: the caller holds them until its
    C call has returned.  items: with the items; formats: "results" with the format handles of the results, "all" with those
    of the items too (where the batch has them); status: with the document status (where the batch has one)."""
    b, keep = capi.SpMatchBatch(), []

    def point(field, array, ctype):
        keep.append(array)
        setattr(b, field, ctypes.cast(array.ctypes.data, ctypes.POINTER(ctype)))

    res = np.ascontiguousarray(mb.results, dtype=np.uint32).reshape(-1, 9)
    offs = np.ascontiguousarray(mb.doc_offsets, dtype=np.uint64)
    b.ndocs, b.nresults = len(offs) - 1, len(res)
    point("results", res, SpResult)
    point("doc_result_offsets", offs, ctypes.c_uint64)
    if items:
        its = np.ascontiguousarray(mb.items, dtype=np.uint32).reshape(-1, 7)
        b.nitems = len(its)
        point("items", its, SpResultItem)
    if status and mb.status is not None:
        point("doc_status", np.ascontiguousarray(mb.status, dtype=np.int32), ctypes.c_int32)
    if formats == "results" and mb.result_format is not None:
        rf = np.ascontiguousarray(mb.result_format, dtype=np.uint32).reshape(-1)
        if len(rf) != len(res):
            raise PatternError("format array of the batch is not parallel to its results")
        point("result_format", rf, ctypes.c_uint32)
    if formats == "all" and mb.result_format is not None and mb.item_format is not None:
        rf = np.ascontiguousarray(mb.result_format, dtype=np.uint32).reshape(-1)
        itf = np.ascontiguousarray(mb.item_format, dtype=np.uint32).reshape(-1, 2)
        if len(rf) != len(res) or len(itf) != b.nitems:
            raise PatternError("format arrays of the batch are not parallel to its results and items")
        point("result_format", rf, ctypes.c_uint32)
        point("item_format", itf, ctypes.c_uint32)
    return b, keep


def _host_text(text, seg_offsets, doc_seg_offsets):
    """The text source arguments of a host twin (text, nbytes, seg_offsets, nseg, doc_seg_offsets), and what they point into"""
    text = bytes(text)
    so = np.ascontiguousarray(seg_offsets, dtype=np.uint64)
    dso = None if doc_seg_offsets is None else np.ascontiguousarray(doc_seg_offsets, dtype=np.uint64)
    return (text, len(text), so.ctypes.data, len(so) - 1, dso.ctypes.data if dso is not None else None), [text, so, dso]


class _ByteFamilies:
    """Bytes per result and per item of a batch (host copies): those of record i of a family are bytes[offsets[i]:offsets[i+1]],
    parallel to the results / items of the batch.  A family that was not asked for is None."""
    _results = _items = None    # the attributes with the bytes of the two families

    def result(self, i):
        return getattr(self, self._results)[int(self.result_offsets[i]):int(self.result_offsets[i + 1])]

    def item(self, i):
        return getattr(self, self._items)[int(self.item_offsets[i]):int(self.item_offsets[i + 1])]


def _byte_families_of(cls, s, result, item, status):
    """the MatchText / MatchValues (`cls`) of its C struct `s` (copies); result, item: the fields (bytes, offsets) of a family
    of `s`, status: its status field"""
    def family(fields, n, total):
        data, offsets = getattr(s, fields[0]), getattr(s, fields[1])
        if not offsets:
            return None, None
        return (ctypes.string_at(data, total) if total else b""), _rows(offsets, n + 1, 0, ctypes.c_uint64)
    return cls(*family(result, s.nresults, s.totals[0]), *family(item, s.nitems, s.totals[1]), _rows(getattr(s, status), s.ndocs, 0, ctypes.c_int32))


class MatchText(_ByteFamilies):
    """The text that the results and items of a finished batch cover (host copies): the bytes of span i of a family are
    text[offsets[i]:offsets[i+1]], parallel to the results / items of the batch.  A family that was not asked for is None."""
    _results, _items = "result_text", "item_text"

    def __init__(self, result_text, result_offsets, item_text, item_offsets, status):
        self.result_text = result_text        # bytes
        self.result_offsets = result_offsets  # (nresults+1,) u64
        self.item_text = item_text
        self.item_offsets = item_offsets      # (nitems+1,) u64
        self.status = status                  # (ndocs,) i32: 0, or 5 for a document with a span outside the text (all its spans empty)


def _match_text_of(t):
    """the MatchText of a capi.SpMatchText (copies)"""
    return _byte_families_of(MatchText, t, ("result_text", "result_text_offsets"), ("item_text", "item_text_offsets"), "doc_text_status")


def batchText(mb, text, seg_offsets, doc_seg_offsets=None, results=True, items=True):
    """The text of a batch already on the host (a MatchBatch in document order with items without gaps: finishedFetch,
    batchFetch, matchDocs), by the rule of the device call (include/strus_pattern_amd.h "matched text"), without a device:
    `text` holds the segments back to back (seg_offsets: nseg+1 byte offsets), document d is the segments
    [doc_seg_offsets[d], doc_seg_offsets[d+1]), or segment d without doc_seg_offsets.  Returns a MatchText."""
    L = capi.lib()
    b, keep = _host_batch(mb, items=True)
    source, keep_text = _host_text(text, seg_offsets, doc_seg_offsets)      # (keep, keep_text: until the call has returned)
    err = ctypes.create_string_buffer(256)
    flags = (SP_TEXT_RESULTS if results else 0) | (SP_TEXT_ITEMS if items else 0)
    return _product(capi.SpMatchText, lambda t: L.sp_match_batch_text(ctypes.byref(b), *source, flags, ctypes.byref(t), err, 256),
                    L.sp_match_text_free, _match_text_of, lambda rc: "no text of the batch (%d): %s" % (rc, err.value.decode()))


class MatchValues(_ByteFamilies):
    """The values of the format strings of a finished batch (host copies): the value of record i of a family is
    values[offsets[i]:offsets[i+1]], parallel to the results / items of the batch; a record without a format has an empty
    range (the format arrays of the batch tell an empty value from no value).  A family that was not asked for is None."""
    _results, _items = "result_values", "item_values"

    def __init__(self, result_values, result_offsets, item_values, item_offsets, status):
        self.result_values = result_values    # bytes
        self.result_offsets = result_offsets  # (nresults+1,) u64
        self.item_values = item_values
        self.item_offsets = item_offsets
        self.status = status                  # (ndocs,) i32: 0, or 5 for a document whose values cannot be built (all of them empty)


def _match_values_of(v):
    """the MatchValues of a capi.SpMatchValues (copies)"""
    return _byte_families_of(MatchValues, v, ("result_values", "result_value_offsets"), ("item_values", "item_value_offsets"), "doc_value_status")


def batchValues(matcher, mb, text, seg_offsets, doc_seg_offsets=None, flags=SP_VALUE_RESULTS | SP_VALUE_ITEMS):
    """The values of the format strings of a batch already on the host (a MatchBatch of `matcher`, a PatternMatcherInstance,
    in document order with items without gaps: finishedFetch, batchFetch, matchDocs), by the rule of the device call
    (include/strus_pattern_amd.h "result values"), without a device.  The text source is that of batchText.  Returns a
    MatchValues."""
    L = capi.lib()
    b, keep = _host_batch(mb, items=True, formats="all")
    source, keep_text = _host_text(text, seg_offsets, doc_seg_offsets)      # (keep, keep_text: until the call has returned)
    err = ctypes.create_string_buffer(512)
    return _product(capi.SpMatchValues, lambda v: L.sp_match_batch_values(matcher._h, ctypes.byref(b), *source, flags, ctypes.byref(v), err, 512),
                    L.sp_match_values_free, _match_values_of, lambda rc: "no values of the batch (%d): %s" % (rc, err.value.decode(errors="replace")))


class PatternFreq:
    """The pattern frequencies of a finished batch (host copies): per document one record per distinct handle, ascending by
    handle, and per handle the sums over the batch (include/strus_pattern_amd.h "pattern frequencies")."""

    def __init__(self, records, doc_offsets, status, handle_results, handle_docs):
        self.records = records                # (n, 4) u32: handle, count, first_ordpos, last_ordend
        self.doc_offsets = doc_offsets        # (ndocs+1,) u64
        self.status = status                  # (ndocs,) i32: 0, or 5 for a document with a handle outside the bound (no records)
        self.handle_results = handle_results  # (handle_bound,) u64: results per handle over the batch (collection frequency)
        self.handle_docs = handle_docs        # (handle_bound,) u32: documents per handle (document frequency)

    def doc(self, i):
        return self.records[int(self.doc_offsets[i]):int(self.doc_offsets[i + 1])]


def _pattern_freq_of(b):
    """the PatternFreq of a capi.SpPatternFreqBatch (copies)"""
    return PatternFreq(_rows(b.records, b.nrecords, 4), _rows(b.doc_offsets, b.ndocs + 1, 0, ctypes.c_uint64),
                       _rows(b.doc_freq_status, b.ndocs, 0, ctypes.c_int32), _rows(b.handle_results, b.handle_bound, 0, ctypes.c_uint64),
                       _rows(b.handle_docs, b.handle_bound, 0))


def batchPatternFreq(mb, handle_bound):
    """The pattern frequencies of a batch already on the host (a MatchBatch in document order: finishedFetch, batchFetch,
    matchDocs), by the rule of the device call, without a device.  handle_bound: PatternMatcherInstance.handleBound().
    Returns a PatternFreq."""
    L = capi.lib()
    b, keep = _host_batch(mb, status=True)      # (keep: until the call has returned)
    err = ctypes.create_string_buffer(256)
    return _product(capi.SpPatternFreqBatch, lambda f: L.sp_match_batch_pattern_freq(ctypes.byref(b), handle_bound, ctypes.byref(f), err, 256),
                    L.sp_pattern_freq_batch_free, _pattern_freq_of, lambda rc: "no pattern frequencies of the batch (%d): %s" % (rc, err.value.decode()))


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

    def __init__(self, records, doc_offsets, result_term, status, flags=SP_TERM_VALUES | SP_TERM_TEXT, handle_bound=0):
        self.handle_bound = handle_bound    # the bound the terms were built with (0: not known; batchDictionary then needs it as an argument)
        self.records = records          # (n, 6) u32: handle, count, first_ordpos, last_ordend, first_result, value_bytes
        self.doc_offsets = doc_offsets  # (ndocs+1,) u64
        self.result_term = result_term  # (nresults,) u32, 0xFFFFFFFF throughout a failed document
        self.status = status            # (ndocs,) i32: 0, or 5 for a failed document (no records)
        self.flags = flags

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


def _match_terms_of(t):
    """the MatchTerms of a capi.SpMatchTerms (copies)"""
    return MatchTerms(_rows(t.records, t.nrecords, 6), _rows(t.doc_term_offsets, t.ndocs + 1, 0, ctypes.c_uint64),
                      _rows(t.result_term, t.nresults, 0), _rows(t.doc_term_status, t.ndocs, 0, ctypes.c_int32), t.flags, t.handle_bound)


def _host_sources(values, text, keep):
    """the C structs (capi.SpMatchValues, capi.SpMatchText) of a MatchValues / MatchText for a host twin, their results family
    only; either may be None.  What they point into is appended to `keep`."""
    def source(cls, family, names):
        if family is None:
            return None
        c = cls()
        c.ndocs, c.nresults = len(family.status), (len(family.result_offsets) - 1 if family.result_offsets is not None else 0)
        st = np.ascontiguousarray(family.status, dtype=np.int32)
        keep.append(st)
        setattr(c, names[2], ctypes.cast(st.ctypes.data, ctypes.POINTER(ctypes.c_int32)))
        if family.result_offsets is not None:
            data = bytes(getattr(family, names[3]))
            ro = np.ascontiguousarray(family.result_offsets, dtype=np.uint64)
            buf = ctypes.create_string_buffer(data, len(data) + 1)
            keep.extend([ro, buf])
            setattr(c, names[0], ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint8)))
            setattr(c, names[1], ctypes.cast(ro.ctypes.data, ctypes.POINTER(ctypes.c_uint64)))
            c.totals[0] = len(data)
        return c

    return (source(capi.SpMatchValues, values, ("result_values", "result_value_offsets", "doc_value_status", "result_values")),
            source(capi.SpMatchText, text, ("result_text", "result_text_offsets", "doc_text_status", "result_text")))


def batchTerms(mb, values=None, text=None, handle_bound=0, flags=SP_TERM_VALUES | SP_TERM_TEXT):
    """The index terms of a batch already on the host (a MatchBatch in document order: finishedFetch, batchFetch, matchDocs)
    with its MatchValues and / or MatchText (their results family), by the rule of the device call, without a device.
    handle_bound: PatternMatcherInstance.handleBound().  Returns a MatchTerms."""
    L = capi.lib()
    b, keep = _host_batch(mb, formats="results", status=True)       # (keep: until the call has returned)
    v, x = _host_sources(values, text, keep)
    err = ctypes.create_string_buffer(256)
    return _product(capi.SpMatchTerms, lambda t: L.sp_match_batch_terms(ctypes.byref(b), ctypes.byref(v) if v is not None else None,
                                                                       ctypes.byref(x) if x is not None else None, handle_bound, flags, ctypes.byref(t), err, 256),
                    L.sp_match_terms_free, _match_terms_of, lambda rc: "no terms of the batch (%d): %s" % (rc, err.value.decode()))


class MatchDictionary:
    """The dictionary of a terms batch (host copies): one entry per distinct pair (handle, value bytes) over all documents, in
    the order of first occurrence, and per term record the index of its entry (include/strus_pattern_amd.h "batch
    dictionary").  An entry owns no bytes: its value is that of term record first_term of document first_doc."""

    def __init__(self, records, term_dict, doc_offsets, handle_terms):
        self.records = records            # (ndict, 8) u32: handle, value_bytes, first_doc, first_term, doc_freq, max_count, count (low, high)
        self.counts = np.ascontiguousarray(records[:, 6:8]).view(np.uint64).reshape(-1)   # (ndict,) u64: the collection frequencies
        self.term_dict = term_dict        # (nterms,) u32, parallel to the term records
        self.doc_offsets = doc_offsets    # (ndocs+1,) u64: the entries first seen in every document
        self.handle_terms = handle_terms  # (handle_bound,) u32: distinct terms per handle

    def entries(self, mb, terms, values=None, text=None):
        """yields (handle, value bytes, doc_freq, count, max_count) per entry, in dictionary order; mb: the finished batch,
        terms: the MatchTerms the dictionary was built from, values / text: the MatchValues / MatchText of those"""
        for (h, size, d, t, df, mx, _, _), count in zip(self.records.tolist(), self.counts.tolist()):
            value = _term_value(terms.flags, mb, values, text, int(mb.doc_offsets[d]) + int(terms.doc(d)[t][4]))
            assert len(value) == size
            yield h, value, df, count, mx


def _match_dictionary_of(d):
    """the MatchDictionary of a capi.SpMatchDictionary (copies)"""
    return MatchDictionary(_rows(d.records, d.ndict, 8), _rows(d.term_dict, d.nterms, 0), _rows(d.doc_dict_offsets, d.ndocs + 1, 0, ctypes.c_uint64),
                           _rows(d.handle_terms, d.handle_bound, 0))


def batchDictionary(mb, terms, values=None, text=None, handle_bound=0):
    """The dictionary of the terms of a batch already on the host (terms: the MatchTerms of finishedTermsFetch or batchTerms,
    mb, values, text: what they were built from), by the rule of the device call, without a device.  The handle bound, which
    is the length of handle_terms, is that of `terms`; a MatchTerms made by hand without one needs `handle_bound`
    (PatternMatcherInstance.handleBound()): it is not guessed from the records.  Returns a MatchDictionary."""
    bound = handle_bound or terms.handle_bound
    if not bound:
        raise PatternError("no dictionary of the batch: the terms carry no handle bound and none was given")
    L = capi.lib()
    b, keep = _host_batch(mb, formats="results", status=True)       # (keep: until the call has returned)
    v, x = _host_sources(values, text, keep)
    t = _host_terms(terms, bound, keep)
    err = ctypes.create_string_buffer(256)
    return _product(capi.SpMatchDictionary, lambda d: L.sp_match_batch_dictionary(ctypes.byref(b), ctypes.byref(v) if v is not None else None,
                                                                                 ctypes.byref(x) if x is not None else None, ctypes.byref(t), ctypes.byref(d), err, 256),
                    L.sp_match_dictionary_free, _match_dictionary_of, lambda rc: "no dictionary of the batch (%d): %s" % (rc, err.value.decode()))


def _host_terms(terms, bound, keep):
    """the capi.SpMatchTerms of a MatchTerms for a host twin; the arrays it points into are appended to `keep`"""
    t = capi.SpMatchTerms()
    rec = np.ascontiguousarray(terms.records, dtype=np.uint32).reshape(-1, 6)
    offs = np.ascontiguousarray(terms.doc_offsets, dtype=np.uint64)
    rt = np.ascontiguousarray(terms.result_term, dtype=np.uint32)
    st = np.ascontiguousarray(terms.status, dtype=np.int32)
    keep.extend([rec, offs, rt, st])
    t.ndocs, t.nresults, t.nrecords, t.flags = len(offs) - 1, len(rt), len(rec), terms.flags
    t.handle_bound = bound
    t.records = ctypes.cast(rec.ctypes.data, ctypes.POINTER(capi.SpMatchTerm))
    t.doc_term_offsets = ctypes.cast(offs.ctypes.data, ctypes.POINTER(ctypes.c_uint64))
    t.result_term = ctypes.cast(rt.ctypes.data, ctypes.POINTER(ctypes.c_uint32))
    t.doc_term_status = ctypes.cast(st.ctypes.data, ctypes.POINTER(ctypes.c_int32))
    t.totals[0] = len(rec)
    return t


class MatchPostings:
    """The postings of a dictionary (host copies): per term record one posting (doc, term, count, first_ordpos), the postings
    of dictionary entry e together and ascending by document, and per term record the index of its posting
    (include/strus_pattern_amd.h "batch postings")."""

    def __init__(self, records, entry_offsets, record_posting):
        self.records = records                # (nterms, 4) u32: doc, term, count, first_ordpos
        self.entry_offsets = entry_offsets    # (ndict+1,) u64: the postings of entry e are records[entry_offsets[e]:entry_offsets[e+1]]
        self.record_posting = record_posting  # (nterms,) u32, parallel to the term records

    def entry(self, e):
        """the postings of dictionary entry e, in document order: rows (doc, term, count, first_ordpos)"""
        return self.records[int(self.entry_offsets[e]):int(self.entry_offsets[e + 1])]

    def docs(self, e):
        """the documents that hold dictionary entry e, ascending"""
        return self.entry(e)[:, 0]


def _match_postings_of(p):
    """the MatchPostings of a capi.SpMatchPostings (copies)"""
    return MatchPostings(_rows(p.postings, p.nterms, 4), _rows(p.entry_offsets, p.ndict + 1, 0, ctypes.c_uint64), _rows(p.record_posting, p.nterms, 0))


def batchPostings(terms, dictionary):
    """The postings of a dictionary already on the host (terms: the MatchTerms, dictionary: the MatchDictionary built from
    them: the fetches of a context, or batchTerms and batchDictionary), by the rule of the device call, without a device.
    Returns a MatchPostings."""
    L = capi.lib()
    keep = []                                                        # (until the call has returned)
    t = _host_terms(terms, terms.handle_bound, keep)
    d = capi.SpMatchDictionary()
    rec = np.ascontiguousarray(dictionary.records, dtype=np.uint32).reshape(-1, 8)
    td = np.ascontiguousarray(dictionary.term_dict, dtype=np.uint32)
    offs = np.ascontiguousarray(dictionary.doc_offsets, dtype=np.uint64)
    ht = np.ascontiguousarray(dictionary.handle_terms, dtype=np.uint32)
    keep.extend([rec, td, offs, ht])
    d.ndocs, d.nterms, d.ndict, d.handle_bound, d.flags = len(offs) - 1, len(td), len(rec), len(ht), terms.flags
    d.records = ctypes.cast(rec.ctypes.data, ctypes.POINTER(capi.SpDictTerm))
    d.term_dict = ctypes.cast(td.ctypes.data, ctypes.POINTER(ctypes.c_uint32))
    d.doc_dict_offsets = ctypes.cast(offs.ctypes.data, ctypes.POINTER(ctypes.c_uint64))
    d.handle_terms = ctypes.cast(ht.ctypes.data, ctypes.POINTER(ctypes.c_uint32))
    d.totals[0] = len(rec)
    err = ctypes.create_string_buffer(256)
    return _product(capi.SpMatchPostings, lambda p: L.sp_match_batch_postings(ctypes.byref(t), ctypes.byref(d), ctypes.byref(p), err, 256),
                    L.sp_match_postings_free, _match_postings_of, lambda rc: "no postings of the batch (%d): %s" % (rc, err.value.decode()))


def _host_postings(postings, ndocs, keep):
    """the capi.SpMatchPostings of a MatchPostings for a host twin; the arrays it points into are appended to `keep`"""
    p = capi.SpMatchPostings()
    rec = np.ascontiguousarray(postings.records, dtype=np.uint32).reshape(-1, 4)
    offs = np.ascontiguousarray(postings.entry_offsets, dtype=np.uint64)
    rp = np.ascontiguousarray(postings.record_posting, dtype=np.uint32)
    keep.extend([rec, offs, rp])
    p.ndocs, p.nterms, p.ndict = ndocs, len(rec), len(offs) - 1
    p.postings = ctypes.cast(rec.ctypes.data, ctypes.POINTER(capi.SpPosting))
    p.entry_offsets = ctypes.cast(offs.ctypes.data, ctypes.POINTER(ctypes.c_uint64))
    p.record_posting = ctypes.cast(rp.ctypes.data, ctypes.POINTER(ctypes.c_uint32))
    p.totals[0] = len(rec)
    return p


class MatchPositions:
    """The positions of the postings of a batch (host copies): per participating result one occurrence (ordpos, result), the
    occurrences of posting p together, ascending by ordpos and then by result, and per posting the number of distinct
    positions (include/strus_pattern_amd.h "posting positions")."""

    def __init__(self, occurrences, posting_offsets, posting_positions, totals):
        self.occurrences = occurrences              # (nocc, 2) u32: ordpos, result (index inside the document's finished block)
        self.posting_offsets = posting_offsets      # (nterms+1,) u64: the occurrences of posting p are occurrences[posting_offsets[p]:posting_offsets[p+1]]
        self.posting_positions = posting_positions  # (nterms,) u32: distinct ordpos per posting
        self.totals = totals                        # (2,) u64: nocc, the sum of posting_positions

    def posting(self, p):
        """the occurrences of posting p, by position: rows (ordpos, result)"""
        return self.occurrences[int(self.posting_offsets[p]):int(self.posting_offsets[p + 1])]

    def positions(self, p):
        """the distinct ordinal positions of posting p, ascending: what an index stores"""
        pos = self.posting(p)[:, 0]
        return pos[np.concatenate(([True], pos[1:] != pos[:-1]))] if len(pos) else pos


def _match_positions_of(p):
    """the MatchPositions of a capi.SpMatchPositions (copies)"""
    return MatchPositions(_rows(p.occurrences, p.nocc, 2), _rows(p.posting_offsets, p.nterms + 1, 0, ctypes.c_uint64),
                          _rows(p.posting_positions, p.nterms, 0), np.array([p.totals[0], p.totals[1]], np.uint64))


def batchPositions(mb, terms, postings):
    """The positions of the postings of a batch already on the host (mb: the finished MatchBatch, terms: its MatchTerms,
    postings: the MatchPostings built from their dictionary: the fetches of a context, or the twins), by the rule of the device
    call, without a device.  Returns a MatchPositions."""
    L = capi.lib()
    b, keep = _host_batch(mb)                                        # (keep: until the call has returned)
    t = _host_terms(terms, terms.handle_bound, keep)
    q = _host_postings(postings, len(terms.doc_offsets) - 1, keep)
    err = ctypes.create_string_buffer(256)
    return _product(capi.SpMatchPositions, lambda p: L.sp_match_batch_positions(ctypes.byref(b), ctypes.byref(t), ctypes.byref(q), ctypes.byref(p), err, 256),
                    L.sp_match_positions_free, _match_positions_of, lambda rc: "no positions of the batch (%d): %s" % (rc, err.value.decode()))


class PatternMatcherContext:
    """PatternMatcherContextInterface (src/patternMatcher.cpp:107-341) + batch mode."""

    def __init__(self, instance, device=0, result_sets=False):
        self._L = capi.lib()
        self._inst = instance  # keeps the instance alive: a context borrows its tables
        self._h = self._L.sp_matcher_ctx_create_ex(instance._h, device, SP_CTX_RESULT_SETS if result_sets else 0)
        if not self._h:
            raise PatternError("failed to create pattern match context: " + self._L.sp_matcher_last_error(instance._h).decode())

    def __del__(self):
        try:
            if self._h:
                self._L.sp_matcher_ctx_free(self._h)
        except Exception:
            pass

    def _err(self):
        return self._L.sp_matcher_ctx_last_error(self._h).decode()

    def setArena(self, max_rules=0, max_triggers=0, bucket_capacity=0, max_items=0, max_follow=0):
        self._L.sp_matcher_ctx_set_arena(self._h, max_rules, max_triggers, bucket_capacity, max_items, max_follow)

    # -- single document mode
    def putInput(self, lexem_id, ordpos, origpos, origsize, origseg=0):
        lx = SpLexem(lexem_id, ordpos, origpos, origsize)
        seg = ctypes.c_uint32(origseg)
        rc = self._L.sp_matcher_ctx_put_input(self._h, ctypes.addressof(lx), ctypes.addressof(seg) if origseg else None, 1)
        if rc != 0:
            raise PatternError("failed to feed input to pattern matcher: " + self._err())

    def fetchResults(self):
        res = ctypes.POINTER(SpResult)()
        items = ctypes.POINTER(SpResultItem)()
        nres = ctypes.c_size_t()
        nitems = ctypes.c_size_t()
        rc = self._L.sp_matcher_ctx_fetch_results(self._h, ctypes.byref(res), ctypes.byref(nres), ctypes.byref(items), ctypes.byref(nitems))
        if rc != 0:
            raise PatternError("failed to fetch pattern match result: " + self._err())
        try:
            r, it = _rows(res, nres.value, 9), _rows(items, nitems.value, 7)
        finally:
            self._L.sp_free(res)
            self._L.sp_free(items)
        return r, it

    def fetchFormats(self, nresults, nitems):
        """format handles of the results / items of the last fetchResults() (None, None without format strings)."""
        rf = ctypes.POINTER(ctypes.c_uint32)()
        itf = ctypes.POINTER(ctypes.c_uint32)()
        self._L.sp_matcher_ctx_fetch_formats(self._h, ctypes.byref(rf), ctypes.byref(itf))
        if not rf and not self._inst.formatCount():
            return None, None
        return _rows(rf, nresults, 0), _rows(itf, nitems, 2)

    def getStatistics(self):
        """the statistics of the last fetch; None in result-set mode on the join kernel, which installs nothing"""
        st = capi.SpMatcherStats()
        if self._L.sp_matcher_ctx_statistics(self._h, ctypes.byref(st)) == SP_ERR_UNAVAILABLE:
            return None
        return {n: getattr(st, n) for n, _ in capi.SpMatcherStats._fields_}

    def reset(self):
        self._L.sp_matcher_ctx_reset(self._h)

    # -- batch mode (host buffers)
    def matchDocs(self, lexems, doc_offsets, origseg=None, check=True):
        """lexems: (n,4) u32 [id, ordpos, origpos, origsize]; doc_offsets: (ndocs+1,) u64."""
        lexems = np.ascontiguousarray(lexems, dtype=np.uint32).reshape(-1, 4)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        ndocs = len(doc_offsets) - 1
        segp = None
        if origseg is not None:
            origseg = np.ascontiguousarray(origseg, dtype=np.uint32)
            segp = origseg.ctypes.data
        b = capi.SpMatchBatch()
        rc = self._L.sp_matcher_ctx_match_docs(self._h, lexems.ctypes.data, segp, doc_offsets.ctypes.data, ndocs, ctypes.byref(b))
        try:
            if rc != 0 and (rc != -5 or check):
                raise PatternError("batch match failed (%d): %s" % (rc, self._err()))
            return _match_batch_of(b)
        finally:
            self._L.sp_match_batch_free(ctypes.byref(b))

    # -- batch mode (device-resident buffers; pointers are raw device addresses, e.g. torch data_ptr())
    def matchDocsDevice(self, d_lexems, d_doc_offsets, ndocs, nlexems, stream=0, d_origseg=0):
        out = capi.SpMatchDeviceBatch()
        rc = self._L.sp_matcher_ctx_match_docs_device(self._h, d_lexems, d_origseg or None, d_doc_offsets, ndocs, nlexems, stream or None, ctypes.byref(out))
        if rc != 0:
            raise PatternError("device batch match failed (%d): %s" % (rc, self._err()))
        return out

    def matchLexedDevice(self, d_lexems, d_doc_ranges, ndocs, nlexems_hint, stream=0):
        """consume the device output of PatternLexerContext.matchDocsDevice in place (fused pipeline)."""
        out = capi.SpMatchDeviceBatch()
        rc = self._L.sp_matcher_ctx_match_lexed_device(self._h, d_lexems, d_doc_ranges, ndocs, nlexems_hint, stream or None, ctypes.byref(out))
        if rc != 0:
            raise PatternError("device batch match failed (%d): %s" % (rc, self._err()))
        return out

    def batchFinishDevice(self, stream=0, canonical=False):
        """finish the last batch on the device (asynchronous on `stream`): document order, `exclusive` applied, failed
        documents empty, items without gaps; returns the device pointers (capi.SpMatchFinishedBatch).  canonical: the
        results of a document in the order of SP_FINISH_CANONICAL, the same bytes from every engine."""
        out = capi.SpMatchFinishedBatch()
        rc = self._L.sp_matcher_ctx_batch_finish_device_ex(self._h, stream or None, SP_FINISH_CANONICAL if canonical else 0, ctypes.byref(out))
        if rc != 0:
            raise PatternError("finishing the batch on the device failed (%d): %s" % (rc, self._err()))
        return out

    def finishedFetch(self):
        """plain host copy of the batch finished by batchFinishDevice: what batchFetch() returns, with no work on the host."""
        return self._fetched(self._L.sp_matcher_ctx_finished_fetch)

    def _fetch_product(self, struct_type, call, free, convert, what):
        """host copy of a product of the last batch: call(handle, ..., struct pointer) fills what `free` frees, `convert` copies"""
        return _product(struct_type, lambda s: call(self._h, ctypes.byref(s)), free, convert,
                        lambda rc: "fetching %s failed (%d): %s" % (what, rc, self._err()))

    def _last_ms(self, fn, what):
        """the one duration a timing call reports, in milliseconds"""
        a = ctypes.c_double(-1.0)
        if fn(self._h, ctypes.byref(a)) != 0:
            raise PatternError("no timed " + what)
        return a.value

    def lastFinishMs(self):
        """(count, offsets, place) pass durations of the last batchFinishDevice in milliseconds"""
        a, b, d = ctypes.c_double(-1.0), ctypes.c_double(-1.0), ctypes.c_double(-1.0)
        if self._L.sp_matcher_ctx_last_finish_ms(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(d)) != 0:
            raise PatternError("no timed finish")
        return a.value, b.value, d.value

    def lastFinishSortMs(self):
        """duration of the sorting pass of the last batchFinishDevice in milliseconds (0.0 without canonical=True)"""
        return self._last_ms(self._L.sp_matcher_ctx_last_finish_sort_ms, "finish")

    def finishedTextDevice(self, d_text, nbytes, d_seg_offsets, nseg, d_doc_seg_offsets=0, results=True, items=True, stream=0):
        """gather the text that the results and / or items of the batch finished by batchFinishDevice cover, on the device
        (the placement is asynchronous on `stream`): d_text is the text the lexer batch ran on, d_seg_offsets the nseg+1
        offsets given to the lexer, d_doc_seg_offsets the ndocs+1 offsets given to the stitch (0: document d is segment d).
        Returns the device pointers (capi.SpMatchTextBatch), valid until the next call."""
        src = capi.SpTextSource(d_text or None, nbytes, d_seg_offsets or None, nseg, d_doc_seg_offsets or None)
        out = capi.SpMatchTextBatch()
        flags = (SP_TEXT_RESULTS if results else 0) | (SP_TEXT_ITEMS if items else 0)
        rc = self._L.sp_matcher_ctx_finished_text_device(self._h, ctypes.byref(src), flags, stream or None, ctypes.byref(out))
        if rc != 0:
            raise PatternError("gathering the text of the batch on the device failed (%d): %s" % (rc, self._err()))
        return out

    def finishedTextFetch(self):
        """plain host copy of the text gathered by finishedTextDevice: a MatchText"""
        return self._fetch_product(capi.SpMatchText, self._L.sp_matcher_ctx_finished_text_fetch, self._L.sp_match_text_free, _match_text_of, "the text of the batch")

    def lastTextMs(self):
        """duration of the passes of the last finishedTextDevice in milliseconds"""
        return self._last_ms(self._L.sp_matcher_ctx_last_text_ms, "text call")

    def finishedValuesDevice(self, d_text, nbytes, d_seg_offsets, nseg, d_doc_seg_offsets=0, flags=SP_VALUE_RESULTS | SP_VALUE_ITEMS, stream=0):
        """build the values of the format strings of the results and / or items of the batch finished by batchFinishDevice,
        on the device (the placement is asynchronous on `stream`); the text source is that of finishedTextDevice.
        Returns the device pointers (capi.SpMatchValuesBatch), valid until the next call."""
        src = capi.SpTextSource(d_text or None, nbytes, d_seg_offsets or None, nseg, d_doc_seg_offsets or None)
        out = capi.SpMatchValuesBatch()
        rc = self._L.sp_matcher_ctx_finished_values_device(self._h, ctypes.byref(src), flags, stream or None, ctypes.byref(out))
        if rc != 0:
            raise PatternError("building the values of the batch on the device failed (%d): %s" % (rc, self._err()))
        return out

    def finishedValuesFetch(self):
        """plain host copy of the values built by finishedValuesDevice: a MatchValues"""
        return self._fetch_product(capi.SpMatchValues, self._L.sp_matcher_ctx_finished_values_fetch, self._L.sp_match_values_free, _match_values_of, "the values of the batch")

    def lastValuesMs(self):
        """duration of the passes of the last finishedValuesDevice in milliseconds"""
        return self._last_ms(self._L.sp_matcher_ctx_last_values_ms, "values call")

    def finishedPatternFreqDevice(self, stream=0):
        """sum the pattern frequencies of the batch finished by batchFinishDevice on the device (the placement is
        asynchronous on `stream`): per document one record per distinct handle, per handle the sums over the batch.
        Returns the device pointers (capi.SpPatternFreqDevice), valid until the next call."""
        out = capi.SpPatternFreqDevice()
        rc = self._L.sp_matcher_ctx_finished_pattern_freq_device(self._h, stream or None, ctypes.byref(out))
        if rc != 0:
            raise PatternError("summing the pattern frequencies of the batch on the device failed (%d): %s" % (rc, self._err()))
        return out

    def finishedPatternFreqFetch(self):
        """plain host copy of the frequencies summed by finishedPatternFreqDevice: a PatternFreq"""
        return self._fetch_product(capi.SpPatternFreqBatch, self._L.sp_matcher_ctx_finished_pattern_freq_fetch, self._L.sp_pattern_freq_batch_free, _pattern_freq_of,
                                   "the pattern frequencies of the batch")

    def lastPatternFreqMs(self):
        """duration of the passes of the last finishedPatternFreqDevice in milliseconds"""
        return self._last_ms(self._L.sp_matcher_ctx_last_pattern_freq_ms, "pattern frequency call")

    def finishedTermsDevice(self, flags=SP_TERM_VALUES | SP_TERM_TEXT, stream=0):
        """group the results of the batch finished by batchFinishDevice into index terms on the device (the placement is
        asynchronous on `stream`): per document one record per distinct (handle, value), per result the index of its term.
        flags: SP_TERM_VALUES (finishedValuesDevice has run since the finish, with the results family), SP_TERM_TEXT
        (finishedTextDevice has, with results=True), or both.  Returns the device pointers (capi.SpMatchTermsDevice), valid
        until the next call."""
        out = capi.SpMatchTermsDevice()
        rc = self._L.sp_matcher_ctx_finished_terms_device(self._h, flags, stream or None, ctypes.byref(out))
        if rc != 0:
            raise PatternError("grouping the terms of the batch on the device failed (%d): %s" % (rc, self._err()))
        return out

    def finishedTermsFetch(self):
        """plain host copy of the terms grouped by finishedTermsDevice: a MatchTerms"""
        return self._fetch_product(capi.SpMatchTerms, self._L.sp_matcher_ctx_finished_terms_fetch, self._L.sp_match_terms_free, _match_terms_of, "the terms of the batch")

    def lastTermsMs(self):
        """duration of the passes of the last finishedTermsDevice in milliseconds"""
        return self._last_ms(self._L.sp_matcher_ctx_last_terms_ms, "terms call")

    def finishedDictionaryDevice(self, stream=0):
        """build the dictionary of the terms grouped by finishedTermsDevice on the device (the placement is asynchronous on
        `stream`): every distinct (handle, value) of the batch once, in the order of first occurrence, with its document
        and collection frequency, and per term record the index of its entry.  Returns the device pointers
        (capi.SpMatchDictionaryDevice), valid until the next call."""
        out = capi.SpMatchDictionaryDevice()
        rc = self._L.sp_matcher_ctx_finished_dictionary_device(self._h, stream or None, ctypes.byref(out))
        if rc != 0:
            raise PatternError("building the dictionary of the batch on the device failed (%d): %s" % (rc, self._err()))
        return out

    def finishedDictionaryFetch(self):
        """plain host copy of the dictionary built by finishedDictionaryDevice: a MatchDictionary"""
        return self._fetch_product(capi.SpMatchDictionary, self._L.sp_matcher_ctx_finished_dictionary_fetch, self._L.sp_match_dictionary_free,
                                   _match_dictionary_of, "the dictionary of the batch")

    def lastDictionaryMs(self):
        """duration of the launches of the last finishedDictionaryDevice in milliseconds"""
        return self._last_ms(self._L.sp_matcher_ctx_last_dictionary_ms, "dictionary call")

    def finishedPostingsDevice(self, stream=0):
        """build the postings of the dictionary built by finishedDictionaryDevice on the device (everything is asynchronous
        on `stream`: the call waits for nothing): per dictionary entry the list of (doc, term, count, first_ordpos) in
        document order, and per term record the index of its posting.  Returns the device pointers
        (capi.SpMatchPostingsDevice), valid until the next call."""
        out = capi.SpMatchPostingsDevice()
        rc = self._L.sp_matcher_ctx_finished_postings_device(self._h, stream or None, ctypes.byref(out))
        if rc != 0:
            raise PatternError("building the postings of the batch on the device failed (%d): %s" % (rc, self._err()))
        return out

    def finishedPostingsFetch(self):
        """plain host copy of the postings built by finishedPostingsDevice: a MatchPostings"""
        return self._fetch_product(capi.SpMatchPostings, self._L.sp_matcher_ctx_finished_postings_fetch, self._L.sp_match_postings_free,
                                   _match_postings_of, "the postings of the batch")

    def lastPostingsMs(self):
        """duration of the launches of the last finishedPostingsDevice in milliseconds"""
        return self._last_ms(self._L.sp_matcher_ctx_last_postings_ms, "postings call")

    def finishedPositionsDevice(self, stream=0):
        """build the positions of the postings built by finishedPostingsDevice on the device (the call waits once, for the
        number of occurrences and the largest position, which set its passes; the placement is asynchronous on `stream`; a stream
        other than the postings' is ordered behind them).  Returns the device pointers (capi.SpMatchPositionsDevice), valid until
        the next call."""
        out = capi.SpMatchPositionsDevice()
        rc = self._L.sp_matcher_ctx_finished_positions_device(self._h, stream or None, ctypes.byref(out))
        if rc != 0:
            raise PatternError("building the positions of the batch on the device failed (%d): %s" % (rc, self._err()))
        return out

    def finishedPositionsFetch(self):
        """plain host copy of the positions built by finishedPositionsDevice: a MatchPositions"""
        return self._fetch_product(capi.SpMatchPositions, self._L.sp_matcher_ctx_finished_positions_fetch, self._L.sp_match_positions_free,
                                   _match_positions_of, "the positions of the batch")

    def lastPositionsMs(self):
        """duration of the launches of the last finishedPositionsDevice in milliseconds (the host's one wait lies inside)"""
        return self._last_ms(self._L.sp_matcher_ctx_last_positions_ms, "positions call")

    def lastPositionsLaunchMs(self):
        """diagnostics: the launches of the last finishedPositionsDevice summed by kind in milliseconds, a dict (keys, histogram,
        scan, scatter, rekey, place); needs capi.lib().sp_test_positions_launch_events(1) before that call"""
        a = (ctypes.c_double * 6)()
        if self._L.sp_matcher_ctx_last_positions_launch_ms(self._h, a) != 0:
            raise PatternError("no positions call with launch events")
        return dict(zip(("keys", "histogram", "scan", "scatter", "rekey", "place"), list(a)))

    def batchFetch(self, first_doc=None, ndocs=None):
        """host copy of the last device batch, grouped by document; with (first_doc, ndocs) only of
        that range of documents."""
        if first_doc is None:
            return self._fetched(self._L.sp_matcher_ctx_batch_fetch)
        return self._fetched(lambda h, b: self._L.sp_matcher_ctx_batch_fetch_docs(h, first_doc, ndocs, b))

    def _fetched(self, call):
        return self._fetch_product(capi.SpMatchBatch, call, self._L.sp_match_batch_free, _match_batch_of, "the batch")

    def batchCounters(self):
        arr = (ctypes.c_uint64 * 8)()
        rc = self._L.sp_matcher_ctx_batch_counters(self._h, arr)
        if rc != 0:
            raise PatternError("reading batch counters failed: " + self._err())
        return {"results": arr[0], "items": arr[1], "events": arr[2], "failed_docs": arr[3], "handed_over": arr[4], "prof": [arr[4], arr[5], arr[6], arr[7]]}

    def batchStatus(self, ndocs):
        st = np.zeros(ndocs, np.int32)
        rc = self._L.sp_matcher_ctx_batch_status(self._h, st.ctypes.data, ndocs)
        if rc != 0:
            raise PatternError("reading batch status failed: " + self._err())
        return st

    def growArena(self):
        return self._L.sp_matcher_ctx_grow_arena(self._h) == 0

    def reserveOutput(self, results, items):
        self._L.sp_matcher_ctx_reserve_output(self._h, results, items)

    def lastKernelMs(self):
        return self._L.sp_matcher_ctx_last_kernel_ms(self._h)

    def kernelKind(self):
        """0 general automaton kernel, 1 LDS-resident kernel (flat rule sets), 2 join kernel (result-set mode)"""
        return self._L.sp_matcher_ctx_kernel_kind(self._h)

    def kernelName(self):
        """name of the kernel that does the work of this context's batches (what rocprofv3 lists)"""
        return self._L.sp_matcher_ctx_kernel_name(self._h).decode()


def _serialize(L, fn, handle, err):
    blob = ctypes.c_void_p()
    size = ctypes.c_size_t()
    if fn(handle, ctypes.byref(blob), ctypes.byref(size)) != 0:
        raise PatternError("serialisation failed: " + err())
    try:
        return ctypes.string_at(blob, size.value)
    finally:
        L.sp_free(blob)


class PatternMatcherInstance:
    """PatternMatcherInstanceInterface (src/patternMatcher.cpp:345-733)."""

    def __init__(self, _handle=None):
        self._L = capi.lib()
        self._h = _handle or self._L.sp_matcher_create()
        if not self._h:
            raise PatternError("failed to create pattern matcher instance")

    def serialize(self):
        """the rule set (tables, names, format strings, options) as bytes: SURVEY.md 8(f).4"""
        return _serialize(self._L, self._L.sp_matcher_serialize, self._h, lambda: self._L.sp_matcher_last_error(self._h).decode())

    @classmethod
    def deserialize(cls, blob):
        L = capi.lib()
        err = ctypes.create_string_buffer(256)
        h = L.sp_matcher_deserialize(blob, len(blob), err, 256)
        if not h:
            raise PatternError("cannot load the rule set: " + err.value.decode())
        return cls(_handle=h)

    def __del__(self):
        try:
            if self._h:
                self._L.sp_matcher_free(self._h)
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise PatternError("%s: %s" % (what, self._L.sp_matcher_last_error(self._h).decode()))

    def defineTermFrequency(self, termid, df):
        self._chk(self._L.sp_matcher_define_term_frequency(self._h, termid, df), "failed to define term frequency")

    def pushTerm(self, termid):
        self._chk(self._L.sp_matcher_push_term(self._h, termid), "failed to push term on the pattern match expression stack")

    def pushExpression(self, joinop, argc, range_, cardinality=0):
        op = JOIN_OP[joinop] if isinstance(joinop, str) else int(joinop)
        self._chk(self._L.sp_matcher_push_expression(self._h, op, argc, range_, cardinality), "failed to push expression on the pattern match expression stack")

    def pushPattern(self, name):
        self._chk(self._L.sp_matcher_push_pattern(self._h, name.encode()), "failed to push pattern reference on the pattern match expression stack")

    def attachVariable(self, name):
        self._chk(self._L.sp_matcher_attach_variable(self._h, name.encode()), "failed to attach variable to top element of the pattern match expression stack")

    def definePattern(self, name, formatstring="", visible=True):
        self._chk(self._L.sp_matcher_define_pattern(self._h, name.encode(), formatstring.encode(), int(visible)), "failed to close pattern definition on the pattern match expression stack")

    def defineOption(self, name, value=0.0):
        self._chk(self._L.sp_matcher_define_option(self._h, name.encode(), value), "failed to define pattern matching automaton option")

    def compile(self):
        self._chk(self._L.sp_matcher_compile(self._h), "failed to compile (optimize) pattern matching automaton")
        return True

    def createContext(self, device=0, result_sets=False):
        """result_sets=True: the context returns per document the right multiset of results and items, not their order
        inside the document and no statistics (getStatistics() is None) -- on the join kernel when resultSetTier() says
        the rule set is eligible, else on the exact engine (include/strus_pattern_amd.h, SP_CTX_RESULT_SETS)."""
        return PatternMatcherContext(self, device, result_sets)

    def handleBound(self):
        """one more than the number of pattern names: every result handle lies in [1, handleBound())"""
        return self._L.sp_matcher_handle_bound(self._h)

    def patternId(self, name):
        return self._L.sp_matcher_pattern_id(self._h, name.encode())

    def patternName(self, handle):
        s = self._L.sp_matcher_pattern_name(self._h, handle)
        return s.decode() if s else None

    def variableId(self, name):
        return self._L.sp_matcher_variable_id(self._h, name.encode())

    def variableName(self, vid):
        s = self._L.sp_matcher_variable_name(self._h, vid)
        return s.decode() if s else None

    def formatCount(self):
        return int(self._L.sp_matcher_format_count(self._h))

    def formatString(self, handle):
        s = self._L.sp_matcher_format_string(self._h, handle)
        return s.decode() if s else None

    def fastTier(self):
        """(True, "") when the rule set is flat and runs on the LDS-resident kernel, else (False, reason)."""
        buf = ctypes.create_string_buffer(256)
        ok = self._L.sp_matcher_fast_tier(self._h, buf, 256)
        return bool(ok), buf.value.decode()

    def resultSetTier(self):
        """(True, "", alt-keyed programs) when a result-set context runs this rule set on the join kernel, else
        (False, reason, 0): the reason why it stays on the exact engine."""
        buf = ctypes.create_string_buffer(256)
        alt = ctypes.c_uint32(0)
        ok = self._L.sp_matcher_result_set_tier(self._h, buf, 256, ctypes.byref(alt))
        return bool(ok), buf.value.decode(), int(alt.value)

    def launchPlan(self, num_cus, ndocs, nlexems, result_sets=False, fast_blocks_per_cu=16, rerun_docs=0, arena_grows=0, min_results=0, min_items=0):
        """what a context created now (createContext(result_sets=...)) on a device of num_cus compute units launches for a batch of
        ndocs documents and nlexems lexems, as a dict of strings (include/strus_pattern_amd.h, sp_matcher_launch_plan); needs no device"""
        buf = ctypes.create_string_buffer(2048)
        self._chk(self._L.sp_matcher_launch_plan(self._h, 1 if result_sets else 0, num_cus, fast_blocks_per_cu, ndocs, nlexems, rerun_docs, arena_grows,
                                                 min_results, min_items, buf, 2048), "no launch plan")
        return dict(f.split("=", 1) for f in buf.value.decode().split("\n") if f)

    def dumpTable(self):
        p = ctypes.POINTER(ctypes.c_uint32)()
        n = self._L.sp_matcher_dump_table(self._h, ctypes.byref(p))
        arr = np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
        self._L.sp_free(p)
        return arr

    def name(self):
        return "std"


class PatternMatcher:
    """PatternMatcherInterface (src/patternMatcher.hpp:31-35)."""

    def getCompileOptionNames(self):
        return ["stopwordOccurrenceFactor", "weightFactor", "maxRange", "exclusive", "maxResultSize"]  # src/patternMatcher.cpp:707-716

    def createInstance(self):
        return PatternMatcherInstance()

    def name(self):
        return "std"


POSITION_BIND = {"content": 0, "successor": 1, "predecessor": 2, "unique": 3}


class LexBatch:
    def __init__(self, lexems, doc_offsets, status):
        self.lexems = lexems            # (n,4) u32: id, ordpos, origpos, origsize
        self.doc_offsets = doc_offsets  # (ndocs+1,) u64
        self.status = status            # (ndocs,) i32

    def doc(self, i):
        return self.lexems[self.doc_offsets[i]:self.doc_offsets[i + 1]]


def _lex_batch_of(b):
    """the LexBatch of a capi.SpLexBatch (copies)"""
    return LexBatch(_rows(b.lexems, b.nlexems, 4), _rows(b.doc_lexem_offsets, b.ndocs + 1, 0, ctypes.c_uint64), _rows(b.doc_status, b.ndocs, 0, ctypes.c_int32))


class PatternLexerContext:
    """PatternLexerContextInterface (src/patternLexer.cpp:681-959) + batch mode."""

    def __init__(self, instance, device=0):
        self._L = capi.lib()
        self._inst = instance
        self._h = self._L.sp_lexer_ctx_create(instance._h, device)
        if not self._h:
            raise PatternError("failed to create term match context: " + self._L.sp_lexer_last_error(instance._h).decode())

    def __del__(self):
        try:
            if self._h:
                self._L.sp_lexer_ctx_free(self._h)
        except Exception:
            pass

    def _err(self):
        return self._L.sp_lexer_ctx_last_error(self._h).decode(errors="replace")

    def match(self, src):
        """std::vector<PatternLexem> match(const char* src, size_t len) (:858)."""
        buf = bytes(src)
        lex = ctypes.POINTER(SpLexem)()
        n = ctypes.c_size_t()
        rc = self._L.sp_lexer_ctx_match(self._h, buf, len(buf), ctypes.byref(lex), ctypes.byref(n))
        if rc != 0:
            raise PatternError("failed to run pattern matching terms with regular expressions: " + self._err())
        try:
            return _rows(lex, n.value, 4)
        finally:
            self._L.sp_free(lex)

    def reset(self):
        self._L.sp_lexer_ctx_reset(self._h)

    def matchDocs(self, text, doc_offsets, check=True):
        buf = bytes(text)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        ndocs = len(doc_offsets) - 1
        b = capi.SpLexBatch()
        rc = self._L.sp_lexer_ctx_match_docs(self._h, buf, doc_offsets.ctypes.data, ndocs, ctypes.byref(b))
        try:
            if rc != 0 and (rc != -5 or check):
                raise PatternError("batch lexer run failed (%d): %s" % (rc, self._err()))
            return _lex_batch_of(b)
        finally:
            self._L.sp_lex_batch_free(ctypes.byref(b))

    def matchDocsDevice(self, d_text, d_doc_offsets, ndocs, nbytes, stream=0):
        out = capi.SpLexDeviceBatch()
        rc = self._L.sp_lexer_ctx_match_docs_device(self._h, d_text, d_doc_offsets, ndocs, nbytes, stream or None, ctypes.byref(out))
        if rc != 0:
            raise PatternError("device batch lexer run failed (%d): %s" % (rc, self._err()))
        return out

    def batchFetch(self, first_doc, ndocs):
        """host copy of the lexems of the documents [first_doc, first_doc+ndocs) of the last device batch."""
        b = capi.SpLexBatch()
        rc = self._L.sp_lexer_ctx_batch_fetch_docs(self._h, first_doc, ndocs, ctypes.byref(b))
        try:
            if rc != 0:
                raise PatternError("fetching the lexer batch failed (%d): %s" % (rc, self._err()))
            return _lex_batch_of(b)
        finally:
            self._L.sp_lex_batch_free(ctypes.byref(b))

    def stitchSegmentsDevice(self, d_doc_seg_offsets, ndocs, stream=0):
        """the "documents" of the last device batch are segments: stitch them to `ndocs` documents on the device (asynchronous
        on `stream`), document d = the segments [doc_seg_offsets[d], doc_seg_offsets[d+1]) (a device array of ndocs+1 u64):
        ordinal positions continued from segment to segment, a parallel origseg array; returns the device pointers
        (capi.SpLexStitchedBatch), which PatternMatcherContext.matchDocsDevice takes as they are."""
        out = capi.SpLexStitchedBatch()
        rc = self._L.sp_lexer_ctx_stitch_segments_device(self._h, d_doc_seg_offsets, ndocs, stream or None, ctypes.byref(out))
        if rc != 0:
            raise PatternError("stitching the segments on the device failed (%d): %s" % (rc, self._err()))
        return out

    def stitchedFetch(self):
        """plain host copy of the batch stitched by stitchSegmentsDevice: (LexBatch, origseg (n,) u32)"""
        b = capi.SpLexBatch()
        seg = ctypes.POINTER(ctypes.c_uint32)()
        rc = self._L.sp_lexer_ctx_stitched_fetch(self._h, ctypes.byref(b), ctypes.byref(seg))
        try:
            if rc != 0:
                raise PatternError("fetching the stitched batch failed (%d): %s" % (rc, self._err()))
            return _lex_batch_of(b), _rows(seg, b.nlexems, 0)
        finally:
            self._L.sp_lex_batch_free(ctypes.byref(b))
            self._L.sp_free(seg)

    def stitchedStatus(self):
        """the per-document status words of the last stitchSegmentsDevice (waits for it)"""
        n = ctypes.c_size_t(0)
        if self._L.sp_lexer_ctx_stitched_status(self._h, None, 0, ctypes.byref(n)) != 0:
            raise PatternError("reading the stitch status failed: " + self._err())
        st = np.zeros(n.value, np.int32)
        if self._L.sp_lexer_ctx_stitched_status(self._h, st.ctypes.data, n.value, None) != 0:
            raise PatternError("reading the stitch status failed: " + self._err())
        return st

    def lastStitchMs(self):
        """duration of the passes of the last stitchSegmentsDevice in milliseconds"""
        a = ctypes.c_double(-1.0)
        if self._L.sp_lexer_ctx_last_stitch_ms(self._h, ctypes.byref(a)) != 0:
            raise PatternError("no timed stitch")
        return a.value

    def batchCounters(self):
        arr = (ctypes.c_uint64 * 8)()
        if self._L.sp_lexer_ctx_batch_counters(self._h, arr) != 0:
            raise PatternError("reading batch counters failed: " + self._err())
        return {"lexems": arr[0], "bytes": arr[1], "raw_reports": arr[2], "failed_docs": arr[3], "scan_units": arr[4], "rescanned_docs": arr[5],
                "word_reports": arr[6], "prof": [arr[4], arr[5], arr[6], arr[7]]}

    def batchStatus(self, ndocs):
        st = np.zeros(ndocs, np.int32)
        if self._L.sp_lexer_ctx_batch_status(self._h, st.ctypes.data, ndocs) != 0:
            raise PatternError("reading batch status failed: " + self._err())
        return st

    def lastKernelMs(self):
        return self._L.sp_lexer_ctx_last_kernel_ms(self._h)

    def lastKernelMsSplit(self):
        """(scan kernel ms, post-processing kernel ms) of the last launch"""
        a, b = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
        if self._L.sp_lexer_ctx_last_kernel_ms_split(self._h, ctypes.byref(a), ctypes.byref(b)) != 0:
            raise PatternError("no timed launch")
        return a.value, b.value

    def lastKernelMsSplit3(self):
        """(scan kernel ms, words kernel ms, post-processing kernel ms) of the last launch"""
        a, b, d = ctypes.c_double(-1.0), ctypes.c_double(-1.0), ctypes.c_double(-1.0)
        if self._L.sp_lexer_ctx_last_kernel_ms_split3(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(d)) != 0:
            raise PatternError("no timed launch")
        return a.value, b.value, d.value

    def wordsKernelName(self):
        """the instance of the words kernel the last launch went through"""
        return self._L.sp_lexer_ctx_words_kernel_name(self._h).decode()

    def scanKernelName(self):
        """the scan kernel the last launch went through"""
        return self._L.sp_lexer_ctx_scan_kernel_name(self._h).decode()

    def reserveOutput(self, lexems):
        self._L.sp_lexer_ctx_reserve_output(self._h, lexems)

    def growArena(self):
        return self._L.sp_lexer_ctx_grow_arena(self._h) == 0


class PatternLexerInstance:
    """PatternLexerInstanceInterface (src/patternLexer.cpp:961-1151)."""

    def __init__(self, _handle=None):
        self._L = capi.lib()
        self._h = _handle or self._L.sp_lexer_create()
        if not self._h:
            raise PatternError("failed to create term match instance")

    def serialize(self):
        """the compiled lexer (automaton, literal and symbol tables, names) as bytes: SURVEY.md 8(f).4"""
        return _serialize(self._L, self._L.sp_lexer_serialize, self._h, lambda: self._L.sp_lexer_last_error(self._h).decode(errors="replace"))

    @classmethod
    def deserialize(cls, blob):
        L = capi.lib()
        err = ctypes.create_string_buffer(256)
        h = L.sp_lexer_deserialize(blob, len(blob), err, 256)
        if not h:
            raise PatternError("cannot load the lexer: " + err.value.decode())
        return cls(_handle=h)

    def __del__(self):
        try:
            if self._h:
                self._L.sp_lexer_free(self._h)
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise PatternError("%s: %s" % (what, self._L.sp_lexer_last_error(self._h).decode(errors="replace")))

    @staticmethod
    def _b(s):
        return s if isinstance(s, bytes) else s.encode()

    def defineLexemName(self, id_, name):
        self._chk(self._L.sp_lexer_define_lexem_name(self._h, id_, self._b(name)), "failed to assign lexem name to lexem or symbol identifier")

    def getLexemName(self, id_):
        s = self._L.sp_lexer_get_lexem_name(self._h, id_)
        return s.decode() if s else None

    def defineLexem(self, id_, expression, resultIndex=0, level=0, posbind="content"):
        pb = POSITION_BIND[posbind] if isinstance(posbind, str) else int(posbind)
        self._chk(self._L.sp_lexer_define_lexem(self._h, id_, self._b(expression), resultIndex, level, pb), "failed to define term match regular expression pattern")

    def defineSymbol(self, symbolid, patternid, name):
        self._chk(self._L.sp_lexer_define_symbol(self._h, symbolid, patternid, self._b(name)), "failed to define regular expression pattern symbol")

    def getSymbol(self, patternid, name):
        return self._L.sp_lexer_get_symbol(self._h, patternid, self._b(name))

    def defineOption(self, name, value=0.0):
        self._chk(self._L.sp_lexer_define_option(self._h, name.encode(), value), "define option failed for pattern lexer")

    def compile(self):
        self._chk(self._L.sp_lexer_compile(self._h), "failed to compile regular expression patterns")
        return True

    def createContext(self, device=0):
        return PatternLexerContext(self, device)

    def dumpTables(self):
        p = ctypes.POINTER(ctypes.c_uint64)()
        n = self._L.sp_lexer_dump_tables(self._h, ctypes.byref(p))
        arr = np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
        self._L.sp_free(p)
        return arr

    def dumpImage(self, which):
        """(offsets, words) of a table image the kernels read: which = 0 all passes, 1 the scanned passes, 2 the words kernel's
        (None for a table without one); offsets = [oChar, oAccept, oStart, oShift, oSelf, oExSrc, oExDst, oShapeFp]"""
        p = ctypes.POINTER(ctypes.c_uint64)()
        n = self._L.sp_lexer_dump_image(self._h, which, ctypes.byref(p))
        if n < 8:
            return None
        arr = np.ctypeslib.as_array(p, shape=(n,)).copy()
        self._L.sp_free(p)
        return [int(x) for x in arr[:8]], arr[8:]

    def launchPlan(self, num_cus, ndocs, nbytes):
        """what a context on a device of num_cus compute units launches for a batch of ndocs documents and nbytes bytes, as a
        dict of strings (include/strus_pattern_amd.h, sp_lexer_launch_plan); needs no device"""
        buf = ctypes.create_string_buffer(1024)
        self._chk(self._L.sp_lexer_launch_plan(self._h, num_cus, ndocs, nbytes, buf, 1024), "no launch plan")
        return dict(f.split("=", 1) for f in buf.value.decode().split())

    def name(self):
        return "std"


class PatternLexer:
    """PatternLexerInterface (src/patternLexer.hpp:22-41)."""

    def getCompileOptionNames(self):
        return ["CASELESS", "DOTALL", "MULTILINE", "ALLOWEMPTY", "UCP"]  # src/patternLexer.cpp:1154-1163

    def createInstance(self):
        return PatternLexerInstance()

    def name(self):
        return "std"


def matchSegmentedDocs(lctx, mctx, text, seg_offsets, doc_seg_offsets, with_text=False, with_values=False, with_terms=False, with_dictionary=False, with_postings=False, with_positions=False):
    """Segmented documents, host buffers in and out: `text` holds the segments back to back (seg_offsets: nseg+1 byte
    offsets), document d consists of the segments [doc_seg_offsets[d], doc_seg_offsets[d+1]).  Lexer -> stitch on the
    device -> rule matcher -> fetch; only the text goes up and the results come down.  Returns the MatchBatch, whose
    status of a document is the stitch's where that is not 0 (a failed segment, a bad segment range), else the matcher's.
    with_text: the batch is finished on the device and the text its results and items cover gathered there; returns
    (MatchBatch, MatchText).  with_values: the values of the format strings are built there too; returns
    (MatchBatch, MatchValues), or (MatchBatch, MatchText, MatchValues) with both.  with_terms: the results are grouped into
    index terms there (value where a result has a format, else text: text and values are built for it); returns
    (MatchBatch, MatchText, MatchValues, MatchTerms).  with_dictionary implies with_terms: the dictionary of the terms is built
    there too and returned as a fifth element, a MatchDictionary.  with_postings implies with_dictionary: the postings of
    the dictionary are built there too and returned as a sixth element, a MatchPostings.  with_positions implies
    with_postings: the positions of every posting are built there too and returned as a seventh element, a MatchPositions."""
    with_postings = with_postings or with_positions
    with_dictionary = with_dictionary or with_postings
    with_terms = with_terms or with_dictionary
    with_text, with_values = with_text or with_terms, with_values or with_terms
    import torch
    text = bytes(text)
    seg_offsets = np.ascontiguousarray(seg_offsets, dtype=np.uint64)
    doc_seg_offsets = np.ascontiguousarray(doc_seg_offsets, dtype=np.uint64)
    nseg, ndocs = len(seg_offsets) - 1, len(doc_seg_offsets) - 1
    d_text = torch.frombuffer(bytearray(text + b"\0" * 16), dtype=torch.uint8).cuda()
    d_so = torch.from_numpy(seg_offsets.view(np.int64)).cuda()
    d_dso = torch.from_numpy(doc_seg_offsets.view(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(12):
        lctx.matchDocsDevice(d_text.data_ptr(), d_so.data_ptr(), nseg, len(text), stream)
        lc = lctx.batchCounters()
        if not lc["failed_docs"] or not set(int(x) for x in lctx.batchStatus(nseg)) & {2, 9}:
            break
        lctx.reserveOutput(int(lc["lexems"] * 1.2) + 1024)      # a segment without room: grow and rerun before stitching
        lctx.growArena()
    st = lctx.stitchSegmentsDevice(d_dso.data_ptr(), ndocs, stream)
    nlexems = int(lc["lexems"])                                 # an upper bound of the stitched total
    for _ in range(12):
        mctx.matchDocsDevice(st.d_lexems, st.d_doc_offsets, ndocs, nlexems, stream, d_origseg=st.d_origseg)
        mc = mctx.batchCounters()
        if not mc["failed_docs"] or not set(int(x) for x in mctx.batchStatus(ndocs)) & {2, 9}:
            break
        mctx.reserveOutput(int(mc["results"] * 1.2) + 1024, int(mc["items"] * 1.2) + 1024)
        mctx.growArena()
    mt = mv = None
    if with_text or with_values:
        mctx.batchFinishDevice(stream)
        if with_text:
            mctx.finishedTextDevice(d_text.data_ptr(), len(text), d_so.data_ptr(), nseg, d_dso.data_ptr(), stream=stream)
        if with_values:
            mctx.finishedValuesDevice(d_text.data_ptr(), len(text), d_so.data_ptr(), nseg, d_dso.data_ptr(), stream=stream)
        if with_terms:
            mctx.finishedTermsDevice(stream=stream)
        if with_dictionary:
            mctx.finishedDictionaryDevice(stream=stream)
        if with_postings:
            mctx.finishedPostingsDevice(stream=stream)
        if with_positions:
            mctx.finishedPositionsDevice(stream=stream)
        mb = mctx.finishedFetch()
        mt = mctx.finishedTextFetch() if with_text else None
        mv = mctx.finishedValuesFetch() if with_values else None
        mterms = mctx.finishedTermsFetch() if with_terms else None
        mdict = mctx.finishedDictionaryFetch() if with_dictionary else None
        mpost = mctx.finishedPostingsFetch() if with_postings else None
        mpos = mctx.finishedPositionsFetch() if with_positions else None
    else:
        mb = mctx.batchFetch()
    stitch_status = lctx.stitchedStatus()
    mb.status = np.where(stitch_status != 0, stitch_status, mb.status).astype(np.int32)
    out = (mb,) + ((mt,) if with_text else ()) + ((mv,) if with_values else ()) + ((mterms,) if with_terms else ()) + ((mdict,) if with_dictionary else ()) \
        + ((mpost,) if with_postings else ()) + ((mpos,) if with_positions else ())
    return out if len(out) > 1 else mb


def device_count():
    return capi.lib().sp_device_count()
