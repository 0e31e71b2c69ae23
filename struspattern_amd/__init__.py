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
from .products import (SP_TERM_TEXT, SP_TERM_VALUES, SP_TEXT_ITEMS, SP_TEXT_RESULTS, SP_VALUE_ITEMS, SP_VALUE_RESULTS,   # noqa: F401 (public names)
                       MatchBatch, MatchDictionary, MatchDictionaryOrder, MatchPositions, MatchPostingBlocks, MatchPostings, MatchTermBlocks, MatchTerms, MatchText, MatchValues, PatternError, PatternFreq,
                       batchDictionary, batchDictionaryOrder, batchPatternFreq, batchPositions, batchPostingBlocks, batchPostings, batchTermBlocks, batchTerms, batchText, batchValues,
                       SP_LOOKUP_PREFIX, Segment, SegmentLookup, segmentLookup,
                       _match_batch_of, _product, _rows)

__all__ = ["PatternMatcher", "PatternMatcherInstance", "PatternMatcherContext", "PatternLexer", "PatternLexerInstance",
           "PatternLexerContext", "PatternError", "JOIN_OP", "POSITION_BIND", "matchSegmentedDocs", "MatchText", "batchText", "MatchValues", "batchValues", "PatternFreq", "batchPatternFreq", "MatchTerms", "batchTerms", "MatchDictionary", "batchDictionary", "MatchPostings", "batchPostings", "MatchPositions", "batchPositions",
           "MatchDictionaryOrder", "batchDictionaryOrder", "MatchTermBlocks", "batchTermBlocks", "MatchPostingBlocks", "batchPostingBlocks", "Segment", "SegmentLookup", "segmentLookup"]

SP_CTX_RESULT_SETS = 1      # include/strus_pattern_amd.h: context flag of result-set mode
SP_FINISH_CANONICAL = 1     # include/strus_pattern_amd.h: finish flag of the canonical order inside a document
SP_ERR_UNAVAILABLE = -6     # include/strus_pattern_amd.h: a value that does not exist for the context

JOIN_OP = {"sequence": 0, "sequence_imm": 1, "sequence_struct": 2, "within": 3, "within_struct": 4, "any": 5, "and": 6}

DOC_STATUS = {
    0: "ok", 1: "term events not fed in ascending order", 2: "working set of the document exceeds the arena",
    3: "pattern with too many identical key events defined", 4: "internal: encountered past trigger with follow",
    5: "term event out of range", 6: "illegal free of event data reference",
}


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
    def _device(self, fn, out_type, phrase, *args):
        """one device call of the library, fn(handle, *args, struct pointer): the struct of `out_type` it fills with device pointers"""
        out = out_type()
        rc = fn(self._h, *args, ctypes.byref(out))
        if rc != 0:
            raise PatternError("%s failed (%d): %s" % (phrase, rc, self._err()))
        return out

    def matchDocsDevice(self, d_lexems, d_doc_offsets, ndocs, nlexems, stream=0, d_origseg=0):
        return self._device(self._L.sp_matcher_ctx_match_docs_device, capi.SpMatchDeviceBatch, "device batch match",
                            d_lexems, d_origseg or None, d_doc_offsets, ndocs, nlexems, stream or None)

    def matchLexedDevice(self, d_lexems, d_doc_ranges, ndocs, nlexems_hint, stream=0):
        """consume the device output of PatternLexerContext.matchDocsDevice in place (fused pipeline)."""
        return self._device(self._L.sp_matcher_ctx_match_lexed_device, capi.SpMatchDeviceBatch, "device batch match",
                            d_lexems, d_doc_ranges, ndocs, nlexems_hint, stream or None)

    def batchFinishDevice(self, stream=0, canonical=False):
        """finish the last batch on the device (asynchronous on `stream`): document order, `exclusive` applied, failed
        documents empty, items without gaps; returns the device pointers (capi.SpMatchFinishedBatch).  canonical: the
        results of a document in the order of SP_FINISH_CANONICAL, the same bytes from every engine."""
        return self._device(self._L.sp_matcher_ctx_batch_finish_device_ex, capi.SpMatchFinishedBatch, "finishing the batch on the device",
                            stream or None, SP_FINISH_CANONICAL if canonical else 0)

    def finishedFetch(self):
        """plain host copy of the batch finished by batchFinishDevice: what batchFetch() returns, with no work on the host."""
        return self._fetched(self._L.sp_matcher_ctx_finished_fetch)

    def _fetch_product(self, cls, call=None):
        """host copy of the product `cls` of the last batch, fetched by its own call of the library or by call(handle, struct pointer)"""
        call = call or getattr(self._L, cls._FETCH)
        return _product(cls, lambda s: call(self._h, ctypes.byref(s)), lambda rc: "fetching the %s failed (%d): %s" % (cls._WHAT, rc, self._err()))

    @staticmethod
    def _text_source(d_text, nbytes, d_seg_offsets, nseg, d_doc_seg_offsets):
        return ctypes.byref(capi.SpTextSource(d_text or None, nbytes, d_seg_offsets or None, nseg, d_doc_seg_offsets or None))

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
        flags = (SP_TEXT_RESULTS if results else 0) | (SP_TEXT_ITEMS if items else 0)
        return self._device(self._L.sp_matcher_ctx_finished_text_device, capi.SpMatchTextBatch, "gathering the text of the batch on the device",
                            self._text_source(d_text, nbytes, d_seg_offsets, nseg, d_doc_seg_offsets), flags, stream or None)

    def finishedTextFetch(self):
        """plain host copy of the text gathered by finishedTextDevice: a MatchText"""
        return self._fetch_product(MatchText)

    def lastTextMs(self):
        """duration of the passes of the last finishedTextDevice in milliseconds"""
        return self._last_ms(self._L.sp_matcher_ctx_last_text_ms, "text call")

    def finishedValuesDevice(self, d_text, nbytes, d_seg_offsets, nseg, d_doc_seg_offsets=0, flags=SP_VALUE_RESULTS | SP_VALUE_ITEMS, stream=0):
        """build the values of the format strings of the results and / or items of the batch finished by batchFinishDevice,
        on the device (the placement is asynchronous on `stream`); the text source is that of finishedTextDevice.
        Returns the device pointers (capi.SpMatchValuesBatch), valid until the next call."""
        return self._device(self._L.sp_matcher_ctx_finished_values_device, capi.SpMatchValuesBatch, "building the values of the batch on the device",
                            self._text_source(d_text, nbytes, d_seg_offsets, nseg, d_doc_seg_offsets), flags, stream or None)

    def finishedValuesFetch(self):
        """plain host copy of the values built by finishedValuesDevice: a MatchValues"""
        return self._fetch_product(MatchValues)

    def lastValuesMs(self):
        """duration of the passes of the last finishedValuesDevice in milliseconds"""
        return self._last_ms(self._L.sp_matcher_ctx_last_values_ms, "values call")

    def finishedPatternFreqDevice(self, stream=0):
        """sum the pattern frequencies of the batch finished by batchFinishDevice on the device (the placement is
        asynchronous on `stream`): per document one record per distinct handle, per handle the sums over the batch.
        Returns the device pointers (capi.SpPatternFreqDevice), valid until the next call."""
        return self._device(self._L.sp_matcher_ctx_finished_pattern_freq_device, capi.SpPatternFreqDevice, "summing the pattern frequencies of the batch on the device", stream or None)

    def finishedPatternFreqFetch(self):
        """plain host copy of the frequencies summed by finishedPatternFreqDevice: a PatternFreq"""
        return self._fetch_product(PatternFreq)

    def lastPatternFreqMs(self):
        """duration of the passes of the last finishedPatternFreqDevice in milliseconds"""
        return self._last_ms(self._L.sp_matcher_ctx_last_pattern_freq_ms, "pattern frequency call")

    def finishedTermsDevice(self, flags=SP_TERM_VALUES | SP_TERM_TEXT, stream=0):
        """group the results of the batch finished by batchFinishDevice into index terms on the device (the placement is
        asynchronous on `stream`): per document one record per distinct (handle, value), per result the index of its term.
        flags: SP_TERM_VALUES (finishedValuesDevice has run since the finish, with the results family), SP_TERM_TEXT
        (finishedTextDevice has, with results=True), or both.  Returns the device pointers (capi.SpMatchTermsDevice), valid
        until the next call."""
        return self._device(self._L.sp_matcher_ctx_finished_terms_device, capi.SpMatchTermsDevice, "grouping the terms of the batch on the device", flags, stream or None)

    def finishedTermsFetch(self):
        """plain host copy of the terms grouped by finishedTermsDevice: a MatchTerms"""
        return self._fetch_product(MatchTerms)

    def lastTermsMs(self):
        """duration of the passes of the last finishedTermsDevice in milliseconds"""
        return self._last_ms(self._L.sp_matcher_ctx_last_terms_ms, "terms call")

    def finishedDictionaryDevice(self, stream=0):
        """build the dictionary of the terms grouped by finishedTermsDevice on the device (the placement is asynchronous on
        `stream`): every distinct (handle, value) of the batch once, in the order of first occurrence, with its document
        and collection frequency, and per term record the index of its entry.  Returns the device pointers
        (capi.SpMatchDictionaryDevice), valid until the next call."""
        return self._device(self._L.sp_matcher_ctx_finished_dictionary_device, capi.SpMatchDictionaryDevice, "building the dictionary of the batch on the device", stream or None)

    def finishedDictionaryFetch(self):
        """plain host copy of the dictionary built by finishedDictionaryDevice: a MatchDictionary"""
        return self._fetch_product(MatchDictionary)

    def lastDictionaryMs(self):
        """duration of the launches of the last finishedDictionaryDevice in milliseconds"""
        return self._last_ms(self._L.sp_matcher_ctx_last_dictionary_ms, "dictionary call")

    def finishedDictionaryOrderDevice(self, stream=0):
        """rank the entries of the dictionary built by finishedDictionaryDevice by (handle, value bytes) on the device (everything
        is asynchronous on `stream`: the call waits for nothing).  Returns the device pointers (capi.SpMatchDictionaryOrderDevice),
        valid until the next call."""
        return self._device(self._L.sp_matcher_ctx_finished_dictionary_order_device, capi.SpMatchDictionaryOrderDevice, "ordering the dictionary of the batch on the device", stream or None)

    def finishedDictionaryOrderFetch(self):
        """plain host copy of the order built by finishedDictionaryOrderDevice: a MatchDictionaryOrder"""
        return self._fetch_product(MatchDictionaryOrder)

    def lastDictionaryOrderMs(self):
        """duration of the launches of the last finishedDictionaryOrderDevice in milliseconds"""
        return self._last_ms(self._L.sp_matcher_ctx_last_dictionary_order_ms, "dictionary order call")

    def finishedTermBlocksDevice(self, stream=0):
        """write the dictionary ranked by finishedDictionaryOrderDevice as front-coded term blocks on the device (the call waits
        once, for the number of bytes; the emitting launch is asynchronous on `stream`): the first product that owns its bytes.
        Returns the device pointers (capi.SpMatchTermBlocksDevice), valid until the next call."""
        return self._device(self._L.sp_matcher_ctx_finished_term_blocks_device, capi.SpMatchTermBlocksDevice, "coding the term blocks of the batch on the device", stream or None)

    def finishedTermBlocksFetch(self):
        """plain host copy of the blocks written by finishedTermBlocksDevice: a MatchTermBlocks"""
        return self._fetch_product(MatchTermBlocks)

    def lastTermBlocksMs(self):
        """duration of the launches of the last finishedTermBlocksDevice in milliseconds"""
        return self._last_ms(self._L.sp_matcher_ctx_last_term_blocks_ms, "term blocks call")

    def finishedPostingBlocksDevice(self, stream=0):
        """write the posting lists of the batch, with their positions, in the order of finishedDictionaryOrderDevice as delta-coded
        posting blocks on the device, from the postings of finishedPostingsDevice and the positions of finishedPositionsDevice (the
        call waits once, for the number of bytes; the emitting launch is asynchronous on `stream`): list k is position k of the
        term blocks.  Returns the device pointers (capi.SpMatchPostingBlocksDevice), valid until the next call."""
        return self._device(self._L.sp_matcher_ctx_finished_posting_blocks_device, capi.SpMatchPostingBlocksDevice, "coding the posting blocks of the batch on the device", stream or None)

    def finishedPostingBlocksFetch(self):
        """plain host copy of the blocks written by finishedPostingBlocksDevice: a MatchPostingBlocks"""
        return self._fetch_product(MatchPostingBlocks)

    def lastPostingBlocksMs(self):
        """duration of the launches of the last finishedPostingBlocksDevice in milliseconds"""
        return self._last_ms(self._L.sp_matcher_ctx_last_posting_blocks_ms, "posting blocks call")

    def finishedPostingsDevice(self, stream=0):
        """build the postings of the dictionary built by finishedDictionaryDevice on the device (everything is asynchronous
        on `stream`: the call waits for nothing): per dictionary entry the list of (doc, term, count, first_ordpos) in
        document order, and per term record the index of its posting.  Returns the device pointers
        (capi.SpMatchPostingsDevice), valid until the next call."""
        return self._device(self._L.sp_matcher_ctx_finished_postings_device, capi.SpMatchPostingsDevice, "building the postings of the batch on the device", stream or None)

    def finishedPostingsFetch(self):
        """plain host copy of the postings built by finishedPostingsDevice: a MatchPostings"""
        return self._fetch_product(MatchPostings)

    def lastPostingsMs(self):
        """duration of the launches of the last finishedPostingsDevice in milliseconds"""
        return self._last_ms(self._L.sp_matcher_ctx_last_postings_ms, "postings call")

    def finishedPositionsDevice(self, stream=0):
        """build the positions of the postings built by finishedPostingsDevice on the device (the call waits once, for the
        number of occurrences and the largest position, which set its passes; the placement is asynchronous on `stream`; a stream
        other than the postings' is ordered behind them).  Returns the device pointers (capi.SpMatchPositionsDevice), valid until
        the next call."""
        return self._device(self._L.sp_matcher_ctx_finished_positions_device, capi.SpMatchPositionsDevice, "building the positions of the batch on the device", stream or None)

    def finishedPositionsFetch(self):
        """plain host copy of the positions built by finishedPositionsDevice: a MatchPositions"""
        return self._fetch_product(MatchPositions)

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
        return self._fetch_product(MatchBatch, call)

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


# The products of a finished batch that matchSegmentedDocs builds, in the order it builds, fetches and returns them: the stem of
# the context's methods (finished<stem>Device, finished<stem>Fetch) and the products it needs.  (The posting blocks are built in
# front of the term blocks, whose row stays the last, and returned behind them: _SEGMENT_LAST.)
_SEGMENT_PRODUCTS = (("Text", ()), ("Values", ()), ("Terms", ("Text", "Values")), ("Dictionary", ("Terms",)), ("Postings", ("Dictionary",)),
                     ("Positions", ("Postings",)), ("DictionaryOrder", ("Dictionary",)), ("PostingBlocks", ("DictionaryOrder", "Positions")),
                     ("TermBlocks", ("DictionaryOrder",)))
_SEGMENT_LAST = "PostingBlocks"


def _rerun(ctx, ndocs, launch, grow, no_room=frozenset((2, 9)), attempts=12):
    """Run, look at the status, grow, rerun: launch() on the context until no document of the batch has failed, or none for
    lack of room (status in no_room); grow(counters) reserves the output before the arena grows.  Returns the counters of the
    last run; documents that still fail after the last attempt keep their status."""
    for _ in range(attempts):
        launch()
        c = ctx.batchCounters()
        if not c["failed_docs"] or not set(int(x) for x in ctx.batchStatus(ndocs)) & no_room:
            break
        grow(c)
        ctx.growArena()
    return c


def matchSegmentedDocs(lctx, mctx, text, seg_offsets, doc_seg_offsets, with_text=False, with_values=False, with_terms=False, with_dictionary=False, with_postings=False, with_positions=False,
                       with_dictionary_order=False, with_term_blocks=False, with_posting_blocks=False):
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
    with_postings: the positions of every posting are built there too and returned as a seventh element, a MatchPositions.
    with_dictionary_order implies with_dictionary: the entries of the dictionary are ranked by (handle, value) there too and the
    MatchDictionaryOrder returned as one more element at the end, behind whatever else was asked for.  with_term_blocks implies
    with_dictionary_order: the sorted dictionary is written as front-coded term blocks there too and the MatchTermBlocks returned
    as the last element, behind the order.  with_posting_blocks implies with_dictionary_order and with_positions: the posting
    lists are written as delta-coded posting blocks in the sorted order there too and the MatchPostingBlocks returned as the very
    last element, behind the term blocks where both were asked for."""
    want = {"Text": with_text, "Values": with_values, "Terms": with_terms, "Dictionary": with_dictionary, "Postings": with_postings, "Positions": with_positions,
            "DictionaryOrder": with_dictionary_order, "TermBlocks": with_term_blocks, "PostingBlocks": with_posting_blocks}
    for name, needs in reversed(_SEGMENT_PRODUCTS):
        if want[name]:
            want.update(dict.fromkeys(needs, True))
    chosen = [name for name, _ in _SEGMENT_PRODUCTS if want[name]]
    import torch
    text = bytes(text)
    seg_offsets = np.ascontiguousarray(seg_offsets, dtype=np.uint64)
    doc_seg_offsets = np.ascontiguousarray(doc_seg_offsets, dtype=np.uint64)
    nseg, ndocs = len(seg_offsets) - 1, len(doc_seg_offsets) - 1
    d_text = torch.frombuffer(bytearray(text + b"\0" * 16), dtype=torch.uint8).cuda()
    d_so = torch.from_numpy(seg_offsets.view(np.int64)).cuda()
    d_dso = torch.from_numpy(doc_seg_offsets.view(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    # (a segment without room: grow and rerun before stitching)
    lc = _rerun(lctx, nseg, lambda: lctx.matchDocsDevice(d_text.data_ptr(), d_so.data_ptr(), nseg, len(text), stream),
                lambda c: lctx.reserveOutput(int(c["lexems"] * 1.2) + 1024))
    st = lctx.stitchSegmentsDevice(d_dso.data_ptr(), ndocs, stream)
    nlexems = int(lc["lexems"])                                 # an upper bound of the stitched total
    _rerun(mctx, ndocs, lambda: mctx.matchDocsDevice(st.d_lexems, st.d_doc_offsets, ndocs, nlexems, stream, d_origseg=st.d_origseg),
           lambda c: mctx.reserveOutput(int(c["results"] * 1.2) + 1024, int(c["items"] * 1.2) + 1024))
    products = ()
    if chosen:
        source = (d_text.data_ptr(), len(text), d_so.data_ptr(), nseg, d_dso.data_ptr())
        mctx.batchFinishDevice(stream)
        for name in chosen:
            getattr(mctx, "finished%sDevice" % name)(*(source if name in ("Text", "Values") else ()), stream=stream)
        mb = mctx.finishedFetch()
        products = tuple(getattr(mctx, "finished%sFetch" % name)() for name in sorted(chosen, key=lambda name: name == _SEGMENT_LAST))
    else:
        mb = mctx.batchFetch()
    stitch_status = lctx.stitchedStatus()
    mb.status = np.where(stitch_status != 0, stitch_status, mb.status).astype(np.int32)
    return (mb,) + products if products else mb


def device_count():
    return capi.lib().sp_device_count()
