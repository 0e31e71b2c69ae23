"""Dictionary order without a device (sp_match_batch_dictionary_order, csrc/match_dictorder.hpp): the twin equals the model
(tests/dictorder_model.py) on hand-made batches -- the empty shapes, every comparator edge of tests/dictorder_cases.py, both
sources in one batch, input already ascending and descending --, every refusal of the header with its message, the struct round
trip of MatchDictionaryOrder in both directions, find() and the sorted listing rule of match.py on host arrays."""
import ctypes

import numpy as np
import pytest

import struspattern_amd as spa
from struspattern_amd import capi, match
from struspattern_amd import products as P
from tests import dictorder_cases as cases
from tests import dictorder_model as model
from tests.finished_support import _batch, DICT_BOUND, _dict_inputs, _family, T, V

BOUND = 8


class Inputs:
    """documents of (handle, value) terms as a finished batch on the host: every term is one result whose text is the value;
    formatted: the (handle, value) pairs whose result has a format, its value in the values and another text"""

    def __init__(self, docs, flags=T, formatted=(), bound=BOUND):
        rows = [[(h, k + 1, k + 2) for k, (h, _) in enumerate(doc)] for doc in docs]
        flat = [t for doc in docs for t in doc]
        formats = [1 if t in formatted else 0 for t in flat]
        self.mb = _batch(rows, formats if flags & V else None)
        self.text = _family(spa.MatchText, [b"?" if f else v for (_, v), f in zip(flat, formats)], len(docs)) if flags & T else None
        self.values = _family(spa.MatchValues, [v if f or flags == V else b"" for (_, v), f in zip(flat, formats)], len(docs)) if flags & V else None
        self.terms = spa.batchTerms(self.mb, values=self.values, text=self.text, handle_bound=bound, flags=flags)
        self.d = spa.batchDictionary(self.mb, self.terms, values=self.values, text=self.text)
        self.entries = model.entries_of(self.mb, self.terms, self.d, self.values, self.text)

    def order(self):
        return spa.batchDictionaryOrder(self.mb, self.terms, self.d, values=self.values, text=self.text)

    def check(self):
        got, want = self.order(), model.dictionary_order(self.entries, self.d.handle_terms)
        model.assert_same(got, want)
        model.check_invariants(got, self.entries, self.d.handle_terms)
        return got

    def sorted_entries(self, got):
        return [self.entries[int(e)] for e in got.order]


def test_symbols_and_signatures():
    vp, Ptr = ctypes.c_void_p, ctypes.POINTER
    for name in ("sp_matcher_ctx_finished_dictionary_order_device", "sp_matcher_ctx_finished_dictionary_order_fetch", "sp_match_dictionary_order_free",
                 "sp_matcher_ctx_last_dictionary_order_ms", "sp_match_batch_dictionary_order", "sp_matcher_dictionary_order_tile"):
        assert name in capi.SIGNATURES and hasattr(capi.lib(), name)
    assert capi.SIGNATURES["sp_matcher_ctx_finished_dictionary_order_device"] == (ctypes.c_int, [vp, vp, Ptr(capi.SpMatchDictionaryOrderDevice)])
    assert capi.SIGNATURES["sp_match_batch_dictionary_order"][1][:6] == [Ptr(capi.SpMatchBatch), Ptr(capi.SpMatchValues), Ptr(capi.SpMatchText), Ptr(capi.SpMatchTerms),
                                                                         Ptr(capi.SpMatchDictionary), Ptr(capi.SpMatchDictionaryOrder)]
    assert [n for n, _ in capi.SpMatchDictionaryOrderDevice._fields_] == ["ndict", "handle_bound", "d_order", "d_rank", "d_prefix_bytes", "d_handle_offsets", "d_totals"]
    assert [n for n, _ in capi.SpMatchDictionaryOrder._fields_] == ["ndict", "handle_bound", "order", "rank", "prefix_bytes", "handle_offsets", "totals"]
    for name in ("finishedDictionaryOrderDevice", "finishedDictionaryOrderFetch", "lastDictionaryOrderMs"):
        assert hasattr(spa.PatternMatcherContext, name)
    for name in ("MatchDictionaryOrder", "batchDictionaryOrder"):
        assert name in spa.__all__
    tile = capi.lib().sp_matcher_dictionary_order_tile()
    assert tile >= 64 and tile & (tile - 1) == 0
    assert ("DictionaryOrder", ("Dictionary",)) in spa._SEGMENT_PRODUCTS


def test_the_header_states_the_rule_and_no_longer_says_not_offered():
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "strus_pattern_amd.h")) as f:
        header = f.read()
    assert "---- dictionary order:" in header and "not offered" not in header


# ---- the shapes
@pytest.mark.parametrize("docs", [[], [[], [], []]], ids=["no documents", "only empty documents"])
def test_no_entries(docs):
    got = Inputs(docs).check()
    assert len(got.order) == len(got.rank) == len(got.prefix_bytes) == 0 and got.handle_offsets.tolist() == [0] * (BOUND + 1)


def test_one_entry():
    got = Inputs([[(3, b"only")], [(3, b"only")]]).check()
    assert got.order.tolist() == [0] and got.rank.tolist() == [0] and got.prefix_bytes.tolist() == [0]
    assert got.handle_offsets.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1]


def test_comparator_edges_written_out():
    pairs = cases.comparator_values()
    x = Inputs(cases.in_documents(pairs, 11))
    got = x.check()
    assert x.sorted_entries(got) == sorted(pairs)
    of_two = [v for h, v in x.sorted_entries(got) if h == 2]
    # the empty value first; the zero paddings by length; unsigned bytes; a value before what it is a prefix of
    assert of_two[:5] == [b"", b"\x01\xfe", cases.LONG[:4], cases.LONG[:15], cases.LONG[:15] + b"atail"]
    at = of_two.index(b"a")
    assert of_two[at:at + 9] == [b"a", b"a\0", b"a\0\0\0", b"a\0\0\0\0", b"ab", b"abc", b"abcd", b"abcde", b"zz\x7f"]
    assert of_two[-4:] == [b"zz\xc3\xa9", b"\x7f", b"\x80", b"\xfe\x01"]
    k = int(got.rank[x.entries.index((2, b"a\0\0\0\0"))])
    assert got.prefix_bytes[k - 3:k + 2].tolist() == [0, 1, 2, 4, 1]           # "a" follows another first byte; then the paddings; then "ab"
    for n in (15, 16, 17):
        head = (cases.LONG * 2)[:n]
        k = int(got.rank[x.entries.index((2, head + b"btail"))])
        assert got.prefix_bytes[k - 1:k + 1].tolist() == [n, n] and x.entries[int(got.order[k - 2])] == (2, head)
    # the same bytes under three handles; handles without an entry are empty ranges
    assert [x.entries[int(e)] for e in got.handle(5)] == [(5, b""), (5, b"abc")] and [x.entries[int(e)] for e in got.handle(1)] == [(1, b"abc")]
    assert len(got.handle(3)) == len(got.handle(4)) == len(got.handle(6)) == len(got.handle(7)) == len(got.handle(0)) == 0
    assert got.prefix_bytes[int(got.handle_offsets[5])] == 0 and got.prefix_bytes[int(got.handle_offsets[2])] == 0


def test_a_long_shared_prefix():
    pairs = cases.long_prefix_group()
    x = Inputs(cases.in_documents(pairs, 33))
    got = x.check()
    assert got.order.tolist() == list(range(69, -1, -1)) and got.prefix_bytes.tolist() == [0] + [300] * 69


@pytest.mark.parametrize("arrival", ["ascending", "descending", "shuffle"])
def test_ascending_descending_and_shuffled_input(arrival):
    pairs = cases.numbered(300, arrival=arrival)
    x = Inputs(cases.in_documents(pairs))
    got = x.check()
    assert x.sorted_entries(got) == sorted(pairs)
    if arrival == "ascending":
        assert got.order.tolist() == got.rank.tolist() == list(range(300))
    if arrival == "descending":                         # (the terms of a document ascend by handle: the documents descend)
        assert x.entries[0] > x.entries[-1] and got.rank[0] > 200 and got.rank[-1] < 97


def test_values_and_text_in_one_batch():
    formatted = {(1, b"eur"), (2, b"b"), (2, b"")}
    docs = [[(1, b"usd"), (1, b"eur"), (2, b"c")], [(2, b"b"), (2, b"a"), (2, b"")], [(1, b"chf")]]
    x = Inputs(docs, flags=V | T, formatted=formatted)
    got = x.check()
    assert x.sorted_entries(got) == [(1, b"chf"), (1, b"eur"), (1, b"usd"), (2, b""), (2, b"a"), (2, b"b"), (2, b"c")]
    # the four documents of the dictionary tests, under every combination of flags
    for flags in (V, T, V | T):
        mb, mv, mt, terms = _dict_inputs(flags)
        d = spa.batchDictionary(mb, terms, values=mv, text=mt)
        entries = model.entries_of(mb, terms, d, mv, mt)
        o = spa.batchDictionaryOrder(mb, terms, d, values=mv, text=mt)
        model.assert_same(o, model.dictionary_order(entries, d.handle_terms))
        model.check_invariants(o, entries, d.handle_terms)
        assert len(o.handle_offsets) == DICT_BOUND + 1


# ---- refusals
def _raw(x, damage=None, null=()):
    """sp_match_batch_dictionary_order over C structs made of the Inputs x; damage(b, t, q) may change them, `null` names the
    arguments passed as NULL.  Returns (rc, message)."""
    keep = []
    mb = spa.MatchBatch(x.mb.results, x.mb.items, x.mb.doc_offsets.copy(), x.mb.stats, x.mb.status, x.mb.result_format, x.mb.item_format)
    b, keep_b = P._host_batch(mb, formats="results", status=True)
    v, t_ = P._host_source(x.values, keep), P._host_source(x.text, keep)
    t = P._to_c(spa.MatchTerms(x.terms.records.copy(), x.terms.doc_offsets.copy(), x.terms.result_term, x.terms.status, x.terms.flags, x.terms.handle_bound), keep)
    q = P._to_c(spa.MatchDictionary(x.d.records.copy(), x.d.term_dict, x.d.doc_offsets, x.d.handle_terms.copy()), keep, flags=x.terms.flags)
    if damage:
        damage(b, t, q)
    args = {"mb": b, "values": v, "text": t_, "terms": t, "dict": q}
    out = capi.SpMatchDictionaryOrder()
    out.ndict = 77                                      # (the call clears `out` first)
    err = ctypes.create_string_buffer(256)
    rc = capi.lib().sp_match_batch_dictionary_order(*[None if k in null or a is None else ctypes.byref(a) for k, a in args.items()], ctypes.byref(out), err, 256)
    if rc == 0:
        assert out.ndict == len(x.d.records) == out.totals[0] and out.handle_bound == len(x.d.handle_terms) and out.order and out.handle_offsets
        capi.lib().sp_match_dictionary_order_free(ctypes.byref(out))
    assert not out.order and not out.rank and not out.prefix_bytes and not out.handle_offsets and out.ndict == 0 and out.totals[0] == 0
    return rc, err.value.decode()


def _set(which, field, value=None, by=0, at=None):
    def damage(b, t, q):
        target = {"b": b, "t": t, "q": q}[which]
        if at is None:
            setattr(target, field, getattr(target, field) + by if value is None else value)
        elif isinstance(at, tuple):
            setattr(getattr(target, field)[at[0]], at[1], value)
        else:
            getattr(target, field)[at] = value
    return damage


REFUSED = [
    # what sp_match_batch_dictionary refuses about its inputs
    ("other counts of documents or results", _set("t", "ndocs", by=-1)),
    ("other counts of documents or results", _set("t", "nresults", by=1)),
    ("unknown or no term flags", lambda b, t, q: (setattr(t, "flags", 0), setattr(q, "flags", 0))),
    ("a handle bound of 0", lambda b, t, q: (setattr(t, "handle_bound", 0), setattr(q, "handle_bound", 0))),
    ("document offsets of the batch do not start", _set("b", "doc_result_offsets", 1, at=0)),
    ("term offsets do not start", _set("t", "doc_term_offsets", 1, at=0)),
    ("term offsets do not ascend", _set("t", "doc_term_offsets", 99, at=1)),
    ("term offsets do not cover", _set("t", "doc_term_offsets", 5, at=2)),
    # the dictionary against its terms
    ("other counts of documents or term records", _set("q", "ndocs", by=1)),
    ("other counts of documents or term records", _set("q", "nterms", by=-1)),
    ("another handle bound or other flags", _set("q", "handle_bound", by=1)),
    ("another handle bound or other flags", _set("q", "flags", value=V)),
    # the entries
    ("a handle outside the bound", _set("q", "records", 0, at=(1, "handle"))),
    ("a handle outside the bound", _set("q", "records", BOUND, at=(1, "handle"))),
    ("whose handle is not that of its term record", _set("q", "records", 3, at=(1, "handle"))),
    ("first_doc lies outside the documents", _set("q", "records", 2, at=(0, "first_doc"))),
    ("first_term lies outside its document's records", _set("q", "records", 3, at=(0, "first_term"))),
    ("first_result lies outside its document", _set("t", "records", 3, at=(0, "first_result"))),
    ("term record whose value_bytes is not the length", _set("t", "records", 9, at=(0, "value_bytes"))),
    ("dictionary entry whose value_bytes is not the length", _set("q", "records", 9, at=(0, "value_bytes"))),
    ("handle_terms that are not the number of entries", _set("q", "handle_terms", 1, at=2)),
    ("two dictionary entries with the same handle and bytes", lambda b, t, q: (setattr(q.records[4], "first_doc", 0), setattr(q.records[4], "first_term", 2))),
]


def _refusal_inputs():
    # document 0: (1, "bb"), (1, "a"), (2, "a"); document 1: (1, "c"), (1, "a"), (2, "d") -> five entries, (2, "d") the last
    return Inputs([[(1, b"bb"), (1, b"a"), (2, b"a")], [(1, b"c"), (1, b"a"), (2, b"d")]])


@pytest.mark.parametrize("message,damage", REFUSED, ids=["%02d %s" % (k, m[:40]) for k, (m, _) in enumerate(REFUSED)])
def test_refusals_with_their_message(message, damage):
    x = _refusal_inputs()
    assert len(x.d.records) == 5 and x.entries[4] == (2, b"d") and x.d.handle_terms.tolist()[:3] == [0, 3, 2]
    assert _raw(x) == (0, "")
    rc, msg = _raw(x, damage)
    assert rc == -1 and message in msg, msg
    assert _raw(x) == (0, "")                           # the same objects then serve a good call


def test_refused_arguments_and_sources():
    x = _refusal_inputs()
    for name, message in (("mb", "no batch"), ("terms", "no terms"), ("dict", "no dictionary"), ("text", "no text of the results")):
        rc, msg = _raw(x, null=(name,))
        assert rc == -1 and message in msg, name
    # a source range outside the source's bytes: the text loses its last byte
    x.text = spa.MatchText(x.text.result_text[:-1], x.text.result_offsets, None, None, x.text.status)
    rc, msg = _raw(x)
    assert rc == -1 and "outside the bytes of its source" in msg
    with pytest.raises(spa.PatternError, match=r"no order of the dictionary \(-1\): a term value outside"):
        x.order()
    # values selected and absent
    y = Inputs([[(1, b"a")]], flags=V | T, formatted={(1, b"a")})
    y.values = None
    with pytest.raises(spa.PatternError, match="no values of the results"):
        y.order()


# ---- the Python class
@pytest.mark.parametrize("n,bound", [(0, 1), (0, 4), (5, 4)])
def test_struct_round_trip_in_both_directions(n, bound):
    want = spa.MatchDictionaryOrder(np.arange(n, dtype=np.uint32)[::-1].copy(), np.arange(n, dtype=np.uint32) + 7, np.arange(n, dtype=np.uint32) * 3,
                                    np.arange(bound + 1, dtype=np.uint64) + (1 << 33))
    keep = []
    s = P._to_c(want, keep)
    assert (s.ndict, s.handle_bound, s.totals[0]) == (n, bound, n) and (bool(s.order) or n == 0) and s.handle_offsets
    got = P._from_c(spa.MatchDictionaryOrder, s)
    for a in spa.MatchDictionaryOrder._ARRAYS:
        g, w = getattr(got, a.attr), getattr(want, a.attr)
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), a.attr
    assert [a.attr for a in spa.MatchDictionaryOrder._ARRAYS] == list(model.FIELDS)
    assert spa.MatchDictionaryOrder._FREE == "sp_match_dictionary_order_free" and spa.MatchDictionaryOrder._FETCH == "sp_matcher_ctx_finished_dictionary_order_fetch"
    assert spa.MatchDictionaryOrder._TOTAL == "ndict" and spa.MatchDictionaryOrder._C is capi.SpMatchDictionaryOrder


def test_find_hits_and_misses():
    pairs = cases.comparator_values() + cases.numbered(40)
    x = Inputs(cases.in_documents(pairs, 13))
    got = x.check()
    where = (x.mb, x.terms, x.d)
    for e, (h, v) in enumerate(x.entries):
        assert got.find(h, v, *where, text=x.text) == e
    for h, v in [(2, b"abcdef"), (2, b"a\0\0"), (2, b"\xff\xff"), (3, b"abc"), (5, b"ab"), (0, b""), (7, b""), (BOUND, b"abc"), (99, b""), (-1, b"")]:
        assert got.find(h, v, *where, text=x.text) is None, (h, v)
    assert Inputs([]).check().find(1, b"", *where, text=x.text) is None


# ---- the listing
def test_sorted_listing_on_host_arrays():
    docs = [[(2, b"b"), (1, b"zeta"), (2, b"a")], [(1, b"alpha"), (2, b"b")]]
    name = "p%d".__mod__
    listings = []
    for files in (docs, docs[::-1]):
        x = Inputs(files)
        order = x.order()
        postings = spa.batchPostings(x.terms, x.d)
        found = (x.mb, x.text, None, x.terms)
        plain = match.dictionary_lines(x.d, found, name)
        assert plain == match.dictionary_lines(x.d, found, name, None)
        listings.append((plain, match.dictionary_lines(x.d, found, name, order), match.postings_lines(postings, x.d, found, name, None, order)))
    assert listings[0][0] != listings[1][0] and sorted(listings[0][0]) == sorted(listings[1][0])      # arrival order depends on the files
    assert listings[0][1] == listings[1][1] == ["dict p1 'alpha': docs 1 count 1", "dict p1 'zeta': docs 1 count 1", "dict p2 'a': docs 1 count 1",
                                               "dict p2 'b': docs 2 count 2"]
    assert listings[0][2] == ["post p1 'alpha': 1:1@1", "post p1 'zeta': 0:1@2", "post p2 'a': 0:1@3", "post p2 'b': 0:1@1 1:1@2"]
    assert [line.split(": ")[0] for line in listings[1][2]] == [line.split(": ")[0] for line in listings[0][2]]
