"""What the tests of the products of a finished batch share: the harness that sets every span itself (hand-made lexems through
small rules on the device), the hand-made batches of the device-free twins, and a few helpers that tests of the device batches
below them use as well.  A test module imports what it needs from here, never from another test module.  Needs no device to
import: torch is imported where a helper uploads."""
import ctypes
import os

import numpy as np

import struspattern_amd as spa
from struspattern_amd import capi, synth
from tests import result_values_model

V, T = spa.SP_TERM_VALUES, spa.SP_TERM_TEXT
BOTH = result_values_model.SP_VALUE_RESULTS | result_values_model.SP_VALUE_ITEMS


# ---- the pair rule over hand-made lexems on the device (tests/test_span_text_gpu.py and every product test after it)
SENTINEL = 64          # bytes of 0xFF behind every text on the device; the texts themselves hold none


def _torch():
    import torch
    return torch


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _pair_matcher():
    m = spa.PatternMatcherInstance()
    m.pushTerm(1)
    m.attachVariable("a")
    m.pushTerm(2)
    m.attachVariable("b")
    m.pushExpression("sequence", 2, 1, 0)
    m.definePattern("pair", "", True)
    m.compile()
    return m


_MATCHER = []


def _ctx():
    """a context of the pair rule (the rule set is compiled once)"""
    if not _MATCHER:
        _MATCHER.append(_pair_matcher())
    return _MATCHER[0].createContext()


def _from_device(ptr, count, dtype):
    out = np.zeros(count, dtype)
    if count:
        fn = capi.lib().hipMemcpy
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        assert fn(out.ctypes.data, ptr, out.nbytes, 2) == 0        # hipMemcpyDeviceToHost
    return out


class Source:
    """a text of segments on the device, with the sentinel behind it"""

    def __init__(self, pieces, doc_seg_offsets=None):
        torch = _torch()
        self.text = b"".join(pieces)
        assert b"\xff" not in self.text
        self.so = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.uint64)
        self.dso = None if doc_seg_offsets is None else np.asarray(doc_seg_offsets, np.uint64)
        self.nseg = len(pieces)
        self.d_text = torch.frombuffer(bytearray(self.text + b"\xff" * SENTINEL), dtype=torch.uint8).cuda()
        self.d_so = torch.from_numpy(self.so.view(np.int64)).cuda()
        self.d_dso = None if self.dso is None else torch.from_numpy(self.dso.view(np.int64)).cuda()

    def gather(self, ctx, stream=None, **kw):
        return ctx.finishedTextDevice(self.d_text.data_ptr(), len(self.text), self.d_so.data_ptr(), self.nseg,
                                      self.d_dso.data_ptr() if self.d_dso is not None else 0, stream=_stream() if stream is None else stream, **kw)


def _random_text(rng, n):
    return bytes(rng.integers(33, 127, n, dtype=np.uint8))


def _pairs(docs, seglens):
    """docs: per document a list of spans (s0, pos, s1, end); seglens: per document the lengths of its segments -> the lexems
    (n, 4), their origseg, the document offsets, and per document the (result, item a, item b) byte ranges inside it as
    (s0, pos, s1, end) tuples"""
    lex, seg, offs, want = [], [], [0], []
    for spans, lens in zip(docs, seglens):
        w = []
        for k, (s0, pos, s1, end) in enumerate(spans):
            if s0 == s1 and pos <= end:
                sa = (end - pos) // 2
                sb = end - pos - sa
            else:
                sa, sb = max(0, min(lens[s0] - pos, 2)) if s0 < len(lens) else 0, min(end, 3)
            lex += [[1, 10 * k + 1, pos, sa], [2, 10 * k + 2, end - sb, sb]]
            seg += [s0, s1]
            w.append(((s0, pos, s1, end), (s0, pos, s0, pos + sa), (s1, end - sb, s1, end)))
        offs.append(len(lex))
        want.append(w)
    return np.array(lex, np.uint32).reshape(-1, 4), np.array(seg, np.uint32), np.array(offs, np.uint64), want


class Run:
    """the pair rule over hand-made lexems on the device, finished"""

    def __init__(self, ctx, lex, seg, offs, canonical=False):
        torch = _torch()
        self.ctx = ctx
        self.d_lex = torch.from_numpy(np.ascontiguousarray(lex).view(np.int32).reshape(-1)).cuda()
        self.d_seg = torch.from_numpy(np.ascontiguousarray(seg).view(np.int32)).cuda()
        self.d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
        self.ndocs, self.nlex = len(offs) - 1, len(lex)
        self.match()
        self.fin = ctx.batchFinishDevice(_stream(), canonical=canonical)

    def match(self):
        for _ in range(6):
            self.ctx.matchDocsDevice(self.d_lex.data_ptr(), self.d_offs.data_ptr(), self.ndocs, self.nlex, _stream(), self.d_seg.data_ptr())
            c = self.ctx.batchCounters()
            if c["failed_docs"] == 0:
                return
            assert set(int(x) for x in self.ctx.batchStatus(self.ndocs) if x) <= {2, 9}
            self.ctx.reserveOutput(int(c["results"] * 1.2) + 1024, int(c["items"] * 1.2) + 1024)
            self.ctx.growArena()
        raise AssertionError("documents still failing after resizing")


# ---- bare-term matchers
_BARE = {}


def _bare(n):
    """a matcher of n bare-term patterns: the handle of term h is h (compiled once per size)"""
    if n not in _BARE:
        m = spa.PatternMatcherInstance()
        for h in range(1, n + 1):
            m.pushTerm(h)
            m.definePattern("p%d" % h, "", True)
        m.compile()
        assert m.handleBound() == n + 1 and m.patternId("p1") == 1 and m.patternId("p%d" % n) == n
        _BARE[n] = m
    return _BARE[n]


# ---- hand-made documents of (handle, value) terms
def _build(docs):
    """docs: per document a list of (handle, value bytes): every occurrence gets its own copy of the value in the document's
    text, one behind the other -> pieces, lexems (n, 4), origseg, document offsets"""
    pieces, lex, offs = [], [], [0]
    for doc in docs:
        text = b""
        for k, (h, value) in enumerate(doc):
            lex.append([h, k + 1, len(text), len(value)])
            text += value
        pieces.append(text)
        offs.append(len(lex))
    return pieces, np.array(lex, np.uint32).reshape(-1, 4), np.zeros(len(lex), np.uint32), np.array(offs, np.uint64)


# ---- documents at the trip edges of a lane per term record
EVERY = (1, b"every")


def _trip_docs():
    """Documents of 0, 1, 63, 64, 65 and 129 term records -- the trip edges of a lane per record -- and one whose terms are all
    known: document k repeats about half of the terms of the documents before it and adds new ones, a third of its terms
    occur twice in it, and EVERY is in each of them."""
    rng = np.random.default_rng(3)
    used, docs, fresh = [], [], 0
    for n in (0, 1, 63, 64, 65, 129):
        doc = [EVERY] if n else []
        doc += [used[int(i)] for i in rng.permutation(len(used))[:max(0, (n - 1) // 2)]]
        while len(doc) < n:
            doc.append((1 + fresh % 7, b"t%04d" % fresh + b"x" * (fresh % 19)))
            fresh += 1
        used += [t for t in doc if t != EVERY and t not in used]
        doc = doc + doc[:n // 3]
        docs.append([doc[int(i)] for i in rng.permutation(len(doc))])
    docs.append([EVERY] + [used[int(i)] for i in rng.permutation(len(used))[:39]])
    return docs


TRIP_RECORDS = [0, 1, 63, 64, 65, 129, 40]


# ---- the documented example and a matcher with chosen format handles
# the program and text of tests/test_formats.py (introduction_struspattern.htm:146-156)
MONEY = r'''
    WORD ^1         : /\b\w+\b/;
    NUMBER ^2       : /\b[0-9]{4}\b/;
    AMOUNT^5        : /\b[0-9]{1,3}'[0-9]{3,3}'[0-9]{3,3}\b/;
    AMOUNT^4        : /\b[0-9]{1,3}'[0-9]{3,3}\b/;
    AMOUNT^3        : /\b[0-9]{1,3}\b/;
    CURRENCY_CHF ^3 : /\b[Ss]{0,1}[Ff][Rr][.]{0,1}\b/;
    CURRENCY_EUR ^3 : /\b[Ee][Uu][Rr][.]{0,1}\b/;
    Currency        = CURRENCY_CHF ["CHF"];
    Currency        = CURRENCY_EUR ["EUR"];
    MoneyAmount     = sequence_imm( value=AMOUNT, currency=Currency | 2) ["{currency} {value}"];
    .Year           = sequence_imm( WORD "in", WORD "the", WORD "year", year=NUMBER | 4) ["{year}"];
    Event           = sequence_imm( when=Year, WORD "something", WORD "happened" | 8) ["{when}"];
    Plain           = sequence( when=Year, what=WORD | 8 );
'''
TEXT = b"He paid 3'645 Eur and 12 sFr. in the year 1984 something happened again"


def matcher_of(formats, variables=("a", "b", "v")):
    """a rule set whose variable handles are 1.. in the order of `variables` and whose format handles are 1.. in the order of
    `formats`; its rules do not matter to the twin"""
    m = spa.PatternMatcherInstance()
    m.pushTerm(1)
    for v in variables:
        m.pushTerm(1)
        m.attachVariable(v)
    m.pushExpression("sequence", len(variables) + 1, 100, 0)
    m.definePattern("p0", formats[0], True)
    for k, f in enumerate(formats[1:]):
        m.pushTerm(2 + k)
        m.definePattern("p%d" % (k + 1), f, True)
    m.compile()
    assert [m.formatString(h + 1) for h in range(m.formatCount())] == list(formats)
    assert [m.variableId(v) for v in variables] == list(range(1, len(variables) + 1))
    return m


# ---- rules with format strings over hand-made lexems on the device
# term -> what a lexem of it fires
T_LIT, T_SPAN, T_J1, T_J2, T_J3, T_NONE, T_YEAR, T_EV, T_PLAIN_A, T_PLAIN_B, T_X1, T_X2 = range(1, 13)


def _rules():
    m = spa.PatternMatcherInstance()

    def term(t, var=None):
        m.pushTerm(t)
        if var:
            m.attachVariable(var)

    def rule(name, fmt, terms, op="sequence", rng=1, visible=True):
        for t, var in terms:
            if isinstance(t, str):
                m.pushPattern(t)
                if var:
                    m.attachVariable(var)
            else:
                term(t, var)
        m.pushExpression(op if len(terms) > 1 else "any", len(terms), rng, 0)
        m.definePattern(name, fmt, visible)

    rule("Lit", "CHF", [(T_LIT, "a")])
    rule("Span", "{a}", [(T_SPAN, "a")])
    rule("J2", "{a|, }", [(T_J1, "a"), (T_J2, "a")])
    rule("J3", "{a|, }", [(T_J1, "a"), (T_J2, "a"), (T_J3, "a")], rng=2)
    rule("E2", "{a|}", [(T_J1, "a"), (T_J2, "a")])
    rule("E3", "<{a|}>", [(T_J1, "a"), (T_J2, "a"), (T_J3, "a")], rng=2)
    rule("None", "[{b}{nosuch}]", [(T_NONE, "a")])
    rule("Year", "{year}", [(T_YEAR, "year")], visible=False)
    rule("Event", "{when}", [("Year", "when"), (T_EV, None)])
    rule("Plain", "", [(T_PLAIN_A, "a"), (T_PLAIN_B, "b")])
    rule("Sub", "", [(T_X1, None), (T_X2, None)], visible=False)
    rule("Cross", "({s})", [("Sub", "s")])
    m.compile()
    return m


def _chain(depth):
    """P0 = term 1 ["x"], Pk = any(v=P(k-1)) ["{v}"]: Pk's value is `k+1` formats deep; beside the chain Q = any(a=term 2)
    ["<{a}>"] and R = sequence(b=term 2, b=term 3) without a format, whose items are formatted by nothing"""
    m = spa.PatternMatcherInstance()
    m.pushTerm(1); m.pushExpression("any", 1, 1, 0); m.definePattern("P0", "x", True)
    for k in range(1, depth):
        m.pushPattern("P%d" % (k - 1)); m.attachVariable("v"); m.pushExpression("any", 1, 1, 0); m.definePattern("P%d" % k, "{v}", True)
    m.pushTerm(2); m.attachVariable("a"); m.pushExpression("any", 1, 1, 0); m.definePattern("Q", "<{a}>", True)
    m.pushPattern("Q"); m.attachVariable("q"); m.pushTerm(3); m.pushExpression("sequence", 2, 1, 0); m.definePattern("R", "", True)
    m.compile()
    return m


_CACHE = {}


def _matcher(key="rules"):
    if key not in _CACHE:
        _CACHE[key] = _rules() if key == "rules" else _chain(key)
    return _CACHE[key]


class Lexems:
    """documents of hand-made lexems: add(term, seg, pos, size) at the next ordinal position"""

    def __init__(self):
        self.lex, self.seg, self.offs, self.ordpos = [], [], [0], 0

    def add(self, term, pos, size, seg=0):
        self.ordpos += 1
        self.lex.append([term, self.ordpos, pos, size])
        self.seg.append(seg)
        return self

    def gap(self):
        self.ordpos += 5
        return self

    def doc(self):
        self.offs.append(len(self.lex))
        self.ordpos = 0
        return self

    def arrays(self):
        return np.array(self.lex, np.uint32).reshape(-1, 4), np.array(self.seg, np.uint32), np.array(self.offs, np.uint64)


class RunAny(Run):
    """Run that lets documents fail in the matcher with a status the test chose (lexems out of order)"""

    def match(self):
        for _ in range(6):
            self.ctx.matchDocsDevice(self.d_lex.data_ptr(), self.d_offs.data_ptr(), self.ndocs, self.nlex, _stream(), self.d_seg.data_ptr())
            c = self.ctx.batchCounters()
            bad = set(int(x) for x in self.ctx.batchStatus(self.ndocs) if x)
            if not bad & {2, 9}:
                return
            self.ctx.reserveOutput(int(c["results"] * 1.2) + 1024, int(c["items"] * 1.2) + 1024)
            self.ctx.growArena()
        raise AssertionError("documents still failing after resizing")


def _values(ctx, src, flags=BOTH, stream=None):
    return ctx.finishedValuesDevice(src.d_text.data_ptr(), len(src.text), src.d_so.data_ptr(), src.nseg,
                                    src.d_dso.data_ptr() if src.d_dso is not None else 0, flags=flags, stream=_stream() if stream is None else stream)


# ---- hand-made batches and byte families without a device
def _batch(docs, formats=None, status=None):
    """docs: per document a list of (handle, ordpos, ordend) -> MatchBatch"""
    rows, offs = [], [0]
    for doc in docs:
        rows += [[h, p, e, 0, 0, 0, 0, 0, 0] for h, p, e in doc]
        offs.append(len(rows))
    n = len(docs)
    return spa.MatchBatch(np.array(rows, np.uint32).reshape(-1, 9), np.zeros((0, 7), np.uint32), np.array(offs, np.uint64),
                          np.zeros((n, 4), np.uint64), np.zeros(n, np.int32) if status is None else np.array(status, np.int32),
                          None if formats is None else np.array(formats, np.uint32), None if formats is None else np.zeros((0, 2), np.uint32))


def _family(cls, strings, ndocs, status=None, pad=b""):
    """a MatchValues / MatchText whose result r has the bytes strings[r]"""
    offs = np.cumsum([0] + [len(s) for s in strings]).astype(np.uint64)
    return cls(b"".join(strings) + pad, offs, None, None, np.zeros(ndocs, np.int32) if status is None else np.array(status, np.int32))


# ---- the four documents of tests/test_dictionary_abi.py and their dictionaries, written out
# four documents; result r has the handle and the text / value / format below
DICT_DOCS = [
    [(1, 1, 2), (1, 3, 4), (2, 5, 6), (1, 7, 8), (3, 9, 10)],
    [(2, 1, 2), (1, 3, 4)],
    [(1, 1, 2), (3, 3, 4), (1, 5, 6), (1, 7, 8)],
    [(1, 1, 2), (2, 3, 4)],
]
DICT_TEXT = [b"eur", b"eur", b"x", b"ab", b"",  b"eur", b"abc",  b"eur", b"", b"eur", b"eur",  b"eur", b"x"]
DICT_VALUES = [b"EUR", b"EUR", b"", b"", b"",  b"", b"eur",  b"", b"", b"EUR", b"",  b"", b"x"]
DICT_FORMATS = [1, 1, 0, 0, 0,  0, 2,  0, 0, 1, 0,  0, 3]
DICT_BOUND = 4

# flags -> (entries [handle, value_bytes, first_doc, first_term, doc_freq, max_count, count], term_dict, doc_offsets, handle_terms)
DICT_EXPECTED = {
    # the text: (1,"eur") in the documents 0, 2 and 3; "eur" under handle 2 in document 1; "ab" and "abc"; the empty text twice
    T: ([[1, 3, 0, 0, 3, 3, 6], [1, 2, 0, 1, 1, 1, 1], [2, 1, 0, 2, 2, 1, 2], [3, 0, 0, 3, 2, 1, 2], [1, 3, 1, 0, 1, 1, 1], [2, 3, 1, 1, 1, 1, 1]],
        [0, 1, 2, 3, 4, 5, 0, 3, 0, 2], [0, 4, 6, 6, 6], [0, 3, 2, 1]),
    # the values: an unformatted result has the empty value, under three handles three entries
    V: ([[1, 3, 0, 0, 2, 2, 3], [1, 0, 0, 1, 3, 2, 4], [2, 0, 0, 2, 2, 1, 2], [3, 0, 0, 3, 2, 1, 2], [1, 3, 1, 0, 1, 1, 1], [2, 1, 3, 1, 1, 1, 1]],
        [0, 1, 2, 3, 4, 2, 1, 0, 3, 1, 5], [0, 4, 5, 5, 6], [0, 3, 2, 1]),
    # both: the formatted value "eur" of document 1 and the text "eur" of unformatted results of the documents 2 and 3 are one
    # entry; so are the text "x" of document 0 and the formatted value "x" of document 3
    V | T: ([[1, 3, 0, 0, 2, 2, 3], [1, 2, 0, 1, 1, 1, 1], [2, 1, 0, 2, 2, 1, 2], [3, 0, 0, 3, 2, 1, 2], [1, 3, 1, 0, 3, 2, 4], [2, 3, 1, 1, 1, 1, 1]],
            [0, 1, 2, 3, 4, 5, 4, 0, 3, 4, 2], [0, 4, 6, 6, 6], [0, 3, 2, 1]),
}


def _dict_inputs(flags, text_status=None):
    mb = _batch(DICT_DOCS, DICT_FORMATS)
    mv, mt = _family(spa.MatchValues, DICT_VALUES, 4), _family(spa.MatchText, DICT_TEXT, 4, status=text_status)
    terms = spa.batchTerms(mb, values=mv, text=mt, handle_bound=DICT_BOUND, flags=flags)
    return mb, mv, mt, terms


# ---- the one document of tests/test_host_twins_abi.py
TWIN_BOUND = 3
TWIN_BAD_OFFSETS = {"not starting at 0": [1, 2], "descending": [2, 1], "not covering the results": [0, 1]}


def _twin_batch():
    """result 0: handle 2, "ab", format 1 over one item "ab" of variable 1; result 1: handle 1, "cd", no format, one item "d" """
    results = [[2, 0, 1, 0, 0, 0, 2, 0, 1], [1, 1, 2, 0, 2, 0, 4, 1, 1]]
    items = [[1, 0, 1, 0, 0, 0, 2], [1, 1, 2, 0, 3, 0, 4]]
    return spa.MatchBatch(np.array(results, np.uint32), np.array(items, np.uint32), np.array([0, 2], np.uint64), np.zeros((1, 4), np.uint64),
                          np.zeros(1, np.int32), np.array([1, 0], np.uint32), np.zeros((2, 2), np.uint32))


# what the terms and the dictionary are built from, written out by hand: the value of result 0, the text of both, their terms
TWIN_VALUES = spa.MatchValues(b"<ab>", np.array([0, 4, 4], np.uint64), None, None, np.zeros(1, np.int32))
TWIN_RESULT_TEXT = spa.MatchText(b"abcd", np.array([0, 2, 4], np.uint64), None, None, np.zeros(1, np.int32))
TWIN_TERM_RECORDS = [[1, 1, 1, 2, 1, 2], [2, 1, 0, 1, 0, 4]]     # (1, "cd") of result 1, (2, "<ab>") of result 0
TWIN_TERMS = spa.MatchTerms(np.array(TWIN_TERM_RECORDS, np.uint32), np.array([0, 2], np.uint64), np.array([1, 0], np.uint32), np.zeros(1, np.int32), V | T, TWIN_BOUND)


# ---- random rule programs with format strings
def _random_program(rng, nterms):
    """token rules with private and public sub-patterns, some with format strings, referenced with variables"""
    calls, names = [], []
    for k in range(14):
        name = "P%d" % k

        def operand(depth=0):
            if names and rng.random() < (0.45 if depth == 0 else 0.25):
                calls.append(("pushPattern", rng.choice(names)))
            elif depth < 2 and rng.random() < 0.2:
                argc = rng.randint(2, 3)
                for _ in range(argc):
                    operand(depth + 1)
                calls.append(("pushExpression", rng.choice(["sequence", "within", "any"]), argc, rng.randint(3, 8), 0))
            else:
                calls.append(("pushTerm", rng.randint(1, nterms)))
            if rng.random() < 0.7:
                calls.append(("attachVariable", "v%d" % rng.randint(0, 3)))
        argc = rng.randint(1, 3)
        for _ in range(argc):
            operand()
        calls.append(("pushExpression", rng.choice(["sequence", "sequence_imm", "within", "any", "sequence_struct"]) if argc > 1 else "any", argc, rng.randint(2, 10), 0))
        fmt = rng.choice(["", "", "<{v0}>", "{v1|,}+{v2}", "const", "{v0}{v3}"])
        calls.append(("definePattern", name, fmt, rng.random() < 0.7))
        names.append(name)
    return calls


def _apply(m, calls):
    for c in calls:
        if c[0] == "pushExpression" and c[1] == "sequence_struct":
            m.pushTerm(1)   # the delimiter operand comes first
            getattr(m, c[0])(c[1], c[2] + 1, c[3], c[4])
            continue
        getattr(m, c[0])(*c[1:])
    m.compile()


# ---- device batches of any rule set
class _Uploaded:
    """lexems and document offsets in device memory (kept alive as long as the batch is looked at)"""

    def __init__(self, lex, offs, origseg=None):
        import torch
        self.lex = torch.from_numpy(np.ascontiguousarray(lex, dtype=np.uint32).view(np.int32).reshape(-1)).cuda()
        self.offs = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.uint64).view(np.int64)).cuda()
        self.seg = torch.from_numpy(np.ascontiguousarray(origseg, dtype=np.uint32).view(np.int32)).cuda() if origseg is not None else None
        self.ndocs, self.nlex = len(offs) - 1, len(lex)

    def run(self, ctx, stream=None):
        return ctx.matchDocsDevice(self.lex.data_ptr(), self.offs.data_ptr(), self.ndocs, self.nlex,
                                   _stream() if stream is None else stream, self.seg.data_ptr() if self.seg is not None else 0)


def _sized(ctx, run, ndocs, what):
    """the device protocol (bench.py size_until_ok): a batch whose output did not fit is rerun with the counted sizes"""
    for _ in range(6):
        run()
        c = ctx.batchCounters()
        if c["failed_docs"] == 0:
            return c
        assert set(int(x) for x in ctx.batchStatus(ndocs) if x) <= {2, 9}, what    # arena / output capacity only
        if "lexems" in c:
            ctx.reserveOutput(int(c["lexems"] * 1.2) + 1024)
        else:
            ctx.reserveOutput(int(c["results"] * 1.2) + 1024, int(c["items"] * 1.2) + 1024)
        ctx.growArena()
    raise AssertionError("%s: documents still failing after resizing" % what)


# ---- random documents of lexems
def _docs(rng, ndocs, n, nfeat, shared_positions):
    lex = np.zeros((ndocs * n, 4), np.uint32)
    offs = np.arange(ndocs + 1, dtype=np.uint64) * n
    for d in range(ndocs):
        ids = rng.integers(1, nfeat + 1, size=n)
        ids[rng.random(n) < 0.06] = synth.DELIM
        pos = np.arange(1, n + 1)
        if shared_positions:
            pos = np.cumsum(rng.random(n) < 0.7) + 1          # several lexems on one position
        lex[d * n:(d + 1) * n, 0] = ids
        lex[d * n:(d + 1) * n, 1] = pos
        lex[d * n:(d + 1) * n, 2] = np.arange(n) * 3
        lex[d * n:(d + 1) * n, 3] = 2
    return lex, offs


# ---- contexts of the configurations of the fast tier
CONFIGS = {
    "default": {},
    "spill": {"SPA_L2_FAST_SIZE": "t"},
    "handover": {"SPA_L2_FAST_SIZE": "t", "SPA_L2_FAST_MAXRULES": "24", "SPA_L2_FAST_MAXSTAGED": "40"},
    "general": {"SPA_L2_FAST": "0"},
}


def _context(m, config):
    env = CONFIGS[config]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return m.createContext()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
