"""sp_match_batch_values (csrc/result_values.hpp), the device-free twin of the value passes: against resultformat.Formatter on
the oracle's results of the documented example and of random rule programs, against the recursive restatement of the rule
(tests/result_values_model.py) over hand-made batches -- malformed input, nesting at the limit, spans used and unused,
segmented documents -- the parser's edges, and the stand-alone program under a sanitizer.  Needs no device."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from struspattern_amd import capi, resultformat, rulelang, synth
from tests import result_values_model as model
from tests.finished_support import _apply, matcher_of, MONEY, _random_program, TEXT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SP_ERR_INVALID = -1
BOTH = model.SP_VALUE_RESULTS | model.SP_VALUE_ITEMS


def make_batch(docs):
    """docs: per document a list of results (format, [items]), item = (variable, format, nsub, span) with span =
    (origseg, origpos, origendseg, origend) -> MatchBatch in the finished layout"""
    results, items, rf, itf, offs = [], [], [], [], [0]
    for doc in docs:
        for k, (fmt, its) in enumerate(doc):
            results.append([7, k, k + 1, 0, 0, 0, 0, len(items), len(its)])
            rf.append(fmt)
            for var, f, nsub, span in its:
                items.append([var, k, k + 1, *span])
                itf.append([f, nsub])
        offs.append(len(results))
    return spa.MatchBatch(np.array(results, np.uint32).reshape(-1, 9), np.array(items, np.uint32).reshape(-1, 7),
                          np.array(offs, np.uint64), np.zeros((len(docs), 4), np.uint64), np.zeros(len(docs), np.int32),
                          np.array(rf, np.uint32), np.array(itf, np.uint32).reshape(-1, 2))


def assert_same(got, want):
    assert np.array_equal(got.status, want["status"])
    for fam in ("result", "item"):
        if want[fam + "_offsets"] is None:
            assert getattr(got, fam + "_values") is None and getattr(got, fam + "_offsets") is None
        else:
            assert np.array_equal(getattr(got, fam + "_offsets"), want[fam + "_offsets"])
            assert getattr(got, fam + "_values") == want[fam + "_values"]


def check(m, mb, text, so, dso=None, flags=BOTH):
    """the twin equals the model"""
    formats = [m.formatString(h + 1).encode() for h in range(m.formatCount())]
    got = spa.batchValues(m, mb, text, so, dso, flags=flags)
    want = model.batch_values(formats, lambda name: m.variableId(name.decode()), mb.results, mb.items, mb.result_format, mb.item_format,
                              mb.doc_offsets, text, np.asarray(so, np.uint64), None if dso is None else np.asarray(dso, np.uint64), flags,
                              max_depth=capi.lib().sp_matcher_value_max_depth())
    assert_same(got, want)
    return got


def test_symbols_and_signatures():
    for name in ("sp_matcher_ctx_finished_values_device", "sp_matcher_ctx_finished_values_fetch", "sp_matcher_ctx_last_values_ms",
                 "sp_match_values_free", "sp_match_batch_values", "sp_matcher_value_max_depth"):
        assert name in capi.SIGNATURES and hasattr(capi.lib(), name)
    vp, P = ctypes.c_void_p, ctypes.POINTER
    assert capi.SIGNATURES["sp_matcher_ctx_finished_values_device"] == (ctypes.c_int, [vp, P(capi.SpTextSource), ctypes.c_uint32, vp, P(capi.SpMatchValuesBatch)])
    assert [n for n, _ in capi.SpMatchValuesBatch._fields_] == ["ndocs", "d_result_values", "d_result_value_offsets", "d_item_values",
                                                                "d_item_value_offsets", "d_doc_value_status", "d_totals"]
    assert [n for n, _ in capi.SpMatchValues._fields_] == ["ndocs", "nresults", "nitems", "result_values", "result_value_offsets", "item_values",
                                                          "item_value_offsets", "doc_value_status", "totals"]
    assert capi.lib().sp_matcher_value_max_depth() == 8
    for name in ("batchValues", "MatchValues"):
        assert hasattr(spa, name)
    for name in ("finishedValuesDevice", "finishedValuesFetch", "lastValuesMs"):
        assert hasattr(spa.PatternMatcherContext, name)


def formatter_values(fm, res, src_of_doc):
    """per formatted result and item record the value of resultformat.Formatter: ({result index: bytes}, {item index: bytes})"""
    rv, iv = {}, {}
    for d in range(len(res.doc_offsets) - 1):
        src = src_of_doc(d)
        for r in range(int(res.doc_offsets[d]), int(res.doc_offsets[d + 1])):
            ib, ic = int(res.results[r][7]), int(res.results[r][8])
            if int(res.result_format[r]):
                rv[r] = fm.evaluate(int(res.result_format[r]), fm.gather(res.items, res.item_format, ib, ib + ic, src), src).encode()
            for i in range(ib, ib + ic):
                f, nsub = int(res.item_format[i][0]), int(res.item_format[i][1])
                if f:
                    iv[i] = fm.evaluate(f, fm.gather(res.items, res.item_format, i + 1, i + 1 + nsub, src), src).encode()
    return rv, iv


def assert_formatter(got, res, rv, iv):
    assert not got.status.any()
    for r in range(len(res.results)):
        assert got.result(r) == rv.get(r, b""), r
    for i in range(len(res.items)):
        assert got.item(i) == iv.get(i, b""), i


def test_documented_example_against_the_formatter():
    olx, omt = oracle.L1Lexer(), oracle.L2Matcher()
    prg = rulelang.load(MONEY, olx, omt)
    lex, offs = olx.matchDocs(TEXT, np.array([0, len(TEXT)], np.uint64))
    res = omt.run(synth.lexems5(lex), offs)
    lx, mt = spa.PatternLexerInstance(), spa.PatternMatcherInstance()
    rulelang.load(MONEY, lx, mt)
    mb = spa.MatchBatch(res.results, res.items, res.doc_offsets, res.stats, res.status, res.result_format, res.item_format)
    got = spa.batchValues(mt, mb, TEXT, [0, len(TEXT)])
    rv, iv = formatter_values(rulelang.formatter(prg, omt), res, lambda d: TEXT)
    assert_formatter(got, res, rv, iv)
    names = [mt.patternName(int(r[0])) for r in res.results]
    by_name = sorted((names[r], got.result(r)) for r in rv)
    assert ("MoneyAmount", b"EUR 3'645") in by_name and ("MoneyAmount", b"CHF 12") in by_name and ("Event", b"1984") in by_name
    # Plain has no format; its item `when`, bound to Year, carries Year's value
    plain = [r for r in range(len(names)) if names[r] == "Plain"]
    assert plain and all(got.result(r) == b"" and int(res.result_format[r]) == 0 for r in plain)
    when = [i for r in plain for i in range(int(res.results[r][7]), int(res.results[r][7]) + int(res.results[r][8]))
            if mt.variableName(int(res.items[i][0])) == "when"]
    assert when and all(got.item(i) == b"1984" for i in when)
    # each family alone gives the same bytes
    only_r = spa.batchValues(mt, mb, TEXT, [0, len(TEXT)], flags=model.SP_VALUE_RESULTS)
    only_i = spa.batchValues(mt, mb, TEXT, [0, len(TEXT)], flags=model.SP_VALUE_ITEMS)
    assert only_r.result_values == got.result_values and only_r.item_values is None
    assert only_i.item_values == got.item_values and only_i.result_values is None
    check(mt, mb, TEXT, [0, len(TEXT)])


@pytest.mark.parametrize("seed", range(3))
def test_random_programs_against_the_formatter(seed):
    rng = random.Random(9100 + seed)
    nterms = 6
    # (the generator attaches v0..v3 and draws formats over them: every format string also names a variable that the
    # rule set does not have, with and without a separator)
    absent = iter(["{nosuch}", "{nosuch|;}"] * 14)
    calls = [(c[0], c[1], c[2] + next(absent), c[3]) if c[0] == "definePattern" and c[2] else c for c in _random_program(rng, nterms)]
    mt, omt = spa.PatternMatcherInstance(), oracle.L2Matcher()
    _apply(mt, calls)
    _apply(omt, calls)
    assert mt.variableId("nosuch") == 0 and all("{nosuch" in mt.formatString(h + 1) for h in range(mt.formatCount()))
    lex, offs = synth.random_documents(12, 60, nterms, seed=50 + seed)
    res = omt.run(synth.lexems5(lex), offs, nthreads=2)
    assert int(res.item_format[:, 0].max()) > 0 and int(res.result_format.max()) > 0
    # a text under the lexems: every document is one segment
    lens = [int((lex[int(offs[d]):int(offs[d + 1]), 2] + lex[int(offs[d]):int(offs[d + 1]), 3]).max()) if offs[d] < offs[d + 1] else 0
            for d in range(len(offs) - 1)]
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    text = bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz,+<>") for _ in range(int(so[-1])))
    formats = [mt.formatString(h + 1) for h in range(mt.formatCount())]
    fm = resultformat.Formatter(lambda h: mt.patternName(h), lambda v: mt.variableName(v), lambda h: formats[h - 1])
    rv, iv = formatter_values(fm, res, lambda d: text[int(so[d]):int(so[d + 1])])
    mb = spa.MatchBatch(res.results, res.items, res.doc_offsets, res.stats, res.status, res.result_format, res.item_format)
    got = check(mt, mb, text, so)
    assert_formatter(got, res, rv, iv)
    assert len(got.result_values) > 0 and len(got.item_values) > 0
    # values of formats that name the absent variable are among them
    used = set(int(f) for f in res.result_format if f) | set(int(f) for f in res.item_format[:, 0] if f)
    assert used and all("{nosuch" in formats[f - 1] for f in used)


def test_parser_edges():
    m = matcher_of(["a{a|, }b\\{c", "{ a }", "{a|}", "{a}{nosuch}\\"])
    text = b"0123456789"
    its = [(1, 0, 0, (0, 0, 0, 2)), (2, 0, 0, (0, 2, 0, 3)), (1, 0, 0, (0, 4, 0, 6)), (1, 0, 0, (0, 9, 0, 10))]
    got = check(m, make_batch([[(1, its), (2, its[:1]), (3, its), (4, its[:2])]]), text, [0, 10])
    assert [got.result(i) for i in range(4)] == [b"a01, 45, 9b{c", b"01", b"01459", b"01\\"]


@pytest.mark.parametrize("fmt", ["{open", "{}", "x{ |,}"])
def test_a_format_that_does_not_parse_fails_the_values_call_only(fmt):
    m = matcher_of(["fine", fmt])               # definePattern and compile succeed, now as before
    mb = make_batch([[(1, [])]])
    with pytest.raises(spa.PatternError) as e:
        spa.batchValues(m, mb, b"abc", [0, 3])
    assert "(%d)" % SP_ERR_INVALID in str(e.value) and fmt in str(e.value)


GOOD = (2, [(1, 0, 0, (0, 0, 0, 2)), (2, 0, 0, (0, 2, 0, 3)), (1, 0, 0, (0, 4, 0, 6))])      # "{a|,}+{b}"
FORMATS = ["<{a}>", "{a|,}+{b}", "x", "{v}", "[{nosuch}]"]
TEXT3, SO3 = b"0123456789abcdefghijABCDEFGHIJ", [0, 10, 20, 30]


def around(doc, **kw):
    """the document between two good ones: -> MatchValues, checked against the model"""
    m = matcher_of(FORMATS)
    got = check(m, make_batch([[GOOD], doc, [GOOD]]), TEXT3, SO3, **kw)
    assert got.status[0] == 0 and got.status[2] == 0
    if got.result_values is not None:
        assert got.result(0) == b"01,45+2" and got.result(len(doc) + 1) == b"AB,EF+C"
    return got


@pytest.mark.parametrize("fmt,nsub", [(3, 2), (6, 1)], ids=["nsub-overruns-its-list", "format-handle-count-plus-1"])
def test_malformed_records_fail_the_document(fmt, nsub):
    got = around([(1, [(1, fmt, nsub, (0, 0, 0, 1)), (1, 0, 0, (0, 1, 0, 2))])])
    assert got.status[1] == model.SP_DOC_ERR_RANGE
    assert got.result(1) == b"" and got.item(3) == b"" and got.item(4) == b""
    assert got.result_offsets[1] == got.result_offsets[2] and len(got.result_values) == 14


def chain(depth):
    """a result of format "{v}" over a chain of "{v}" items around one "x": `depth` formats inside each other"""
    return (4, [(3, 4 if k + 1 < depth else 3, depth - 1 - k, (0, 0, 0, 1)) for k in range(1, depth)])


def test_depth_at_the_limit_and_beyond():
    limit = capi.lib().sp_matcher_value_max_depth()
    got = around([chain(limit)])
    assert got.status[1] == 0 and got.result(1) == b"x" and [got.item(3 + k) for k in range(limit - 1)] == [b"x"] * (limit - 1)
    got = around([chain(limit + 1), GOOD])
    assert got.status[1] == model.SP_DOC_ERR_RANGE
    assert got.result(1) == b"" and got.result(2) == b"" and not any(got.item(3 + k) for k in range(limit + 3))
    # the items alone start one level further in: the same records are valid
    got = around([chain(limit + 1)], flags=model.SP_VALUE_ITEMS)
    assert got.status[1] == 0 and got.item(3) == b"x" and got.result_values is None
    got = around([chain(limit + 1)], flags=model.SP_VALUE_RESULTS)
    assert got.status[1] == model.SP_DOC_ERR_RANGE and got.item_values is None


def test_invalid_spans_used_and_unused():
    bad = (0, 5, 0, 11)                         # ends beyond the document's segment
    got = around([(1, [(2, 0, 0, bad), (1, 0, 0, (0, 1, 0, 3))])])      # "<{a}>" does not use b
    assert got.status[1] == 0 and got.result(1) == b"<bc>"
    got = around([(1, [(1, 0, 0, bad), (1, 0, 0, (0, 1, 0, 3))])])
    assert got.status[1] == model.SP_DOC_ERR_RANGE and got.result(1) == b""
    # inside a nested value that is used / behind a record that has no format and is not used
    got = around([(4, [(3, 1, 1, (0, 0, 0, 1)), (1, 0, 0, bad)])])
    assert got.status[1] == model.SP_DOC_ERR_RANGE
    got = around([(3, [(3, 1, 1, (0, 0, 0, 1)), (2, 0, 0, bad)])])
    assert got.status[1] == 0 and got.result(1) == b"x" and got.item(3) == b"<>"


def test_unknown_variable_and_items_outside_the_document():
    m = matcher_of(FORMATS)
    mb = make_batch([[(5, [(1, 0, 0, (0, 0, 0, 1))])], [(1, [(1, 0, 0, (0, 0, 0, 1))])]])
    mb.results[1, 7] = 0                        # the second document's result points into the first one's items
    got = check(m, mb, TEXT3[:20], SO3[:3])
    assert got.result(0) == b"[]" and list(got.status) == [0, model.SP_DOC_ERR_RANGE]


def test_segmented_documents():
    pieces = [b"alpha beta", b"", b"gamma", b"delta eps", b"zeta"]
    text = b"".join(pieces)
    so = np.concatenate([[0], np.cumsum([len(p) for p in pieces])])
    dso = [0, 3, 3, 5]                          # document 1 has no segments
    m = matcher_of(FORMATS)
    docs = [
        [(2, [(1, 0, 0, (0, 6, 2, 3)), (2, 0, 0, (2, 0, 2, 5)), (1, 0, 0, (1, 0, 1, 0))])],       # across two borders, an empty span
        [],
        [(1, [(1, 0, 0, (0, 6, 1, 4))]), (4, [(3, 1, 1, (1, 0, 1, 4)), (1, 0, 0, (1, 0, 1, 4))])],
    ]
    got = check(m, make_batch(docs), text, so, dso)
    assert not got.status.any()
    assert [got.result(i) for i in range(3)] == [b"betagam,+gamma", b"<epszeta>", b"<zeta>"]
    assert got.item(4) == b"<zeta>"
    # a span in a segment that the document does not have
    docs[2][0] = (1, [(1, 0, 0, (0, 6, 2, 0))])
    got = check(m, make_batch(docs), text, so, dso)
    assert list(got.status) == [0, 0, model.SP_DOC_ERR_RANGE] and got.result(0) == b"betagam,+gamma" and got.item(4) == b""


def test_matcher_without_formats_and_refused_arguments():
    m = spa.PatternMatcherInstance()
    m.pushTerm(1); m.attachVariable("a"); m.definePattern("p", "", True); m.compile()
    mb = make_batch([[(0, [(1, 0, 0, (0, 0, 0, 2))])], []])
    got = spa.batchValues(m, mb, b"abcd", [0, 2, 4])
    assert not got.status.any() and got.result_values == b"" and got.item_values == b""
    assert list(got.result_offsets) == [0, 0] and list(got.item_offsets) == [0, 0]
    m2 = matcher_of(FORMATS)
    for kw, what in ((dict(flags=0), "flags"), (dict(flags=4), "flags"), (dict(so=[0, 4]), "nseg")):
        with pytest.raises(spa.PatternError) as e:
            spa.batchValues(m2, mb, b"abcd", kw.get("so", [0, 2, 4]), flags=kw.get("flags", BOTH))
        assert "(%d)" % SP_ERR_INVALID in str(e.value) and what in str(e.value)
    mb.doc_offsets = np.array([0, 0, 0], np.uint64)     # a result outside the documents
    with pytest.raises(spa.PatternError):
        spa.batchValues(m2, mb, b"abcd", [0, 2, 4])


def test_a_loaded_rule_set_has_the_same_values_and_the_same_blob():
    m = matcher_of(FORMATS)
    blob = m.serialize()
    m2 = spa.PatternMatcherInstance.deserialize(blob)
    assert m2.serialize() == blob
    mb = make_batch([[GOOD, (1, GOOD[1])]])
    a, b = spa.batchValues(m, mb, TEXT3[:10], [0, 10]), spa.batchValues(m2, mb, TEXT3[:10], [0, 10])
    assert a.result_values == b.result_values == b"01,45+2<01 45>"


def test_format_table_follows_a_later_compile():
    """a variable that a format names is attached only after the first compile, by a pattern without a format string: the
    counts of formats stay, the table is resolved again"""
    m = spa.PatternMatcherInstance()
    m.pushTerm(1); m.attachVariable("a"); m.pushExpression("any", 1, 1, 0); m.definePattern("p", "{a}/{late}", True)
    m.compile()
    mb = make_batch([[(1, [(1, 0, 0, (0, 0, 0, 2)), (2, 0, 0, (0, 3, 0, 5))])]])
    assert spa.batchValues(m, mb, b"ab cd", [0, 5]).result(0) == b"ab/"
    m.pushTerm(2); m.attachVariable("late"); m.pushExpression("any", 1, 1, 0); m.definePattern("q", "", True)
    assert m.variableId("late") == 2 and m.formatCount() == 1
    m.compile()
    assert spa.batchValues(m, mb, b"ab cd", [0, 5]).result(0) == b"ab/cd"


def test_stand_alone_program_under_a_sanitizer(tmp_path):
    """tests/micro/result_values_host_check.cpp with result_values.cpp and span_text.cpp under ASan and UBSan: the malformed
    batches above over arrays that are exactly as long as what they hold.  Nothing of it is loaded into Python."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "struspattern_amd", "csrc")
    exe = str(tmp_path / "result_values_host_check")
    # (a stand-alone program should not depend on where the dynamic loader puts the sanitizer runtimes: linked statically)
    gnu = "Free Software Foundation" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = ["-static-libasan", "-static-libubsan"] if gnu else []
    subprocess.check_call([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I" + csrc,
                           os.path.join(ROOT, "tests", "micro", "result_values_host_check.cpp"), os.path.join(csrc, "result_values.cpp"),
                           os.path.join(csrc, "span_text.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "result_values_host_check: ok" in p.stdout, p.stdout + p.stderr
