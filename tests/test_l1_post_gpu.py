"""GPU tests of the cluster-per-lane handler route of the lexer's post-processing kernel (postDocumentClusters,
l1_post_kernel.hip): the merge of its two report queues, the boundaries of a view, the handler of a lane and everything it
hands back to handleReport, at every window phase (tests/l1_post_cases.py).  Every batch runs on the cluster route whole
and in chunks of 64 and 1024 bytes and, as a control, with one report after the other (SPA_L1_POST_SEQ), says which route
and which words kernel ran, and compares status, lexem offsets and lexems with the CPU oracle, no tolerance anywhere.
tests/test_l1_post_model.py asserts on the CPU, from the model's trace, which lanes and paths the batches reach."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from struspattern_amd import capi
from tests import l1_post_cases as cases
from tests import l1_post_model as model
from tests import l1_words_model as words

pytestmark = pytest.mark.gpu

MODES = {"clusters": (None, False), "sequential": (None, True), "clusters-64": (64, False), "clusters-1024": (1024, False)}     # (chunk, SPA_L1_POST_SEQ)
WORDS_KERNEL = "spa_l1_words_kernel_w16"


def _device_enum(name):
    """a value of the enum of the device counters, read from l1_device.h"""
    with open(os.path.join(os.path.dirname(spa.__file__), "csrc", "l1_device.h")) as f:
        found = re.findall(r"\b%s\s*=\s*(\d+)" % name, f.read())
    assert len(found) == 1, name
    return int(found[0])


OVER_EVENTS = _device_enum("L1C_OVER_EVENTS")      # documents whose event array was too small
COUNTERS = _device_enum("L1C_ALLOC")               # counters the context allocates
_ORACLE = {}
_REF = {}
_MODEL = {}


def _oracle(name):
    if name not in _ORACLE:
        _ORACLE[name] = oracle.L1Lexer()
        cases.build(_ORACLE[name], name)
    return _ORACLE[name]


def _reference(name, docs):
    """the oracle's (lexems, offsets) of a batch, computed once"""
    key = (name, tuple(docs))
    if key not in _REF:
        _REF[key] = _oracle(name).matchDocs(b"".join(docs), cases.offsets(docs), nthreads=8)
    return _REF[key]


def _expected_reports(name, docs, chunk):
    key = (name, tuple(docs), chunk)
    if key not in _MODEL:
        _MODEL[key] = words.word_reports(cases.tables(name), docs, words.chunk_of(chunk))
    return _MODEL[key]


def _context(monkeypatch, name, mode):
    """a lexer compiled and a context created, the mode's switches set for the launches"""
    for k in ("SPA_L1_SHAPES", "SPA_L1_NO_WORDS_KERNEL", "SPA_L1_WORD_WAVES", "SPA_L1_POST_SEQ", "SPA_L1_CHUNK_BYTES", "SPA_L1_NO_LANES"):
        monkeypatch.delenv(k, raising=False)
    chunk, seq = MODES[mode]
    if seq:
        monkeypatch.setenv("SPA_L1_POST_SEQ", "1")
    if chunk is not None:
        monkeypatch.setenv("SPA_L1_CHUNK_BYTES", str(chunk))
    lx = spa.PatternLexerInstance()
    cases.build(lx, name)
    plan = lx.launchPlan(256, 8, 4096)
    assert plan["post_clusters"] == ("0" if seq else "1") and plan["words_kernel"] == WORDS_KERNEL
    assert int(plan["chunk_bytes"]) == words.chunk_of(chunk)
    return lx, lx.createContext()


def _assert_route(ctx, mode):
    print("mode %s: words kernel %r, scan kernel %r" % (mode, ctx.wordsKernelName(), ctx.scanKernelName()))
    assert ctx.wordsKernelName() == WORDS_KERNEL


def _assert_oracle(got, name, docs):
    ref, roffs = _reference(name, docs)
    assert np.array_equal(got.status, np.zeros(len(docs), np.int32))
    assert np.array_equal(got.doc_offsets, roffs)
    assert np.array_equal(got.lexems, ref)


def _assert_counters(c, name, mode, docs, chunk=None):
    chunk = MODES[mode][0] if chunk is None else chunk
    assert c["scan_units"] == sum(words.units(len(d), words.chunk_of(chunk)) for d in docs)
    assert c["failed_docs"] == 0
    assert c["word_reports"] == _expected_reports(name, docs, chunk)


KEYS = ("lexems", "raw_reports", "scan_units", "rescanned_docs", "word_reports", "failed_docs")


def _check(monkeypatch, name, mode, docs):
    """the batch in this mode against the oracle and the model, and again on the same context behind a differently cut batch"""
    docs = list(docs)
    lx, ctx = _context(monkeypatch, name, mode)
    text, offs = b"".join(docs), cases.offsets(docs)
    first = ctx.matchDocs(text, offs, check=False)
    _assert_route(ctx, mode)
    c1 = ctx.batchCounters()
    _assert_counters(c1, name, mode, docs)
    _assert_oracle(first, name, docs)
    other = docs[3::5][:12]
    monkeypatch.setenv("SPA_L1_CHUNK_BYTES", "128")
    _assert_oracle(ctx.matchDocs(b"".join(other), cases.offsets(other), check=False), name, other)
    _assert_counters(ctx.batchCounters(), name, mode, other, 128)
    chunk = MODES[mode][0]
    if chunk is None:
        monkeypatch.delenv("SPA_L1_CHUNK_BYTES")
    else:
        monkeypatch.setenv("SPA_L1_CHUNK_BYTES", str(chunk))
    second = ctx.matchDocs(text, offs, check=False)
    c2 = ctx.batchCounters()
    assert np.array_equal(first.lexems, second.lexems) and np.array_equal(first.doc_offsets, second.doc_offsets) and np.array_equal(first.status, second.status)
    assert [c1[k] for k in KEYS] == [c2[k] for k in KEYS]


SWEEP_BATCHES = [(name, i) for name in sorted(cases.STRUCTURES) for i in range(len(cases.sweep_batches(name)))]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name,part", SWEEP_BATCHES, ids=["%s-%d" % b for b in SWEEP_BATCHES])
def test_every_structure_at_every_window_phase(name, part, mode, monkeypatch):
    """survivors on one word (5, 6, 7, 8; six deleted, six and an ignored report, six and a seventh), clusters of 62 to
    129 and 201 reports, starts and ends that tie with each other and with the carry, matches that reach behind the
    carry, a selection that moves its end, hard clusters at lane 0, in the middle, as the last and twice in a view,
    symbol lookups, ties of the two queues, the group of a split expression -- each behind 0..64 isolated words"""
    _check(monkeypatch, name, mode, cases.sweep_batches(name)[part][0])


@pytest.mark.parametrize("mode", list(MODES))
def test_documents_that_end_on_a_view(mode, monkeypatch):
    """63, 64, 65, 127, 128 and 129 live records: the view of exactly 64 is not seen as the last, its last cluster waits"""
    _check(monkeypatch, "survivors", mode, cases.ending_docs()[0])


@pytest.mark.parametrize("mode", list(MODES))
def test_one_queue_alone_and_both_merge_branches(mode, monkeypatch):
    """reports of one queue only, more live records of A than of B in a refill and the reverse, more than 64 of one queue
    in front of the other's first (the `limit` rule), the group of a split expression across the entries 63 | 64"""
    _check(monkeypatch, "merge", mode, cases.queue_docs()[0])


@pytest.mark.parametrize("mode", list(MODES))
def test_clusters_across_chunks_and_empty_slices(mode, monkeypatch):
    _check(monkeypatch, "chain", mode, cases.long_docs()[0])


def _from_device(ptr, count, dtype):
    out = np.zeros(count, dtype)
    fn = capi.lib().hipMemcpy
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert fn(out.ctypes.data, ptr, out.nbytes, 2) == 0        # hipMemcpyDeviceToHost
    return out


def _device_batch(ctx, docs):
    import torch
    text = b"".join(docs)
    d_text = torch.frombuffer(bytearray(text + b"\0" * 16), dtype=torch.uint8).cuda()
    d_offs = torch.from_numpy(cases.offsets(docs).view(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    out = ctx.matchDocsDevice(d_text.data_ptr(), d_offs.data_ptr(), len(docs), len(text), stream)
    c = ctx.batchCounters()
    st = ctx.batchStatus(len(docs))
    c["over_events"] = int(_from_device(out.d_counters, COUNTERS, np.uint64)[OVER_EVENTS])
    return c, st, (d_text, d_offs)


def _capacity_model():
    """per capacity document its records of the word queue and its model trace, computed once (the stream of records does
    not depend on the chunk size: tests/test_l1_post_model.py)"""
    if "capacity" not in _MODEL:
        t = cases.tables("capacity")
        recs = [model.records(t, d) for d in cases.capacity_docs()]
        _MODEL["capacity"] = ([sum(1 for r in rs if r.id == 1) for rs in recs], [model.trace(rs) for rs in recs])
    return _MODEL["capacity"]


@pytest.mark.parametrize("mode", list(MODES))
def test_event_array_at_its_capacity(mode, monkeypatch):
    """E = cap-3 .. cap events of isolated words.  The cluster route appends the last r < 64 events at once and asks for
    nEvents + total + 2 <= cap, with nEvents + total = E: it fails from E = cap-1 on.  The sequential route asks for
    nEvents + 2 <= cap in front of every report, nEvents = E-1 at the last: it fails from E = cap on.  So the two differ
    at E = cap-1, where the cluster route reports the arena status on a document the sequential route passes (it asks
    for room for a symbol's twin behind all it appends, not behind each event)."""
    docs = cases.capacity_docs()
    seq = MODES[mode][1]
    word_records, traces = _capacity_model()
    want = [model.event_capacity(tr, cases.CAP, "sequential" if seq else "clusters") for tr in traces]
    cap = cases.CAP
    failing = [cap, cap] if seq else [cap - 1, cap]
    assert want == [model.ARENA if i % 2 == 0 and cases.CAPACITY_EVENTS[i // 2] in failing else 0 for i in range(len(docs))]
    short = set(i for i, s in enumerate(want) if s)
    lx, ctx = _context(monkeypatch, "capacity", mode)
    ctx.reserveOutput(sum(len(d) for d in docs))
    ref, roffs = _reference("capacity", docs)
    c, st, keep = _device_batch(ctx, docs)
    _assert_route(ctx, mode)
    assert st.tolist() == want and c["failed_docs"] == len(short)
    assert (c["over_events"] != 0) == bool(short) and c["over_events"] == len(short)
    got = ctx.batchFetch(0, len(docs))
    for di in range(len(docs)):                     # (a failed document has no lexems, the others all of theirs)
        assert np.array_equal(got.doc(di), ref[int(roffs[di]):int(roffs[di + 1])] if di not in short else ref[:0]), di
    assert ctx.growArena()
    c, st, keep = _device_batch(ctx, docs)
    assert st.tolist() == [0] * len(docs) and c["over_events"] == 0 and c["failed_docs"] == 0
    # (a table without shapes: no candidate of the words kernel is dead, its records are the live ones of the model)
    assert c["word_reports"] == sum(word_records) and c["scan_units"] == sum(words.units(len(d), words.chunk_of(MODES[mode][0])) for d in docs)
    _assert_oracle(ctx.batchFetch(0, len(docs)), "capacity", docs)
    # the host entry point: a fresh context, the retry inside
    ctx = lx.createContext()
    got = ctx.matchDocs(b"".join(docs), cases.offsets(docs))
    _assert_route(ctx, mode)
    _assert_oracle(got, "capacity", docs)


@pytest.mark.parametrize("mode", list(MODES))
def test_lexem_of_65534_bytes_and_one_too_long(mode, monkeypatch):
    docs = cases.lexemsize_docs()
    assert [max(len(w) for w in d.split()) for d in docs] == [3, 65534, 3, 65535, 4]
    lx, ctx = _context(monkeypatch, "lexemsize", mode)
    got = ctx.matchDocs(b"".join(docs), cases.offsets(docs), check=False)
    _assert_route(ctx, mode)
    assert got.status.tolist() == [0, 0, 0, 7, 0]
    assert ctx.batchCounters()["failed_docs"] == 1
    for di in (0, 1, 2, 4):
        ref, roffs = _reference("lexemsize", [docs[di]])
        assert np.array_equal(got.doc(di), ref), di
    assert len(got.doc(3)) == 0
    assert int(got.doc(1)[:, 3].max()) == 65534
