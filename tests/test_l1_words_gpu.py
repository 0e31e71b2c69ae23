"""GPU tests of the words kernel of the lexer (spa_l1_words_kernel_w16 / spa_l1_words_kernel: wordsUnit, wordsFlush,
confirmWalk, runStartBefore, l1_words_kernel.hip) at the edges of its runs, keys, tiles, ring and chunks.  Every case runs on
the 16-wave instance, on the 12-wave instance (SPA_L1_WORD_WAVES) and, as a control, without the kernel (the table
compiled under SPA_L1_SHAPES=0, the context created under SPA_L1_NO_WORDS_KERNEL: scan kernels and the post kernel's own
literal probe), says which kernel ran, and compares status, lexem offsets and lexems with the CPU oracle, no tolerance
anywhere; the records the kernel queued and the units of the batch are the ones tests/l1_words_model.py predicts
(tests/test_l1_words_model.py asserts on the CPU that the batches contain what they are meant to)."""
import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from tests import l1_words_cases as cases
from tests import l1_words_model as model

pytestmark = pytest.mark.gpu

MODES = ("w16", "w12", "control")
KERNEL = {"w16": "spa_l1_words_kernel_w16", "w12": "spa_l1_words_kernel"}
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
        _MODEL[key] = model.word_reports(cases.tables(name), docs, model.chunk_of(chunk))
    return _MODEL[key]


def _context(monkeypatch, name, mode, chunk):
    """a lexer compiled and a context created under the mode's switches, the chunk size set for the launches"""
    monkeypatch.delenv("SPA_L1_SHAPES", raising=False)
    monkeypatch.delenv("SPA_L1_NO_WORDS_KERNEL", raising=False)
    monkeypatch.delenv("SPA_L1_WORD_WAVES", raising=False)
    if mode == "control":
        monkeypatch.setenv("SPA_L1_SHAPES", "0")
    lx = spa.PatternLexerInstance()
    cases.build(lx, name)
    monkeypatch.delenv("SPA_L1_SHAPES", raising=False)
    if mode == "control":
        monkeypatch.setenv("SPA_L1_NO_WORDS_KERNEL", "1")
    if mode == "w12":
        monkeypatch.setenv("SPA_L1_WORD_WAVES", "1")
    if chunk is None:
        monkeypatch.delenv("SPA_L1_CHUNK_BYTES", raising=False)
    else:
        monkeypatch.setenv("SPA_L1_CHUNK_BYTES", str(chunk))
    plan = lx.launchPlan(256, 8, 4096)
    if mode == "control":
        assert plan["words_kernel"] == "(none)"
    else:
        assert plan["words_kernel"] == KERNEL[mode]
    return lx, lx.createContext(), plan


def _assert_kernel(ctx, mode):
    name = ctx.wordsKernelName()
    print("mode %s: words kernel %r, scan kernel %r" % (mode, name, ctx.scanKernelName()))
    if mode == "control":
        assert name == "(none)"
    else:
        assert name == KERNEL[mode]


def _assert_oracle(got, name, docs):
    ref, roffs = _reference(name, docs)
    assert np.array_equal(got.status, np.zeros(len(docs), np.int32))
    assert np.array_equal(got.doc_offsets, roffs)
    assert np.array_equal(got.lexems, ref)


def _assert_counters(c, name, mode, chunk, docs):
    assert c["scan_units"] == sum(model.units(len(d), model.chunk_of(chunk)) for d in docs)
    assert c["failed_docs"] == 0
    if mode != "control":
        assert c["word_reports"] == _expected_reports(name, docs, chunk)


def _check(monkeypatch, name, mode, chunk, docs):
    """the batch in this mode against the oracle and the model"""
    lx, ctx, plan = _context(monkeypatch, name, mode, chunk)
    got = ctx.matchDocs(b"".join(docs), cases.offsets(docs), check=False)
    _assert_kernel(ctx, mode)
    _assert_counters(ctx.batchCounters(), name, mode, chunk, docs)
    _assert_oracle(got, name, docs)
    return ctx, plan


@pytest.mark.parametrize("mode", MODES)
def test_literal_lengths_and_tails(mode, monkeypatch):
    """literals of 1 to 64 bytes (the compare beyond the 16 inline bytes with a rest of 1, 2, 3 and 4, the byte-wise
    loads within the last bytes of a document), twins that differ at byte 17, 20 and 64, a word in three expressions,
    a run of 65 bytes.  A table without shapes: the kernel reads its tables from global memory (wordsDocuments<false>),
    the launch plan stages no image."""
    docs = cases.edge_docs()[0]
    ctx, plan = _check(monkeypatch, "lits", mode, None, docs)
    if mode != "control":
        assert plan["word_lds_words"] == "0"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["keys", "keys_prev"])
def test_shape_keys_at_their_length_edges(name, mode, monkeypatch):
    """every variant the compiler emits (PREFIX(o,k) up to o + k = 7: keys from single bytes; SUFFIX(k) at ends below
    4), runs as long as a key's place and one byte short, lists of two and three expressions, a word that hits every
    variant and a literal at once.  The image is staged in LDS (wordsDocuments<true>)."""
    docs = cases.edge_docs()[0]
    ctx, plan = _check(monkeypatch, name, mode, None, docs)
    if mode != "control":
        assert int(plan["word_lds_words"]) > 0


@pytest.mark.parametrize("mode", MODES)
def test_more_variants_than_the_table_holds(mode, monkeypatch):
    _check(monkeypatch, "variants12", mode, None, cases.edge_docs()[0])


@pytest.mark.parametrize("mode", MODES)
def test_previous_word_across_tiles_and_at_the_document_start(mode, monkeypatch):
    _check(monkeypatch, "prev", mode, None, cases.edge_docs()[0])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chunk", cases.CHUNKS)
@pytest.mark.parametrize("name", ["keys", "lits", "prev"])
def test_run_carries_and_document_ends(name, chunk, mode, monkeypatch):
    """the edge batch in chunks of 64 and 1024 bytes (whole: the tests above): runs that start, end and straddle at the
    tile offsets, runs over two tiles and more, documents of the edge lengths that end in a word and in a separator"""
    _check(monkeypatch, name, mode, chunk, cases.edge_docs(chunk)[0])


@pytest.mark.parametrize("mode", MODES)
def test_ninety_five_waiting_ends_and_mixed_merges(mode, monkeypatch):
    _check(monkeypatch, "dense", mode, None, cases.dense_docs()[0])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chunk", [None, 1024])
def test_walks_at_the_ring_boundary(chunk, mode, monkeypatch):
    _check(monkeypatch, "ring", mode, chunk, cases.ring_docs()[0])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chunk", cases.CHUNKS)
@pytest.mark.parametrize("name", ["prev", "keys", "ring"])
def test_chunk_ownership_and_back_off(name, chunk, mode, monkeypatch):
    _check(monkeypatch, name, mode, chunk, cases.chunk_docs(chunk)[0])


def _device_batch(ctx, docs):
    import torch
    text = b"".join(docs)
    d_text = torch.frombuffer(bytearray(text + b"\0" * 16), dtype=torch.uint8).cuda()
    d_offs = torch.from_numpy(cases.offsets(docs).view(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    ctx.matchDocsDevice(d_text.data_ptr(), d_offs.data_ptr(), len(docs), len(text), stream)
    c = ctx.batchCounters()
    st = ctx.batchStatus(len(docs))
    return c, st, (d_text, d_offs)


@pytest.mark.parametrize("mode", ["w16", "w12"])
def test_word_queue_short_of_space_on_the_device_entry(mode, monkeypatch):
    """a unit that queues a record per byte and one that queues 1.75 per byte: the device entry point reports the arena
    status on exactly the documents the model names, their neighbours are what they are without them, and the batch is
    clean after growArena() -- twice for the denser one; matchDocs grows and runs again by itself.  (Not run in the
    control mode: there the same records go to the automaton's queue, which the lanes suite pins.)"""
    docs = cases.overflow_docs()[0]
    t = cases.tables("dense")
    over = [set(di for di, u in model.overflowing(t, docs, model.DEFAULT_CHUNK, m)) for m in (8, 16, 32)]
    assert len(over[0]) == 2 and len(over[1]) == 1 and not over[2]
    lx, ctx, plan = _context(monkeypatch, "dense", mode, None)
    ref, roffs = _reference("dense", docs)
    for short in over:
        c, st, keep = _device_batch(ctx, docs)
        _assert_kernel(ctx, mode)
        assert st.tolist() == [2 if i in short else 0 for i in range(len(docs))] and c["failed_docs"] == len(short)
        assert c["scan_units"] == len(docs)
        if short:
            got = ctx.batchFetch(0, len(docs))
            for di in range(len(docs)):                     # (a failed document has no lexems, the others all of theirs)
                want = ref[int(roffs[di]):int(roffs[di + 1])] if di not in short else ref[:0]
                assert np.array_equal(got.doc(di), want), di
            assert ctx.growArena()
    _assert_counters(c, "dense", mode, None, docs)
    _assert_oracle(ctx.batchFetch(0, len(docs)), "dense", docs)
    reports = c["word_reports"]
    # the host entry point: a fresh context, the retry inside
    ctx = lx.createContext()
    got = ctx.matchDocs(b"".join(docs), cases.offsets(docs))
    _assert_kernel(ctx, mode)
    _assert_oracle(got, "dense", docs)
    assert ctx.batchCounters()["word_reports"] == reports
    c, st, keep = _device_batch(ctx, docs)                  # (the queue of this context has grown: clean at once)
    assert st.tolist() == [0] * len(docs) and c["failed_docs"] == 0 and c["word_reports"] == reports


@pytest.mark.parametrize("mode", MODES)
def test_the_same_batch_twice_on_one_context(mode, monkeypatch):
    """the records of a unit are counted per unit and batch: a batch gives the same lexems and counters when it runs
    again on a context whose word queue and wordCount[] hold the records of another (smaller, differently cut) batch"""
    big = cases.edge_docs(64)[0]
    small = cases.chunk_docs(64)[0][:6]
    lx, ctx, plan = _context(monkeypatch, "keys_prev", mode, 64)
    text, offs = b"".join(big), cases.offsets(big)
    first = ctx.matchDocs(text, offs)
    c1 = ctx.batchCounters()
    _assert_kernel(ctx, mode)
    monkeypatch.setenv("SPA_L1_CHUNK_BYTES", "128")
    _assert_oracle(ctx.matchDocs(b"".join(small), cases.offsets(small)), "keys_prev", small)
    _assert_counters(ctx.batchCounters(), "keys_prev", mode, 128, small)
    monkeypatch.setenv("SPA_L1_CHUNK_BYTES", "64")
    second = ctx.matchDocs(text, offs)
    c2 = ctx.batchCounters()
    _assert_kernel(ctx, mode)
    assert np.array_equal(first.lexems, second.lexems) and np.array_equal(first.doc_offsets, second.doc_offsets) and np.array_equal(first.status, second.status)
    keys = ("lexems", "raw_reports", "scan_units", "rescanned_docs", "word_reports", "failed_docs")
    assert [c1[k] for k in keys] == [c2[k] for k in keys]
    _assert_counters(c1, "keys_prev", mode, 64, big)
    _assert_oracle(second, "keys_prev", big)
