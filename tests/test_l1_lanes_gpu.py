"""GPU tests of the lane-per-stream scan kernel of the lexer (spa_l1_scan_lanes_kernel: scanUnitLanes /
scanDocumentsLanes, l1_scan_lanes_kernel.hip) at the edges of its pieces, of its warm-up proof and of its per-lane queue
regions.  Every case runs on the lane-per-stream kernel and, with SPA_L1_NO_LANES, on the wave-per-unit kernel, says
which kernel ran, and compares status, lexem offsets and lexems with the CPU oracle; the units of the batch, the
documents scanned again and the documents short of queue space are the ones tests/l1_lanes_model.py predicts
(tests/test_l1_lanes_model.py asserts on the CPU that the batches contain what they are meant to)."""
import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from tests import l1_lanes_cases as cases
from tests import l1_lanes_model as model

pytestmark = pytest.mark.gpu

LANES_KERNEL = "spa_l1_scan_lanes_kernel"
MODES = ("lanes", "no_lanes")
_ORACLE = {}


def _both(name):
    lx = spa.PatternLexerInstance()
    cases.build(lx, name)
    if name not in _ORACLE:
        _ORACLE[name] = oracle.L1Lexer()
        cases.build(_ORACLE[name], name)
    return lx, _ORACLE[name]


def _env(monkeypatch, mode, chunk):
    if mode == "no_lanes":
        monkeypatch.setenv("SPA_L1_NO_LANES", "1")
    else:
        monkeypatch.delenv("SPA_L1_NO_LANES", raising=False)
    if chunk is None:
        monkeypatch.delenv("SPA_L1_CHUNK_BYTES", raising=False)
    else:
        monkeypatch.setenv("SPA_L1_CHUNK_BYTES", str(chunk))


def _assert_kernel(ctx, mode, lanes_table=True):
    name = ctx.scanKernelName()
    if mode == "lanes" and lanes_table:
        assert name == LANES_KERNEL
    else:
        assert name != LANES_KERNEL and name.startswith("spa_l1_scan_kernel_p1")


def _assert_oracle(got, o, docs):
    text, offs = b"".join(docs), cases.offsets(docs)
    ref, roffs = o.matchDocs(text, offs)
    assert np.array_equal(got.status, np.zeros(len(docs), np.int32))
    assert np.array_equal(got.doc_offsets, roffs)
    assert np.array_equal(got.lexems, ref)


def _run(monkeypatch, name, mode, chunk, docs, lanes_table=True):
    """a fresh context, one batch through matchDocs under the mode's environment: (context, batch, counters)"""
    _env(monkeypatch, mode, chunk)
    lx, o = _both(name)
    ctx = lx.createContext()
    got = ctx.matchDocs(b"".join(docs), cases.offsets(docs), check=False)
    _assert_kernel(ctx, mode, lanes_table)
    return ctx, got, ctx.batchCounters()


_MODEL = {}


def _expected_rescans(name, mode, chunk, docs, lanes_table=True):
    """the documents the model sends to the sequential pass (computed once per table, kernel and batch)"""
    by_lanes = mode == "lanes" and lanes_table
    key = ("rescans", name, by_lanes, chunk, tuple(docs))
    if key not in _MODEL:
        t = cases.tables(name)
        c = model.chunk_of(chunk)
        _MODEL[key] = model.rescanned(t, docs, c) if by_lanes else model.rescanned_by_chunks(t, docs, c)
    return _MODEL[key]


def _expected_raw(name, docs):
    """the records the model's automaton queues for the batch"""
    key = ("raw", name, tuple(docs))
    if key not in _MODEL:
        t = cases.tables(name)
        _MODEL[key] = sum(len(model.scan_reports(t, d)) for d in docs)
    return _MODEL[key]


def _assert_counters(c, name, mode, chunk, docs, lanes_table=True, scanned=None):
    """units and re-scans of the batch as the model says; the raw reports are the records the model's automaton queues
    for the documents the scan kernel finished (`scanned`: all by default) -- one number for both modes, so the two
    kernels count the same"""
    assert c["scan_units"] == sum(model.units(len(d), model.chunk_of(chunk)) for d in docs)
    assert c["rescanned_docs"] == len(_expected_rescans(name, mode, chunk, docs, lanes_table))
    assert c["raw_reports"] == sum(_expected_raw(name, [d]) for i, d in enumerate(docs) if scanned is None or i in scanned)


def _check(monkeypatch, name, mode, chunk, docs, lanes_table=True):
    """the batch in this mode against the oracle and the model"""
    lx, o = _both(name)
    ctx, got, c = _run(monkeypatch, name, mode, chunk, docs, lanes_table)
    _assert_counters(c, name, mode, chunk, docs, lanes_table)
    assert c["failed_docs"] == 0
    _assert_oracle(got, o, docs)
    return ctx, c


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chunk", cases.EDGE_CHUNKS)
@pytest.mark.parametrize("name", cases.LANE_TABLES)
def test_piece_edges(name, chunk, mode, monkeypatch):
    """documents of the lengths where the piece size and the number of live lanes change, with matches planted on the
    piece boundaries (straddling one, ending at one, a character split by one, ending with the document), whole and in
    chunks of 64 bytes (four live lanes, 16 bytes each) and of 1024; tables of 1, 2, 3 and 4 scanned automaton words,
    with exception rows, with a multi-byte class"""
    docs, _ = cases.edge_docs(chunk)
    assert model.scan_words(cases.tables(name)) == cases.TABLES[name][1]
    _check(monkeypatch, name, mode, chunk, docs)


@pytest.mark.parametrize("mode", MODES)
def test_five_automaton_words_are_not_scanned_by_lanes(mode, monkeypatch):
    docs, _ = cases.edge_docs(1024)
    assert model.scan_words(cases.tables("w5")) > model.MAX_LANE_WORDS
    _check(monkeypatch, "w5", mode, 1024, docs, lanes_table=False)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chunk", [None, 1024])
def test_failed_proof_sends_the_document_to_the_sequential_pass(chunk, mode, monkeypatch):
    """digit runs of 256 bytes and more before a piece boundary: exactly the documents the model names are scanned
    again in one piece -- in a batch without a chunked document (unitStart[] and the _ch instance of the sequential
    pass have to hold there too) and in chunks of 1024 bytes (a run over a chunk boundary, a run over a piece boundary
    only) --, next to documents whose runs the warm-up can prove"""
    docs, _ = cases.proof_docs(chunk)
    ctx, c = _check(monkeypatch, "w1", mode, chunk, docs)
    if mode == "lanes":
        assert 1 <= c["rescanned_docs"] < len(docs)
    if chunk is None:
        assert c["scan_units"] == len(docs)


@pytest.mark.parametrize("mode", MODES)
def test_lexem_too_long_in_a_rescanned_document_leaves_its_neighbours_alone(mode, monkeypatch):
    """a run of 70000 digits: the document fails its proof, is scanned again and ends with the status of a lexem of
    65535 bytes or more; the documents around it are what they are without it"""
    docs, _ = cases.proof_docs(None)
    docs = list(docs[:3]) + [cases.too_long_doc()] + list(docs[3:])
    lx, o = _both("w1")
    ctx, got, c = _run(monkeypatch, "w1", mode, None, docs)
    assert c["scan_units"] == len(docs) + 2
    # (the long document fails behind the scan kernels, where the lexem is made: its records are queued and counted)
    _assert_counters(c, "w1", mode, None, docs)
    assert got.status.tolist() == [7 if i == 3 else 0 for i in range(len(docs))] and c["failed_docs"] == 1
    assert got.doc_offsets[4] == got.doc_offsets[3]
    for di, d in enumerate(docs):
        if di != 3:
            assert got.doc(di).tolist() == o.match(d).tolist(), di
    with pytest.raises(spa.PatternError):
        ctx.matchDocs(b"".join(docs), cases.offsets(docs))


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


@pytest.mark.parametrize("mode", MODES)
def test_one_lane_short_of_queue_space(mode, monkeypatch):
    """a stretch of digits that three expressions accept at every byte, inside one piece: the lane's part of the queue
    slice (1/64 of the unit's) is short although the unit as a whole has room.  The device entry point reports the
    arena status on exactly the documents the model names and is clean after growArena(); matchDocs grows and runs
    again by itself (a context it has run is clean on the device path at once)."""
    docs, _ = cases.overflow_docs()
    t = cases.tables("dense")
    lx, o = _both("dense")
    _env(monkeypatch, mode, None)
    over = model.overflowing(t, docs, model.DEFAULT_CHUNK, 8) if mode == "lanes" else set()
    ctx = lx.createContext()
    c, st, keep = _device_batch(ctx, docs)
    _assert_kernel(ctx, mode)
    assert c["scan_units"] == len(docs) and c["rescanned_docs"] == 0
    assert st.tolist() == [2 if i in over else 0 for i in range(len(docs))] and c["failed_docs"] == len(over)
    # (a unit that is short of space has queued nothing that counts)
    _assert_counters(c, "dense", mode, None, docs, scanned=set(range(len(docs))) - over)
    if mode == "lanes":
        assert len(over) == 2 and ctx.growArena()
        c, st, keep = _device_batch(ctx, docs)
        assert not model.overflowing(t, docs, model.DEFAULT_CHUNK, 16)
    assert st.tolist() == [0] * len(docs) and c["failed_docs"] == 0
    _assert_counters(c, "dense", mode, None, docs)
    _assert_oracle(ctx.batchFetch(0, len(docs)), o, docs)
    raw = c["raw_reports"]
    # the host entry point: a fresh context, the retry inside
    ctx = lx.createContext()
    got = ctx.matchDocs(b"".join(docs), cases.offsets(docs))
    _assert_kernel(ctx, mode)
    _assert_oracle(got, o, docs)
    assert ctx.batchCounters()["raw_reports"] == raw
    c, st, keep = _device_batch(ctx, docs)              # (the queue of this context has grown: clean at once)
    assert st.tolist() == [0] * len(docs) and c["failed_docs"] == 0
    # 200 dense bytes over several lanes: the queue has to grow three times
    docs2 = list(docs) + [cases.very_dense_doc()]
    ctx = lx.createContext()
    got = ctx.matchDocs(b"".join(docs2), cases.offsets(docs2))
    _assert_kernel(ctx, mode)
    _assert_counters(ctx.batchCounters(), "dense", mode, None, docs2)
    _assert_oracle(got, o, docs2)
    # a unit that is short as a whole, on either kernel (the wave-per-unit kernel stops in the middle of it): its
    # records do not count, its neighbours' do
    docs3 = list(docs) + [cases.full_unit_doc(), docs[0]]
    short = set(i for i, d in enumerate(docs3) if sum(model.lane_counts(t, d, model.DEFAULT_CHUNK).values()) > model.unit_cap(sum(len(x) for x in docs3[:i]), 0, len(d), 8))
    assert short == {len(docs)}
    ctx = lx.createContext()
    c, st, keep = _device_batch(ctx, docs3)
    _assert_kernel(ctx, mode)
    assert st.tolist() == [2 if i in over | short else 0 for i in range(len(docs3))] and c["failed_docs"] == len(over | short)
    _assert_counters(c, "dense", mode, None, docs3, scanned=set(range(len(docs3))) - over - short)


@pytest.mark.parametrize("mode", MODES)
def test_the_same_batch_twice_on_one_context(mode, monkeypatch):
    """the lanes' parts are moved to the front of the slice and counted per unit: a batch gives the same lexems when
    it runs again on a context whose queue holds the records of another (smaller, differently cut) batch"""
    big, _ = cases.edge_docs(1024)
    small, _ = cases.proof_docs(None)
    small = small[:4]
    lx, o = _both("w4")
    _env(monkeypatch, mode, 1024)
    ctx = lx.createContext()
    text, offs = b"".join(big), cases.offsets(big)
    first = ctx.matchDocs(text, offs)
    c1 = ctx.batchCounters()
    _assert_kernel(ctx, mode)
    _assert_oracle(ctx.matchDocs(b"".join(small), cases.offsets(small)), o, small)
    _assert_counters(ctx.batchCounters(), "w4", mode, 1024, small)
    second = ctx.matchDocs(text, offs)
    c2 = ctx.batchCounters()
    _assert_kernel(ctx, mode)
    assert np.array_equal(first.lexems, second.lexems) and np.array_equal(first.doc_offsets, second.doc_offsets) and np.array_equal(first.status, second.status)
    assert [c1[k] for k in ("lexems", "raw_reports", "scan_units", "rescanned_docs", "word_reports")] == [c2[k] for k in ("lexems", "raw_reports", "scan_units", "rescanned_docs", "word_reports")]
    _assert_counters(c1, "w4", mode, 1024, big)
    _assert_counters(c2, "w4", mode, 1024, big)
    _assert_oracle(second, o, big)
