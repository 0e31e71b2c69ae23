"""The frame around the flat-tier state machine (struspattern_amd/csrc/l2_fast_kernel.hip, runKernel() and setCurrentPos()):
what is decided once per tile of 64 lexems -- the order and range checks of putInput, the count of lexems on one position and
its hand-over, the values carried across a tile edge -- and the search for the next expiry row with rules.  Every batch runs on
spa_l2_fast_kernel_n against the CPU oracle, bit for bit, at the smallest shapes where that code can go wrong: documents around
one and two tiles, offences at lane 0, lane 63 and in the middle, runs of 60 and 61 lexems inside a tile and across an edge,
position jumps around the number of expiry rows W."""
import numpy as np
import pytest

import oracle
import struspattern_amd as spa
from struspattern_amd import synth

ORDER, RANGE = 1, 5                  # SPD_ERR_ORDER, SPD_ERR_RANGE
BIG = 0x7FFFFFFF
NOID = 99                            # a lexem id no rule mentions
KERNEL = "spa_l2_fast_kernel_n"


# ---------------------------------------------------------------- rule sets
def _rules(maxrange):
    """two-term rules over the ids 1..6, every operator of the flat tier, ranges 1..maxrange (W = the power of two above it)"""
    ops = ["sequence", "within", "any", "sequence_struct", "within_struct"]
    ranges = sorted({1, 2, 3, maxrange // 2 + 1, maxrange - 1, maxrange})
    rules = []
    for a in range(1, 7):
        for k, rg in enumerate(ranges):
            b = 1 + (a + k) % 6
            rules.append(("%s_%d_%d" % (ops[(a + k) % 5], a, rg), ops[(a + k) % 5], rg, [a, b]))
    return rules


def _burst_rules(maxrange):
    """40 rules keyed by 7 that finish on 8 (a dispose list of 40) and 40 keyed by 9 that wait three positions for 10 (an
    expiry row of 40), beside the rules of _rules()"""
    rules = _rules(maxrange)
    for i in range(40):
        rules.append(("fin_%d" % i, "sequence", 5, [7, 8]))
        rules.append(("exp_%d" % i, "sequence", 3, [9, 10]))
    return rules


def _matchers(rules, compile_=True):
    m, o = spa.PatternMatcherInstance(), oracle.L2Matcher()
    synth.apply_rules(m, rules, compile=compile_)
    synth.apply_rules(o, rules, compile=compile_)
    return m, o


# ---------------------------------------------------------------- documents
def _doc(ids, pos):
    lex = np.zeros((len(ids), 4), np.uint32)
    lex[:, 0] = ids
    lex[:, 1] = pos
    lex[:, 2] = np.arange(len(ids)) * 3
    lex[:, 3] = 2
    return lex


def _plain(n, seed, steps=(1,), first=1):
    """n lexems with ids 1..6 and a few delimiters; the position advances by one of `steps` per lexem"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, 7, size=n)
    ids[rng.random(n) < 0.08] = synth.DELIM
    st = rng.choice(list(steps), size=n)
    st[0] = first
    return _doc(ids, np.cumsum(st))


def _batch(docs, seg=None):
    offs = np.zeros(len(docs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in docs])
    lex = np.concatenate(docs)
    return lex, offs, (np.zeros(len(lex), np.uint32) if seg is None else seg)


def _between(docs, seed):
    """every document of `docs` between two complete neighbours"""
    out = [_plain(70, seed)]
    for i, d in enumerate(docs):
        out += [d, _plain(70, seed + 1 + i)]
    return out


def _tile_edge_docs():
    return [_plain(n, 200 + n + s, steps=(0, 0, 1, 1, 2), first=f) for n in (63, 64, 65, 129) for s, f in ((0, 1), (1, 0), (2, 1))]


def _order_docs():
    """a position that descends at lexem 0 of the second and of the third tile, at lane 63 and in the middle of a tile"""
    docs = []
    for at in (64, 128, 63, 30, 100):
        d = _plain(129, 300 + at)
        d[at, 1] = d[at - 1, 1] - 1
        docs.append(d)
    return docs, [ORDER] * 5


def _range_docs():
    """origpos / origsize / origseg >= 0x7FFFFFFF on a lexem that stays on the position of the one before it (error), on
    one that advances (fine), on the first lexem of a document at position 0 (stays: error) and at position 1 (fine)"""
    docs, segs, want = [], [], []
    for at, col, share in [(64, 2, True), (63, 3, True), (30, "seg", True), (65, 3, True), (64, 2, False), (63, 3, False), (30, "seg", False),
                           (0, 3, True), (0, 3, False)]:
        d = _plain(129, 400 + at + (10 if share else 0), first=(0 if (at == 0 and share) else 1))
        seg = np.zeros(len(d), np.uint32)
        d[at, 0] = NOID
        if at and share:
            d[at:, 1] -= d[at, 1] - d[at - 1, 1]
        if col == "seg":
            seg[at] = BIG
        else:
            d[at, col] = BIG
        docs.append(d)
        segs.append(seg)
        want.append(RANGE if share else 0)
    return docs, segs, want


def _id_docs():
    docs = []
    for at, val in [(64, 1 << 29), (63, 0xFFFFFFFF), (30, (1 << 29) + 5), (0, 1 << 30)]:
        d = _plain(129, 500 + at)
        d[at, 0] = val
        docs.append(d)
    return docs, [RANGE] * 4


def _two_offence_docs():
    """two offences in one tile -- the first in lexem order decides -- and two on one lexem: the order error goes first"""
    docs, want = [], []
    for first, second, status in [("id", "order", RANGE), ("order", "id", ORDER), ("field", "order", RANGE), ("order", "field", ORDER)]:
        d = _plain(129, 600 + len(docs))
        for what, at in ((first, 70), (second, 90)):
            if what == "id":
                d[at, 0] = 1 << 29
            elif what == "order":
                d[at, 1] = d[at - 1, 1] - 1
            else:
                d[at, 0] = NOID
                d[at:, 1] -= d[at, 1] - d[at - 1, 1]
                d[at, 3] = BIG
        docs.append(d)
        want.append(status)
    d = _plain(129, 610)
    d[64, 1] = d[63, 1] - 1
    d[64, 0] = 1 << 29
    d[64, 3] = BIG
    docs.append(d)
    want.append(ORDER)
    return docs, want


def _run_docs(length):
    """`length` lexems on one position: inside one tile, across the first and the second tile edge, and from the start of a
    document at position 0"""
    docs = []
    for start, n in [(2, 129), (40, 129), (0, 129), (120, 200)]:
        rng = np.random.default_rng(700 + start)
        d = _plain(n, 700 + start + length, first=(0 if start == 0 else 1))
        ids = np.full(length, NOID)
        ids[rng.choice(length, size=6, replace=False)] = rng.integers(1, 7, size=6)
        d[start:start + length, 0] = ids
        d[start:start + length, 1] = d[start, 1]
        d[start + length:, 1] = d[start, 1] + np.arange(1, n - start - length + 1)
        docs.append(d)
    return docs


def _jump_docs(W):
    """position jumps of 1, 2, W-1, W, W+1 and 300 in every order, so rules expire in rows before, at and after the wrap of the
    row index; with the burst rules: a dispose list of 40 meets an expiry row of 40 (together more than a batch of 64: the
    list goes alone, the row comes round again), followed by each of the jumps"""
    jumps = [1, 2, W - 1, W, W + 1, 300]
    docs = []
    for s in range(4):
        docs.append(_plain(150, 800 + s, steps=jumps))
    for j in jumps:
        ids, pos = [], []
        p = 1 + j % 5
        for rep in range(3):
            ids += [9, 7, 8, 1, 2, 10]
            pos += [p, p + 1, p + 2, p + 2 + j, p + 3 + j, p + 4 + j]
            p += 5 + j + W - 2 + rep
        docs.append(_doc(ids, pos))
    return docs


# ---------------------------------------------------------------- the checks
ORACLE_SAYS = {ORDER: "ascending order", RANGE: "range"}


def _reference(o, docs, segs, want):
    """The oracle's output for the documents expected to complete (it raises for a batch with a failing document), and its
    own verdict on each of the others, fed alone."""
    good = [i for i in range(len(docs)) if want[i] == 0]
    for i in range(len(docs)):
        if want[i]:
            lex, offs, seg = _batch([docs[i]], segs[i])
            l5 = synth.lexems5(lex)
            l5[:, 2] = seg
            with pytest.raises(oracle.OracleError, match=ORACLE_SAYS[int(want[i])]):
                o.run(l5, offs)
    lex, offs, seg = _batch([docs[i] for i in good], np.concatenate([segs[i] for i in good]))
    l5 = synth.lexems5(lex)
    l5[:, 2] = seg
    ref = o.run(l5, offs)
    assert (_results_per_doc(ref) > 0).all()
    return ref


def _results_per_doc(ref):
    return np.diff(ref.doc_offsets.astype(np.int64))


def _split(docs, seg):
    if seg is None:
        return [np.zeros(len(d), np.uint32) for d in docs]
    ends = np.cumsum([len(d) for d in docs])
    return np.split(seg, ends[:-1])


def _check(rules, docs, seg=None, want=None, handed_over=0, compile_=True):
    m, o = _matchers(rules, compile_)
    lex, offs, seg = _batch(docs, seg)
    ndocs = len(docs)
    want = np.zeros(ndocs, np.int32) if want is None else np.asarray(want, np.int32)
    ctx = m.createContext()
    assert ctx.kernelKind() == 1 and ctx.kernelName() == KERNEL
    gpu = ctx.matchDocs(lex, offs, seg, check=False)
    assert ctx.kernelKind() == 1 and ctx.kernelName() == KERNEL
    ref = _reference(o, docs, _split(docs, seg), want)
    assert np.array_equal(gpu.status, want)
    assert ctx.batchCounters()["handed_over"] == handed_over
    # a failing document has no results: what the batch holds is what the complete documents hold, in their order
    ok = want == 0
    per = _results_per_doc(gpu)
    assert np.array_equal(per[ok], _results_per_doc(ref)) and (per[~ok] == 0).all()
    assert np.array_equal(gpu.results[:, :7], ref.results[:, :7])
    assert np.array_equal(gpu.results[:, 8], ref.results[:, 8])
    assert np.array_equal(gpu.items, ref.items)
    assert np.array_equal(gpu.stats[ok], ref.stats)
    return gpu, ref


def _with_neighbours(docs, want, seed, segs=None):
    all_docs = _between(docs, seed)
    all_want = [0] * len(all_docs)
    all_want[1::2] = want
    seg = None
    if segs is not None:
        parts = [np.zeros(len(d), np.uint32) for d in all_docs]
        parts[1::2] = segs
        seg = np.concatenate(parts)
    return all_docs, all_want, seg


@pytest.mark.gpu
def test_documents_around_one_and_two_tiles():
    _check(_rules(7), _tile_edge_docs())


@pytest.mark.gpu
def test_descending_position_at_lane_0_lane_63_and_between():
    docs, want = _order_docs()
    docs, want, _ = _with_neighbours(docs, want, 31)
    _check(_rules(7), docs, want=want)


@pytest.mark.gpu
def test_field_out_of_range_counts_only_on_a_lexem_that_stays_on_the_position():
    docs, segs, want = _range_docs()
    docs, want, seg = _with_neighbours(docs, want, 41, segs)
    _check(_rules(7), docs, seg=seg, want=want)


@pytest.mark.gpu
def test_id_out_of_range():
    docs, want = _id_docs()
    docs, want, _ = _with_neighbours(docs, want, 51)
    _check(_rules(7), docs, want=want)


@pytest.mark.gpu
def test_first_of_two_offences_decides_and_neighbours_are_complete():
    docs, want = _two_offence_docs()
    docs, want, _ = _with_neighbours(docs, want, 61)
    _check(_rules(7), docs, want=want)


@pytest.mark.gpu
@pytest.mark.parametrize("length,handed", [(60, 0), (61, 4)])
def test_hand_over_at_61_lexems_on_one_position(length, handed):
    _check(_rules(7), _run_docs(length), handed_over=handed)


@pytest.mark.gpu
@pytest.mark.parametrize("maxrange", [7, 63])
def test_position_jumps_around_the_number_of_expiry_rows(maxrange):
    _check(_burst_rules(maxrange), _jump_docs(maxrange + 1))


def _stop_word_case():
    rules = synth.random_rules(800, 40, 125, "sequence_struct") + synth.random_rules(400, 40, 126, "within")
    lex, offs = synth.random_documents(24, 130, 40, 1125)
    docs = [lex[int(offs[d]):int(offs[d + 1])] for d in range(len(offs) - 1)]
    return rules, docs


@pytest.mark.gpu
def test_alternative_keys_and_stop_words():
    rules, docs = _stop_word_case()
    _, ref = _check(rules, docs)
    assert ref.stats[:, 1].sum() > 0            # programs installed by an alternative key: the stop-word log was read


def test_every_document_of_these_batches_has_results():
    """CPU, oracle alone: every complete document of the batches above yields results, every failing one fails in the oracle
    too and yields results without its offence -- no comparison above is one of nothing with nothing"""
    def run(rules, docs, want=None, segs=None):
        o = oracle.L2Matcher()
        synth.apply_rules(o, rules)
        segs = [np.zeros(len(d), np.uint32) for d in docs] if segs is None else segs
        return _reference(o, docs, segs, [0] * len(docs) if want is None else want)

    def clean(docs):
        out = []
        for d in docs:
            c = d.copy()
            c[:, 1] = np.maximum.accumulate(c[:, 1])
            c[c[:, 0] >= (1 << 29), 0] = NOID
            c[c[:, 2] >= BIG, 2] = 0
            c[c[:, 3] >= BIG, 3] = 2
            out.append(c)
        return out

    rules = _rules(7)
    run(rules, _tile_edge_docs())
    for docs, want in (_order_docs(), _id_docs(), _two_offence_docs()):
        docs2, want2, _ = _with_neighbours(docs, want, 1)
        run(rules, docs2, want2)
        run(rules, clean(docs))
    docs, segs, want = _range_docs()
    run(rules, docs, want, segs)
    run(rules, clean(docs))
    for length in (60, 61):
        run(rules, _run_docs(length))
    for maxrange in (7, 63):
        ref = run(_burst_rules(maxrange), _jump_docs(maxrange + 1))
        assert (_results_per_doc(ref)[4:] >= 120).all()        # the 40 fin_* rules complete three times in each burst document
    rules, docs = _stop_word_case()
    assert run(rules, docs).stats[:, 1].sum() > 0
