"""Test utility: a pure-Python model of the lane-per-stream scan kernel of the lexer (scanUnitLanes,
l1_scan_lanes_kernel.hip) on top of tests/l1_table_sim.Tables: how a unit is cut into 64 pieces, the warm-up proof
of a piece's start state, which documents go to the sequential re-scan, how many report records a lane
writes into its part of the unit's queue slice and how large that part is.  It restates the kernel's
arithmetic, so the CPU tests can say what a GPU batch is going to exercise before it runs.  Test code
only: nothing in the product imports this."""
from tests.l1_table_sim import CTX_EDGE, M64

LANES = 64
WARM = 256                  # bytes of warm-up before a piece (SPA_L1_LANE_WARM)
DEFAULT_CHUNK = 32768       # launchLex
MAX_LANE_WORDS = 4          # planL1Launch (l1_image.cpp): the lane-per-stream route


def scan_words(t):
    """automaton words the scan kernel runs: 1 + the highest word of a pattern entry in a scanned pass"""
    words = [p["word"] for p in t.patterns if (p["word"] >> 6) < t.scan_passes]
    return 1 + max(words) if words else 0


def chunk_of(chunk_bytes):
    """the chunk size the launch uses for a value of SPA_L1_CHUNK_BYTES (None: the default)"""
    if chunk_bytes is None:
        return DEFAULT_CHUNK
    assert 64 <= chunk_bytes <= 1 << 30
    return chunk_bytes & ~63


def units(doc_len, chunk_bytes):
    return max(1, -(-doc_len // chunk_bytes))


def segments(doc_len, chunk_bytes):
    """[(seg_beg, seg_end)] of the units of a document"""
    return [(k * chunk_bytes, min(doc_len, (k + 1) * chunk_bytes)) for k in range(units(doc_len, chunk_bytes))]


def piece_bytes(span):
    return (((span + 63) >> 6) + 15) & ~15


def pieces(seg_beg, seg_end):
    """the 64 (b0, b1) of a unit, lane by lane"""
    per = piece_bytes(seg_end - seg_beg)
    out = []
    for lane in range(LANES):
        b0 = min(seg_beg + lane * per, seg_end)
        out.append((b0, min(b0 + per, seg_end)))
    return out


def _cls(t, doc, pos):
    return t.byteClass[doc[pos]]        # (no classes by code point on this kernel)


def _ctx(t, doc, pos):
    return CTX_EDGE if pos < 0 or pos >= len(doc) else t.classCtx[_cls(t, doc, pos)]


def step(t, st, cls, prevctx, inject, nwords):
    """one byte of the forward recurrence over the first nwords words of pass 0 (stepWords)"""
    out = []
    for x in range(nwords):
        s0 = st[x]
        nxt = ((s0 << 1) & M64 & t.shiftDst[x]) | (s0 & t.selfLoop[x])
        if inject:
            nxt |= t.startMask[prevctx * 64 + x]
        for e in range(t.exCount[0]):
            if s0 & t.exSrc[e * 64 + x]:
                nxt |= t.exDst[e * 64 + x]
        out.append(nxt & t.charMask[cls * 64 + x])
    return out


def run(t, doc, st, beg, end, inject, nwords):
    prevctx = _ctx(t, doc, beg - 1)
    for i in range(beg, end):
        c = _cls(t, doc, i)
        st = step(t, st, c, prevctx, inject, nwords)
        prevctx = t.classCtx[c]
    return st


def exact_state(t, doc, pos, nwords=None):
    """the state before the byte at pos, stepped from the first byte of the document"""
    n = scan_words(t) if nwords is None else nwords
    return run(t, doc, [0] * n, 0, pos, True, n)


def proof(t, doc, b0):
    """(proven, S): the start state of a piece at b0 from its warm-up, and whether the kernel trusts it (F inside S)"""
    n = scan_words(t)
    q = b0 - WARM if b0 > WARM else 0
    S = run(t, doc, [0] * n, q, b0, True, n)
    if q == 0:
        return True, S                  # the warm-up started at the document's first byte
    F = run(t, doc, [M64] * n, q, b0, False, n)
    return all((F[x] & ~S[x]) == 0 for x in range(n)), S


def proven(t, doc, b0):
    """proof(..)[0], without the S warm-up where F dies out on the way (without starts an empty F stays empty)"""
    if b0 <= WARM:
        return True
    n = scan_words(t)
    F = [M64] * n
    prevctx = _ctx(t, doc, b0 - WARM - 1)
    for i in range(b0 - WARM, b0):
        c = _cls(t, doc, i)
        F = step(t, F, c, prevctx, False, n)
        prevctx = t.classCtx[c]
        if not any(F):
            return True
    return proof(t, doc, b0)[0]


def unproven_pieces(t, doc, chunk_bytes):
    """[(unit of the document, lane)] of the non-empty pieces whose proof fails"""
    out = []
    for u, (sb, se) in enumerate(segments(len(doc), chunk_bytes)):
        for lane, (b0, b1) in enumerate(pieces(sb, se)):
            if b0 < b1 and b0 > 0 and not proven(t, doc, b0):
                out.append((u, lane))
    return out


def rescanned(t, docs, chunk_bytes):
    """the documents the lane-per-stream kernel hands to the sequential pass"""
    return set(di for di, d in enumerate(docs) if unproven_pieces(t, d, chunk_bytes))


def rescanned_by_chunks(t, docs, chunk_bytes):
    """the same of the wave-per-unit kernel (scanDocument): only the start of a later chunk needs a proof"""
    return set(di for di, d in enumerate(docs) if any(sb and not proven(t, d, sb) for sb, _ in segments(len(d), chunk_bytes)))


def scan_reports(t, doc):
    """[(to, patterns entry)] of the records the scan kernel writes for a document, in (to, word, bit) order: one per
    entry with an accepting position in the state before the byte at `to`"""
    n = scan_words(t)
    by_word = [[(pi, p["mask"]) for pi, p in enumerate(t.patterns) if p["word"] == x] for x in range(n)]
    out = []
    st = [0] * n
    prevctx = CTX_EDGE
    for i in range(len(doc) + 1):
        ctx = _ctx(t, doc, i)
        if len(doc):
            for x in range(n):
                acc = st[x] & t.acceptMask[ctx * 64 + x]
                out.extend((i, pi) for pi, m in sorted(by_word[x], key=lambda e: e[1] & -e[1]) if acc & m)
        if i < len(doc):
            c = _cls(t, doc, i)
            st = step(t, st, c, prevctx, True, n)
            prevctx = ctx
    return out


def lane_counts(t, doc, chunk_bytes):
    """{(unit of the document, lane): records}: what every lane writes into its part of the queue slice"""
    reps = [to for to, _ in scan_reports(t, doc)]
    out = {}
    for u, (sb, se) in enumerate(segments(len(doc), chunk_bytes)):
        pcs = pieces(sb, se)
        for lane, (b0, b1) in enumerate(pcs):
            n = sum(1 for to in reps if b0 <= to < b1)
            if se == len(doc) and b1 == se and b0 < b1:
                n += sum(1 for to in reps if to == len(doc))       # the lane that holds the document's last byte
            out[(u, lane)] = n
    return out


def region_cap(doc_beg, seg_beg, seg_end, queue_mul):
    """records a lane's part of the unit's queue slice holds (queueBase: queue_mul/16 records per text byte + 64 per unit)"""
    lo = ((doc_beg + seg_beg) * queue_mul) >> 4
    hi = (((doc_beg + seg_end) * queue_mul) >> 4) + 64
    return (hi - lo) >> 6


def unit_cap(doc_beg, seg_beg, seg_end, queue_mul):
    """records the whole queue slice of a unit holds"""
    return ((((doc_beg + seg_end) * queue_mul) >> 4) + 64) - (((doc_beg + seg_beg) * queue_mul) >> 4)


def overflowing(t, docs, chunk_bytes, queue_mul):
    """the documents with a lane that writes more records than its part holds"""
    out = set()
    beg = 0
    for di, d in enumerate(docs):
        counts = lane_counts(t, d, chunk_bytes)
        for u, (sb, se) in enumerate(segments(len(d), chunk_bytes)):
            cap = region_cap(beg, sb, se, queue_mul)
            if any(counts[(u, lane)] > cap for lane in range(LANES)):
                out.add(di)
        beg += len(d)
    return out
