"""Test utility: a pure-Python model of the words kernel of the lexer (wordsUnit, wordsFlush, confirmWalk and
runStartBefore, l1_words_kernel.hip) on top of tests/l1_table_sim.Tables: where a unit begins after its back-off, which run
ends it owns, the candidates of an end (the whole-word literal and one key per shape variant), the records it queues
(with the leftmost start and the dead mark of the confirming walk), how many ends wait from tile to tile, when a batch
of them is flushed and whether a walk leaves the ring.  It restates the kernel's arithmetic, so the CPU tests can say
what a GPU batch is going to exercise before it runs.  The fingerprint of the compact shape table is not modelled: the
CPU test asserts once that no key of the fixed inputs collides (fingerprint_collisions).  Test code only: nothing in
the product imports this."""
from tests.l1_lanes_model import DEFAULT_CHUNK, chunk_of, segments, unit_cap, units       # noqa: F401 (shared with the lanes model)
from tests.l1_table_sim import CTX_EDGE

TILE = 64
RING = 512                  # WORD_RING
ENDS = 96                   # WORD_ENDS
MAX_VARIANTS = 8            # SHAPE_MAXVARIANTS
BACK_OFF = 160              # wordsUnit: bytes before the unit it begins at
PRESSURE = RING - 192       # a batch is flushed when the oldest end waits for more than this many bytes
RUN_CAP = 65                # runLen saturates here; 64 is the longest word a literal or PREVWORD key takes
PREFIX, SUFFIX, PREVWORD = 1, 2, 3
M32 = 0xFFFFFFFF
LITHASH_MUL = 0x9E3779B1


# ---------------------------------------------------------------- hashes (l1_tables.h)
def _mix(h):
    h ^= h >> 16
    h = (h * 0x7feb352d) & M32
    h ^= h >> 15
    h = (h * 0x846ca68b) & M32
    h ^= h >> 16
    return h or 1


def word_hash(word):
    """literalHashFinish of the polynomial hash of a word: the key of a PREVWORD shape"""
    h = 0
    for b in word:
        h = (h * LITHASH_MUL + b + 1) & M32
    return _mix(h)


def shape_fingerprint(tag, key, salt):
    return _mix((((key ^ salt) * 0x85EBCA6B) + tag * 0xC2B2AE35) & M32)


def shape_salt(t):
    """the salt the compiler settles on: the first one that makes the fingerprints of the table's keys unique"""
    for salt in range(1002):
        if len(set(shape_fingerprint(tag, key, salt) for tag, key in t.shapes)) == len(t.shapes):
            return salt
    raise AssertionError("no salt")


# ---------------------------------------------------------------- the table
def variants(t):
    """the variants the kernel probes at every end: one per (kind, place, length), PREVWORD whatever the length"""
    return sorted(set(PREVWORD if (tag & 3) == PREVWORD else tag for tag, _ in t.shapes))


def variant_fields(var):
    return var & 3, (var >> 2) & 3, (var >> 4) & 7         # kind, offset, length


def is_word(t, b):
    return t.classCtx[t.byteClass[b]] == 0


def _ctx(t, doc, pos):
    return CTX_EDGE if pos < 0 or pos >= len(doc) else t.classCtx[t.byteClass[doc[pos]]]


# ---------------------------------------------------------------- runs and ends
def runs(t, doc, beg=0):
    """[(from, to)] of the maximal runs of word characters of doc[beg:]"""
    out = []
    i, n = beg, len(doc)
    while i < n:
        if is_word(t, doc[i]):
            j = i
            while j < n and is_word(t, doc[j]):
                j += 1
            out.append((i, j))
            i = j
        else:
            i += 1
    return out


def run_ends(t, doc, beg=0):
    """(to, from, length, prev_len, prev_hash_ok) per maximal run of doc[beg:]: the lengths saturate at 65; the word
    before is the run that ends exactly one byte before this one starts, its hash counts at a length of 1..64"""
    out = []
    last = None
    for frm, to in runs(t, doc, beg):
        plen = 0
        if last is not None and last[1] == frm - 1 and frm >= 2:
            plen = min(last[1] - last[0], RUN_CAP)
        out.append((to, frm, min(to - frm, RUN_CAP), plen, 1 <= plen <= 64))
        last = (frm, to)
    return out


def run_start_before(t, doc, pos):
    """runStartBefore: start of the run byte pos-1 belongs to"""
    while pos > 0 and is_word(t, doc[pos - 1]):
        pos -= 1
    return pos


def back_off(t, doc, seg_beg):
    """(w0, steps): where the unit begins -- 160 bytes before it, then at the start of a run, then one run further
    back when that one could be the word before a run of the unit; steps = which runStartBefore steps were taken"""
    w0 = seg_beg - BACK_OFF if seg_beg > BACK_OFF else 0
    steps = []
    if w0 > 0 and is_word(t, doc[w0 - 1]):
        w0 = run_start_before(t, doc, w0)
        steps.append(1)
    if w0 >= 2 and is_word(t, doc[w0 - 2]):
        w0 = run_start_before(t, doc, w0 - 1)
        steps.append(2)
    return w0, steps


def owner(to, doc_len, chunk):
    """the unit of its document that emits the end at `to`: to in [segBeg, segEnd), and the last unit the end at
    to == segEnd == len"""
    segs = segments(doc_len, chunk)
    for u, (sb, se) in enumerate(segs):
        if sb <= to < se or (to == se and se == doc_len):
            return u
    raise AssertionError("no owner")


# ---------------------------------------------------------------- candidates of an end
def shape_key(doc, end, var):
    """(tag, key) the kernel looks up for a variant at an end, None where the run is too short for it"""
    to, frm, ln, plen, pok = end
    kind, o, k = variant_fields(var)
    if kind == PREVWORD:
        if not pok:
            return None
        return PREVWORD | (plen << 8), word_hash(doc[frm - 1 - plen:frm - 1])
    if kind == PREFIX:
        if ln < o + k:
            return None
        return var, int.from_bytes(doc[frm + o:frm + o + k], "little")
    if ln < k:
        return None
    return var, int.from_bytes(doc[to - k:to], "little")


def candidate_lists(t, doc, end):
    """the lists an end hits: [literal list or None] + [shape list or None per variant]"""
    to, frm, ln, plen, pok = end
    out = [t.literals.get(bytes(doc[frm:to])) if t.literals and ln <= 64 else None]
    for var in variants(t):
        tk = shape_key(doc, end, var)
        out.append(t.shapes.get(tk) if tk else None)
    return out


def candidates(t, doc, end):
    """the ordered (pattern, is_literal) of an end: by pattern index, as wordsFlush writes them"""
    ls = candidate_lists(t, doc, end)
    out = [(p, True) for p in (ls[0] or [])]
    for l in ls[1:]:
        out.extend((p, False) for p in (l or []))
    return sorted(out, key=lambda c: (c[0], not c[1]))


def missed_keys(t, doc, end):
    """the (tag, key) an end looks up that the table does not hold (what a fingerprint could collide on)"""
    out = []
    for var in variants(t):
        tk = shape_key(doc, end, var)
        if tk and tk not in t.shapes:
            out.append(tk)
    return out


def fingerprint_collisions(t, docs):
    """the text keys of the documents whose fingerprint equals that of a key of the table they are not"""
    salt = shape_salt(t)
    held = set(shape_fingerprint(tag, key, salt) for tag, key in t.shapes)
    out = set()
    for d in docs:
        for e in run_ends(t, d):
            out.update(tk for tk in missed_keys(t, d, e) if shape_fingerprint(tk[0], tk[1], salt) in held)
    return out


def literal_probe(t, doc, end):
    """how the literal compare of an end reads the text, None without a probe: `first16_bytewise` (the word lies within
    the last 16 bytes of the document), and for a word the table holds `rems` (pLen - k of the k = 16, 20, .. steps)
    and `tail_bytewise` (a step whose four bytes would reach behind the document)"""
    to, frm, ln, plen, pok = end
    if not t.literals or ln > 64:
        return None
    hit = bytes(doc[frm:to]) in t.literals
    ks = list(range(16, ln, 4)) if hit else []
    return dict(hit=hit, first16_bytewise=frm + 16 > len(doc), rems=[ln - k for k in ks], tail_bytewise=any(frm + k + 4 > len(doc) for k in ks))


# ---------------------------------------------------------------- the confirming walk
def walk(t, doc, pi, to, ring_lo=0):
    """confirmWalk of patterns entry pi from the end offset `to`: (leftmost start, dead, left the ring)"""
    pat = t.patterns[pi]
    w = pat["word"]
    p, ln = divmod(w, 64)
    C = t.nofClasses
    R = pat["mask"] & t.acceptMask[(p * 4 + _ctx(t, doc, to)) * 64 + ln] & t.charMask[(p * C + t.byteClass[doc[to - 1]]) * 64 + ln]
    if not R:
        return to, True, False
    frm, j, left = to, to, False
    shift, loop = t.shiftDst[w], t.selfLoop[w]
    while R and j > 0:
        if j >= 2 and j - 2 < ring_lo:
            left = True                                     # (from here on leftmostStart does the same steps from global memory)
        if R & t.startMask[(p * 4 + _ctx(t, doc, j - 2)) * 64 + ln]:
            frm = j - 1
        if j == 1:
            break
        Rp = ((R & shift) >> 1) | (R & loop)
        for e in range(t.exCount[p]):
            at = (p * t.E + e) * 64 + ln
            if R & t.exDst[at]:
                Rp |= t.exSrc[at]
        R = Rp & pat["mask"] & t.charMask[(p * C + t.byteClass[doc[j - 2]]) * 64 + ln]
        j -= 1
    return frm, frm == to, left


# ---------------------------------------------------------------- a unit: the collection loop of wordsUnit
def unit_trace(t, doc, seg_beg, seg_end):
    """the unit as wordsUnit runs it: dict of
       w0, steps        where it begins (back_off)
       ends             the ends it owns, in order
       max_waiting      the most ends that wait after a tile (the occupancy of the array of WORD_ENDS entries)
       flushes          per wordsFlush: dict(count, pressure, ring_lo, lanes: candidates per end, total,
                        walks: [(to, pattern, left the ring)]), in order
       records          [(to, pattern, from, dead)] as queued, in order"""
    n = len(doc)
    w0, steps = back_off(t, doc, seg_beg)
    seen = run_ends(t, doc, w0)
    owned = [e for e in seen if (seg_beg <= e[0] < seg_end) or (e[0] == seg_end and seg_end == n)]
    out = dict(w0=w0, steps=steps, ends=owned, max_waiting=0, flushes=[], records=[])
    waiting = []
    first_tile = 0

    def flush(batch, pressure, ring_lo):
        lanes, walks = [], []
        for e in batch:
            cs = candidates(t, doc, e)
            lanes.append(len(cs))
            for pi, lit in cs:
                if lit:
                    out["records"].append((e[0], pi, e[1], False))
                else:
                    frm, dead, left = walk(t, doc, pi, e[0], ring_lo)
                    walks.append((e[0], pi, left))
                    out["records"].append((e[0], pi, frm, dead))
        out["flushes"].append(dict(count=len(batch), pressure=pressure, ring_lo=ring_lo, lanes=lanes, total=sum(lanes), walks=walks))

    at = 0
    tile = w0
    while tile <= n and tile <= seg_end:
        new = []
        while at < len(owned) and owned[at][0] < tile + TILE:
            new.append(owned[at])
            at += 1
        if new:
            if not waiting:
                first_tile = tile
            waiting.extend(new)
        out["max_waiting"] = max(out["max_waiting"], len(waiting))
        assert len(waiting) < ENDS
        pressure = bool(waiting) and tile + TILE - first_tile > PRESSURE
        while len(waiting) >= 64 or (pressure and waiting):
            ring_lo = tile + TILE - RING if tile + TILE > w0 + RING else w0
            flush(waiting[:64], len(waiting) < 64, ring_lo)
            waiting = waiting[64:]
            first_tile = tile
        tile += TILE
    assert at == len(owned)
    if waiting:
        flush(waiting, False, tile - RING if tile > w0 + RING else w0)
    return out


def flush_trace(t, doc, chunk):
    """unit_trace of every unit of a document"""
    return [unit_trace(t, doc, sb, se) for sb, se in segments(len(doc), chunk)]


def records(t, doc, chunk):
    """per unit of the document the records the kernel queues: [(to, pattern, from, dead)]"""
    return [u["records"] for u in flush_trace(t, doc, chunk)]


def word_reports(t, docs, chunk):
    """the records the words kernel queues for a batch, dead candidates included"""
    return sum(len(r) for d in docs for r in records(t, d, chunk))


def overflowing(t, docs, chunk, queue_mul):
    """{(document, unit of the document)} whose records do not fit the unit's slice of the word queue (the kernel fails
    at the first flush whose cumulative count is above the slice: the count only grows, so that is total > cap)"""
    out = set()
    beg = 0
    for di, d in enumerate(docs):
        for u, ((sb, se), recs) in enumerate(zip(segments(len(d), chunk), records(t, d, chunk))):
            if len(recs) > unit_cap(beg, sb, se, queue_mul):
                out.add((di, u))
        beg += len(d)
    return out


# ---------------------------------------------------------------- the table as a whole, for the completeness check
def automaton_reports(t, doc, scanned_only):
    """[(patterns entry, from, to)] of the automaton passes of the table (the scanned ones only, or all of them) and,
    with all of them, of the whole-word literals, in (to, entry) order: what Tables.raw_reports runs, restricted to the
    words in use (no classes by code point, no empty matches: the tables of the words kernel)"""
    assert not t.cpBlocks and not t.ucp and not t.nullable
    npass = t.scan_passes if scanned_only else t.nofPasses
    by_word = {}
    for pi, p in enumerate(t.patterns):
        if p["word"] != M32 and (p["word"] >> 6) < npass:
            by_word.setdefault(p["word"], []).append((pi, p["mask"]))
    C = t.nofClasses
    words = sorted(by_word)
    state = dict((w, 0) for w in words)
    out = []
    prevctx = CTX_EDGE
    n = len(doc)
    for i in range(n + 1):
        ctx = _ctx(t, doc, i)
        cls = t.byteClass[doc[i]] if i < n else 0
        for w in words:
            st = state[w]
            p, ln = divmod(w, 64)
            acc = st & t.acceptMask[(p * 4 + ctx) * 64 + ln]
            if acc:
                for pi, m in by_word[w]:
                    if acc & m:
                        out.append((pi, t.som(doc, pi, i, acc & m), i))
            if i < n:
                nxt = ((st << 1) & t.shiftDst[w]) | (st & t.selfLoop[w]) | t.startMask[(p * 4 + prevctx) * 64 + ln]
                for e in range(t.exCount[p]):
                    at = (p * t.E + e) * 64 + ln
                    if st & t.exSrc[at]:
                        nxt |= t.exDst[at]
                state[w] = nxt & t.charMask[(p * C + cls) * 64 + ln]
        prevctx = ctx
    if not scanned_only:
        for frm, to in runs(t, doc):
            out.extend((pi, frm, to) for pi in t.literals.get(bytes(doc[frm:to]), []))
    out.sort(key=lambda r: (r[2], r[0]))
    return out


def by_definition(t, reports):
    """(definition 1-based, from, to) of (patterns entry, from, to), in (to, definition) order"""
    return sorted(((t.patterns[pi]["defIndex"] + 1, frm, to) for pi, frm, to in reports), key=lambda r: (r[2], r[0]))


def merged_reports(t, doc, chunk):
    """what the post kernel merges for a document: the live records of the words kernel of every unit and the reports
    of the scanned passes, as (definition, from, to) in (to, definition) order"""
    live = [(pi, frm, to) for recs in records(t, doc, chunk) for to, pi, frm, dead in recs if not dead]
    return by_definition(t, live + automaton_reports(t, doc, True))
