"""Constructed inputs that put the join kernel of result-set mode (csrc/l2_join_kernel.hip, l2_join.h, l2_join_tables.cpp)
on the edges of its own mechanics: the 64-lexem chunks and the prefix carried across them, the packed per-lexem count
`matches | items << 16` and its limit of 0x7FFF, the count array of the counting pass (countsCapacity), the two-step output
reservation, the open-addressing pair table with its LDS filter, the input checks, the predicate at its boundaries, the
keys the optimizer moved (JOIN_ALT_*), segments and format strings.

Every builder returns (build(m), lex4, offs, origseg, claims): `build` drives an oracle.L2Matcher or the product's
PatternMatcherInstance, lex4 is (n,4) u32 [id, ordpos, origpos, origsize], `claims` names the numbers the case exists to
produce.  tests/test_l2_join_cases.py recomputes every claim from tests/result_set_model.py and the oracle and holds it to
the kernel's constants; tests/test_l2_join_edges_gpu.py runs the cases on the GPU."""
import itertools
from collections import Counter

import numpy as np

import oracle
from struspattern_amd import synth

from .result_set_model import ALT_LINGER, ALT_REPLAY, ALT_SEQ, SELF, _pair_count, join_rules, results_multiset

# the kernel's constants (csrc/l2_join.h, l2_join_kernel.hip)
LANES = 64                      # lexems per chunk of a document
COUNT_MAX = 0x7FFF              # JOIN_COUNT_MAX: matches that may end at one lexem
FILTER_BITS = 4096 * 32         # JOIN_FILTER_WORDS x 32
JOIN_SELF = 0xFFFFFFFF
SP_DOC_ERR_ORDER, SP_DOC_ERR_RANGE, SP_DOC_ERR_OUTPUT = 1, 5, 9

FILLER = 7                      # a lexem no rule mentions
DEL = 9                         # the delimiter of the *_struct rules
A, B, C, D, E, F, G, H, I = range(11, 20)
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- the table, restated
def join_hash(first, second):
    """joinHash of csrc/l2_join.h (ints, or numpy uint64 arrays for `first`)"""
    h = ((first * 0x9E3779B1) & M32) ^ ((((second + 0x7F4A7C15) & M32) * 0x85EBCA6B) & M32)
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & M32
    h ^= h >> 12
    return h


def filter_bit(first, second):
    return (join_hash(first, second) >> 8) % FILTER_BITS


def table_size(nkeys):
    """the sizing rule of buildJoinTables"""
    size = 1
    while size < nkeys * 2 + 1:
        size <<= 1
    return size


def join_keys(rules):
    """the pair keys of the join entries of tests/result_set_model.join_rules"""
    return sorted(set((JOIN_SELF if r.kind == SELF else r.first, r.second) for r in rules))


def build_table(keys):
    """slot -> key (or None), filled as buildJoinTables does: keys ascending, linear probing"""
    size = table_size(len(keys))
    slots = [None] * size
    for k in sorted(keys):
        s = join_hash(*k) & (size - 1)
        while slots[s] is not None:
            s = (s + 1) & (size - 1)
        slots[s] = k
    return slots


def probe(slots, key):
    """the slots the kernel reads for `key`, in order: up to the key or to an empty slot"""
    mask = len(slots) - 1
    s = join_hash(*key) & mask
    seen = []
    for _ in range(len(slots)):
        seen.append(s)
        if slots[s] is None or slots[s] == key:
            break
        s = (s + 1) & mask
    return seen


# ---------------------------------------------------------------- helpers
def _rule(m, name, op, terms, rng, variables=(), fmt=""):
    n = len(terms)
    if op.endswith("_struct"):
        m.pushTerm(DEL)
        n += 1
    for i, t in enumerate(terms):
        m.pushTerm(t)
        if i in variables:
            m.attachVariable("v%d" % i)
    m.pushExpression(op, n, rng, 0)
    m.definePattern(name, fmt, True)


def _batch(docs, seg_every=0):
    """docs: lists of (id, ordpos) or (id, ordpos, origpos, origsize) -> lex4, offs, origseg"""
    rows, offs, seg = [], [0], []
    for doc in docs:
        for i, lx in enumerate(doc):
            rows.append(tuple(lx) if len(lx) == 4 else (lx[0], lx[1], 3 * i, 2))
            seg.append(i // seg_every if seg_every else 0)
        offs.append(len(rows))
    return np.array(rows, np.uint32).reshape(-1, 4), np.array(offs, np.uint64), np.array(seg, np.uint32)


def _plain_doc(n, pairs, extra=()):
    """n lexems on the positions 1..n: fillers, (A, B) on the lexems (i, i+1) of `pairs`, `extra` (index, id) on top"""
    doc = [(FILLER, i + 1) for i in range(n)]
    for i in pairs:
        doc[i], doc[i + 1] = (A, i + 1), (B, i + 2)
    for i, t in extra:
        doc[i] = (t, i + 1)
    return doc


def lexems5(lex4, seg):
    l5 = synth.lexems5(lex4)
    l5[:, 2] = seg
    return l5


class Reference:
    """the oracle's output per document: status (0, or the SP_DOC_* code of the message the oracle fails the document
    with), the multiset of results with their items, the numbers of results and items"""

    def __init__(self, o, lex4, offs, seg):
        l5 = lexems5(lex4, seg)
        ndocs = len(offs) - 1
        self.status = np.zeros(ndocs, np.int32)
        try:
            whole = o.run(l5, offs)
            parts = [(whole, d) for d in range(ndocs)]
        except oracle.OracleError:
            parts = []
            for d in range(ndocs):          # the oracle stops a batch at its first bad document: one by one
                try:
                    parts.append((o.run(l5[int(offs[d]):int(offs[d + 1])], [0, int(offs[d + 1] - offs[d])]), 0))
                except oracle.OracleError as e:
                    self.status[d] = SP_DOC_ERR_ORDER if "ascending order" in str(e) else SP_DOC_ERR_RANGE
                    assert self.status[d] == SP_DOC_ERR_ORDER or "out of range" in str(e), str(e)
                    parts.append(None)
        self.multisets, self.nresults, self.nitems = [], [], []
        for p in parts:
            ms = results_multiset(*p) if p else Counter()
            self.multisets.append(ms)
            self.nresults.append(sum(ms.values()))
            self.nitems.append(sum(k[7] * v for k, v in ms.items()))

    def failing(self, doc, code):
        """the document fails in result-set mode alone (the limit of csrc/l2_join.h): empty, with `code`"""
        self.status[doc] = code
        self.multisets[doc], self.nresults[doc], self.nitems[doc] = Counter(), 0, 0
        return self


def model_pairs(rules, delimiter, lex):
    """(i, x, rule, multiplicity) of every matching pair of one document, i == x for the `any` entries; as
    result_set_model.document_results counts them"""
    byself, bypair, maxrange = {}, {}, 0
    for r in rules:
        if r.kind == SELF:
            byself.setdefault(r.second, []).append(r)
        else:
            bypair.setdefault((r.first, r.second), []).append(r)
            maxrange = max(maxrange, r.range)
    out = []
    for x, lx in enumerate(lex):
        for r in byself.get(lx[0], ()):
            out.append((x, x, r, 1))
        for i in range(x - 1, -1, -1):
            if lex[i][1] + maxrange < lx[1]:
                break
            seen = {}
            for r in bypair.get((lex[i][0], lx[0]), ()):
                sig = (r.kind, r.range, r.struct)
                if sig not in seen:
                    seen[sig] = _pair_count(r, lex, i, x, delimiter)
                if seen[sig]:
                    out.append((i, x, r, seen[sig]))
    return out


# ---------------------------------------------------------------- chunk geometry
GEOMETRY_SIZES = [0, 0, 1, 63, 64, 65, 0, 127, 128, 129, 200, 200, 0]


def _geometry_build(m):
    _rule(m, "ab", "sequence", [A, B], 3, variables=(0, 1))
    _rule(m, "cd", "within", [C, D], 2, variables=(0,))
    _rule(m, "ac", "sequence_struct", [A, C], 4)
    _rule(m, "ef", "any", [E, F], 1, variables=(0,))


def _geometry_docs():
    return [
        [], [], [(E, 1)],
        _plain_doc(63, [10, 61]),
        _plain_doc(64, [62], [(20, C), (22, D)]),
        _plain_doc(65, [63]),
        [],
        _plain_doc(127, [63, 125]),
        _plain_doc(128, [63, 126]),
        _plain_doc(129, [63, 127], [(1, E)]),
        # matches in every chunk, one pair across each chunk end; a delimiter between A and C
        _plain_doc(200, [5, 63, 100, 127, 150, 191, 198], [(30, C), (31, D), (140, A), (141, DEL), (143, C)]),
        # nothing ends in the chunk 64..127
        _plain_doc(200, [5, 40, 130, 195]),
        [],
    ]


def chunk_geometry():
    lex4, offs, seg = _batch(_geometry_docs())
    claims = {
        "lexems_per_document": list(GEOMETRY_SIZES),
        "matches_crossing_a_chunk_end": [(5, 63, 64), (7, 63, 64), (8, 63, 64), (9, 63, 64), (9, 127, 128), (10, 63, 64), (10, 127, 128), (10, 191, 192)],
        "matches_per_chunk_of_the_long_documents": [[2, 2, 2, 2], [2, 0, 1, 1]],
    }
    return _geometry_build, lex4, offs, seg, claims


def single_document():
    lex4, offs, seg = _batch([_plain_doc(70, [10, 63])])
    return _geometry_build, lex4, offs, seg, {"lexems_per_document": [70], "matches_crossing_a_chunk_end": [(0, 63, 64)]}


DEFAULT_WAVES = 256 * 32        # what the launch plan gives a device of 256 compute units (join_blocks of a large batch)


def more_docs_than_waves(waves=DEFAULT_WAVES):
    """tiny documents of one match each, more than twice as many as the launch has waves: every wave takes several"""
    ndocs = 2 * waves + 5
    docs = [[(A, 1), (B, 2)] if d % 2 else [(FILLER, 1), (A, 2), (B, 3)] for d in range(ndocs)]
    lex4, offs, seg = _batch(docs)
    return _geometry_build, lex4, offs, seg, {"documents": ndocs, "waves": waves, "matches_per_document": [1, 1]}


# ---------------------------------------------------------------- count limit
def _count_limit(nrules, nfirst):
    def build(m):
        for r in range(nrules):
            _rule(m, "p%d" % r, "sequence", [A, B], nfirst, variables=(0, 1))
        _rule(m, "cd", "within", [C, D], 2, variables=(0,))

    peak = [(A, p + 1) for p in range(nfirst)] + [(B, nfirst + 1)]
    side = [(FILLER, 1), (A, 2), (B, 3), (C, 4), (D, 5), (FILLER, 6)]
    lex4, offs, seg = _batch([side, peak, side])
    claims = {"peak_matches_at_one_lexem": nrules * nfirst, "peak_items_at_one_lexem": 2 * nrules * nfirst, "lexems_of_the_peak_document": nfirst + 1}
    return build, lex4, offs, seg, claims


def count_limit_32767():
    return _count_limit(217, 151)


def count_limit_32768():
    return _count_limit(256, 128)


def count_limit_66000():
    return _count_limit(300, 220)


# the documents that fail in result-set mode alone: case -> {document: status}
FAILING = {"count_limit_32768": {1: SP_DOC_ERR_RANGE}, "count_limit_66000": {1: SP_DOC_ERR_RANGE}}


# ---------------------------------------------------------------- count array
GAP = [(A, 1), (B, 2), (A, 3), (B, 4), (C, 5)]     # unused lexems between the ranges: they would match if they were read


def scattered(lex4, offs):
    """the documents of a batch as hand-made (first, count) ranges of a larger lexem buffer: not ascending, gaps between
    them -> (buffer (n,4), ranges (ndocs,2) u64, hints): nlexems_hint = 0 (every document counted twice), inside the
    range of one document (a mix), the exact end of the last range (every count stored)"""
    ndocs = len(offs) - 1
    order = list(range(ndocs))[::-1]
    order = order[3:] + order[:3]
    gap, _, _ = _batch([GAP])
    parts, ranges, at = [gap], np.zeros((ndocs, 2), np.uint64), len(gap)
    for d in order:
        doc = lex4[int(offs[d]):int(offs[d + 1])]
        ranges[d] = (at, len(doc))
        parts += [doc, gap]
        at += len(doc) + len(gap)
    longest = int(np.argmax(ranges[:, 1]))
    end = int((ranges[:, 0] + ranges[:, 1]).max())
    return np.concatenate(parts), ranges, [0, int(ranges[longest, 0] + ranges[longest, 1] // 2), end]


def count_array():
    lex4, offs, seg = _batch(_geometry_docs())
    _, ranges, hints = scattered(lex4, offs)
    stored = [int(((ranges[:, 0] + ranges[:, 1]) <= h).sum()) for h in hints]
    claims = {"ranges_ascending": False, "unused_lexems": len(GAP) * (len(offs)), "stored_documents_per_hint": stored}
    return _geometry_build, lex4, offs, seg, claims


# ---------------------------------------------------------------- output capacity
def _capacity_build(m):
    for r in range(40):
        _rule(m, "o%d" % r, "sequence", [A, B], 12, variables=(0, 1) if r % 2 == 0 else (1,))


def output_capacity():
    big = [(A, p + 1) for p in range(10)] + [(B, 11)]        # 400 results, 600 items
    small = [(FILLER, 1), (A, 2), (B, 3)]                    # 40 results, 60 items
    lex4, offs, seg = _batch([small, big, big, small, big, big, big, small, big, big])
    return _capacity_build, lex4, offs, seg, {"results": 3 * 40 + 7 * 400, "items": 3 * 60 + 7 * 600}


# ---------------------------------------------------------------- input checks
LIM = 0x7FFFFFFF


def _checked_docs():
    def rows(doc):
        return [[t, p, 3 * i, 2] for i, (t, p) in enumerate(doc)]

    good = [(FILLER, 1), (A, 2), (B, 3), (C, 4), (D, 5)]
    docs, status = [], []

    def add(doc, st):
        docs.append([tuple(r) for r in doc])
        status.append(st)

    add(rows(good), 0)
    for ident, st in ((1 << 29, SP_DOC_ERR_RANGE), ((1 << 29) - 1, 0)):
        add(rows(good + [(ident, 6), (A, 7), (B, 8)]), st)
    # origpos / origsize: the reference checks them on a lexem that stays on the current position
    for col in (2, 3):
        for v, st in ((LIM, SP_DOC_ERR_RANGE), (LIM - 1, 0)):
            d = rows(good + [(A, 6), (B, 7), (B, 7), (A, 8), (B, 9)])
            d[7][col] = v
            add(d, st)
    d = rows(good + [(A, 6), (B, 7), (A, 8)])       # ... and not on a lexem that opens a new position
    d[6][2] = LIM
    add(d, 0)
    d = rows([(B, 0), (A, 1), (B, 2)])              # the current position before the first lexem is 0
    d[0][3] = LIM
    add(d, SP_DOC_ERR_RANGE)
    d = rows(_plain_doc(70, [10, 63]))              # descending between the lexems 63 and 64
    d[64][1] = d[63][1] - 1
    add(d, SP_DOC_ERR_ORDER)
    d = rows(_plain_doc(30, [5, 20]))               # ... between the last two
    d[29][1] = d[28][1] - 1
    add(d, SP_DOC_ERR_ORDER)
    # both in one document: the first one in the order of the lexems decides; on the same lexem the order
    d = rows(good + [(A, 6), (B, 7), (B, 7), (A, 8), (B, 5)])
    d[7][2] = LIM
    add(d, SP_DOC_ERR_RANGE)
    d = rows(good + [(A, 6), (B, 4), (B, 7), (B, 7)])
    d[8][2] = LIM
    add(d, SP_DOC_ERR_ORDER)
    d = rows(good + [(A, 6), (1 << 29, 3)])
    add(d, SP_DOC_ERR_ORDER)
    d = rows(good + [(1 << 29, 6), (A, 7), (B, 2)])
    add(d, SP_DOC_ERR_RANGE)
    add(rows(good), 0)
    return docs, status


def input_checks():
    docs, status = _checked_docs()
    lex4, offs, seg = _batch(docs)
    return _geometry_build, lex4, offs, seg, {"status_per_document": status}


# ---------------------------------------------------------------- table and filter
TABLE_SIZE = 32
CHAIN_SLOT = 5
E1, E2, S2 = 40, 41, 42


def _first_ids(second, pred, count, start=100, stop=1 << 22):
    """the first `count` ids x >= start for which pred(hash of (x, second), x) holds"""
    x = np.arange(start, stop, dtype=np.uint64)
    hit = x[pred(join_hash(x, second))]
    assert len(hit) >= count
    return [int(v) for v in hit[:count]]


def _table_ids():
    mask = TABLE_SIZE - 1
    ids = {}
    ids["chain"] = _first_ids(E1, lambda h: (h & mask) == CHAIN_SLOT, 3)                    # three keys with one home slot
    ids["wrap"] = _first_ids(E2, lambda h: (h & mask) == mask, 2)                           # the last slot twice: on to slot 0
    # an `any` key whose home slot lies inside that chain (JOIN_SELF sorts last: it is placed behind the pair keys)
    ids["self"] = next(s for s in range(100, 100000) if join_hash(JOIN_SELF, s) & mask == CHAIN_SLOT + 1)
    ids["multi"] = next((a, b) for a in range(100, 400) for b in range(400, 420) if 10 <= (join_hash(a, b) & mask) <= 18)
    return ids


def _table_keys(ids):
    return [(x, E1) for x in ids["chain"]] + [(x, E2) for x in ids["wrap"]] + [(JOIN_SELF, ids["self"]), (JOIN_SELF, S2), ids["multi"]]


def _table_strangers(ids):
    """pairs (x, e) that are no keys but whose filter bit another key has set: one whose home slot is empty, one whose
    probe passes over the foreign keys of the chain first"""
    keys = _table_keys(ids)
    slots = build_table(keys)
    bits = np.array(sorted(set(filter_bit(*k) for k in keys)), np.uint64)
    mask = TABLE_SIZE - 1
    empty = [s for s in range(TABLE_SIZE) if slots[s] is None]

    def passes(h):
        return np.isin((h >> np.uint64(8)) % np.uint64(FILTER_BITS), bits)

    x_empty = _first_ids(E1, lambda h: passes(h) & np.isin(h & np.uint64(mask), np.array(empty, np.uint64)), 1, start=1000)[0]
    x_chain = _first_ids(E1, lambda h: passes(h) & ((h & np.uint64(mask)) == CHAIN_SLOT), 1, start=1000, stop=1 << 27)[0]
    return x_empty, x_chain


_TABLE = {}


def _table():
    if not _TABLE:
        ids = _table_ids()
        _TABLE.update(ids=ids, strangers=_table_strangers(ids))
    return _TABLE


def _table_build(m):
    ids = _table()["ids"]
    for n, x in enumerate(ids["chain"]):
        _rule(m, "chain%d" % n, "sequence", [x, E1], 2, variables=(n % 2,))
    for n, x in enumerate(ids["wrap"]):
        _rule(m, "wrap%d" % n, "sequence", [x, E2], 2, variables=(0, 1))
    _rule(m, "self", "any", [ids["self"], S2], 1, variables=(0, 1))
    a, b = ids["multi"]
    # one key, several rules: ranges 1..5, struct and plain, variables on the first term, the second, both, none
    _rule(m, "m_none", "sequence", [a, b], 1)
    _rule(m, "m_first", "sequence", [a, b], 3, variables=(0,))
    _rule(m, "m_second", "sequence_struct", [a, b], 5, variables=(1,))
    _rule(m, "m_both", "sequence", [a, b], 2, variables=(0, 1))
    _rule(m, "m_struct", "sequence_struct", [a, b], 2)


def table_collisions():
    t = _table()
    ids, (x_empty, x_chain) = t["ids"], t["strangers"]
    a, b = ids["multi"]
    docs = []
    for first, second in _table_keys(ids):
        docs.append([(second, 1)] if first == JOIN_SELF else [(FILLER, 1), (first, 2), (second, 3), (FILLER, 4)])
    docs.append([(x_empty, 1), (E1, 2), (ids["chain"][1], 3), (E1, 4)])            # a stranger, then a key of the chain
    docs.append([(x_chain, 1), (E1, 2), (x_chain, 3), (ids["chain"][2], 3), (E1, 4)])
    docs.append([(a, 1), (b, 2), (a, 5), (b, 8), (a, 10), (DEL, 11), (b, 12), (a, 20), (b, 25), (a, 30), (b, 36)])
    docs.append([(ids["self"], 1), (S2, 1), (ids["self"], 2), (ids["wrap"][0], 3), (ids["wrap"][1], 3), (E2, 4)])
    lex4, offs, seg = _batch(docs)
    claims = {
        "table_size": TABLE_SIZE,
        "keys_with_one_home_slot": 3,
        "chain_wraps_to_slot_0": True,
        "self_key_behind_pair_keys_of_its_chain": True,
        "strangers_that_pass_the_filter": 2,
        "foreign_keys_a_stranger_passes": [0, 4],
        "rules_of_one_key": 5,
    }
    return _table_build, lex4, offs, seg, claims


# ---------------------------------------------------------------- predicate edges
def _predicate_build(m):
    _rule(m, "ab", "sequence", [A, B], 3, variables=(0, 1))
    _rule(m, "cd_s", "sequence_struct", [C, D], 4, variables=(1,))
    _rule(m, "cd", "sequence", [C, D], 4)
    _rule(m, "ef_s", "within_struct", [E, F], 4, variables=(0,))
    _rule(m, "gg", "any", [G, G], 1, variables=(0, 1))
    _rule(m, "hh", "within", [H, H], 3, variables=(0,))
    _rule(m, "ii", "sequence", [I, I], 3, variables=(1,))


def predicate_edges():
    docs = [
        [(A, 1), (B, 1), (FILLER, 2), (A, 3), (B, 4)],                      # same position: no match; one later: match
        [(A, 1), (B, 1), (B, 2), (FILLER, 5), (A, 10), (B, 11), (B, 12)],      # a B on A's own position does not take, a later one does
        [(A, 1), (B, 4), (A, 10), (B, 14), (A, 20), (FILLER, 21), (999999, 22), (B, 23)],   # distance = range, range + 1
        [(C, 1), (DEL, 2), (D, 3)],                                         # the delimiter between the terms,
        [(C, 1), (DEL, 1), (D, 2), (FILLER, 9), (DEL, 10), (C, 10), (D, 11)],  # on the first term's position (behind it, before it),
        [(C, 1), (DEL, 2), (D, 2), (FILLER, 9), (C, 10), (D, 11), (DEL, 11)],  # on the second term's position (before it, behind it)
        [(E, 1), (F, 2), (F, 5), (E, 6), (DEL, 7), (F, 8), (E, 9)],
        [(G, 1), (FILLER, 2), (G, 3), (G, 3)],
        [(H, 1), (H, 2), (H, 3), (H, 3), (H, 7)],
        [(I, 1), (I, 2), (I, 3), (I, 3), (I, 7)],
        [(FILLER, 1), (999999, 2), (FILLER, 3)],                            # nothing any rule mentions
    ]
    lex4, offs, seg = _batch(docs)
    return _predicate_build, lex4, offs, seg, {"results_per_document": [2, 2, 2, 1, 3, 3, 4, 6, 4, 2, 0]}


def _no_struct_build(m):
    _rule(m, "ab", "sequence", [A, B], 3, variables=(0, 1))
    _rule(m, "cd", "within", [C, D], 4, variables=(1,))


def delimiter_without_struct():
    """no *_struct rule: the kernel's delimiter is 0, and the id the other cases use as one is a lexem like any other"""
    docs = [[(A, 1), (DEL, 2), (B, 3)], [(C, 1), (DEL, 2), (synth.DELIM, 2), (D, 3), (0, 4), (C, 5)]]
    lex4, offs, seg = _batch(docs)
    return _no_struct_build, lex4, offs, seg, {"results_per_document": [1, 2]}


# ---------------------------------------------------------------- moved keys
ALT_GOALS = {
    ALT_SEQ: ["no_a_between", "a_between", "not_taken", "taken", "b_beside", "earlier_b"],
    ALT_REPLAY: ["no_a_between", "a_between"],
    ALT_LINGER: ["not_taken", "taken", "no_b_before", "b_before"],
}


def alt_brackets(r, lex, i, x, delimiter):
    """the bracketed terms of the JOIN_ALT_* formulas of csrc/l2_join.h for the pair (i, x) of the entry r, as a set of
    the names of ALT_GOALS; None where the pair fails the common condition (range, delimiter)"""
    pi, px = lex[i][1], lex[x][1]
    if not pi < px <= pi + r.range:
        return None
    a, b = lex[i][0], lex[x][0]
    between = lex[i + 1:x]
    if r.struct and any(l[0] == delimiter for l in between):
        return None
    out = set()
    out.add("taken" if any(l[0] == b and l[1] > pi for l in between) else "not_taken")
    if r.kind == ALT_LINGER:
        out.add("b_before" if any(l[0] == b and l[1] + r.range >= pi for l in lex[:i]) else "no_b_before")
        return out
    out.add("a_between" if any(l[0] == a for l in between) else "no_a_between")
    if r.kind == ALT_REPLAY:
        return out - {"taken", "not_taken"}
    for l in between:
        if l[0] == a:
            break
        if l[0] == b and l[1] == pi:
            out.add("b_beside")
    prev_a = [l[1] for l in lex[:i] if l[0] == a]
    lim = prev_a[-1] + r.range if prev_a else -1
    for l in reversed(lex[:i]):
        if l[1] + r.range < px or l[1] <= lim or (r.struct and l[0] == delimiter):
            break
        if l[0] == b:
            out.add("earlier_b")
    return out


def _moved_rules():
    """a small random rule set (those of tests/test_result_sets_gpu.py) whose compiled form has entries of every JOIN_ALT_* kind"""
    return synth.random_rules(50, 8, 1, op="sequence") + [(n + "_w", o, rg, p) for n, o, rg, p in synth.random_rules(50, 8, 1, op="within")]


def _moved_build(m):
    m.defineOption("weightFactor", 1.5)
    synth.apply_rules(m, _moved_rules(), compile=True)


_MOVED = {}
MOVED_FILLER = 999        # (the random rules use the ids 1..8)


def _as_lex(doc):
    return [(t, p, 0, 3 * i, 2) for i, (t, p) in enumerate(doc)]


def _moved_docs():
    """for every kind of moved entry: short documents, found by enumeration, in which each bracketed term of its formula
    holds and in which it does not; a pair that matches more than once; the same with its look-back across lexem 64"""
    if _MOVED:
        return _MOVED
    o = oracle.L2Matcher()
    _moved_build(o)
    rules, delimiter = join_rules(o.dumpTable())
    docs, covered, multiple = [], {}, None
    for kind, goals in ALT_GOALS.items():
        r = next(r for r in rules if r.kind == kind and r.first != r.second and r.range >= 2)
        todo = list(goals) + (["multiple"] if kind == ALT_SEQ else [])
        for n in range(2, 6):
            for ids in itertools.product((r.first, r.second, MOVED_FILLER), repeat=n):
                for steps in itertools.product((0, 1), repeat=n - 1):
                    if not todo:
                        break
                    pos = [1 + sum(steps[:k]) for k in range(n)]
                    doc = list(zip(ids, pos))
                    lex = _as_lex(doc)
                    got = set()
                    for i in range(n):
                        for x in range(i + 1, n):
                            if lex[i][0] == r.first and lex[x][0] == r.second:
                                br = alt_brackets(r, lex, i, x, delimiter)
                                if br is not None:
                                    got |= br
                                    if _pair_count(r, lex, i, x, delimiter) > 1:
                                        got.add("multiple")
                                        if multiple is None:
                                            multiple = (doc, x)
                    new = [g for g in todo if g in got]
                    if new:
                        docs.append(doc)
                        for g in new:
                            todo.remove(g)
                            covered.setdefault(kind, []).append(g)
        assert not todo, (kind, todo)
    # the pair that matches more than once, its completing lexem at index 64
    doc, x = multiple
    pad = LANES - x
    docs.append([(MOVED_FILLER, p + 1) for p in range(pad)] + [(t, p + pad + 2) for t, p in doc])
    _MOVED.update(docs=docs, covered=covered, rules=rules, delimiter=delimiter, crossing=len(docs) - 1)
    return _MOVED


def moved_keys():
    mv = _moved_docs()
    lex4, offs, seg = _batch(mv["docs"])
    mult = Counter()
    crossing = 0
    for d, doc in enumerate(mv["docs"]):
        for i, x, r, m in model_pairs(mv["rules"], mv["delimiter"], _as_lex(doc)):
            if r.kind in ALT_GOALS:
                mult[m] += 1
                if m > 1 and d == mv["crossing"] and i < LANES <= x:
                    crossing = max(crossing, m)
    claims = {
        "covered": {k: sorted(g for g in v if g != "multiple") for k, v in mv["covered"].items()},
        "multiplicities_of_moved_pairs": dict(mult),
        "multiplicity_across_lexem_64": crossing,
    }
    return _moved_build, lex4, offs, seg, claims


# ---------------------------------------------------------------- segments and formats
def segments():
    """origseg changes every three lexems: inside the pairs (5, 6) and (20, 21)"""
    lex4, offs, seg = _batch([_plain_doc(40, [5, 20, 30]), _plain_doc(9, [2, 5])], seg_every=3)
    return _geometry_build, lex4, offs, seg, {"results_spanning_segments": 4, "results": 5}


def _formats_build(m):
    _rule(m, "ab", "sequence", [A, B], 3, variables=(0, 1), fmt="<{v0}|{v1}>")
    _rule(m, "ab2", "sequence", [A, B], 2, variables=(1,), fmt="{v1}")
    _rule(m, "cd", "within", [C, D], 2, variables=(0,), fmt="const")
    _rule(m, "ef", "any", [E, F], 1, variables=(0,))


def formats():
    lex4, offs, seg = _batch([_plain_doc(70, [5, 63], [(20, C), (21, D), (30, E)]), [(A, 1), (B, 4), (D, 5), (C, 6), (F, 7)]])
    return _formats_build, lex4, offs, seg, {"formats": 3, "results_with_a_format": 7, "results_without": 2}


def _bare_build(m):
    _rule(m, "ab", "sequence", [A, B], 3)
    _rule(m, "cd", "within_struct", [C, D], 2)
    _rule(m, "ef", "any", [E, F], 1)


def no_variables():
    lex4, offs, seg = _batch([_plain_doc(70, [5, 63], [(20, C), (21, D), (30, E)]), [(A, 1), (B, 4), (D, 5), (C, 6), (F, 7)]])
    return _bare_build, lex4, offs, seg, {"items": 0, "results": 7}


CASES = {
    "chunk_geometry": chunk_geometry,
    "single_document": single_document,
    "more_docs_than_waves": more_docs_than_waves,
    "count_limit_32767": count_limit_32767,
    "count_limit_32768": count_limit_32768,
    "count_limit_66000": count_limit_66000,
    "count_array": count_array,
    "output_capacity": output_capacity,
    "input_checks": input_checks,
    "table_collisions": table_collisions,
    "predicate_edges": predicate_edges,
    "delimiter_without_struct": delimiter_without_struct,
    "moved_keys": moved_keys,
    "segments": segments,
    "formats": formats,
    "no_variables": no_variables,
}
