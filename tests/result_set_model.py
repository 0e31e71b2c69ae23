"""Pure-Python restatement of the result-set mode of the rule automaton (csrc/l2_join.h): the multiset of results, with
their captured items, of a flat rule set of two-term programs (sequence, within, sequence_struct, within_struct, any) on
one document -- the predicate the join kernel evaluates, lexem pair by lexem pair.

It reads the compiled program table (the word dump of `dumpTable()`, the same on the oracle and on the product), so it
follows the key index the optimizer left behind:

* a key reference without a past event installs an instance at every occurrence of its key event; the instance takes
  the first later lexem of the other term at a position behind the key's and expires `range` positions after it:
  (A at i, B at x) matches iff ordpos(i) < ordpos(x) <= ordpos(i) + range and no B lies in (i, x) at a position
  behind ordpos(i);
* a key reference with a past event (the optimizer moved a program keyed by a frequent event A onto its other term B)
  installs an instance at every B.  It replays the LATEST logged A if that one is still in range, fires B's key trigger
  afterwards, is cancelled by a delimiter logged after the replayed A (`_struct`), and, if it does not complete at its
  own B, lingers until it expires and may complete later -- so the same pair can come out more than once.

Counted per pair (i, x) with i < x, ordpos(i) < ordpos(x) <= ordpos(i) + range and (for `_struct`) no delimiter in
(i, x), with A = id(i), B = id(x):

  normal       1 if no B in (i, x) at a position behind ordpos(i) ("not taken")
  alt_seq      sequence( A, B) moved onto B:
               [no A in (i, x)]                                          the replay of the instance installed at x
             + [not taken] * #{ j in (i, next A after i): id(j) = B, ordpos(j) = ordpos(i) }
                                                                          instances of earlier Bs at A's position
                                                                          that replayed i and waited for a later B
             + [not taken] * #{ j < i: id(j) = B, ordpos(j) >= ordpos(x) - range,
                                ordpos(j) > ordpos(latest A before i) + range, no delimiter in (j, i) }
                                                                          instances of earlier Bs without a replay
                                                                          that took i as their first A
  alt_replay   within( A, B) keyed at B with past A: [no A in (i, x)]     (the replayed A, completed by x)
  alt_linger   within( B, A) keyed at B with past A, pair (B at i, A at x): [not taken] *
               [no A before i at a position >= ordpos(i) - range]         (no replay: the instance waits for an A)

The first two lines of alt_seq come from oracle/l2_oracle.cpp installProgram / replayPastEvent / fireSignal; the tests
check this model against the oracle itself (tests/test_result_set_model.py).
"""
from collections import Counter, defaultdict

SIG_ANY, SIG_SEQUENCE, SIG_SEQUENCE_IMM, SIG_WITHIN, SIG_DEL, SIG_AND = range(6)
NORMAL, SELF, ALT_SEQ, ALT_REPLAY, ALT_LINGER = range(5)


class JoinRule:
    __slots__ = ("first", "second", "range", "handle", "kind", "struct", "vfirst", "vsecond")

    def __init__(self, first, second, range_, handle, kind, struct, vfirst, vsecond):
        self.first, self.second, self.range, self.handle = first, second, range_, handle
        self.kind, self.struct, self.vfirst, self.vsecond = kind, struct, vfirst, vsecond


def parse_table(words):
    """dumpTable() words -> (programs, keyrefs): programs[p] = (positionRange, resultHandle, [(event, isKey, sigtype,
    sigval, variable)]) for p = 1..n; keyrefs[p] = [(key event, past event)]."""
    w = [int(x) for x in words]
    nprg, nkeys = w[0], w[1]
    at = 3
    programs = {}
    for p in range(1, nprg + 1):
        rng, handle, ntrig = w[at + 5], w[at + 3], w[at + 6]
        at += 7
        trig = [tuple(w[at + 5 * t:at + 5 * t + 5]) for t in range(ntrig)]
        at += 5 * ntrig
        programs[p] = (rng, handle, trig)
    keyrefs = defaultdict(list)
    for _ in range(nkeys):
        ev, n = w[at], w[at + 1]
        at += 2
        for r in range(n):
            keyrefs[w[at + 2 * r]].append((ev, w[at + 2 * r + 1]))
        at += 2 * n
    return programs, keyrefs


def join_rules(words):
    """The join entries of a compiled flat rule set: (rules, delimiter).  Raises ValueError outside the envelope."""
    programs, keyrefs = parse_table(words)
    rules, delimiter = [], 0
    for p, (rng, handle, trig) in programs.items():
        terms = [t for t in trig if t[2] != SIG_DEL]
        dels = [t for t in trig if t[2] == SIG_DEL]
        if len(terms) != 2 or len(dels) > 1:
            raise ValueError("program %d is not a two-term program" % p)
        struct = bool(dels)
        if struct:
            if delimiter and delimiter != dels[0][0]:
                raise ValueError("more than one delimiter")
            delimiter = dels[0][0]
        sigtype = terms[0][2]
        refs = keyrefs.get(p, [])
        plain = Counter(k for k, past in refs if not past)
        alt = [(k, past) for k, past in refs if past]
        if sigtype == SIG_ANY:
            same = terms[0][0] == terms[1][0]
            for t in range(2):
                if same:
                    rules.append(JoinRule(0, terms[t][0], rng, handle, SELF, False, terms[0][4], terms[1][4]))
                else:
                    rules.append(JoinRule(0, terms[t][0], rng, handle, SELF, False, 0, terms[t][4]))
        elif sigtype == SIG_SEQUENCE:
            a = terms[0] if terms[0][3] == 2 else terms[1]
            b = terms[1] if a is terms[0] else terms[0]
            if plain[a[0]]:
                rules.append(JoinRule(a[0], b[0], rng, handle, NORMAL, struct, a[4], b[4]))
            for k, past in alt:
                assert k == b[0] and past == a[0]
                rules.append(JoinRule(a[0], b[0], rng, handle, ALT_SEQ, struct, a[4], b[4]))
        elif sigtype == SIG_WITHIN:
            same = terms[0][0] == terms[1][0]
            for t in range(2):
                x = terms[0] if same else terms[t]
                if plain[terms[t][0]] >= (t + 1 if same else 1):
                    rules.append(JoinRule(terms[t][0], terms[1 - t][0], rng, handle, NORMAL, struct, x[4],
                                          terms[1 - t][4] if not same else terms[1][4]))
            for k, past in alt:
                kt = terms[0] if terms[0][0] == k else terms[1]
                pt = terms[1] if kt is terms[0] else terms[0]
                rules.append(JoinRule(pt[0], kt[0], rng, handle, ALT_REPLAY, struct, pt[4], kt[4]))
                rules.append(JoinRule(kt[0], pt[0], rng, handle, ALT_LINGER, struct, kt[4], pt[4]))
        else:
            raise ValueError("program %d is neither sequence, within nor any" % p)
    return rules, delimiter


def _item(var, lx):
    ident, pos, seg, opos, size = lx
    return (var, pos, pos + 1, seg, opos, seg, opos + size)


def _record(r, li, lx, items):
    its = [it for it in items if it[0]]
    return (r.handle, li[1], lx[1] + 1, li[2], li[3], lx[2], lx[3] + lx[4], len(its)) + tuple(v for it in its for v in it)


def _pair_count(r, lex, i, x, delimiter):
    """multiplicity of the pair (i, x) for the rule r (module docstring)"""
    pi, px = lex[i][1], lex[x][1]
    if not pi < px <= pi + r.range:
        return 0
    a, b = lex[i][0], lex[x][0]
    between = lex[i + 1:x]
    if r.struct and any(l[0] == delimiter for l in between):
        return 0
    taken = any(l[0] == b and l[1] > pi for l in between)
    if r.kind == NORMAL:
        return 0 if taken else 1
    if r.kind == ALT_REPLAY:
        return 0 if any(l[0] == a for l in between) else 1
    if r.kind == ALT_LINGER:
        if taken:
            return 0
        return 0 if any(l[0] == b and l[1] + r.range >= pi for l in lex[:i]) else 1
    # ALT_SEQ
    m = 0 if any(l[0] == a for l in between) else 1
    if taken:
        return m
    for l in between:
        if l[0] == a:
            break
        if l[0] == b and l[1] == pi:
            m += 1
    prev_a = [l[1] for l in lex[:i] if l[0] == a]
    lim = prev_a[-1] + r.range if prev_a else -1
    for j in range(i - 1, -1, -1):
        lj = lex[j]
        if lj[1] + r.range < px or lj[1] <= lim:
            break
        if r.struct and lj[0] == delimiter:
            break
        if lj[0] == b:
            m += 1
    return m


def document_results(rules, delimiter, lex):
    """lex: list of (id, ordpos, origseg, origpos, origsize) of one document -> Counter of result records
    (the 7 result fields, the item count, the items' 7 fields each, latest captured first)."""
    byself = defaultdict(list)
    bypair = defaultdict(list)
    maxrange = 0
    for r in rules:
        if r.kind == SELF:
            byself[r.second].append(r)
        else:
            bypair[(r.first, r.second)].append(r)
            maxrange = max(maxrange, r.range)
    out = Counter()
    for x, lx in enumerate(lex):
        for r in byself.get(lx[0], ()):
            out[_record(r, lx, lx, [_item(r.vsecond, lx), _item(r.vfirst, lx)])] += 1
        for i in range(x - 1, -1, -1):
            li = lex[i]
            if li[1] + maxrange < lx[1]:
                break
            for r in bypair.get((li[0], lx[0]), ()):
                m = _pair_count(r, lex, i, x, delimiter)
                if m:
                    out[_record(r, li, lx, [_item(r.vsecond, lx), _item(r.vfirst, li)])] += m
    return out


def results_multiset(batch, d):
    """Counter of the records of document d of a result batch (results (n,9), items (m,7), doc_offsets)"""
    out = Counter()
    for r in batch.results[batch.doc_offsets[d]:batch.doc_offsets[d + 1]].tolist():
        it = batch.items[r[7]:r[7] + r[8]]
        out[tuple(r[:7]) + (r[8],) + tuple(it.reshape(-1).tolist())] += 1
    return out
