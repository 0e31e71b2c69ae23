"""Test utility: a pure-Python model of the cluster-per-lane handler route of the lexer's post-processing kernel
(postDocumentClusters, l1_post_kernel.hip) on top of tests/l1_words_model: the live records of a document in the order the
kernel merges its two report queues in, the views of up to 64 records it looks at, where it sees a boundary, what it does
with a view (reports handed to handleReport one after the other, clusters run by lanes, the first cluster a lane cannot
take), the handler of a lane on its little event array and the reference's handler on the whole array.  It restates the
kernel's arithmetic, so the CPU tests can say what a GPU batch is going to exercise before it runs: which lanes head a
cluster, which hand-back reason a step has, when the event array is too small.  Test code only: nothing in the product
imports this."""
import collections

from tests import l1_words_model as words

VIEW = 64                   # records the boundaries are found in at once (one per lane)
LOC_CAP = 6                 # SPA_L1_POST_LOC_CAP: events of a lane's cluster
EVENT_CAP = 32768           # eventCap of a new context (capi_l1.cpp)
REC_SYMBOL = 1 << 16
REC_SIZEERR = 1 << 31
HARD = "HARD"
LEXEMSIZE = 7               # SP_DOC_ERR_LEXEMSIZE
ARENA = 2                   # SP_DOC_ERR_ARENA

# why a step hands reports to handleReport one after the other
BEFORE_FIRST_BOUNDARY = "before_first_boundary"     # first > 0: they may reach into the array
VIEW_LONG_CLUSTER = "view_long_cluster"             # procEnd == 0: one cluster as long as the view
MORE_THAN_LOC_CAP = "more_than_loc_cap"             # a seventh event would be inserted
SYMBOL_LOOKUP = "symbol_lookup"
SIZE_ERROR = "size_error"
REASONS = (BEFORE_FIRST_BOUNDARY, VIEW_LONG_CLUSTER, MORE_THAN_LOC_CAP, SYMBOL_LOOKUP, SIZE_ERROR)

# {end, start, lexem id, level | posbind << 8 | flags} of preparedRecord, and the twin id of a symbol lookup (0: none)
Record = collections.namedtuple("Record", "to frm id fl sym")
# an event of the handler's array
Event = collections.namedtuple("Event", "id pos size lb")
ZERO = Event(0, 0, 0, 0)


# ---------------------------------------------------------------- the records of a document
def prepared(pat, frm, to):
    """preparedRecord: (to, from, id, flags) of a resolved report with its sub expression selection applied, None where
    the report is dropped"""
    lb = pat["levelBind"]
    fl = lb & 0x1FFFF
    if to - frm >= 65535:
        fl |= REC_SIZEERR
    if lb & (1 << 17):
        if pat["prefixLen"] + pat["suffixLen"] > to - frm:
            if not fl & REC_SIZEERR:
                return None
        else:
            frm += pat["prefixLen"]
            to -= pat["suffixLen"]
    return to, frm, pat["id"], fl


def queue_records(t, doc, chunk):
    """(A, B): the live entries (end, patterns entry, start) of the automaton's queue and of the word queue, each in
    (end, entry) order.  An expression cut into several patterns entries reports once per entry: the last report of a
    group (one definition, one end) takes the leftmost start, the others are skipped (nextBatch)."""
    a = []
    for pi, frm, to in words.automaton_reports(t, doc, True):
        d = t.patterns[pi]["defIndex"]
        if a and a[-1][0] == to and t.patterns[a[-1][1]]["defIndex"] == d:
            frm = min(frm, a[-1][2])
            a.pop()
        a.append((to, pi, frm))
    b = [(to, pi, frm) for recs in words.records(t, doc, chunk) for to, pi, frm, dead in recs if not dead]
    assert a == sorted(a) and b == sorted(b)
    return a, b


def records(t, doc, chunk=words.DEFAULT_CHUNK, symbols=None):
    """the live record stream of a document as the window holds it: both queues merged by (end offset, patterns entry)
    -- not by (end offset, definition), not by the end the selection leaves -- and prepared.  symbols: {(lexem id,
    text): symbol id} of the table's defineSymbol calls."""
    a, b = queue_records(t, doc, chunk)
    out = []
    for to, pi, frm in sorted(a + b):
        r = prepared(t.patterns[pi], frm, to)
        if r is None:
            continue
        sym = 0
        if r[3] & REC_SYMBOL and not r[3] & REC_SIZEERR:
            sym = (symbols or {}).get((r[2], bytes(doc[r[1]:r[0]])), 0)
        out.append(Record(r[0], r[1], r[2], r[3], sym))
    return out


def refills(a, b, consumed):
    """the passes of the refill loop: [(live records taken of A, of B, the `limit` rule kept a record of a batch back)].
    For a document of ONE scan unit whose queues hold live entries only (a, b of queue_records with no dead candidate and
    no skipped report of a split expression: the kernel resolves 64 queue entries at a time, which are then 64 live
    ones; the term of the limit for a further chunk does not come in).  consumed: the records every step of trace()
    moves the window by -- the loop runs in front of a step while the window holds fewer than 64 records and a queue
    has any.  Nothing behind a batch's last key is known yet, so a pass takes the entries up to the smaller of the last
    keys of the batches that have more behind them."""
    out = []
    qa = qb = 0                 # next entry
    ba = bb = 0                 # begin of the resolved batch
    have = 0                    # records in the window
    for used in consumed:
        while have < VIEW and (qa < len(a) or qb < len(b)):
            ea, eb = min(ba + 64, len(a)), min(bb + 64, len(b))
            limit = None
            if qa < len(a) and ea < len(a):
                limit = a[ea - 1][:2]
            if qb < len(b) and eb < len(b) and (limit is None or b[eb - 1][:2] < limit):
                limit = b[eb - 1][:2]
            ta = [x for x in a[qa:ea] if limit is None or x[:2] <= limit]
            tb = [x for x in b[qb:eb] if limit is None or x[:2] <= limit]
            assert ta or tb
            out.append((len(ta), len(tb), len(ta) < ea - qa or len(tb) < eb - qb))
            qa += len(ta)
            qb += len(tb)
            have += len(ta) + len(tb)
            if qa == ea:
                ba = qa
            if qb == eb:
                bb = qb
        assert used <= min(have, VIEW)
        have -= used
    assert qa == len(a) and qb == len(b) and have == 0
    return out


# ---------------------------------------------------------------- views and boundaries
def view_at(recs, wi):
    """(view, final) at the window start wi.  The refill loop runs while the window holds fewer than 64 records and a
    queue has any, so a view is the next min(64, remaining) live records; `exhausted` is only set by a pass of that loop
    that finds both queues empty, which needs fewer than 64 records in the window: a view is final iff fewer than 64
    records remain (a document that ends exactly on a view of 64 is seen as not yet ended)."""
    left = len(recs) - wi
    return recs[wi:wi + min(VIEW, left)], left < VIEW


def views(recs):
    """the successive views if every view were consumed whole (what the refill loop yields; trace() moves the window by
    what a step consumes instead)"""
    return [view_at(recs, wi)[0] for wi in range(0, len(recs), VIEW)]


def bounds(view, carryF=0, carryT=0):
    """the indices a boundary stands before: the start of every record from i on is greater than every earlier start of
    the view and the carry, and so the ends; both strict.  (The carries are 1 + the greatest start / end handled so far,
    0 for none, as the kernel keeps them.)"""
    n = len(view)
    sufF, sufT = [0] * (n + 1), [0] * (n + 1)
    sufF[n] = sufT[n] = 1 << 32
    for i in range(n - 1, -1, -1):
        sufF[i], sufT[i] = min(sufF[i + 1], view[i].frm + 1), min(sufT[i + 1], view[i].to + 1)
    out = []
    exclF, exclT = carryF, carryT
    for i in range(n):
        if sufF[i] > exclF and sufT[i] > exclT:
            out.append(i)
        exclF, exclT = max(exclF, view[i].frm + 1), max(exclT, view[i].to + 1)
    return out


def carry_to(view, upto, carryF, carryT):
    """carryTo: the reports [0, upto) of the view are done"""
    if not upto:
        return carryF, carryT
    return max(carryF, max(r.frm + 1 for r in view[:upto])), max(carryT, max(r.to + 1 for r in view[:upto]))


# ---------------------------------------------------------------- the two handlers
def lane_handler(cluster, cap=LOC_CAP):
    """the delete, ignore and insert passes of a lane on the events of its own cluster: the survivors, or HARD when a
    record carries the symbol or the size error flag or a (cap+1)th event would be inserted.  A report that is ignored
    is never inserted, so it never makes a cluster hard."""
    loc = []
    for r in cluster:
        if r.fl & (REC_SYMBOL | REC_SIZEERR):
            return HARD
        level, frm, last = r.fl & 0xFF, r.frm, r.to
        deletes = 0
        q = len(loc)
        while q > 0:
            m = loc[q - 1]
            if not m.pos >= frm:
                break
            mlevel = m.lb & 0xFF
            if (r.id == m.id and m.pos == frm and mlevel == level) or (mlevel < level and m.pos + m.size <= last):
                del loc[q - 1]
                deletes += 1
            q -= 1
        ignored = False
        if not deletes:
            for m in reversed(loc):
                if not m.pos + m.size >= last:
                    break
                if (m.lb & 0xFF) > level and m.pos <= frm:
                    ignored = True
                    break
        if ignored:
            continue
        if len(loc) == cap:
            return HARD
        at = len(loc)
        while at > 0 and loc[at - 1].pos > frm:
            at -= 1
        loc.insert(at, Event(r.id, frm, last - frm, r.fl & 0xFFFF))
    return loc


def hard_reason(cluster):
    """why lane_handler gives a cluster back"""
    for r in cluster:
        if r.fl & REC_SIZEERR:
            return SIZE_ERROR
        if r.fl & REC_SYMBOL:
            return SYMBOL_LOOKUP
    return MORE_THAN_LOC_CAP


def sequential(events, r):
    """the reference's handler (handleReport / handleReportArena) with one record on the whole array, in place; the twin
    event of a symbol with the reference's element moves (the first event moved goes up two slots, the others one).
    Returns LEXEMSIZE for a record with the size error flag, else 0."""
    if r.fl & REC_SIZEERR:
        return LEXEMSIZE
    level, lb = r.fl & 0xFF, r.fl & 0xFFFF
    ev = Event(r.id, r.frm, r.to - r.frm, lb)
    twin = Event(r.sym, r.frm, r.to - r.frm, lb) if r.sym and r.sym != r.id else None
    deletes = 0
    k = len(events)
    while k > 0:
        m = events[k - 1]
        if not m.pos >= ev.pos:
            break
        mlevel = m.lb & 0xFF
        if (ev.id == m.id and m.pos == ev.pos and mlevel == level) or (mlevel < level and m.pos + m.size <= r.to):
            del events[k - 1]
            deletes += 1
        k -= 1
    if not deletes:
        for m in reversed(events):
            if not m.pos + m.size >= r.to:
                break
            if (m.lb & 0xFF) > level and m.pos <= ev.pos:
                return 0
    n = len(events)
    slots = 2 if twin else 1
    events.extend([ZERO] * slots)
    prev, mi = n + slots - 1, n - 1
    while mi >= 0:
        m = events[mi]
        if not m.pos > ev.pos:
            break
        events[prev] = m
        prev, mi = mi, mi - 1
    mi += 1
    events[mi] = ev
    if twin:
        events[mi + 1] = twin
    return 0


def sequential_run(recs):
    """every record through the reference's handler, one after the other (SPA_L1_POST_SEQ): dict(events, err, counts:
    the length of the array in front of every report)"""
    events, counts = [], []
    for r in recs:
        counts.append(len(events))
        err = sequential(events, r)
        if err:
            return dict(events=[], err=err, counts=counts)
    return dict(events=events, err=0, counts=counts)


# ---------------------------------------------------------------- a view, a document
def step(view, final, carryF, carryT):
    """what the kernel does with a view: dict of
       kind         "sequential" (the reports [0, consumed) one after the other, `reason` says why) or "lanes"
       bounds       the boundaries of the view
       first        the first boundary (64: none)
       heads, lens  "lanes": the lane and the length of every complete cluster, in order
       results      "lanes": lane_handler of each
       first_hard   "lanes": the lane of the first cluster a lane cannot take (64: none), `reason` why
       appended     "lanes": the lanes whose survivors are appended (those in front of first_hard)
       proc_end     "lanes": the end of the last complete cluster
       consumed     records the window moves on by
       carry_in     (carryF, carryT) in front of the step
       carry        (carryF, carryT) after the step"""
    avail = len(view)
    b = bounds(view, carryF, carryT)
    first = b[0] if b else VIEW
    out = dict(bounds=b, first=first, final=final, avail=avail, carry_in=(carryF, carryT))
    if first:
        e = min(first, avail)
        out.update(kind="sequential", reason=BEFORE_FIRST_BOUNDARY, consumed=e, carry=carry_to(view, e, carryF, carryT))
        return out
    proc_end = avail if final else b[-1]
    if proc_end == 0:
        out.update(kind="sequential", reason=VIEW_LONG_CLUSTER, consumed=avail, carry=carry_to(view, avail, carryF, carryT))
        return out
    heads = [i for i in b if i < proc_end]
    lens = [min(([j for j in b if j > i] + [VIEW])[0], proc_end) - i for i in heads]
    results = [lane_handler(view[i:i + n]) for i, n in zip(heads, lens)]
    hard = [i for i, r in zip(heads, results) if r is HARD]
    first_hard = hard[0] if hard else VIEW
    out.update(kind="lanes", heads=heads, lens=lens, results=results, first_hard=first_hard, proc_end=proc_end,
               appended=[i for i in heads if i < first_hard], reason=None)
    if hard:
        hlen = lens[heads.index(first_hard)]
        out.update(reason=hard_reason(view[first_hard:first_hard + hlen]), consumed=first_hard + hlen)
    else:
        out.update(consumed=proc_end)
    out["carry"] = carry_to(view, out["consumed"], carryF, carryT)
    return out


def trace(recs):
    """the document through postDocumentClusters: dict(steps, events, err, checks).  Every step carries `wi`, the index
    of its view's first record in the stream.  checks: the tests against the capacity of the event array in the order
    the kernel makes them, ("append", events so far, events to append) per lane step and ("report", events so far) per
    report handed to handleReport."""
    events, steps, checks = [], [], []
    wi, carryF, carryT = 0, 0, 0
    err = 0

    def hand_back(rs):
        for r in rs:
            if r.fl & REC_SIZEERR:
                return LEXEMSIZE
            checks.append(("report", len(events)))
            sequential(events, r)
        return 0
    while wi < len(recs) and not err:
        view, final = view_at(recs, wi)
        s = step(view, final, carryF, carryT)
        s["wi"] = wi
        steps.append(s)
        if s["kind"] == "sequential":
            err = hand_back(view[:s["consumed"]])
        else:
            new = [e for i, r in zip(s["heads"], s["results"]) if i < s["first_hard"] for e in r]
            checks.append(("append", len(events), len(new)))
            events.extend(new)
            if s["first_hard"] < VIEW:
                err = hand_back(view[s["first_hard"]:s["consumed"]])
        assert s["consumed"] > 0
        wi += s["consumed"]
        carryF, carryT = s["carry"]
    return dict(steps=steps, events=[] if err else events, err=err, checks=checks, seq=sequential_run(recs))


def event_capacity(tr, cap=EVENT_CAP, mode="clusters"):
    """the status of the document with an event array of cap events: SP_DOC_ERR_ARENA where it is too small, else the
    document's own (0 or the lexem size error).  The cluster route asks for nEvents + total + 2 <= cap at every append
    (and what handleReport asks at every report it hands back), the sequential route for nEvents + 2 <= cap at every
    report (l1_handler.h)."""
    if mode == "sequential":
        if any(n + 2 > cap for n in tr["seq"]["counts"]):
            return ARENA
        return tr["seq"]["err"]
    for c in tr["checks"]:
        if (c[1] + c[2] + 2 if c[0] == "append" else c[1] + 2) > cap:
            return ARENA
    return tr["err"]


def spans(events):
    """(id, origpos, origsize) of the events: what the output keeps of them beside the ordinal position"""
    return [(e.id, e.pos, e.size) for e in events]


def isolated(tr):
    """the document's trace holds only single-report clusters run by lanes"""
    return bool(tr["steps"]) and all(s["kind"] == "lanes" and s["first_hard"] == VIEW and all(n == 1 for n in s["lens"]) for s in tr["steps"])
