"""Constructed inputs that put the general rule kernel (csrc/l2_kernel.hip) on its batch and capacity edges: the
128-entry expiry list, the 32-per-bucket partition and the 8-removal replay rounds of a deactivation batch, the serial
path a rule with continuation blocks forces on its 64-block, the runs an install batch is cut into, the far-expiry heap
at the 64-position window boundary, and the default arena capacities.

Every builder returns (build(m), lex4, offs, origseg, claims): `build` drives an oracle.L2Matcher or the product's
PatternMatcherInstance, lex4 is (n,4) u32 [id, ordpos, origpos, origsize], `claims` names the numbers the case exists to
produce.  tests/test_l2_general_cases.py recomputes every claim with the plain model of tests/l2_general_model.py and
holds it to the thresholds of the kernel; tests/test_l2_general_edges_gpu.py runs the cases on the GPU.

Term ids are event handles (term events have type bits 0), so the trigger bucket of a term is evhash(id) & 15."""
import numpy as np

from .l2_general_model import bucket_of

FILLER = 7              # a term no rule waits for
LA, LB = 3, 4           # keys of the long-lived rules installed before and after the rules under test


def terms_in_bucket(bucket, count, start):
    """the first `count` term ids >= start whose events hash into `bucket`"""
    out = []
    t = start
    while len(out) < count:
        if bucket_of(t) == bucket:
            out.append(t)
        t += 1
    return out


def _documents(docs, segments=False):
    """docs: lists of (term id, ordinal position) -> lex4, offs, origseg"""
    rows, offs, seg = [], [0], []
    for doc in docs:
        last = 0
        for i, (tid, pos) in enumerate(doc):
            assert pos >= last and pos > 0
            last = pos
            rows.append((tid, pos, 3 * i, 2))
            seg.append(i // 90 if segments else 0)
        offs.append(len(rows))
    return np.array(rows, np.uint32).reshape(-1, 4), np.array(offs, np.uint64), np.array(seg, np.uint32)


def _rule(m, name, op, terms, rng, card=0, variables=()):
    for i, t in enumerate(terms):
        m.pushTerm(t)
        if i in variables:
            m.attachVariable("v%d" % i)
    m.pushExpression(op, len(terms), rng, card)
    m.definePattern(name, "", True)


def _long_lived(m, events, per_event, rng=60):
    """rules keyed by LA and by LB that wait for `events` (per_event[e] of each): they sit below and above the rules under
    test in the buckets, survive them, get moved by their removals and fire afterwards in bucket order"""
    for key, tag in ((LA, "a"), (LB, "b")):
        for e in events:
            for j in range(per_event.get(e, 1) if isinstance(per_event, dict) else per_event):
                _rule(m, "l%s_%d_%d" % (tag, e, j), "sequence", [key, e], rng, variables=(1,) if j % 2 else ())


class _Doc:
    def __init__(self):
        self.lex = []
        self.pos = 0

    def at(self, pos, *terms):
        assert pos >= self.pos
        self.pos = pos
        for t in terms:
            self.lex.append((t, pos))
        return self

    def step(self, *terms, by=1):
        return self.at(self.pos + by, *terms)

    def fill(self, until):
        while self.pos < until:
            self.step(FILLER)
        return self


# ---------------------------------------------------------------- expiry_list
EXPIRY_N = [63, 64, 65, 127, 128, 129, 130, 192, 193, 257]
EXPIRY_RANGE = 6
EXPIRY_EVENTS = [terms_in_bucket(b, 1, 2000)[0] for b in range(8)]        # 8 events in 8 buckets


def _expiry_build(m):
    for d, n in enumerate(EXPIRY_N):
        for i in range(n):
            _rule(m, "e%d_%d" % (d, i), "sequence", [10 + d, EXPIRY_EVENTS[i % 8]], EXPIRY_RANGE, variables=(1,) if i % 3 == 0 else ())
    _long_lived(m, EXPIRY_EVENTS, 3)


def _expiry_doc(d, holes):
    doc = _Doc()
    for base in (1, 100):
        # the long-lived rules, the N rules of key d, long-lived rules again; then nothing the N rules wait for until
        # they have expired (position of the key + range), then every event
        doc.at(base, LA).step(10 + d).step(LB)
        if holes:
            doc.step(EXPIRY_EVENTS[1]).step(EXPIRY_EVENTS[4], EXPIRY_EVENTS[6])
        doc.fill(base + 1 + EXPIRY_RANGE + 1)
        for e in EXPIRY_EVENTS:
            doc.step(e)
    return doc.lex


def expiry_list(holes=False):
    lex4, offs, seg = _documents([_expiry_doc(d, holes) for d in range(len(EXPIRY_N))])
    claims = {
        "expiring_per_document": list(EXPIRY_N),
        "max_expiring_at_one_position": max(EXPIRY_N),
        # (the rules that completed stay in the list of their position as entries without triggers)
        "holes_in_the_longest_list_per_document": [sum(1 for i in range(n) if i % 8 in (1, 4, 6)) if holes else 0 for n in EXPIRY_N],
    }
    return _expiry_build, lex4, offs, seg, claims


def expiry_list_holes():
    return expiry_list(True)


# ---------------------------------------------------------------- bucket_partition / dispose_by_firing
PARTITION_K = [8, 9, 16, 17, 32, 33, 64]
BUCKET_A, BUCKET_B = 5, 9
A_EVENTS = terms_in_bucket(BUCKET_A, 3, 3000)
B_EVENTS = terms_in_bucket(BUCKET_B, 2, 3000)
OTHER_EVENTS = [terms_in_bucket(b, 1, 3000)[0] for b in range(16) if b not in (BUCKET_A, BUCKET_B)]


def _partition_events(k, k2):
    """the awaited events of the 64 rules of a block: k in bucket A (two events), k2 in bucket B, the others spread"""
    ev = [A_EVENTS[i % 2] for i in range(k)] + [B_EVENTS[i % 2] for i in range(k2)]
    ev += [OTHER_EVENTS[i % len(OTHER_EVENTS)] for i in range(64 - len(ev))]
    order = np.random.default_rng(1000 + k).permutation(64)
    return [ev[i] for i in order]


def _partition_build(m):
    for d, (k, k2) in enumerate([(k, 0) for k in PARTITION_K] + [(31, 33)]):
        for i, e in enumerate(_partition_events(k, k2)):
            _rule(m, "p%d_%d" % (d, i), "sequence", [10 + d, e], EXPIRY_RANGE, variables=(1,) if i % 4 == 0 else ())
    per = {e: 1 for e in OTHER_EVENTS}
    per.update({e: 6 for e in A_EVENTS[:2] + B_EVENTS})
    _long_lived(m, A_EVENTS[:2] + B_EVENTS + OTHER_EVENTS, per)


def _partition_doc(d):
    doc = _Doc()
    for base in (1, 100):
        doc.at(base, LA).step(10 + d).step(LB)
        doc.fill(base + 1 + EXPIRY_RANGE + 1)
        for e in A_EVENTS[:2] + B_EVENTS + OTHER_EVENTS[:3]:
            doc.step(e)
    return doc.lex


def bucket_partition():
    lex4, offs, seg = _documents([_partition_doc(d) for d in range(len(PARTITION_K) + 1)])
    claims = {
        "block_bucket_max_per_document": PARTITION_K + [33],
        "max_triggers_of_one_block_in_one_bucket": 64,
        "two_buckets_of_one_block": [31, 33],
    }
    return _partition_build, lex4, offs, seg, claims


FIRED_Y, FIRED_Y2 = A_EVENTS[0], A_EVENTS[1]     # the event that completes the rules; another one in the same bucket
FIRED_DELIM = B_EVENTS[0]                        # a delimiter in bucket B
FIRED_Z = A_EVENTS[2]                            # delimiter and content term of the same rules
FIRED_DUP = 40


def _fired_build(m):
    for d, k in enumerate(PARTITION_K):
        for i in range(k):
            _rule(m, "f%d_%d" % (d, i), "sequence", [10 + d, FIRED_Y], 20, variables=(1,) if i % 4 == 0 else ())
    d = len(PARTITION_K)
    for i in range(33):     # 33 complete on one event: 33 triggers in its bucket, the 31 delimiter triggers in another
        if i % 16 == 7:
            _rule(m, "f%d_%d" % (d, i), "sequence", [10 + d, FIRED_Y], 20)
        else:
            _rule(m, "f%d_%d" % (d, i), "sequence_struct", [FIRED_DELIM, 10 + d, FIRED_Y], 20, variables=(2,) if i % 4 == 0 else ())
    d += 1
    for i in range(FIRED_DUP):      # deleted and finished by the same event: listed twice
        _rule(m, "f%d_%d" % (d, i), "sequence_struct", [FIRED_Z, 10 + d, FIRED_Z], 20, variables=(2,) if i % 4 == 0 else ())
    # (defined last = installed first: its single entry puts the two entries of a later rule on both sides of a block end)
    _rule(m, "f%d_odd" % d, "sequence", [10 + d, FIRED_Z], 20)
    _long_lived(m, [FIRED_Y2, FIRED_DELIM], 3)


def _fired_doc(d):
    doc = _Doc()
    for base in (1, 100):
        doc.at(base, LA).step(10 + d).step(LB).step(FILLER)
        doc.step(FIRED_Z if d == len(PARTITION_K) + 1 else FIRED_Y)
        doc.step(FIRED_Y2).step(FIRED_DELIM)
    return doc.lex


def dispose_by_firing():
    lex4, offs, seg = _documents([_fired_doc(d) for d in range(len(PARTITION_K) + 2)])
    claims = {
        "fired_list_max_per_document": PARTITION_K + [33, 2 * FIRED_DUP + 1],
        "two_buckets_of_one_block": [31, 33],
        "duplicate_entries": 2 * FIRED_DUP,               # both rounds of the document
        "duplicates_in_a_later_block": 2,
    }
    return _fired_build, lex4, offs, seg, claims


# ---------------------------------------------------------------- long_chain_in_block
CHAIN_CASES = [(64, 0), (64, 31), (64, 63), (65, 0), (65, 31), (65, 63), (65, 64)]       # (rules expiring, index of the wide one)
WIDE_TERMS = [terms_in_bucket(b, 1, 4000)[0] for b in (1, 5, 5, 9, 12)]
WIDE_TERMS[2] = terms_in_bucket(5, 2, 4000)[1]


def _chain_build(m):
    events = A_EVENTS[:2] + B_EVENTS + OTHER_EVENTS
    for d, (n, at) in enumerate(CHAIN_CASES):
        for i in range(n):
            if i == at:     # 5 installed triggers: one continuation block
                _rule(m, "c%d_wide" % d, "sequence", [10 + d] + WIDE_TERMS, EXPIRY_RANGE, variables=(1, 3))
            else:
                _rule(m, "c%d_%d" % (d, i), "sequence", [10 + d, events[i % len(events)]], EXPIRY_RANGE, variables=(1,) if i % 4 == 0 else ())
    _long_lived(m, events, 2)


def _chain_doc(d):
    doc = _Doc()
    events = A_EVENTS[:2] + B_EVENTS + OTHER_EVENTS
    for base in (1, 100):
        doc.at(base, LA).step(10 + d).step(LB)
        doc.step(WIDE_TERMS[0]).step(WIDE_TERMS[1])     # the wide rule gets two of its five terms
        doc.fill(base + 1 + EXPIRY_RANGE + 1)
        for e in events[:6]:
            doc.step(e)
    return doc.lex


def long_chain_in_block():
    lex4, offs, seg = _documents([_chain_doc(d) for d in range(len(CHAIN_CASES))])
    claims = {"expiring_per_document": [n for n, _ in CHAIN_CASES], "wide_rule_at_list_index": [at for _, at in CHAIN_CASES], "wide_rules_per_list": 1}
    return _chain_build, lex4, offs, seg, claims


# ---------------------------------------------------------------- install_runs
INSTALL_SIZES = [64, 65, 128, 129]
INSTALL_EVENTS = [terms_in_bucket(b, 1, 5000)[0] for b in range(16)]
FAR_RANGE = 70


def _install_slots(n):
    """what sits at slot s of the key list of a key with n programs"""
    plan = {0: "far", 1: "wide", 62: "bare", 63: "bare"}       # (the `any` program has two key triggers: listed twice)
    if n > 64:
        plan[64] = "far"
    return [plan.get(s, "plain") for s in range(n)]


def _install_build(m):
    for d, n in enumerate(INSTALL_SIZES):
        key = 10 + d
        slots = _install_slots(n)
        s = n - 1
        while s >= 0:               # a key list is walked last defined first
            kind = slots[s]
            e = INSTALL_EVENTS[s % 16]
            if kind == "far":
                _rule(m, "i%d_%d" % (d, s), "sequence", [key, e], FAR_RANGE, variables=(1,))
            elif kind == "wide":
                _rule(m, "i%d_%d" % (d, s), "within", [key, e, INSTALL_EVENTS[(s + 1) % 16], INSTALL_EVENTS[(s + 5) % 16]], 30, variables=(0, 2))
            elif kind == "bare":
                _rule(m, "i%d_%d" % (d, s), "any", [key, key], 9, card=2, variables=(0,))
                s -= 1
            else:
                op = ["sequence", "within", "sequence_imm"][s % 3]
                _rule(m, "i%d_%d" % (d, s), op, [key, e], 1 + (s * 7) % 63, variables=(s % 2,) if s % 3 else ())
            s -= 1
    _long_lived(m, INSTALL_EVENTS, 1)


def _install_doc(d):
    doc = _Doc()
    rng = np.random.default_rng(500 + d)
    doc.at(1, LA).step(10 + d).step(LB)
    for i in range(16):
        doc.step(INSTALL_EVENTS[(5 * i) % 16])
    doc.step(10 + d, 10 + d)                # the key twice at one position: freed rule records and chunks are reused
    for i in range(70):
        doc.step(INSTALL_EVENTS[int(rng.integers(0, 16))], by=int(rng.integers(0, 3)))
    doc.step(10 + d)
    for i in range(60):                     # a random tail
        doc.step([FILLER, 10 + d, LA][int(rng.integers(0, 12)) // 5] if i % 9 == 0 else INSTALL_EVENTS[int(rng.integers(0, 16))], by=int(rng.integers(0, 4)))
    return doc.lex


def install_runs():
    lex4, offs, seg = _documents([_install_doc(d) for d in range(len(INSTALL_SIZES))], segments=True)
    claims = {
        "programs_on_one_key_event": INSTALL_SIZES,
        "slow_program_slots": [0, 1, 62, 63, 64],
        "slow_program_kinds": ["bare_capture", "far", "wide"],
    }
    return _install_build, lex4, offs, seg, claims


ALT_KEY, ALT_STOP = 10, 11      # the key with many programs; the frequent term whose programs the optimizer moves onto it


def _install_alt_build(m):
    m.defineTermFrequency(ALT_KEY, 0.0001)
    m.defineTermFrequency(ALT_STOP, 1000.0)
    for s in range(70):
        e = INSTALL_EVENTS[s % 16]
        _rule(m, "k_%d" % s, ["sequence", "within"][s % 2], [ALT_KEY, e], 1 + (s * 5) % 63, variables=(1,) if s % 3 == 0 else ())
    _rule(m, "alt_seq", "sequence", [ALT_STOP, ALT_KEY], 5, variables=(0,))                 # replays the logged stop word
    _rule(m, "alt_within", "within", [ALT_STOP, ALT_KEY], 4, variables=(1,))
    _rule(m, "alt_match", "within", [ALT_STOP, ALT_KEY], 5, card=1, variables=(0,))          # ... and matches on the replay
    _rule(m, "alt_struct", "sequence_struct", [FILLER, ALT_STOP, ALT_KEY], 5, variables=(1,))  # ... cancelled by a later delimiter
    m.compile()


def install_runs_alt():
    docs = []
    for d in range(4):
        doc = _Doc()
        rng = np.random.default_rng(600 + d)
        doc.at(1, ALT_STOP).step(ALT_KEY)                           # replay in range
        doc.step(INSTALL_EVENTS[3]).step(ALT_STOP).step(FILLER).step(ALT_KEY)     # a delimiter between the two
        doc.step(ALT_STOP, by=3).step(ALT_KEY, by=5).step(ALT_KEY, by=1)          # at the end of the range, one behind it
        for i in range(80):
            t = [ALT_STOP, ALT_KEY, FILLER][int(rng.integers(0, 3))] if i % 4 == 0 else INSTALL_EVENTS[int(rng.integers(0, 16))]
            doc.step(t, by=int(rng.integers(0, 4)))
        docs.append(doc.lex)
    lex4, offs, seg = _documents(docs)
    # (the two `within` rules of the stop word are keyed by both of their terms: listed as they are and moved)
    claims = {"programs_on_one_key_event": [76] * 4, "alt_keyed_slots": [72, 73, 74, 75]}
    return _install_alt_build, lex4, offs, seg, claims


# ---------------------------------------------------------------- far_heap
HEAP_KEY, HEAP_NEAR_KEY = 10, 11
HEAP_RANGES = [64, 64, 64, 65, 65, 99, 100, 100, 100, 101, 126, 127, 127, 128, 128, 128, 129, 130, 190, 191, 191, 192, 192, 193,
               200, 200, 200, 200, 255, 256, 256, 257, 290, 299, 300, 300, 64, 128, 192, 256]
HEAP_EVENTS = [terms_in_bucket(b, 1, 6000)[0] for b in range(16)]


def _heap_build(m):
    for i, rg in enumerate(HEAP_RANGES):
        _rule(m, "h_%d" % i, ["sequence", "within"][i % 2], [HEAP_KEY, HEAP_EVENTS[i % 16]], rg, variables=(1,) if i % 3 == 0 else ())
    for i in range(20):
        _rule(m, "n_%d" % i, "sequence", [HEAP_NEAR_KEY, HEAP_EVENTS[(3 * i) % 16]], 1 + 3 * i, variables=(1,) if i % 2 else ())


def far_heap():
    ev = HEAP_EVENTS
    docs = []
    # window boundaries: the position lands on 64k-1, 64k, 64k+1
    d = _Doc().at(1, HEAP_KEY).step(HEAP_NEAR_KEY).step(HEAP_KEY)
    for pos in (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257):
        d.at(pos, ev[pos % 16], HEAP_NEAR_KEY if pos % 64 == 0 else ev[(pos + 7) % 16])
    d.at(301, ev[0]).step(ev[1], by=40)
    docs.append(d.lex)
    # one before, on and one after the position of a heap entry (ranges 99, 100, 101 from position 1; 126..130)
    d = _Doc().at(1, HEAP_KEY)
    for pos in (99, 100, 101, 102, 103, 126, 127, 128, 129, 130, 131, 132):
        d.at(pos, ev[pos % 16], ev[(pos + 3) % 16])
    d.step(HEAP_KEY).step(ev[2], by=63).step(ev[3]).step(ev[4], by=2).step(ev[5], by=64).step(ev[6], by=65).step(ev[7], by=200)
    docs.append(d.lex)
    # jumps of more than 64: the window loop stops after its 64 steps, the heap is emptied behind it
    d = _Doc().at(5, HEAP_KEY, HEAP_NEAR_KEY).at(200, ev[8], HEAP_KEY).at(201, ev[9]).at(330, ev[10], HEAP_KEY, HEAP_NEAR_KEY)
    d.at(395, ev[11]).at(460, HEAP_KEY).at(1000, ev[12], ev[13])
    docs.append(d.lex)
    # more far rules alive than the default heap holds: 8 x 40
    d = _Doc()
    for pos in range(1, 9):
        d.at(pos, HEAP_KEY)
    for pos in range(60, 140):
        d.at(pos, ev[pos % 16])
    d.at(190, HEAP_NEAR_KEY).at(191, ev[1]).at(192, ev[2], ev[3]).at(193, ev[4]).at(256, ev[5]).at(257, ev[6]).at(320, ev[7])
    docs.append(d.lex)
    # random tails
    for seed in (701, 702):
        rng = np.random.default_rng(seed)
        d = _Doc().at(1, HEAP_KEY)
        for i in range(200):
            t = [HEAP_KEY, HEAP_NEAR_KEY][i % 2] if rng.random() < 0.12 else ev[int(rng.integers(0, 16))]
            d.step(t, by=int(rng.choice([0, 1, 1, 1, 2, 5, 31, 63, 64, 65, 130])))
        docs.append(d.lex)
    lex4, offs, seg = _documents(docs, segments=True)
    claims = {"heap_peak": 324, "positions_mod_64": [0, 1, 63], "landings_at_heap_entries": [-1, 0, 1], "jumps_over_64": True,
              "tie_migrations": True, "disposed_behind_the_window": True}
    return _heap_build, lex4, offs, seg, claims


# ---------------------------------------------------------------- bucket_capacity
CAP_ONE_KEY, CAP_MANY_KEY = 10, 11
CAP_EVENTS = terms_in_bucket(BUCKET_A, 4, 7000)


def _capacity_build(m):
    for i in range(90):
        _rule(m, "one_%d" % i, "sequence", [CAP_ONE_KEY, CAP_EVENTS[0]], 50, variables=(1,) if i % 8 == 0 else ())
    for i in range(90):
        _rule(m, "many_%d" % i, "sequence", [CAP_MANY_KEY, CAP_EVENTS[1 + i % 3]], 50, variables=(1,) if i % 8 == 0 else ())


def bucket_capacity():
    docs = []
    for key, events in ((CAP_ONE_KEY, CAP_EVENTS[:1]), (CAP_MANY_KEY, CAP_EVENTS[1:])):
        for fire in (True, False):
            d = _Doc().at(1, key).step(key).step(FILLER).step(key)
            if fire:
                for e in events:            # the events that fire all of them
                    d.step(e)
            d.step(key, by=60).step(events[0])      # ... or they expire, and the records are used again
            docs.append(d.lex)
    lex4, offs, seg = _documents(docs)
    claims = {"max_triggers_in_one_bucket": 270, "events_in_it_per_document": [1, 1, 3, 3], "max_fired_list": 270}
    return _capacity_build, lex4, offs, seg, claims


CASES = {
    "expiry_list": expiry_list,
    "expiry_list_holes": expiry_list_holes,
    "bucket_partition": bucket_partition,
    "dispose_by_firing": dispose_by_firing,
    "long_chain_in_block": long_chain_in_block,
    "install_runs": install_runs,
    "install_runs_alt": install_runs_alt,
    "far_heap": far_heap,
    "bucket_capacity": bucket_capacity,
}
# the cases whose claim exceeds a default capacity of the arena: a device batch reports the arena status until it has grown
CAPACITY_CASES = ["expiry_list", "far_heap", "bucket_capacity"]
