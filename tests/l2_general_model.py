"""Plain Python restatement of the rule automaton (oracle/l2_oracle.cpp: doTransition, fireSignal, installProgram,
replayPastEvent, setCurrentPos) on the compiled table of `dumpTable()`, without captured items.  It exists to COUNT: how
many rules expire at one position, how many triggers of one 64-rule block of a deactivation list sit in one of the 16
trigger buckets, how many programs one key event installs and which of them leave the lane-parallel path of the general
kernel (csrc/l2_kernel.hip), how full the far-expiry heap and the buckets get.  The numbers are the `claims` of
tests/l2_general_cases.py.

The model keeps the orders that decide the firing order (bucket arrays with swap-with-last removal, LIFO lists per expiry
position, libstdc++ push_heap/pop_heap order of the far-expiry queue), so besides the statistics it reproduces the
oracle's results in their order; tests/test_l2_general_cases.py holds it to that on every case."""

SIG_ANY, SIG_SEQUENCE, SIG_SEQUENCE_IMM, SIG_WITHIN, SIG_DEL, SIG_AND = range(6)
WINDOW = 64          # DisposeWindowSize: expiry positions nearer than this are kept per position, later ones in the heap
BLOCK = 64           # rules per deactivation batch / programs per install batch of the kernel (one per lane)
MAXT = 3             # trigger templates the kernel's install batch handles (enum in l2_kernel.hip)


def evhash(a):
    a &= 0xFFFFFFFF
    a = (a + (~(a >> 5) & 0xFFFFFFFF)) & 0xFFFFFFFF
    a = (a + ((a << 3) & 0xFFFFFFFF)) & 0xFFFFFFFF
    a ^= a >> 4
    return a


def bucket_of(event):
    return evhash(event) & 15


class Program:
    __slots__ = ("initsigval", "initcount", "event", "handle", "range", "trigs")


class Table:
    """dumpTable() words: programs[1..n], keylist[event] = [(program, past event)] in installation order, stop words"""

    def __init__(self, words):
        w = [int(x) for x in words]
        nprg, nkeys, nstop = w[0], w[1], w[2]
        at = 3
        self.programs = {}
        for p in range(1, nprg + 1):
            g = Program()
            g.initsigval, g.initcount, g.event, g.handle, _fmt, g.range, ntrig = w[at:at + 7]
            at += 7
            g.trigs = [tuple(w[at + 5 * t:at + 5 * t + 5]) for t in range(ntrig)]     # (event, isKey, sigtype, sigval, variable)
            at += 5 * ntrig
            self.programs[p] = g
        self.keylist = {}
        for _ in range(nkeys):
            ev, n = w[at], w[at + 1]
            at += 2
            self.keylist[ev] = [(w[at + 2 * r], w[at + 2 * r + 1]) for r in range(n)]
            at += 2 * n
        self.stopwords = set(w[at:at + nstop])
        assert at + nstop == len(w)


class _Rule:
    __slots__ = ("program", "value", "count", "start", "end", "active", "done", "trigs", "nvars")


class _Trig:
    __slots__ = ("event", "rule", "sigtype", "sigval", "variable", "bucket", "pos")


class Automaton:
    def __init__(self, table):
        self.t = table
        self.curpos = 0
        self.buckets = [[] for _ in range(16)]
        self.window = [[] for _ in range(WINDOW)]       # per position, in definition order (walked last first)
        self.heap = []                                  # [pos, rule] in libstdc++ heap order
        self.stoplog = {}
        self.timestamp = 0
        self.ntrig = 0
        self.results = []                               # (handle, start ordpos, end ordpos) in firing order
        self.stats = [0, 0, 0, 0]                       # installed, alt-keyed installed, signals, sum of open triggers
        # what the cases claim
        self.expiry_lists = []          # per list of one position taken by setCurrentPos: (length, entries whose rule had
                                        # completed before and is inactive)
        self.blocks = []                # per 64-block of a deactivation list: dict (see _deactivate_list)
        self.fired_lists = []           # lengths of the lists of rules finished or deleted by one event
        self.key_events = []            # per key event with programs: dict (see _install_all)
        self.heap_peak = 0
        self.heap_migrated = 0          # entries moved from the heap into the window (curpos & 63 == 0)
        self.heap_tie_migrations = 0    # ... that had the same position as the entry migrated before them
        self.heap_disposed_directly = 0 # entries disposed by the jump behind the 64 window steps
        self.long_jumps = 0             # position steps of more than 64
        self.pos_mod64 = set()          # curpos & 63 of the positions the document lands on
        self.heap_landings = set()      # -1, 0, +1: a landing one before, on, one after the position of a heap entry
        self.bucket_peak = [0] * 16
        self.bucket_peak_events = [0] * 16      # distinct events in the bucket at its peak
        self.rules_peak = 0
        self.nrules = 0

    # ---- trigger buckets
    def _add_trigger(self, rule, event, sigtype, sigval, variable):
        t = _Trig()
        t.event, t.rule, t.sigtype, t.sigval, t.variable = event, rule, sigtype, sigval, variable
        t.bucket = bucket_of(event)
        b = self.buckets[t.bucket]
        t.pos = len(b)
        b.append(t)
        rule.trigs.append(t)
        self.ntrig += 1
        if len(b) > self.bucket_peak[t.bucket]:
            self.bucket_peak[t.bucket] = len(b)
            self.bucket_peak_events[t.bucket] = len(set(x.event for x in b))

    def _remove_trigger(self, t, doomed):
        b = self.buckets[t.bucket]
        assert b[t.pos] is t
        moved = 0
        last = b[-1]
        if last is not t:
            b[t.pos] = last
            last.pos = t.pos
            if id(last) not in doomed:
                moved = 1
        b.pop()
        self.ntrig -= 1
        return moved

    def _deactivate(self, rule, doomed=()):
        moved = 0
        if rule.active:
            rule.active = False
            for t in reversed(rule.trigs):              # the rule's trigger list: last installed first
                moved += self._remove_trigger(t, doomed)
            rule.trigs = []
            self.nrules -= 1
        return moved

    def _deactivate_list(self, rules, kind):
        """deactivateRule for a list in order; per 64-block of it (the kernel's deactivateBatch) the record
        {kind, n, per_bucket: removals per bucket, wide_at: list index of rules with more than 4 triggers,
         survivors_moved: triggers of other rules that a swap-with-last moved, dups: entries whose rule an earlier entry
         of the list has already deactivated, dup_blocks: blocks between such an entry and the first one}"""
        first_at = {}
        for base in range(0, len(rules), BLOCK):
            blk = rules[base:base + BLOCK]
            rec = {"kind": kind, "n": len(blk), "per_bucket": [0] * 16, "wide_at": [], "survivors_moved": 0, "dups": 0, "dup_blocks": []}
            doomed = set()
            for r in blk:
                if r.active:
                    for t in r.trigs:
                        doomed.add(id(t))
            for i, r in enumerate(blk):
                if id(r) in first_at:
                    rec["dups"] += 1
                    rec["dup_blocks"].append((base + i) // BLOCK - first_at[id(r)] // BLOCK)
                    continue
                first_at[id(r)] = base + i
                if r.active:
                    if len(r.trigs) > 4:
                        rec["wide_at"].append(base + i)
                    for t in r.trigs:
                        rec["per_bucket"][t.bucket] += 1
                rec["survivors_moved"] += self._deactivate(r, doomed)
            self.blocks.append(rec)

    # ---- far-expiry queue: std::push_heap / std::pop_heap with comp(a, b) = a.pos > b.pos
    def _heap_push(self, pos, rule):
        h = self.heap
        h.append(None)
        hole = len(h) - 1
        while hole > 0:
            parent = (hole - 1) >> 1
            if not h[parent][0] > pos:
                break
            h[hole] = h[parent]
            hole = parent
        h[hole] = (pos, rule)
        self.heap_peak = max(self.heap_peak, len(h))

    def _heap_pop(self):
        h = self.heap
        n = len(h)
        if n > 1:
            ln = n - 1
            value = h[ln]
            hole = child = 0
            while child < (ln - 1) // 2:
                child = 2 * (child + 1)
                if h[child][0] > h[child - 1][0]:
                    child -= 1
                h[hole] = h[child]
                hole = child
            if ln % 2 == 0 and child == (ln - 2) // 2:
                child = 2 * (child + 1)
                h[hole] = h[child - 1]
                hole = child - 1
            while hole > 0:
                parent = (hole - 1) >> 1
                if not h[parent][0] > value[0]:
                    break
                h[hole] = h[parent]
                hole = parent
            h[hole] = value
        h.pop()

    # ---- expiry
    def _define_dispose(self, pos, rule):
        assert pos >= self.curpos
        if pos < self.curpos + WINDOW:
            self.window[pos % WINDOW].append(rule)
        else:
            self._heap_push(pos, rule)

    def set_current_pos(self, pos):
        assert pos >= self.curpos
        if pos == self.curpos:
            return
        if pos - self.curpos > WINDOW:
            self.long_jumps += 1
        for hp, _ in self.heap:
            if -1 <= pos - hp <= 1:
                self.heap_landings.add(pos - hp)
        wcnt = 0
        while wcnt < WINDOW and self.curpos < pos:
            widx = self.curpos % WINDOW
            if widx == 0:
                before = None
                while self.heap and self.heap[0][0] < self.curpos + WINDOW:
                    wcnt = 0
                    hp, hr = self.heap[0]
                    self.window[hp % WINDOW].append(hr)
                    self._heap_pop()
                    self.heap_migrated += 1
                    if hp == before:
                        self.heap_tie_migrations += 1
                    before = hp
            lst = self.window[widx]
            if lst:
                self.window[widx] = []
                self.expiry_lists.append((len(lst), sum(1 for r in lst if not r.active)))
                self._deactivate_list(lst[::-1], "expiry")
            wcnt += 1
            self.curpos += 1
        if self.curpos < pos:
            self.curpos = pos
            while self.heap and self.heap[0][0] < self.curpos:
                self._deactivate(self.heap[0][1])
                self._heap_pop()
                self.heap_disposed_directly += 1
        self.pos_mod64.add(pos % WINDOW)

    # ---- signals
    def _fire(self, rule, sigtype, sigval, variable, sord, eord, dispose, follow):
        self.stats[2] += 1
        match = take = fin = False
        if sigtype == SIG_ANY:
            take = True
            if rule.count > 0:
                match = True
                rule.count -= 1
                fin = rule.count == 0
                rule.end = max(rule.end, eord)
        elif sigtype == SIG_AND:
            if rule.count > 0:
                if not rule.value:
                    rule.value = sord
                    rule.end = min(rule.end, eord)
                if rule.value == sord:
                    match = take = True
                    rule.count -= 1
                    fin = rule.count == 0
        elif sigtype in (SIG_SEQUENCE, SIG_SEQUENCE_IMM, SIG_WITHIN):
            if sigtype == SIG_WITHIN:
                ok = (sigval & rule.value) != 0 and rule.end <= sord
            else:
                ok = sigval == rule.value and (rule.end <= sord if sigtype == SIG_SEQUENCE else rule.end == sord)
            if ok:
                rule.end = eord
                rule.value = (rule.value & ~sigval) if sigtype == SIG_WITHIN else sigval - 1
                if rule.count > 0:
                    rule.count -= 1
                    match = rule.count == 0
                else:
                    match = True
                fin = rule.value == 0
                take = True
        else:
            rule.count = rule.value = 0
            dispose.append(rule)
            return False
        bare = False
        if take:
            if variable:
                rule.nvars += 1
            if rule.start == 0 or rule.start > sord:
                rule.start = sord
        if match:
            if not rule.done:
                g = self.t.programs[rule.program]
                bare = rule.nvars == 0
                if g.event:
                    follow.append((g.event, rule.start, rule.end))
                if g.handle:
                    self.results.append((g.handle, rule.start, rule.end))
                rule.done = True
            if fin:
                dispose.append(rule)
        return bare

    def _replay(self, rule, past, rng):
        lg = self.stoplog.get(past)
        if lg is None or lg[0] + rng < self.curpos:
            return
        dispose, follow, dels = [], [], []
        for t in reversed(list(rule.trigs)):
            if t.sigtype == SIG_DEL:
                dels.append(t.event)
            if t.event == past:
                self._fire(rule, t.sigtype, t.sigval, t.variable, lg[0], lg[1], dispose, follow)
        for ev in dels:
            other = self.stoplog.get(ev)
            if other is not None and other[2] > lg[2]:
                self._deactivate(rule)
                break
        for r in dispose:
            self._deactivate(r)
        assert not follow

    def _install(self, keyevent, program, past, sord, eord, dispose, follow):
        """-> how the kernel's install batch sees the program: None (not installed: expired) or a set of
        'far', 'wide', 'alt', 'bare_capture'"""
        g = self.t.programs[program]
        if sord + g.range < self.curpos:
            return None
        kinds = set()
        if sord + g.range >= self.curpos + WINDOW:
            kinds.add("far")
        if len(g.trigs) > MAXT:
            kinds.add("wide")
        if past:
            kinds.add("alt")
        r = _Rule()
        r.program, r.value, r.count, r.start, r.end = program, g.initsigval, g.initcount & 0xFFFF, 0, 0
        r.active, r.done, r.trigs, r.nvars = True, False, [], 0
        self.nrules += 1
        self.rules_peak = max(self.rules_peak, self.nrules)
        self._define_dispose(sord + g.range, r)
        keys = []
        has_key = False
        for ev, is_key, sigtype, sigval, variable in g.trigs:
            install = True
            if ev == keyevent:
                keys.append((sigtype, sigval, variable))
                needs = sigtype == SIG_ANY and r.count > 1
                if is_key and not has_key:
                    has_key = True
                    install = needs
                elif sigtype == SIG_DEL:
                    install = needs
            if install:
                self._add_trigger(r, ev, sigtype, sigval, variable)
        self.stats[0] += 1
        if past:
            self.stats[1] += 1
            self._replay(r, past, g.range)
        if keys and r.active:
            bare = False
            for sigtype, sigval, variable in keys:
                bare = self._fire(r, sigtype, sigval, variable, sord, eord, dispose, follow) or bare
            if bare and r.nvars:
                kinds.add("bare_capture")       # a result staged before the rule had captured anything, then a capture
        return kinds

    def _install_all(self, ev, sord, eord, dispose, follow):
        lst = self.t.keylist.get(ev)
        if not lst:
            return
        rec = {"event": ev, "programs": len(lst), "slow_slots": {}, "alt_slots": [], "expiry_positions_per_batch": []}
        positions = set()
        for slot, (program, past) in enumerate(lst):
            if slot % BLOCK == 0 and slot:
                rec["expiry_positions_per_batch"].append(len(positions))
                positions = set()
            kinds = self._install(ev, program, past, sord, eord, dispose, follow)
            if kinds is None:
                continue
            if "alt" in kinds:
                rec["alt_slots"].append(slot)
            slow = kinds - {"alt"}
            if slow:
                rec["slow_slots"][slot] = sorted(slow)
            else:
                positions.add(sord + self.t.programs[program].range)
        rec["expiry_positions_per_batch"].append(len(positions))
        self.key_events.append(rec)

    def put(self, event, sord):
        """one lexem (term event) at ordinal position sord"""
        if sord > self.curpos:
            self.set_current_pos(sord)
        self.stats[3] += self.ntrig
        follow = [(event, sord, sord + 1)]
        fi = 0
        while fi < len(follow):
            ev, s, e = follow[fi]
            fi += 1
            dispose = []
            for t in [x for x in self.buckets[bucket_of(ev)] if x.event == ev]:
                self._fire(t.rule, t.sigtype, t.sigval, t.variable, s, e, dispose, follow)
            self._install_all(ev, s, e, dispose, follow)
            if dispose:
                self.fired_lists.append(len(dispose))
                self._deactivate_list(dispose, "fired")
            if ev in self.t.stopwords:
                self.timestamp += 1
                self.stoplog[ev] = (s, e, self.timestamp)


def run_document(table, lex):
    """lex: rows [id, ordpos, ...] of one document -> the Automaton after it"""
    a = Automaton(table)
    for row in lex:
        a.put(int(row[0]), int(row[1]))
    return a
