"""Tables and document sets of the tests of the cluster-per-lane handler route of the lexer's post-processing kernel
(postDocumentClusters), shared by the CPU guards (tests/test_l1_post_model.py: what every batch is meant to contain, said by
tests/l1_post_model.py) and the GPU tests (tests/test_l1_post_gpu.py).  The kernel has no counter that says which path a
cluster took, so every structure is placed at every window phase: behind k = 0..64 isolated words (one report, one event,
one boundary each) and in front of a tail of 70 of them.  Every table is one of the words kernel (whole-word literals,
prefix, suffix and previous-word shapes) with scanned automaton expressions beside them, and binds every lexem as
content: the lexems of a document are its events.  A batch stays under 48 KB of text, the two batches at the capacity of
the event array and at the lexem size limit excepted."""
import functools

from tests import l1_post_model as model
from tests import l1_words_cases as wcases

ISO = b"k"                  # the isolated word
PHASES = range(65)
TAIL = 70
NUMBER = ("[0-9]+[.][0-9]", 1)
DOTTED = ("[a-z]+[.][a-z]+", 3)
SUB = ("\\b(x)([a-z]+)(y)\\b", 2, 2)            # (expression, level, result index)

# (expression, level) or (expression, level, result index); the lexem id is 1 + the index in the list
TABLES = {
    # bandana 5, banananana 6, bananana 7 and banana 8 events of one span and level: 6 fit a lane, 7 do not
    "survivors": [("\\bk\\b", 1), ("\\bba[a-z]*\\b", 2), ("\\bban[a-z]*\\b", 2), ("\\bbana[a-z]*\\b", 2), ("[a-z]+na\\b", 2), ("[a-z]+ana\\b", 2),
                  ("[a-z]+nana\\b", 2), ("\\bbanana\\b", 2), ("\\b(banana|bandana)\\b", 2), ("\\b(bananana|zz)\\b", 2), ("\\bmm\\b", 1), NUMBER],
    # bananana: six events of level 1, then one of level 2 that deletes them; banananana: six, then a seventh; cananana:
    # six of level 3, then three reports of level 1 they make the handler ignore
    "levels": [("\\b(cananana|yy)\\b", 3), ("\\b(cananana|xx)\\b", 3), ("\\b(cananana|ww)\\b", 3), ("\\bk\\b", 1),
               ("\\bba[a-z]*\\b", 1), ("\\bban[a-z]*\\b", 1), ("\\bbana[a-z]*\\b", 1), ("\\bca[a-z]*\\b", 3), ("\\bcan[a-z]*\\b", 3), ("\\bcana[a-z]*\\b", 3),
               ("[a-z]+na\\b", 1), ("[a-z]+ana\\b", 1), ("[a-z]+nana\\b", 1), ("\\b(bananana|zz)\\b", 2), ("\\b(banananana|vv)\\b", 1), NUMBER],
    # "aa " * r: every "aa" and every "aa aa" -- one cluster of 2r + 1 reports with the word behind it, one more with kab
    "chain": [("\\bk\\b", 1), ("\\baa\\b", 1), ("\\baa\\s\\w+\\b", 1), ("[a-z]+ab\\b", 1), ("\\bkab\\b", 1), ("\\bzab\\b", 1), ("\\b(zab|zz)\\b", 1), NUMBER],
    # starts and ends that tie, a start one above the one before, a selection that moves its end to the left, a symbol
    "bounds": [("\\bk\\b", 1), ("[.][a-z]+", 2), ("\\bbanana\\b", 1), ("[a-z]+na\\b", 1), ("\\bx[a-z]*\\b", 1), SUB,
               ("\\bmm\\b", 1), ("\\bmm\\s\\w+\\b", 2), ("\\bnn\\b", 1), ("[w]", 1)],
    # both queues: a dotted pair ends where a suffix shape ends, its expression defined before and after the shape's;
    # an alternation of more positions than an automaton word holds (several patterns entries)
    "merge": [("\\bk\\b", 1), DOTTED, ("[a-z]+ab\\b", 2), ("[a-z]+[.]c[a-z]+", 1), NUMBER, ("\\bkab\\b", 1),
              ("(" + "|".join("[a-z]%s[.]q" % (c * 11) for c in "bcdefgh") + "|[a-z]+[.]q)", 2), ("\\bq\\b", 1)],
    "capacity": [("\\ba\\b", 1), NUMBER],
    "lexemsize": [("\\bab[a-z]*\\b", 1), ("\\bk\\b", 1), NUMBER],
}
SYMBOLS = {"bounds": [(900, 9, b"nn")]}        # (symbol id, lexem id, text)


def build(x, name):
    for i, d in enumerate(TABLES[name]):
        x.defineLexem(i + 1, d[0], d[2] if len(d) > 2 else 0, d[1], "content")
    for sym, lid, text in SYMBOLS.get(name, []):
        x.defineSymbol(sym, lid, text)
    x.compile()


def symbols(name):
    return dict(((lid, text), sym) for sym, lid, text in SYMBOLS.get(name, []))


@functools.lru_cache(maxsize=None)
def tables(name):
    """the compiled tables of the product (host side only, no GPU)"""
    import struspattern_amd as spa
    from tests.l1_table_sim import Tables
    lx = spa.PatternLexerInstance()
    build(lx, name)
    return Tables(lx.dumpTables())


offsets = wcases.offsets


def iso(n):
    return (ISO + b" ") * n


def sweep(structure):
    """the structure behind 0..64 isolated words and in front of 70"""
    return [iso(k) + structure + b" " + iso(TAIL) for k in PHASES]


def chain(r, last=b"k"):
    return b"aa " * r + last


SPLIT_WORD = b"kbbbbbbbbbbb.q"        # two alternatives of the wide alternation end here, one in either patterns entry

# structure -> text, per table; the guards say from the model's trace what each one is
STRUCTURES = {
    "survivors": {
        "five": b"bandana", "six": b"banananana", "seven": b"bananana", "eight": b"banana",
        "hard_then_hard": b"banana k k bananana", "hard_middle": b"k bandana banana banananana k",
    },
    "levels": {"six_deleted": b"bananana", "six_and_a_seventh": b"banananana", "six_and_ignored": b"cananana"},
    "chain": {
        "cluster_63": chain(31), "cluster_65": chain(32), "cluster_127": chain(63), "cluster_62": chain(30, b"kab"), "cluster_64": chain(31, b"kab"),
        "cluster_128": chain(63, b"kab"), "cluster_129": chain(63, b"zab"), "cluster_201": chain(100),
    },
    "bounds": {
        "same_start": b"mm k", "same_end": b"mm banana", "same_end_same_start": b"banana", "start_one_above": b"k.mm", "selection_moves_end": b"xkky",
        "reaches_back": b"mm k k mm k", "symbol": b"nn", "symbol_in_cluster": b"mm nn", "end_one_above": b"mm k www",
        # [w] reports inside the word behind "mm": the match of \\bmm\\s\\w+\\b comes 124 records behind the report of "mm"
        "reaches_back_far": b"mm " + b"w" * 123,
    },
    "merge": {"tie": b"x.cab", "tie_twice": b"x.cab k x.cab x.cab", "split_group": SPLIT_WORD, "dotted": b"k.k k k.k"},
}


@functools.lru_cache(maxsize=None)
def sweep_docs(name):
    """(documents, what each one is: (structure, phase))"""
    docs, what = [], []
    for s, text in STRUCTURES[name].items():
        for k, d in zip(PHASES, sweep(text)):
            docs.append(d)
            what.append((s, k))
    return docs, what


@functools.lru_cache(maxsize=None)
def sweep_batches(name):
    """the sweep documents of a table cut into the fewest batches of less than 48 KB, of about the same size:
    [(documents, what)]"""
    docs, what = sweep_docs(name)
    total = sum(len(d) for d in docs)
    parts = -(-total // (47 * 1024))
    out, at, size = [], 0, 0
    for i, d in enumerate(docs):
        if size + len(d) > -(-total // parts) + 1024 and i > at:
            out.append((tuple(docs[at:i]), tuple(what[at:i])))
            at, size = i, 0
        size += len(d)
    out.append((tuple(docs[at:]), tuple(what[at:])))
    assert all(sum(len(d) for d in b) < 48 * 1024 and len(b) >= 20 for b, w in out)
    return out


@functools.lru_cache(maxsize=None)
def ending_docs():
    """(documents, what) for the `survivors` table: documents that end exactly at 63, 64, 65, 127, 128 and 129 live
    records -- in isolated words, with a cluster of 5 or a hard one of 7 as the first and as the last thing; the empty
    document"""
    docs, what = [], []
    for n in (63, 64, 65, 127, 128, 129):
        docs.append(iso(n)); what.append(("isolated", n))
        docs.append(b"bandana " + iso(n - 5)); what.append(("cluster_first", n))
        docs.append(iso(n - 5) + b"bandana"); what.append(("cluster_last", n))
        docs.append(b"bananana " + iso(n - 7)); what.append(("hard_first", n))
        docs.append(iso(n - 7) + b"bananana"); what.append(("hard_last", n))
    docs.append(iso(63) + ISO); what.append(("isolated_no_blank", 64))
    docs.append(b""); what.append(("empty", 0))
    return docs, what


@functools.lru_cache(maxsize=None)
def long_docs():
    """(documents, what) for the `chain` table, of more than a chunk of 1024 bytes: a cluster across the chunk boundary,
    a cluster over several chunks, chunks in which only one of the queues has records, last chunks without any"""
    docs = [iso(500) + chain(20) + b" " + iso(100), b"1.5 " * 300 + b" " * 1100 + chain(5), chain(400) + b" " * 1500, iso(40) + b" " * 1200 + b"1.5 k 1.5"]
    return docs, ["across", "one_queue_each", "over_chunks", "gap"]


@functools.lru_cache(maxsize=None)
def queue_docs():
    """(documents, what) for the `merge` table: reports of the words kernel only, of the automaton only, more of the one
    than of the other in one refill, more than 64 of one queue in front of the first of the other"""
    one = b"1.5 "
    # (a cluster of two in front of each: "m.mm" of the automaton's queue alone, "kab" of the word queue alone)
    docs = [b"kab " + iso(150), b"m.mm " + one * 150, b"m.mm " + (one * 3 + iso(1)) * 60, b"kab " + (iso(3) + one) * 60, b"kab " + iso(70) + one * 70 + iso(70),
            b"m.mm " + one * 70 + iso(70) + one * 70, (b"x.cab " + one) * 50, b"kab " + iso(62) + one * 64 + iso(64) + one]
    what = ["words_only", "automaton_only", "more_a", "more_b", "words_first", "automaton_first", "ties", "whole_batches"]
    # the group of the wide alternation (two records of one definition and one end) at the records 58.. to 67.. of its queue
    for j in SPLIT_AT:
        docs.append(one * j + SPLIT_WORD + b" " + iso(5)); what.append(("split_group_at", j))
    return docs, what


SPLIT_AT = range(57, 67)
CAP = model.EVENT_CAP
CAPACITY_EVENTS = [CAP - 3, CAP - 2, CAP - 1, CAP]


@functools.lru_cache(maxsize=None)
def capacity_docs():
    """"a " * E: E reports, E events, for E around the capacity of the event array, a short document between any two"""
    docs = []
    for e in CAPACITY_EVENTS:
        docs += [b"a " * e, b"a a 1.5 a"]
    return docs


@functools.lru_cache(maxsize=None)
def lexemsize_docs():
    """a word of 65534 bytes (the longest lexem) and one of 65535 under a prefix shape, short documents around them"""
    return [b"k abk k", b"k " + b"ab" + b"k" * 65532 + b" k", b"abk", b"k " + b"ab" + b"k" * 65533 + b" k", b"k abkk"]


CHUNKS = [64, 1024]
