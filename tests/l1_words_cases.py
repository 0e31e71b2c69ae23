"""Tables and document sets of the tests of the words kernel of the lexer (whole-word literals and word shapes), shared
by the CPU guards (tests/test_l1_words_model.py: what every batch is meant to contain, said by the model) and the GPU
tests (tests/test_l1_words_gpu.py).  Everything is deterministic and small: a batch stays under 48 KB of text, so the
oracle (a Thompson simulation) takes seconds."""
import functools
import random

from tests import l1_words_model as model

NUMBER = ("[0-9]+[.][0-9]+", 2, "content")      # one scanned automaton expression in every table: the two-queue merge stays in play


def word(n, salt=0):
    """a word of n letters a..j, the same first 16 bytes for every salt-free length"""
    return bytes(0x61 + (i * 7 + i // 10 + salt) % 10 for i in range(n))


def _differs_at(w, at):
    """w with its byte `at` (1-based) replaced: equal before it"""
    return w[:at - 1] + (b"j" if w[at - 1:at] != b"j" else b"i") + w[at:]


LIT_LENGTHS = [1, 3, 4, 5, 8, 12, 15, 16, 17, 18, 19, 20, 31, 32, 33, 63, 64]
LITS = dict((n, word(n)) for n in LIT_LENGTHS)
LIT_TWINS = [_differs_at(LITS[17], 17), _differs_at(LITS[20], 20), _differs_at(LITS[64], 64)]
LIT65 = word(65)
SHARED_LITERAL = LITS[3]
# the longest word an expression \bW\sE\b takes (W, the separator and E have to fit one automaton word of 64 positions)
PREV_LONG = [61, 62]
PREV_TOO_LONG = [63, 64]
ALL_VARIANTS_WORD = b"abcdefgxdcab"     # bytes [0,2) [0,4) [1,3) [2,6) [3,7) and the last 2, 3, 4: every variant of `keys`, and a literal


def _lits():
    out = [("\\b%s\\b" % LITS[n].decode(), 1 + i % 3, ("content", "successor", "predecessor")[i % 3]) for i, n in enumerate(LIT_LENGTHS)]
    out += [("\\b%s\\b" % w.decode(), 2, "content") for w in LIT_TWINS]
    s = SHARED_LITERAL.decode()
    out += [("\\b(%s|xyz)\\b" % s, 1, "content"), ("\\b(y|%s)\\b" % s, 3, "successor"), NUMBER]
    return out


def _keys(prev):
    out = [("\\bab[a-z]*\\b", 1, "content"), ("\\babcd[a-z]*\\b", 2, "content"), ("\\b[a-z]bc[a-z]*\\b", 3, "predecessor"),
           ("\\b[a-z][a-z]cdef[a-z]*\\b", 1, "content"), ("\\b[a-z][a-z][a-z]defg\\w*\\b", 2, "successor"),
           ("[a-z]+ab\\b", 1, "content"), ("[a-z]+cab\\b", 3, "content"),
           # the same (tag, key) again: lists of 3 (PREFIX(0,2) "ab") and of 2 (SUFFIX(2) "ab")
           ("\\bab\\w*\\b", 2, "content"), ("\\bab[a-j]*\\b", 3, "successor"), ("\\b[a-z]+ab\\b", 2, "predecessor"),
           # other keys of the same variants
           ("\\bba[a-z]*\\b", 1, "content"), ("[a-z]+ba\\b", 2, "content"), ("\\b[a-z]cd\\w*\\b", 1, "content"),
           ("\\b%s\\b" % ALL_VARIANTS_WORD.decode(), 1, "content"), ("\\bab\\b", 2, "content"), ("\\b(cab|dcab|b)\\b", 1, "content"), NUMBER]
    if prev:
        out += [("\\bab\\s\\w+\\b", 1, "content"), ("\\bab[-][a-z]{2,}\\b", 2, "content"), ("\\ba[^\\w]\\w+\\b", 3, "content")]
    else:
        out += [("[a-z]+dcab\\b", 2, "content"), ("[a-z]+xcab\\b", 1, "content")]
    return out


def _variants12():
    """12 variants: 8 with two expressions each, 4 with one"""
    two = ["\\bab[a-z]*\\b", "\\bba[a-z]*\\b", "\\babc[a-z]*\\b", "\\bbcd[a-z]*\\b", "\\babcd[a-z]*\\b", "\\bbcda[a-z]*\\b",
           "\\b[a-z]bc[a-z]*\\b", "\\b[a-z]cd[a-z]*\\b", "\\b[a-z]bcd[a-z]*\\b", "\\b[a-z]cda[a-z]*\\b",
           "[a-z]+ab\\b", "[a-z]+ba\\b", "[a-z]+cab\\b", "[a-z]+dab\\b", "\\bab\\s\\w+\\b", "\\bb\\s\\w+\\b"]
    one = ["\\b[a-z][a-z]cd[a-z]*\\b", "\\b[a-z][a-z]cdef[a-z]*\\b", "\\b[a-z][a-z][a-z]defg\\w*\\b", "[a-z]+dcab\\b"]
    return [(e, 1 + i % 3, "content") for i, e in enumerate(two + one)] + [("\\bab\\b", 2, "content"), NUMBER]


VARIANTS12_DROPPED = [model.PREFIX | (2 << 2) | (2 << 4), model.PREFIX | (2 << 2) | (4 << 4), model.PREFIX | (3 << 2) | (4 << 4), model.SUFFIX | (4 << 4)]


def _prev():
    w61, w62 = word(61, 3).decode(), word(62, 5).decode()
    return [("\\ba\\s\\w+\\b", 1, "content"), ("\\bab\\s\\w+\\b", 2, "content"), ("\\bab[-][a-z]{2,}\\b", 3, "successor"),
            ("\\b%s[-]\\w+\\b" % w61, 1, "content"), ("\\b%s\\s\\w+\\b" % w62, 2, "predecessor"), ("\\bc[,;][a-z]{2,}\\b", 1, "content"),
            # (a negated class is no separator of a PREVWORD shape: this one stays in the scanned pass)
            ("\\bc[^\\w][a-z]{2,}\\b", 2, "content"), ("\\bab\\s[a-z]+ing\\b", 3, "content"), ("\\bdd[-][a-z]+ing\\b", 1, "content"), ("\\bab\\b", 2, "content"), ("\\b[a-z]+\\b", 1, "content"), NUMBER]


def _ring():
    return [("\\bab[a-z]*\\b", 1, "content"), ("[a-z]+ab\\b", 2, "content"), ("\\b[a-z]+ab\\b", 3, "successor"), ("\\bab\\s\\w+\\b", 1, "content"),
            ("\\bab\\b", 2, "content"), NUMBER]


def _dense():
    return [("\\ba\\b", 1, "content"), ("\\b(a|b)\\b", 2, "content"), ("\\b(zz|a)\\b", 3, "successor"),
            ("\\ba\\s\\w+\\b", 1, "content"), ("\\ba\\s[a-z]+\\b", 2, "content"), ("\\bb\\s\\w+\\b", 3, "content"),
            ("\\bab[a-z]*\\b", 1, "content"), ("\\bab\\w*\\b", 2, "predecessor"), ("[a-z]+ab\\b", 1, "content"), ("\\bba\\w*\\b", 3, "content"),
            ("[a-z]+ba\\b", 1, "content"), ("\\bab\\b", 2, "content"), ("\\b(ab|ba)\\b", 1, "content"), ("\\bab\\s\\w+\\b", 2, "content"),
            ("\\bba\\s\\w+\\b", 3, "content"), NUMBER]


TABLES = {"lits": _lits(), "keys": _keys(False), "keys_prev": _keys(True), "variants12": _variants12(), "prev": _prev(), "ring": _ring(),
          "dense": _dense()}
PREV_W61, PREV_W62 = word(61, 3), word(62, 5)


def build(x, name):
    for i, (expr, level, bind) in enumerate(TABLES[name]):
        x.defineLexem(i + 1, expr, 0, level, bind)
    x.compile()


@functools.lru_cache(maxsize=None)
def tables(name, shapes=True):
    """the compiled tables of the product (host side only, no GPU); shapes=False: compiled with SPA_L1_SHAPES=0, every
    expression in the scanned passes"""
    import os
    import struspattern_amd as spa
    from tests.l1_table_sim import Tables
    lx = spa.PatternLexerInstance()
    old = os.environ.get("SPA_L1_SHAPES")
    try:
        if shapes:
            os.environ.pop("SPA_L1_SHAPES", None)
        else:
            os.environ["SPA_L1_SHAPES"] = "0"
        build(lx, name)
    finally:
        if old is None:
            os.environ.pop("SPA_L1_SHAPES", None)
        else:
            os.environ["SPA_L1_SHAPES"] = old
    return Tables(lx.dumpTables())


def offsets(docs):
    import numpy as np
    offs = np.zeros(len(docs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in docs])
    return offs


# ---------------------------------------------------------------- text
FILLER_WORDS = [b"k", b"kk", b"mmm", b"nkm", b"kmnk", b"mnmnmn", b"42", b"3.14", b"n"]


def filler(rng, n, digits=True):
    """n bytes whose runs match nothing of the tables' literals and shapes; ends with a blank"""
    words = FILLER_WORDS if digits else [w for w in FILLER_WORDS if not w[:1].isdigit()]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + rng.choice([b" ", b" ", b"  ", b". ", b"\n"])
    out = out[:n]
    if n:
        out[n - 1:n] = b" "
    if n >= 2 and out[n - 2:n - 1] == b"." and n >= 3 and out[n - 3:n - 2].isdigit():
        out[n - 2:n - 1] = b" "
    return bytes(out)


def long_word(n):
    """a run of n letters that starts and ends with "ab": \\bab[a-z]*\\b and [a-z]+ab\\b match it whole"""
    assert n >= 5
    return b"ab" + b"k" * (n - 4) + b"ab"


def _place(rng, n, at, what):
    """a document of n bytes: filler with `what` at offset `at`, a blank on either side of it where there is room"""
    d = bytearray(filler(rng, n))
    assert 0 <= at and at + len(what) <= n, (n, at, len(what))
    d[at:at + len(what)] = what
    if at > 0:
        d[at - 1:at] = b" "
    if at >= 2 and d[at - 2:at - 1] == b".":
        d[at - 2:at - 1] = b" "
    if at + len(what) < n:
        d[at + len(what):at + len(what) + 1] = b" "
    return bytes(d)


TILE_OFFSETS = [0, 1, 62, 63, 64, 65, 127, 128]
RUN_LENGTHS = [63, 64, 65, 66, 128, 130]
DOC_LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129]
FEATURES = [ALL_VARIANTS_WORD, b"ab " + ALL_VARIANTS_WORD, LITS[64], LIT_TWINS[0], LITS[20], LITS[33], b"a kk", b"ab going", PREV_W62 + b" mm",
            PREV_W61 + b"-kk", b"ab-kk", b"xyzdefg", LITS[17], LIT_TWINS[2], b"c,kk", b"dd-going", LITS[63], b"abcd"]
# pLen equal to o + k (or k) of every variant of `keys`, and one less
KEY_EDGE_WORDS = [b"ab", b"a", b"abcd", b"abc", b"xbc", b"xb", b"xycdef", b"xycde", b"xyzdefg", b"xyzdef", b"cab", b"dcab", b"xcab", b"b", b"kab", b"ba"]


@functools.lru_cache(maxsize=None)
def edge_docs(chunk=None):
    """(documents, what each one is): a planted word or word pair in filler -- starting at, ending at and straddling the
    tile offsets, runs of the lengths around the cap of 64/65, documents of the edge lengths that end in a word and in a
    separator, literals within the last bytes of a document, words and predecessors in the first bytes, separators of
    several bytes.  (The chunk only seeds the filler: the tile offsets count from the document's first byte.)"""
    rng = random.Random(4100 + (chunk or 0))
    docs, what = [], []

    def add(kind, d):
        docs.append(d)
        what.append(kind)
    turn = 0
    for p in TILE_OFFSETS:
        for how in ("starts", "ends", "straddles"):
            if how != "starts" and p == 0:
                continue
            for _ in range(2):
                # (the next feature in turn that has room before the offset; one and two letters at offset 1)
                room = [f for f in FEATURES[turn % len(FEATURES):] + FEATURES[:turn % len(FEATURES)] if how == "starts" or (len(f) if how == "ends" else len(f) // 2) <= p]
                f = room[0] if room and p > 1 else FEATURES[turn % len(FEATURES)] if how == "starts" else b"a" if how == "ends" else b"ab"
                turn += 1
                at = p if how == "starts" else p - len(f) if how == "ends" else p - len(f) // 2
                add("%s_%d" % (how, p), _place(rng, at + len(f) + 40, at, f))
    for n in RUN_LENGTHS:
        add("run_%d" % n, _place(rng, n + 90, 37, long_word(n)))
        add("prev_run_%d" % n, _place(rng, n + 90, 29, b"k" * n + b" going"))
    add("lit_63", _place(rng, 150, 41, LITS[63]))
    add("lit_64", _place(rng, 150, 41, LITS[64]))
    add("lit_65", _place(rng, 150, 41, LIT65))
    add("all_literals", b"kk " + b" ".join([LITS[n] for n in LIT_LENGTHS] + LIT_TWINS + [b"xyz", b"y", LIT65]) + b".")
    add("len_0", b"")
    for n in DOC_LENGTHS:
        for tail in (b"ab", b"cab ", b"a", b" "):
            if n >= len(tail):
                add("len_%d_%s" % (n, "word" if tail.strip() and not tail.endswith(b" ") else "sep"), _place(rng, n, n - len(tail), tail))
    for w in (LITS[15], LITS[16], LITS[17], LITS[3], LITS[18], LITS[19], LITS[20], LITS[64], LIT_TWINS[1]):
        add("lit_at_len-%d" % len(w), _place(rng, 70 + len(w), 70, w))
        add("lit_at_len-%d_and_1" % len(w), _place(rng, 71 + len(w), 70, w))
    for at in range(4):
        for w in (b"ab", b"cab", b"b", b"a kk", b"ab going", b"a"):
            add("word_at_%d" % at, _place(rng, at + len(w) + 9, at, w))
    for w in KEY_EDGE_WORDS:
        add("key_edge", _place(rng, 30 + len(w), 11, w))
    for s in ("ab going kk", "kk aäkk ab—abcab c kk", "äabü " + ALL_VARIANTS_WORD.decode() + "ä", "dd—going a b"):
        add("utf8", s.encode("utf8"))
    return docs, what


@functools.lru_cache(maxsize=None)
def dense_docs():
    """ends in every second byte (for the `dense` table): 31 + 32 + 32 ends in three tiles running (63 wait, 32 more
    come), several candidates each; a tile of lanes with lists next to lanes with one candidate"""
    docs, what = [], []
    docs.append(b"  " + b"a " * 31 + b"a b " * 240); what.append("a_b")
    docs.append(b"ab ba " * 160); what.append("ab_ba")
    docs.append(b"  " + b"a " * 31 + b"a " * 400 + b"a"); what.append("a_a")
    docs.append(b"a a b kk b ab ba zz kmn b " * 40); what.append("mixed")
    return docs, what


RING_LENGTHS = [190, 255, 256, 257, 318, 319, 320, 321, 384, 448, 510, 511, 512, 513, 514, 600]
RING_ALIGN = [0, 31, 63]


@functools.lru_cache(maxsize=None)
def ring_docs():
    """(documents, what): a word of L letters whose end lies at a tile offset of 0, 31 and 63, the document ending with
    it (the walks of the last flush reach back to the ring's oldest bytes); "ab" with 250 to 330 blanks, and with 600,
    between (a flush for one waiting end, ends at tile offsets 0 and 1)"""
    docs, what = [], []
    for L in RING_LENGTHS:
        for a in RING_ALIGN:
            pad = 128 + (a - L - 128) % 64
            d = b"kk" + b" " * (pad - 2) + long_word(L)
            assert len(d) % 64 == a
            docs.append(d); what.append(("word", L, a))
    rng = random.Random(4300)
    d = bytearray(b" " * 62)
    for gap in (600, 601, 250, 270, 290, 310, 318, 319, 320, 321, 330, 250, 330, 600, 62, 700):
        d += b"ab" + b" " * gap
    docs.append(bytes(d) + b"ab"); what.append(("sparse", 0, 0))
    docs.append(b" " * 63 + b"ab ab" + b" " * 571 + b"kab" + b" " * 700 + b"ab going" + b" " * 633 + filler(rng, 100)); what.append(("sparse", 1, 0))
    return docs, what


CHUNKS = [64, 1024]


@functools.lru_cache(maxsize=None)
def chunk_docs(chunk):
    """(documents, what) around a chunk boundary B: run ends at B-1, B, B+1; runs of 1, 2, 159, 160, 161 and 300 bytes
    that end at B+1; a run over a whole chunk; PREVWORD pairs with the separator at B-1, at B and with the predecessor
    ending at B-161 (before the back-off); a last chunk that ends in a word; documents of a whole number of chunks"""
    rng = random.Random(4400 + chunk)
    B = 1024 if chunk == 1024 else 384
    n = B + chunk + 37
    docs, what = [], []

    def add(kind, d):
        docs.append(d)
        what.append(kind)
    for to in (B - 1, B, B + 1):
        add("end_at_B%+d" % (to - B), _place(rng, n, to - 5, b"abkab"))
    for ln in (1, 2, 159, 160, 161, 162, 300):
        w = b"a" if ln == 1 else b"ab" if ln == 2 else long_word(ln)
        add("run_%d" % ln, _place(rng, n, B + 1 - ln, w))
    add("run_over_chunk", _place(rng, n + chunk, B - 10, long_word(chunk + 20)))
    add("sep_at_B-1", _place(rng, n, B - 3, b"ab going"))
    add("sep_at_B", _place(rng, n, B - 2, b"ab going"))
    add("sep_at_B_dash", _place(rng, n, B - 2, b"ab-kk"))
    add("prev_ends_at_B-161", _place(rng, n, B - 163, b"ab " + b"k" * 158 + b"ing"))
    add("prev_before_back_off", _place(rng, n, B - 212, b"ab " + b"k" * 220))
    add("last_chunk_ends_in_word", _place(rng, B + 11, B + 6, b"abcab"))
    add("whole_chunks_word", _place(rng, B + chunk, B + chunk - 2, b"ab"))
    add("whole_chunks_pair", _place(rng, B + chunk, B + chunk - 5, b"ab kk"))
    add("whole_chunks_sep", filler(rng, B + chunk))
    add("one_chunk", _place(rng, chunk, chunk - 3, b"cab"))
    return docs, what


@functools.lru_cache(maxsize=None)
def overflow_docs():
    """(documents, what) for the `dense` table: between ordinary documents one whose unit queues a record per byte (its
    slice of the word queue is short at the default size, large enough at twice that) and one that queues 1.75 per byte
    (short until the queue has grown twice)"""
    rng = random.Random(4500)
    # (no digits: nothing for the scan kernel to queue, so only the word queue can be short)
    docs = [filler(rng, 300, False) + b"ab ba a", b"a kk " * 100, filler(rng, 200, False) + b"a b ab", b"a b " * 100, b"", filler(rng, 500, False)]
    return docs, ["plain", "dense", "plain", "very_dense", "empty", "plain"]
