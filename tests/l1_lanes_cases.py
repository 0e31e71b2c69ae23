"""Tables and document sets of the tests of the lane-per-stream scan kernel of the lexer, shared by the CPU guards
(tests/test_l1_lanes_model.py: what every batch is meant to contain, said by the model) and the GPU tests
(tests/test_l1_lanes_gpu.py).  Everything is deterministic and small: a batch is some tens of documents."""
import functools
import random

from tests import l1_lanes_model as model

# whole-word literals and word shapes (the words kernel is on, one scanned pass) + scanned expressions that cannot
# stay live across a blank: one automaton word
BASE = [("\\b\\w+\\b", 1), ("\\bab[a-z]*\\b", 1), ("[a-z]+ing\\b", 1), ("\\bthe\\b", 2), ("\\bof\\b", 2),
        ("[0-9]+[.][0-9]+", 2), ("[0-9]+", 1)]


def alternatives(n):
    return ["q%02d%s" % (i, "xyz"[i % 3] * (1 + i % 2)) for i in range(n)]


def alternation(n):
    """a wide alternation, cut into several automaton words"""
    return ("(%s)" % "|".join(a + "[.][0-9]+" for a in alternatives(n)), 3)


# name -> (expressions, scan_words, on the lane-per-stream kernel)
TABLES = {
    "w1": (BASE, 1, True),
    "w2": (BASE + [alternation(14)], 2, True),
    "w3": (BASE + [alternation(19)], 3, True),
    "w4": (BASE + [alternation(26)], 4, True),
    "w5": (BASE + [alternation(60)], None, False),        # (five words or more: not on the kernel)
    # an optional and a repeated group: exception rows in the scanned pass, no cycle through ' '
    "ex": (BASE + [("x(ab)?c[.][0-9]+", 3), ("z(ab)+[.]", 3)], 1, True),
    # multi-byte literal class (bytes, no classes by code point)
    "utf": (BASE + [("[äöü]+[.]", 3)], 1, True),
    # three expressions that accept at every digit
    "dense": (BASE + [("[0-9]+[.]?", 1), ("[0-9]", 1)], 1, True),
}
LANE_TABLES = [n for n in ("w1", "w2", "w3", "w4", "ex", "utf")]


def build(x, name):
    for i, (expr, level) in enumerate(TABLES[name][0]):
        x.defineLexem(i + 1, expr, 0, level, "content")
    x.compile()


@functools.lru_cache(maxsize=None)
def tables(name):
    """the compiled tables of the product (host side only, no GPU)"""
    import struspattern_amd as spa
    from tests.l1_table_sim import Tables
    lx = spa.PatternLexerInstance()
    build(lx, name)
    return Tables(lx.dumpTables())


def offsets(docs):
    import numpy as np
    offs = np.zeros(len(docs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in docs])
    return offs


# ---------------------------------------------------------------- piece edges
EDGE_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 1008, 1023, 1024, 1025, 1040, 2047, 2048, 2049, 4096, 4097]
EDGE_CHUNKS = [None, 64, 1024]
# what is planted on a boundary b (bytes, offset of b inside them)
FEATURES = {
    "straddle": (b" 123.456 ", 5),                              # a number that straddles b, '.' last byte of the piece
    "straddle_dot": (b" 12.5 ", 3),                             # ... '.' first byte of the next piece
    "ends_at": (b" 12.5 ", 5),                                  # a match that ends exactly at b
    "split_char": (" äö. ".encode("utf8"), 2),        # a two-byte character split by b
    "shape_ends_at": (b" abcde ", 6),                           # a word shape match (\bab[a-z]*\b) that ends at b
    "ing_ends_at": (b" going ", 6),                             # [a-z]+ing\b ends at b
    "alt_straddle": (b" q01yy.77 ", 4),                         # an alternative of the wide alternation over b
}
ENDINGS = [b" 12.5", b" going", " öä.".encode("utf8"), b" q00x.5", b" abz", b" 7"]


def boundaries(doc_len, chunk):
    """the piece boundaries inside a document: every b1 of a non-empty piece below the document's end"""
    out = set()
    for sb, se in model.segments(doc_len, model.chunk_of(chunk)):
        out.update(b1 for b0, b1 in model.pieces(sb, se) if b0 < b1 and b1 < doc_len)
    return sorted(out)


def _filler(rng, n, digits=True):
    words = ["the", "of", "ab", "abx", "going", "sing", "x1", "42", "3.14", "zz", "q00x.5", "q13yy.08", "xabc.1", "xc.2", "zabab.", "äü.", "bö",
             "q05z.77", "q18x.3", "q25yy.9", "q40yy.1"]
    if not digits:
        words = [w for w in words if not any(c.isdigit() for c in w)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words).encode("utf8") + rng.choice([b" ", b" ", b"  ", b". ", b"\n"])
    return out[:n]


@functools.lru_cache(maxsize=None)
def edge_docs(chunk):
    """one document per length of EDGE_LENGTHS for a chunk size: text with one feature planted on every piece
    boundary it has room for (the features in turn), and one of ENDINGS at the document's end.  Returns
    (documents, planted: [(document, boundary, feature)])."""
    rng = random.Random(1000 + (chunk or 0))
    docs, planted = [], []
    names = sorted(FEATURES)
    turn = 0
    for li, n in enumerate(EDGE_LENGTHS):
        d = _filler(rng, n)
        last = -100
        for b in boundaries(n, chunk):
            feat, at = FEATURES[names[turn % len(names)]]
            lo, hi = b - at, b - at + len(feat)
            if lo < 0 or hi > n or lo < last:
                continue
            d[lo:hi] = feat
            planted.append((li, b, names[turn % len(names)]))
            last = hi
            turn += 1
        end = ENDINGS[li % len(ENDINGS)]
        if n >= len(end) and last <= n - len(end):
            d[n - len(end):] = end
        assert len(d) == n
        docs.append(bytes(d))
    return docs, planted


# ---------------------------------------------------------------- proof failure
def _proof_doc(rng, n, run_len, run_end, tail=b".25 "):
    """text of n bytes with a run of run_len digits that ends at run_end, followed by `tail`"""
    d = _filler(rng, n)
    beg = run_end - run_len
    assert beg >= 1 and run_end + len(tail) <= n
    d[beg - 1:beg] = b" "
    d[beg:run_end] = bytes(0x30 + (i % 10) for i in range(run_len))
    d[run_end:run_end + len(tail)] = tail
    return bytes(d)


@functools.lru_cache(maxsize=None)
def proof_docs(chunk):
    """digit runs around piece (and chunk) boundaries that lie more than 256 bytes into the document: the warm-up of
    the piece behind a run of 256 digits and more cannot prove its state ([0-9]+[.][0-9]+ may be in its second part
    or not).  Returns (documents, what each one is)."""
    rng = random.Random(2000 + (chunk or 0))
    docs, what = [], []

    def add(kind, d):
        docs.append(d)
        what.append(kind)

    def pb(n, lane, unit=0):
        """the start of piece `lane` of unit `unit` of a document of n bytes"""
        sb, se = model.segments(n, model.chunk_of(chunk))[unit]
        return model.pieces(sb, se)[lane][0]
    # runs that cross a piece boundary: 300, 600 and 1500 digits
    for n, run in ((1536, 300), (3000, 600), (6000, 1500)):
        lane = 40 if chunk is None else 20
        unit = 0 if chunk is None else 1
        b = pb(n, lane, unit)
        if chunk is not None:
            # inside one chunk where the run fits one (a piece boundary only), else over chunk boundaries as well
            run = min(run, 600)
        add("run%d_over_piece_boundary" % run, _proof_doc(rng, n, run, b + 20))
    n = 4000
    b = pb(n, 30, 0 if chunk is None else 2)
    add("run256_ends_at_boundary", _proof_doc(rng, n, 256, b))
    add("run255_ends_at_boundary", _proof_doc(rng, n, 255, b))
    add("run257_ends_at_boundary", _proof_doc(rng, n, 257, b))
    add("run257_ends_behind_boundary", _proof_doc(rng, n, 257, b + 1))
    add("run_inside_first_256_bytes", _proof_doc(rng, 2000, 200, 230))
    add("plain", bytes(_filler(rng, 3000)))
    add("empty", b"")
    if chunk is not None:
        c = model.chunk_of(chunk)
        add("run_over_chunk_boundary", _proof_doc(rng, 3 * c + 100, 400, 2 * c + 90))
        add("plain_chunked", bytes(_filler(rng, 2 * c + 17)))
    return docs, what


TOO_LONG = 70000        # a lexem of 65535 bytes or more is an error of its document


def too_long_doc():
    return b"ab " + bytes(0x30 + (i % 10) for i in range(TOO_LONG)) + b".5 the end"


# ---------------------------------------------------------------- per-lane queue regions
DENSE_BYTES = 13        # digits without a blank: three records per byte ("dense" table)


@functools.lru_cache(maxsize=None)
def overflow_docs():
    """blanks and words with one dense stretch of digits inside ONE piece: the lane's part of the queue slice (1/64 of
    the unit's) is too small at the default queue size and large enough at twice that, the slice as a whole is never
    short.  Returns (documents, what each one is)."""
    rng = random.Random(3000)
    docs, what = [], []

    def dense(n, lane, at_end=False):
        d = bytearray(b" " * n)
        d[0:40] = _filler(rng, 40, digits=False)
        b0, b1 = model.pieces(0, n)[lane]
        assert b1 - b0 >= DENSE_BYTES + 8
        if at_end:
            d[n - DENSE_BYTES:n] = b"7" * DENSE_BYTES
        else:
            d[b0 + 4:b0 + 4 + DENSE_BYTES] = b"1234567890123456789"[:DENSE_BYTES - 3] + b".45"
        return bytes(d)
    docs.append(bytes(_filler(rng, 1500, digits=False))); what.append("plain")
    docs.append(dense(4096, 17)); what.append("dense_lane17")
    docs.append(bytes(_filler(rng, 700, digits=False))); what.append("plain")
    docs.append(dense(4000, 62, at_end=True)); what.append("dense_last_live_lane")
    docs.append(b""); what.append("empty")
    docs.append(bytes(_filler(rng, 4096, digits=False))); what.append("plain")
    return docs, what


def very_dense_doc():
    """200 bytes of digits and '.' without a blank in a document of 4096 bytes: several lanes are short until the
    queue has grown three times"""
    d = bytearray(b" " * 4096)
    d[1000:1200] = (b"1234567.89" * 20)
    return bytes(d)


def full_unit_doc():
    """a digit in every second byte: three records per two bytes, more than the slice of the whole unit holds at the
    default queue size (and than every lane's part of it); no run the warm-up could not prove"""
    return b"7 " * 2048
