"""Tables and documents for the tests of the loops of the words kernel's flush path (probe depth in the literal and the
shape table, variants per tile, the merge of a lane's lists into output rounds, the waiting ends, document edges), shared
by the CPU guard (tests/test_l1_words_loops_model.py) and the GPU test (tests/test_l1_words_loops_gpu.py).  The tables
of tests/l1_words_cases.py are used where they fit; `probes` is new: enough literals and shape keys that the open-addressing
tables hold chains of three and more.  Both hash tables are rebuilt here slot by slot as the compiler lays them out
(l1_compile.cpp: a power of two >= 2n+1, linear probing, insertion in key order), so a test can say at which probe a
word is found or given up."""
import functools
import random

from tests import l1_words_cases as cases
from tests import l1_words_model as model

LETTERS = b"pqrstuvwxyz"            # (the filler of l1_words_cases uses k, m, n and digits only)
LONG_LITERAL = b"pqrstuvwxyzpqrstuvwxyz"    # 22 bytes: the compare behind the 16 inline bytes runs, with a rest of 2


def _words(seed, count, lengths):
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        w = bytes(rng.choice(LETTERS) for _ in range(rng.choice(lengths)))
        if w not in out:
            out.append(w)
    return out


PROBE_LITERALS = _words(5100, 140, [3, 4, 5, 6, 7, 9]) + [LONG_LITERAL]
PROBE_PREFIXES = _words(5200, 84, [2])
PROBE_SUFFIXES = _words(5300, 42, [2])


def _probes():
    out = [("\\b%s\\b" % w.decode(), 1 + i % 3, "content") for i, w in enumerate(PROBE_LITERALS)]
    out += [("\\b%s[a-z]*\\b" % w.decode(), 1 + i % 3, "content") for i, w in enumerate(PROBE_PREFIXES)]
    out += [("[a-z]+%s\\b" % w.decode(), 1 + i % 3, "content") for i, w in enumerate(PROBE_SUFFIXES)]
    return out + [("\\bpq\\s\\w+\\b", 1, "content"), cases.NUMBER]


TABLES = {"probes": _probes()}


def build(x, name):
    """the lexer of a table of this module or of l1_words_cases"""
    if name not in TABLES:
        return cases.build(x, name)
    for i, (expr, level, bind) in enumerate(TABLES[name]):
        x.defineLexem(i + 1, expr, 0, level, bind)
    x.compile()


@functools.lru_cache(maxsize=None)
def tables(name):
    if name not in TABLES:
        return cases.tables(name)
    import struspattern_amd as spa
    from tests.l1_table_sim import Tables
    lx = spa.PatternLexerInstance()
    build(lx, name)
    return Tables(lx.dumpTables())


# ---------------------------------------------------------------- the hash tables, slot by slot
def _table_size(n):
    size = 1
    while size < 2 * n + 1:
        size <<= 1
    return size


def shape_slot_hash(tag, key):
    h = ((key * 0x9E3779B1) ^ (tag * 0x85EBCA6B)) & model.M32
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & model.M32
    h ^= h >> 12
    return h


def _fill(keys, hash_of):
    slots = [None] * _table_size(len(keys))
    for k in keys:
        s = hash_of(k) & (len(slots) - 1)
        while slots[s] is not None:
            s = (s + 1) & (len(slots) - 1)
        slots[s] = k
    return slots


def _depth(slots, key, hash_of):
    """(probes before the answer, found): 0 = the first slot looked at holds the key or is empty"""
    s, d = hash_of(key) & (len(slots) - 1), 0
    while slots[s] is not None and d < len(slots):
        if slots[s] == key:
            return d, True
        s = (s + 1) & (len(slots) - 1)
        d += 1
    return d, False


@functools.lru_cache(maxsize=None)
def literal_slots(name):
    return _fill(sorted(tables(name).literals), model.word_hash)


@functools.lru_cache(maxsize=None)
def shape_slots(name):
    return _fill(sorted(tables(name).shapes), lambda tk: shape_slot_hash(*tk))


def literal_depth(name, word):
    return _depth(literal_slots(name), bytes(word), model.word_hash)


def shape_depth(name, tag_key):
    return _depth(shape_slots(name), tag_key, lambda tk: shape_slot_hash(*tk))


# ---------------------------------------------------------------- documents
def _missing(seed, taken, length, want, depth_of):
    """words of `length` letters that are no key and are given up after `want(depth)` probes"""
    rng = random.Random(seed)
    out = []
    for _ in range(20000):
        w = bytes(rng.choice(LETTERS) for _ in range(length))
        d, found = depth_of(w)
        if w not in taken and not found and want(d) and w not in out:
            out.append(w)
            if len(out) == 3:
                break
    return out


@functools.lru_cache(maxsize=None)
def probe_words():
    """dict of word lists by what their probe does: lit_0 / lit_1 / lit_3 (found at probe 0, 1, >= 3), lit_miss_0 (the first slot
    is empty), lit_miss_chain (given up after >= 2 occupied slots); the same for the PREFIX(0,2) key of a word: key_0, key_1,
    key_3, key_miss_0, key_miss_chain"""
    t = tables("probes")
    out = dict((k, []) for k in ("lit_0", "lit_1", "lit_3", "key_0", "key_1", "key_3"))
    for w in sorted(t.literals):
        d, found = literal_depth("probes", w)
        assert found
        if d in (0, 1) or d >= 3:
            out["lit_%d" % min(d, 3)].append(w)
    var = model.PREFIX | (0 << 2) | (2 << 4)
    for tag, key in sorted(t.shapes):
        if tag == var:
            d, found = shape_depth("probes", (tag, key))
            assert found
            if d in (0, 1) or d >= 3:
                out["key_%d" % min(d, 3)].append(key.to_bytes(2, "little") + b"kmk")
    lits = set(t.literals)
    out["lit_miss_0"] = _missing(5400, lits, 5, lambda d: d == 0, lambda w: literal_depth("probes", w))
    out["lit_miss_chain"] = _missing(5401, lits, 5, lambda d: d >= 2, lambda w: literal_depth("probes", w))
    keys = set(PROBE_PREFIXES)
    key_depth = lambda w: shape_depth("probes", (var, int.from_bytes(w[:2], "little")))
    out["key_miss_0"] = [w + b"kmk" for w in _missing(5402, keys, 2, lambda d: d == 0, key_depth)]
    out["key_miss_chain"] = [w + b"kmk" for w in _missing(5403, keys, 2, lambda d: d >= 2, key_depth)]
    return out


@functools.lru_cache(maxsize=None)
def probe_docs():
    """the words of probe_words() in filler, every kind in one 64-end batch and again a tile apart; the long literal, and a twin
    of it that differs behind byte 16"""
    pw = probe_words()
    rng = random.Random(5500)
    words = [w for k in sorted(pw) for w in pw[k][:3]] + [LONG_LITERAL, LONG_LITERAL[:-1] + b"p", b"pq", b"kk"]
    d1 = cases.filler(rng, 40) + b" ".join(words) + b" " + cases.filler(rng, 30)
    rng.shuffle(words)
    d2 = b" ".join(words)
    return [d1, d2, b"pq " + b" kk ".join(words[:20])]


def variant_docs():
    """for the `keys` table: one tile with words of no variant, of one, and of all eight; a batch of one-letter words (no lane
    has a key for any PREFIX or SUFFIX variant: every one of them is two bytes and more)"""
    one_tile = b"kk bak " + cases.ALL_VARIANTS_WORD + b" mmm n bak kk " + cases.ALL_VARIANTS_WORD + b" kk"
    assert len(one_tile) <= 64
    return [one_tile, b"k n m k " * 12, b"k " * 40 + cases.ALL_VARIANTS_WORD + b" n" * 30]


def merge_docs():
    """for the `dense` table: "zz" queues one record (a literal of one expression), "a" a literal list of three and more: flushes
    of 63, 64 and 65 records, one of them with every lane on the simple path; a list of two and more beside simple lanes; an end
    with a literal and shape lists at once ("ab", "ba")"""
    return [b"zz " * 63, b"zz " * 64, b"zz " * 65, b"zz " * 62 + b"a", b"zz " * 62 + b"ba", b"zz " * 30 + b"a zz ab zz ba a b " * 3, b"ab ba " * 20 + b"zz a " * 8]


def ends_docs():
    """for the `dense` table: 63, 64, 65, 127 and 128 run ends in a unit, an end in every second byte (a drain at 64 leaves a rest
    of 0; 32 ends a tile on top of 63 waiting ones leave the largest rest there is, 31); a drain under pressure with fewer than
    64 ends; the unit's last ends flushed behind the loop"""
    docs = [b"a " * n for n in (63, 64, 65, 127, 128)]
    docs.append(b"  " + b"a " * 31 + b"b " * 64 + b"a")                 # 63 wait, 32 more come: rest 31
    docs.append(b"ab" + b" " * 400 + b"ba a" + b" " * 330 + b"b zz")     # pressure
    return docs


def edge_docs():
    """for the `keys_prev` table: a word within the first four bytes and one within the last four of a document, documents of less
    than four bytes, an empty document between two others"""
    return [b"ab kk mmm cab", b"a", b"ab", b"cab", b"", b"k ab", b"", b"", b"abcd kk n xcab", b"b a"]


GROUPS = {"probes": ("probes", probe_docs), "variants": ("keys", variant_docs), "merge": ("dense", merge_docs), "ends": ("dense", ends_docs),
          "edges": ("keys_prev", edge_docs)}
