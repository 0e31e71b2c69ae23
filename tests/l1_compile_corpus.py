"""Named expression sets, one per way the compiled lexer tables (struspattern_amd/csrc/l1_compile.cpp) can come out, and the
digest of the tables each of them compiles to.  The serialised lexer holds every field of the tables, so equal digests are
equal tables: tests/test_l1_compile_golden.py compares digests() with tests/golden/l1_compile_digests.json.

A random_regex_N entry is one table of all the expressions of the 25 random sets of seed N together.

The fixture is regenerated only by a change that means to alter the compiled tables, with

    python -m tests.l1_compile_corpus > tests/golden/l1_compile_digests.json

A change that means to leave them alone (a refactoring of the compiler) must pass against the fixture as it is."""
import hashlib
import itertools
import json
import os
import random
import re
import struct
import sys

import struspattern_amd as spa
from struspattern_amd import synth
from tests import l1_cases, l1_plan_cases
from tests.l1_table_sim import Tables

SWITCHES = ("SPA_L1_SHAPES", "SPA_L1_SHARE")


class _Environ:
    """what the corpus uses of pytest's monkeypatch, for the command line"""

    def setenv(self, name, value):
        os.environ[name] = value

    def delenv(self, name, raising=True):
        if raising or name in os.environ:
            del os.environ[name]


def random_regex_sets(seed, count=25):
    """(expressions, text) of the random tables of tests/test_l1_compile.py: 1..6 random expressions that Python's `re`
    and this lexer accept, and a short random text"""
    rng = random.Random(1000 + seed)
    for _ in range(count):
        pats = []
        while len(pats) < rng.randint(1, 6):
            p = l1_cases.random_regex(rng)
            try:
                re.compile(p)
            except re.error:
                continue
            try:        # documented limit of this version: 64 byte positions per expression
                one = spa.PatternLexerInstance()
                one.defineOption("DOTALL")
                one.defineLexem(1, p, 0, 1, "content")
                one.compile()
            except spa.PatternError as e:
                assert "too complex" in str(e) or "matches empty buffer" in str(e), str(e)
                continue
            pats.append(p)
        text = l1_cases.random_text(rng, rng.randint(0, 30)).encode()
        yield pats, text


def _plain(pats, options=("DOTALL",)):
    def build(lx, env):
        for o in options:
            lx.defineOption(o)
        for i, p in enumerate(pats):
            lx.defineLexem(i + 1, p, 0, 1, "content")
        lx.compile()
    return build


def _synth(npatterns, nvocab, vseed, seed):
    return lambda lx, env: synth.apply_lexer_patterns(lx, synth.lexer_patterns(npatterns, synth.vocabulary(nvocab, vseed), seed))


TLDS = "aero|asia|biz|cat|com|coop|edu|gov|info|int|jobs|mil|mobi|museum|name|net|org|pro|tel|travel|ac|ad|ae|af|ag|ai|al|am|an|ao|aq|ar|as|at|au|aw|ax|az|ba|bb|bd|be|ch|de|uk|us"
# the sets of test_patterns_sharing_their_first_position and test_sharing_the_first_position_saves_a_pass (tests/test_l1_compile.py)
SHARED_HEAD_PATTERNS = [
    "[a-z]+ing\\b", "[a-z]+ed\\b", "[a-z]+s\\b", "[a-z]+ings\\b", "\\bun[a-z]+\\b", "\\bup[a-z]*\\b", "\\bunder\\s\\w+\\b", "\\bu\\b",
    "\\b[A-Z]an[a-z]*\\b", "\\b[A-Z][a-z]+\\b", "\\b[A-Z]\\.", "a+b", "a+c", "ab", "ac", "a+", "(ab)+c", "(ab)+d",
    "[0-9]+th\\b", "[0-9]+st\\b", "[0-9]+\\b", "x[0-9]{1,3}y", "x[0-9]{2}z",
]
_SUFS = ["".join(t) for t in itertools.product(l1_plan_cases.LETTERS[:12], l1_plan_cases.LETTERS[:10], l1_plan_cases.LETTERS[:5])]
SHARED_PASS_PATTERNS = list(dict.fromkeys(["[a-z]+%s\\b" % s for s in _SUFS[:520]] + ["\\b%s[a-z]*\\b" % s for s in _SUFS[40:560]]
                                          + ["\\b[A-Z]%s[a-z]*\\b" % s[:2] for s in _SUFS[::5][:110]]))
SHARE_SETS = {"share_heads": SHARED_HEAD_PATTERNS, "share_pass": SHARED_PASS_PATTERNS}
SHARE_MODES = ("unset", "off", "on", "force")
# eleven variants of word shapes (suffix of 2..4 bytes; prefix of 2..4 bytes behind 0..1 single positions; previous word) with
# different populations: more than the SHAPE_MAXVARIANTS = 8 the lexer probes, so the least populated ones stay automata
_SHAPE_FORMS = ["[a-z]+%s\\b", "\\b%s[a-z]*\\b", "\\b[A-Z]%s[a-z]*\\b"]
SHAPE_VARIANT_PATTERNS = ([form % (tail * 2)[:n] for fi, form in enumerate(_SHAPE_FORMS) for n in (2, 3, 4)
                           for tail in ("abcd", "efgh", "klmn", "pqrs", "tuvw")[:1 + (3 * fi + n) % 5]]
                          + ["\\b[A-Z][a-z]%s[a-z]*\\b" % t for t in ("ab", "cd", "ef")] + ["\\bunder\\s\\w+\\b", "\\bover\\s\\w+\\b", "[0-9]+"])

# name -> (environment at compile time, function that defines and compiles the set on a PatternLexerInstance)
CORPUS = {}
for _name in l1_plan_cases.TABLES:
    CORPUS["plan_" + _name] = ({}, lambda lx, env, _name=_name: l1_plan_cases.build(lx, _name, env))
for _i, _case in enumerate(l1_cases.load_char_regex_cases()):
    CORPUS["char_regex_%d" % _i] = ({}, lambda lx, env, _case=_case: l1_cases.build_case(lx, _case))
for _seed in range(8):
    CORPUS["random_regex_%d" % _seed] = ({}, lambda lx, env, _seed=_seed: _plain([p for pats, _ in random_regex_sets(_seed) for p in pats])(lx, env))
CORPUS.update({
    "caseless": ({}, _plain(["stra\u00dfe", "[a-z]+k", "\u00c4\u00d6[\u00fc]+", "\u03a3\u03af\u03c3\u03c5\u03c6\u03bf\u03c2", "[\u0430-\u044f]+", "x\u017f"], ("DOTALL", "CASELESS"))),
    "multiline": ({}, _plain(["^b", "a$", "b$", "^[a-z]+$"], ("MULTILINE",))),
    "allowempty": ({}, _plain(["a*", "\\b", "x?\\b", "(?:ab)*c?", "\\B", "^", "$", "[0-9]+"], ("DOTALL", "ALLOWEMPTY"))),
    "ucp": ({}, _plain(["\\b\\w+\\b", "\\b\\p{Lu}\\p{Ll}*\\b", "\\d+", "\\s+", "\\B[a-z\u00df]", "[\u00e4\u00f6\u00fc]\\b", "x\\b.", "\\b\u00e9", "\\bber\\b",
                        "\\b\u00fcber\\b", "\\W+"], ("DOTALL", "UCP"))),
    "properties_without_ucp": ({}, _plain(["\\p{Lu}\\p{Ll}*", "\\b\\p{Ll}+\\b", "[\\p{Nd}x]+", "\\P{L}+", "[^\\p{L}\\s]", "\\pL\\p{^L}", "[\u00e4\u00f6]"])),
    "bytechar": ({}, _plain(["abc", "stra\u00dfe", "x y"], ("BYTECHAR",))),
    "approx_multibyte": ({}, _plain(["stra\u00dfe ~2", "gr\u00f6\u00dfer ~1", "\u65e5\u672c\u8a9e\u3067\u3059 ~2", "plain"], ())),
    "wide_alternations": ({}, _plain(["([^\\s/?\\.#-][^\\s/?\\.#-]+\\.)(%s)" % TLDS, "\\b\\w+\\b", "x(%s)y|z(%s)" % (TLDS, TLDS)], ())),
    "size_ordered_packing": ({"SPA_L1_SHAPES": "0"}, _synth(4800, 6000, 77, 6)),
    "shapes_behind_scanned_passes": ({}, _synth(4800, 6000, 77, 6)),
    "non_ascii_classes_a": ({}, _plain(["a.b", "[^a-z ]+", "\\b[^\\s]+\\b", ".", "[^\\x00-\\x7f]{2}", "x[^q]y"])),
    "non_ascii_classes_a_nodotall": ({}, _plain(["a.b", "[^a-z ]+", "\\b[^\\s]+\\b", ".", "[^\\x00-\\x7f]{2}", "x[^q]y"], ())),
    "non_ascii_classes_b": ({}, _plain(["[^.]{3}", "(?:.|q){2}z"])),
    "non_ascii_classes_b_nodotall": ({}, _plain(["[^.]{3}", "(?:.|q){2}z"], ())),
    "shape_variants_cut": ({}, _plain(SHAPE_VARIANT_PATTERNS)),
    "too_many_nullable": ({}, _plain(["(?:x%dy)*" % i for i in range(65)], ("DOTALL", "ALLOWEMPTY"))),
    "synth_1500": ({}, _synth(1500, 6000, 77, 6)),
})
for _set, _mode in itertools.product(SHARE_SETS, SHARE_MODES):
    CORPUS["%s_%s" % (_set, _mode)] = ({} if _mode == "unset" else {"SPA_L1_SHARE": _mode}, _plain(SHARE_SETS[_set], ("DOTALL",) if _set == "share_heads" else ()))

# element sizes of the vectors a serialised lexer holds between its eight leading words and (scanPasses, scanWords, lanesOk, nofShapes)
_BLOB_VECTORS = (1, 1, 2, 1, 8, 8, 8, 8, 8, 4, 8, 8, 4, 4, 4, 32, 32, 1, 48, 1, 4, 128, 16)


def _scan_fields(blob, tables):
    """(scanWords, lanesOk) of a serialised lexer, the two fields dumpTables() does not hold.  The walk follows LexCompiler::save();
    the two neighbours that dumpTables() does hold tell whether it still does"""
    at = 8 + 8 * 4
    for size in _BLOB_VECTORS:
        at += 8 + size * struct.unpack_from("<Q", blob, at)[0]
    scan_passes, scan_words, lanes_ok, nof_shapes = struct.unpack_from("<4I", blob, at)
    assert (scan_passes, nof_shapes) == (tables.scan_passes, tables.nof_shapes), "the blob format changed: update _BLOB_VECTORS"
    return scan_words, bool(lanes_ok)


def digest(name, env=None):
    """the digest entry of the set `name`: {"error": message} for a set that does not compile, else the sha256 of the serialised
    lexer and the fields that tell what moved.  `env` is pytest's monkeypatch (default: the process environment itself)"""
    env = env or _Environ()
    for var in SWITCHES:
        env.delenv(var, raising=False)
    switches, build = CORPUS[name]
    for var, value in switches.items():
        env.setenv(var, value)
    lx = spa.PatternLexerInstance()
    try:
        build(lx, env)
    except spa.PatternError as e:
        return {"error": str(e)}
    finally:
        for var in SWITCHES:
            env.delenv(var, raising=False)
    blob = lx.serialize()
    dump = lx.dumpTables()
    tables = Tables(dump)
    scan_words, lanes_ok = _scan_fields(blob, tables)
    return {"sha256": hashlib.sha256(blob).hexdigest(), "nofPasses": tables.nofPasses, "scanPasses": tables.scan_passes, "scanWords": scan_words,
            "nofShapes": tables.nof_shapes, "nofLiterals": tables.nofLiterals, "reportsOrdered": bool(dump[6]), "lanesOk": lanes_ok}


def digests(env=None):
    return {name: digest(name, env) for name in CORPUS}


if __name__ == "__main__":
    json.dump(digests(), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
