"""Lexer tables shared by tests/test_l1_image.py (CPU) and tests/test_l1_plan_gpu.py: one per way the three table images
and the launch plan of a batch (struspattern_amd/csrc/l1_image.hpp) can come out."""
import itertools

LETTERS = "abcdefghijklmnopqrstuvwxyz"

# name -> (options, environment at compile time, expressions)
TABLES = {
    # one scanned automaton word without exception rows, word shapes and whole-word literals behind it: the lane-per-stream route
    "no_exceptions": (("DOTALL",), {}, ["[0-9]+[.][0-9]+", "\\bun[a-z]*\\b", "[a-z]+ing\\b", "\\bthe\\b", "\\bcat\\b"]),
    # the same with expressions that need exception rows (bounded repeats, a loop over a group)
    "exceptions": (("DOTALL",), {}, ["x[0-9]{1,3}y", "(ab)+c", "[0-9]+[.][0-9]+", "\\bun[a-z]*\\b", "[a-z]+ing\\b", "\\bthe\\b"]),
    # word shapes that fill two passes of their own behind one scanned pass
    "shapes_behind_one_pass": (("DOTALL",), {}, ["[0-9]+[.][0-9]+", "x[0-9]{2}z", "a+b"]
                               + ["\\b%s[a-z]*\\b" % "".join(t) for t in itertools.islice(itertools.product(LETTERS[:13], LETTERS[:12], LETTERS[:10]), 1500)]),
    # every expression in the scanned passes
    "shapes_off": (("DOTALL",), {"SPA_L1_SHAPES": "0"}, ["[0-9]+[.][0-9]+", "\\bun[a-z]*\\b", "[a-z]+ing\\b", "\\bthe\\b", "\\bcat\\b"]),
    # nothing to scan
    "literals_only": (("DOTALL",), {}, ["\\bthe\\b", "\\bcat\\b", "\\bsat\\b"]),
    # classes by code point: no words kernel, the _cp instances
    "unicode_class": (("DOTALL",), {}, ["\\b\\p{Lu}\\p{Ll}*\\b", "[0-9]+", "\\bthe\\b"]),
    # approximate literal table
    "approx": ((), {}, ["abc ~1"]),
}
IMAGE_TABLES = ("no_exceptions", "exceptions", "shapes_behind_one_pass", "shapes_off", "literals_only", "unicode_class")

DOCS = [b"the cat sat 3.14 unhappy singing x12y ababc x45z aab", "Ärger The Cat 12 abd abc".encode("utf8"), b"", b"undo the thing 1.5"]


def long_doc():
    """70 KB: more than two chunks of the default size"""
    return (b"the cat is undoing 12.75 things x7y ababc aab The End. " * 1400)[:70 * 1024]


def build(lx, name, monkeypatch=None):
    """defines and compiles the table `name` (ids 1.., level by position) on a product or oracle lexer instance"""
    options, env, pats = TABLES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for o in options:
        lx.defineOption(o)
    for i, p in enumerate(pats):
        lx.defineLexem(i + 1, p, 0, 1 + i % 3, "content")
    lx.compile()
    for k in env:
        monkeypatch.delenv(k)
    return lx
