"""The compiled lexer tables of the corpus in tests/l1_compile_corpus.py are, byte for byte, the ones pinned in
tests/golden/l1_compile_digests.json (CPU, no device).  The fixture is regenerated only by a change that means to alter the
compiled tables, with `python -m tests.l1_compile_corpus > tests/golden/l1_compile_digests.json`; anything else has to pass
against it unchanged."""
import json
import os
import struct

import numpy as np
import pytest

import struspattern_amd as spa
from tests import l1_cases, l1_compile_corpus as corpus

with open(os.path.join(l1_cases.GOLDEN, "l1_compile_digests.json")) as f:
    PINNED = json.load(f)


def test_the_fixture_holds_the_corpus():
    assert sorted(PINNED) == sorted(corpus.CORPUS)


@pytest.mark.parametrize("name", sorted(corpus.CORPUS))
def test_compiled_tables_are_the_pinned_ones(name, monkeypatch):
    assert corpus.digest(name, monkeypatch) == PINNED[name]


def test_the_corpus_covers_the_ways_tables_come_out():
    """what the sets are in the corpus for, read from the pinned fields"""
    assert PINNED["size_ordered_packing"]["reportsOrdered"] is False and PINNED["size_ordered_packing"]["nofShapes"] == 0
    assert PINNED["shapes_behind_scanned_passes"]["scanPasses"] < PINNED["shapes_behind_scanned_passes"]["nofPasses"]
    assert PINNED["synth_1500"]["nofPasses"] > 1 and PINNED["synth_1500"]["nofShapes"] > 0 and PINNED["synth_1500"]["nofLiterals"] > 0
    assert 0 < PINNED["shape_variants_cut"]["nofShapes"] < len(corpus.SHAPE_VARIANT_PATTERNS) - 1      # the population cut ran
    assert PINNED["too_many_nullable"] == {"error": "failed to compile regular expression patterns: too many expressions that match the empty string (ALLOWEMPTY: at most 64)"}
    assert PINNED["share_pass_on"]["nofPasses"] < PINNED["share_pass_off"]["nofPasses"]
    for name in corpus.SHARE_SETS:
        unset, off, on, force = (PINNED["%s_%s" % (name, mode)] for mode in corpus.SHARE_MODES)
        # SPA_L1_SHARE set to anything, "off" included, turns the word shapes off: "off" is not the default
        assert unset["nofShapes"] > 0 and off["nofShapes"] == 0 and off["sha256"] != unset["sha256"]
        assert force["sha256"] != off["sha256"] and force["reportsOrdered"] is False and on["nofShapes"] == 0


def test_a_failed_compile_leaves_the_compiled_tables_as_they_were():
    """compile() builds into tables of its own and commits them at its end.  A compiled lexer takes no further expression, so the
    compile that fails is one after an option that the expressions do not go with: the tables stay, and the serialised lexer
    differs from the earlier one in the option word alone."""
    lx = spa.PatternLexerInstance()
    corpus.CORPUS["plan_exceptions"][1](lx, corpus._Environ())
    blob, dump = lx.serialize(), lx.dumpTables()
    options = struct.unpack_from("<I", blob, 8)[0]
    lx.defineOption("BYTECHAR")
    with pytest.raises(spa.PatternError, match="plain literal expressions only"):
        lx.compile()
    assert np.array_equal(lx.dumpTables(), dump)
    after = lx.serialize()
    assert after[:8] == blob[:8] and struct.unpack_from("<I", after, 8)[0] == options | 32 and after[12:-8] == blob[12:-8]
