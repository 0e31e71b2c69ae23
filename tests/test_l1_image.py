"""CPU tests (no GPU) of the host layer of a lexer launch (struspattern_amd/csrc/l1_image.hpp): the three table images the
kernels read hold the rows of the compiled tables where their offsets say, and the launch plan of a batch -- route, kernel
names, grids, workgroup size, LDS -- is the one the routing conditions give (expected values worked out by hand from the
conditions, for a device of 256 compute units)."""
import pytest

import struspattern_amd as spa
from tests import l1_plan_cases as cases
from tests.l1_table_sim import Tables

M32 = 1 << 32
LDS_PER_WORD_WAVE = 512 * 2 + 96 * 5 * 4     # l1_device.h: L1_WORDS_LDS_PER_WAVE


def _lexer(name, monkeypatch):
    return cases.build(spa.PatternLexerInstance(), name, monkeypatch)


def _u32(x):
    return x & 0xFFFFFFFF


def _shape_fingerprint(tag, key, salt):
    h = _u32(_u32((key ^ salt) * 0x85EBCA6B) + _u32(tag * 0xC2B2AE35))
    h ^= h >> 16; h = _u32(h * 0x7feb352d); h ^= h >> 15; h = _u32(h * 0x846ca68b); h ^= h >> 16
    return h or 1


def _shape_slot(tag, key):
    h = _u32(key * 0x9E3779B1) ^ _u32(tag * 0x85EBCA6B)
    h ^= h >> 15; h = _u32(h * 0x2C1B3C6D); h ^= h >> 12
    return h


def _compact_shape_table(shapes):
    """the table the kernel probes, rebuilt from the dumped entries {(tag, key): patterns} as l1_tables.h describes it"""
    size = 1
    while size < 2 * len(shapes) + 1:
        size <<= 1
    keys = sorted(shapes)
    salt = 0
    while len(set(_shape_fingerprint(t, k, salt) for t, k in keys)) != len(keys):
        salt += 1
    slots = [None] * size
    table = [0] * size
    begin = 0
    for t, k in keys:
        s = _shape_slot(t, k) & (size - 1)
        while slots[s] is not None:
            s = (s + 1) & (size - 1)
        slots[s] = (t, k)
        pats = shapes[(t, k)]
        info = (len(pats) << 24) | (pats[0] if len(pats) == 1 else begin)
        table[s] = _shape_fingerprint(t, k, salt) | (info << 32)
        begin += len(pats)
    return table


def _assert_rows(T, image, first, end):
    """every row of the passes [first, end) of the seven tables lies at offset + absolute pass * rows per pass"""
    o, w = image
    w = [int(x) for x in w]
    C, E = T.nofClasses, T.E
    tables = [(T.charMask, C * 64), (T.acceptMask, 4 * 64), (T.startMask, 4 * 64), (T.shiftDst, 64), (T.selfLoop, 64), (T.exSrc, E * 64), (T.exDst, E * 64)]
    for (table, stride), off in zip(tables, o[:7]):
        for p in range(first, end):
            at = (off + p * stride) % M32
            assert at + stride <= len(w)
            assert w[at:at + stride] == table[p * stride:(p + 1) * stride]
    return w


@pytest.mark.parametrize("name", cases.IMAGE_TABLES)
def test_images_hold_the_table_rows(name, monkeypatch):
    lx = _lexer(name, monkeypatch)
    T = Tables(lx.dumpTables())
    words_kernel = name != "unicode_class"
    scanned = T.scan_passes if words_kernel else T.npasses
    shape_table = _compact_shape_table(T.shapes)
    if name == "no_exceptions":
        assert T.maxEx == 0 and 0 < T.scan_passes < T.npasses
    if name == "exceptions":
        assert T.maxEx > 0 and 0 < T.scan_passes < T.npasses
    if name == "shapes_behind_one_pass":
        assert T.scan_passes == 1 and T.npasses >= 3
    if name == "shapes_off":
        assert T.nof_shapes == 0 and T.scan_passes == T.npasses
    if name == "literals_only":
        assert T.scan_passes == 0
    if name == "unicode_class":
        assert T.cpBlocks

    o, _ = img = lx.dumpImage(0)                # all passes + shape table
    w = _assert_rows(T, img, 0, T.npasses)
    assert o[0] == 0 and w[o[7]:] == shape_table

    o, _ = img = lx.dumpImage(1)                # the scanned passes, no shape table
    w = _assert_rows(T, img, 0, scanned)
    assert o[0] == 0 and (w == [0] and o[7] == 0 if scanned == 0 else o[7] == len(w))

    img = lx.dumpImage(2)                       # words kernel: the passes behind the scanned ones (by ABSOLUTE pass) + shape table
    if not words_kernel:
        assert img is None
    else:
        o, _ = img
        w = _assert_rows(T, img, T.scan_passes, T.npasses)
        assert w[o[7]:] == shape_table
        assert o[0] == (-T.scan_passes * T.nofClasses * 64) % M32


def _plan(lx, ndocs, nbytes):
    return lx.launchPlan(256, ndocs, nbytes)


LAUNCH_SWITCHES = ("SPA_L1_NO_LANES", "SPA_L1_CHUNK_BYTES", "SPA_L1_WORD_WAVES", "SPA_L1_POST_SEQ", "SPA_L1_POST_WAVES_PER_CU", "SPA_L1_NO_WORDS_KERNEL")


@pytest.fixture
def no_switches(monkeypatch):
    for s in LAUNCH_SWITCHES:
        monkeypatch.delenv(s, raising=False)
    return monkeypatch


def test_plan_of_a_literals_and_shapes_table(no_switches):
    lx = _lexer("no_exceptions", no_switches)
    T = Tables(lx.dumpTables())
    assert int(lx.dumpTables()[6]) == 1         # (reports ordered: a condition of the lane-per-stream route)
    p = _plan(lx, 3, 300)
    assert p["route"] == "lanes" and p["scan_kernel"] == "spa_l1_scan_lanes_kernel" and p["words_kernel"] == "spa_l1_words_kernel_w16"
    assert p["cp"] == "0" and p["chunk_bytes"] == "32768" and p["max_units"] == "5" and 1 <= int(p["scan_words"]) <= 4
    # 5 units: two workgroups of four lane-kernel waves, one of 16 words-kernel waves; 3 documents: one workgroup of four post waves
    assert (p["lane_grid"], p["word_grid"], p["word_waves"], p["post_waves"], p["post_grid"], p["post_clusters"]) == ("2", "1", "16", "4", "1", "1")
    # a small one-pass image: five copies per CU share 20 waves -> workgroups of four waves; staged whole
    assert p["scan_threads"] == "256" and p["scan_grid"] == "2" and int(p["scan_lds"]) == 8 * int(p["scan_image_words"]) > 0
    assert p["word_lds_words"] == p["words_image_words"] and int(p["image_words"]) == len(lx.dumpImage(0)[1])
    assert int(p["scan_image_words"]) == len(lx.dumpImage(1)[1]) and int(p["words_image_words"]) == len(lx.dumpImage(2)[1])
    # the per-launch switches
    no_switches.setenv("SPA_L1_NO_LANES", "1")
    q = _plan(lx, 3, 300)
    assert q["route"] == "passes(1)" and q["scan_kernel"] == "spa_l1_scan_kernel_p1" and q["scan_words"] == "0" and q["words_kernel"] == p["words_kernel"]
    no_switches.delenv("SPA_L1_NO_LANES")
    no_switches.setenv("SPA_L1_WORD_WAVES", "12")
    q = _plan(lx, 40, 3000)
    assert q["words_kernel"] == "spa_l1_words_kernel" and q["word_waves"] == "12" and q["word_grid"] == "4" and q["route"] == "lanes"   # 42 units / 12 waves
    no_switches.delenv("SPA_L1_WORD_WAVES")
    no_switches.setenv("SPA_L1_POST_SEQ", "1")
    no_switches.setenv("SPA_L1_POST_WAVES_PER_CU", "2")
    q = _plan(lx, 1000, 30000)
    assert q["post_clusters"] == "0" and q["post_waves"] == "512" and q["post_grid"] == "128"
    no_switches.delenv("SPA_L1_POST_SEQ")
    no_switches.delenv("SPA_L1_POST_WAVES_PER_CU")
    assert _plan(lx, 1000, 30000)["post_waves"] == "1000" and _plan(lx, 7000, 30000)["post_waves"] == str(256 * 24)
    # the grids are bounded by the device: 20 scan waves, 4 lane-kernel workgroups, one words-kernel workgroup per CU
    q = _plan(lx, 100000, 1 << 20)
    assert (q["scan_grid"], q["lane_grid"], q["word_grid"]) == (str(256 * 20 // 4), "1024", "256")
    # SPA_L1_NO_WORDS_KERNEL: everything is scanned, nothing goes through the lane kernel
    no_switches.setenv("SPA_L1_NO_WORDS_KERNEL", "1")
    lx2 = _lexer("shapes_off", no_switches)
    q = _plan(lx2, 3, 300)
    assert q["words_kernel"] == "(none)" and q["words_image_words"] == "0" and q["route"] == "passes(%d)" % Tables(lx2.dumpTables()).npasses
    assert T.scan_passes == 1


def test_plan_of_a_long_document_follows_the_chunk_size(no_switches):
    lx = _lexer("no_exceptions", no_switches)
    n = 70 * 1024
    assert _plan(lx, 1, n)["max_units"] == str(1 + n // 32768 + 2) == "5"
    no_switches.setenv("SPA_L1_CHUNK_BYTES", "64")
    p = _plan(lx, 1, n)
    assert p["chunk_bytes"] == "64" and p["max_units"] == str(1 + n // 64 + 2) == "1123"
    no_switches.setenv("SPA_L1_CHUNK_BYTES", "200")        # rounded down to a multiple of 64
    assert _plan(lx, 1, n)["chunk_bytes"] == "192"
    no_switches.setenv("SPA_L1_CHUNK_BYTES", "63")         # out of range: ignored
    assert _plan(lx, 1, n)["chunk_bytes"] == "32768"


def test_plan_of_the_other_routes(no_switches):
    p = _plan(_lexer("unicode_class", no_switches), 3, 300)
    assert p["cp"] == "1" and p["words_kernel"] == "(none)" and p["route"] == "passes(1)" and p["scan_kernel"] == "spa_l1_scan_kernel_p1"
    p = _plan(_lexer("approx", no_switches), 3, 300)
    assert p["route"] == "approx" and p["scan_kernel"] == "spa_l1_approx_kernel" and p["words_kernel"] == "(none)"
    p = _plan(_lexer("literals_only", no_switches), 3, 300)
    assert p["route"] == "none" and p["scan_kernel"] == "(none)" and p["words_kernel"] == "spa_l1_words_kernel_w16"
    assert p["scan_image_words"] == "1" and p["word_lds_words"] == "0"      # (no shapes: the words kernel stages nothing)
    # an expression that can stay live across blanks: the documents are scanned whole, on the wave-per-unit kernel
    lx = spa.PatternLexerInstance()
    lx.defineOption("DOTALL")
    lx.defineLexem(1, "<[^>]*>", 0, 1, "content")
    lx.defineLexem(2, "\\bthe\\b", 0, 1, "content")
    lx.compile()
    p = _plan(lx, 1, 70 * 1024)
    assert p["chunk_bytes"] == str(0xFFFFFFC0) and p["max_units"] == "3" and p["route"] == "passes(1)" and p["scan_words"] == "0"
    # shapes in two passes of their own behind one scanned pass
    lx = _lexer("shapes_behind_one_pass", no_switches)
    p = _plan(lx, 3, 300)
    assert p["route"] == "lanes" and p["word_lds_words"] == p["words_image_words"]
    assert int(p["words_image_words"]) * 8 + 16 * LDS_PER_WORD_WAVE <= 160 * 1024 and p["words_kernel"] == "spa_l1_words_kernel_w16"


def test_plan_of_a_scan_image_too_large_for_lds(no_switches):
    """three passes of many byte classes: more than 144 KB, read from global memory by workgroups of four waves"""
    no_switches.setenv("SPA_L1_SHARE", "off")
    lx = spa.PatternLexerInstance()
    lx.defineOption("DOTALL")
    n = 0
    for i in range(135):                                    # one automaton word each: three passes of 64 words
        n += 1
        lx.defineLexem(n, "q%s[a-z]{55}" % "".join(cases.LETTERS[(i // k) % 26] for k in (1, 26)), 0, 1, "content")
    for b in list(range(1, 32)) + [ord(c) for c in "!#%&',/:;<=>@_`~0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"]:
        n += 1
        lx.defineLexem(n, "\\x%02x\\x%02x" % (b, b), 0, 1, "content")       # a byte class of its own
    lx.compile()
    T = Tables(lx.dumpTables())
    p = _plan(lx, 3, 300)
    assert T.npasses == 3 and int(p["scan_image_words"]) * 8 > 144 * 1024
    assert p["scan_lds"] == "0" and p["scan_threads"] == "256" and p["route"] == "passes(3)" and p["scan_kernel"] == "spa_l1_scan_kernel_p3"
    assert p["scan_grid"] == "2"                             # 5 units on workgroups of four waves
