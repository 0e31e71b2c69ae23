#!/usr/bin/env python3
"""Static instruction counts of one kernel's device assembly, by source phase and by loop body.

    usage: tests/micro/asm_loops.py k.s KERNEL SOURCE.hip [first:last=phase ...]

k.s is compiled with line tables (tests/micro/kernel_resources.sh FILE . -gline-tables-only with KEEP_ASM set).  Every
instruction is attributed to the last `.loc` line of SOURCE.hip seen before it (code inlined from headers counts for the
line that called it) and classified by its prefix: scalar (s_), vector ALU (v_), LDS (ds_), memory (global_/flat_/
buffer_/scratch_).  Printed: the counts per phase (ranges of source lines given on the command line) and, for every
backward branch, the text range it closes as a loop body: source lines covered, counts (inner loops included).
The counts are static: what a loop costs per byte of text is its body times its trip count, which the caller supplies."""
import collections
import re
import sys

LOC_RE = re.compile(r"^\s*\.loc\s+(\d+)\s+(\d+)")
FILE_RE = re.compile(r'^\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]*)"')
LABEL_RE = re.compile(r"^(\.L[A-Za-z0-9_$.]+):")
BRANCH_RE = re.compile(r"^\s*s_c?branch\S*\s+(\.L[A-Za-z0-9_$.]+)")


def kind(op):
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    return None


def main(argv):
    if len(argv) < 4:
        print(__doc__)
        return 2
    path, kernel, source = argv[1:4]
    phases = []
    dump = None
    for a in argv[4:]:
        rng, name = a.split("=")
        lo, hi = rng.split(":")
        if name == "dump":          # lo:hi=dump prints the instructions of that range (indices as in the loop lines)
            dump = (int(lo), int(hi))
        else:
            phases.append((int(lo), int(hi), name))
    src_ids, inside, line = set(), False, 0
    insts, labels = [], {}          # (kind, source line, text), label -> index of the next instruction
    for raw in open(path):
        m = FILE_RE.match(raw)
        if m and m.group(2).endswith(source.split("/")[-1]):
            src_ids.add(m.group(1))
        if not inside:
            inside = raw.startswith(kernel + ":")
            continue
        if raw.startswith(".Lfunc_end"):
            break
        m = LOC_RE.match(raw)
        if m:
            if m.group(1) in src_ids:
                line = int(m.group(2))
            continue
        m = LABEL_RE.match(raw)
        if m:
            labels[m.group(1)] = len(insts)
            continue
        text = raw.split(";", 1)[0].strip()
        if not text or text.startswith("."):
            continue
        k = kind(text.split()[0])
        if k:
            insts.append((k, line, text))

    def counts(lo, hi):
        c = collections.Counter(k for k, _, _ in insts[lo:hi])
        return "%5d salu %5d valu %4d lds %4d vmem" % (c["salu"], c["valu"], c["lds"], c["vmem"])

    if dump:
        at = collections.defaultdict(list)
        for name, i in labels.items():
            at[i].append(name)
        for i in range(dump[0], min(dump[1], len(insts))):
            for name in at[i]:
                print("%s:" % name)
            print("%6d  line %4d  %s" % (i, insts[i][1], insts[i][2]))
        return 0
    print("%s: %s" % (kernel, counts(0, len(insts))))
    by_phase = collections.defaultdict(collections.Counter)
    for k, ln, _ in insts:
        name = next((n for lo, hi, n in phases if lo <= ln <= hi), "other")
        by_phase[name][k] += 1
    for name, c in by_phase.items():
        print("  phase %-28s %5d salu %5d valu %4d lds %4d vmem" % (name, c["salu"], c["valu"], c["lds"], c["vmem"]))
    loops = []
    for i, (_, _, text) in enumerate(insts):
        m = BRANCH_RE.match(text)
        if m and m.group(1) in labels and labels[m.group(1)] <= i:
            loops.append((labels[m.group(1)], i + 1))
    for lo, hi in sorted(set(loops)):
        lines = collections.Counter(ln for _, ln, _ in insts[lo:hi])
        top = ",".join(str(l) for l, _ in lines.most_common(4))
        print("  loop [%6d,%6d) lines %d-%d (most: %s): %s" % (lo, hi, min(lines), max(lines), top, counts(lo, hi)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
