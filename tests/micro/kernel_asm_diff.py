#!/usr/bin/env python3
"""Compares the functions of device assembly files (`hipcc -S --cuda-device-only`, as tests/micro/kernel_resources.sh
compiles with KEEP_ASM) as text: what a source file's functions were compiled to before and after the source was moved around.

    usage: tests/micro/kernel_asm_diff.py old.s new.s [new2.s ...]

Every file is split into its functions; comments and directives are dropped and the local labels (.L...) renamed by order
of appearance inside the function.  One line per function of old.s and per new file that has it: SAME or DIFF with the line
counts; then the names found on one side only.  A function that several new files have is compared once per file.
Exit status 1 when a function differs or is missing from the new files."""
import re
import sys

TYPE_RE = re.compile(r"^\s*\.type\s+([^\s,]+),@function")
LABEL_RE = re.compile(r"\.L[A-Za-z0-9_$.]+")


def functions(path):
    """name -> list of normalised instruction and label lines"""
    out = {}
    pending, name, body = set(), None, None
    with open(path) as f:
        for raw in f:
            m = TYPE_RE.match(raw)
            if m:
                pending.add(m.group(1))
                continue
            line = raw.split(";", 1)[0].strip()
            if not line:
                continue
            if name is None:
                if line.endswith(":") and line[:-1] in pending:
                    name, body = line[:-1], []
                    pending.discard(name)
                continue
            if line.startswith(".Lfunc_end") or line.startswith(".size"):
                out[name] = relabel(body)
                name, body = None, None
                continue
            if line.startswith(".") and not (line.startswith(".L") and line.endswith(":")):
                continue  # a directive
            body.append(" ".join(line.split()))
    if name is not None:
        out[name] = relabel(body)
    return out


def relabel(lines):
    names = {}
    def sub(m):
        return names.setdefault(m.group(0), ".L%d" % len(names))
    return [LABEL_RE.sub(sub, l) for l in lines]


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    old = functions(argv[1])
    news = [(p, functions(p)) for p in argv[2:]]
    bad = 0
    for name in sorted(old):
        found = False
        for path, fn in news:
            if name not in fn:
                continue
            found = True
            same = fn[name] == old[name]
            bad += not same
            print("%s %s  %d -> %d lines  (%s)" % ("SAME" if same else "DIFF", name, len(old[name]), len(fn[name]), path))
        if not found:
            bad += 1
            print("ONLY IN OLD %s  %d lines" % (name, len(old[name])))
    for path, fn in news:
        for name in sorted(fn):
            if name not in old:
                print("ONLY IN NEW %s  %d lines  (%s)" % (name, len(fn[name]), path))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
