# The host fetch of a finished device batch (csrc/batch_fetch.hpp) by wall time, on the shapes of perf_l2_finish.py: the
# `exclusive` rule set over 300 documents of 600 lexems (whole batch, 64 single documents, a host matchDocs) and the pipeline
# workload's lexer over `ndocs` documents of 64 KiB (whole batch, 64 single documents).  Every figure: median, min and max of
# REPEATS calls after a warm-up call.
#   python tests/micro/perf_batch_fetch.py [out.json] [lexer documents, default 1024]
#       SPA_TREE=<checkout of another commit, its library built>: times that commit's package and library instead
#   python tests/micro/perf_batch_fetch.py compare parent.json this.json out.json
#       both sets in one file; a median of `this` may exceed the parent's by no more than the parent's own max - min
import json, os, statistics, sys, time

REPEATS = 9


def compare(parent_file, this_file, out_file):
    with open(parent_file) as f:
        parent = json.load(f)
    with open(this_file) as f:
        this = json.load(f)
    verdict = {}
    for name, p in parent["timings"].items():
        t = this["timings"][name]
        verdict[name] = {"parent_median_ms": p["median_ms"], "this_median_ms": t["median_ms"], "parent_spread_ms": p["max_ms"] - p["min_ms"],
                         "within_spread": t["median_ms"] <= p["median_ms"] + (p["max_ms"] - p["min_ms"])}
        print(name, json.dumps(verdict[name]))
    with open(out_file, "w") as f:
        json.dump({"parent": parent, "this": this, "verdict": verdict}, f, indent=1)
    return 0 if all(v["within_spread"] for v in verdict.values()) else 1


if len(sys.argv) > 1 and sys.argv[1] == "compare":
    sys.exit(compare(*sys.argv[2:5]))

import numpy as np, torch
ROOT = os.environ.get("SPA_TREE") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
import struspattern_amd as spa
from struspattern_amd import synth

lexdocs = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
stream = torch.cuda.current_stream().cuda_stream
out = {"tree": os.path.abspath(ROOT), "library": spa.capi._build.LIB, "repeats": REPEATS, "lexer_docs": lexdocs, "timings": {}}


def sized(ctx, run, n, reserve):
    for _ in range(8):
        run()
        c = ctx.batchCounters()
        if c["failed_docs"] == 0:
            return c
        codes = set(int(x) for x in ctx.batchStatus(n) if x)
        assert codes <= {2, 9}, codes
        reserve(c)
        ctx.growArena()
    raise SystemExit("documents still failing after resizing")


def timed(name, fn):
    fn()
    ms = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    out["timings"][name] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "all_ms": ms}
    print(name, json.dumps(out["timings"][name]), flush=True)


# rule matcher: the `exclusive` input of perf_l2_finish.py
rules = synth.random_rules(400, 30, 3)
lex, offs = synth.random_documents(300, 600, 30, 4)
m = spa.PatternMatcherInstance()
m.defineOption("exclusive")
m.defineOption("maxResultSize", 30)
synth.apply_rules(m, rules)
ctx = m.createContext()
d_lex = torch.from_numpy(lex.view(np.int32)).cuda()
d_off = torch.from_numpy(offs.view(np.int64)).cuda()
ndocs = len(offs) - 1
c = sized(ctx, lambda: ctx.matchDocsDevice(d_lex.data_ptr(), d_off.data_ptr(), ndocs, len(lex), stream), ndocs,
          lambda c: ctx.reserveOutput(int(c["results"] * 1.2) + 1024, int(c["items"] * 1.2) + 1024))
out["matcher"] = {"ndocs": ndocs, "raw_results": c["results"], "raw_items": c["items"], "kept_results": len(ctx.batchFetch().results)}
timed("matcher_batch_fetch_whole", lambda: ctx.batchFetch())
timed("matcher_batch_fetch_64_single_docs", lambda: [ctx.batchFetch(i, 1) for i in range(64)])
timed("matcher_host_match_docs", lambda: ctx.matchDocs(lex, offs))

# lexer: the pipeline workload's pattern set
vocab = synth.vocabulary(30000, 1)
pats, _ = synth.pipeline_workload(10000, 10000, vocab, seed=4)
text, toffs = bench.text_corpus(lexdocs * 4, 16384, vocab, seed=1000, utf8=True)
toffs = np.ascontiguousarray(toffs[::4])
lxi = spa.PatternLexerInstance()
synth.apply_lexer_patterns(lxi, pats)
lctx = lxi.createContext()
d_text = torch.from_numpy(text).cuda()
d_toffs = torch.from_numpy(toffs.view(np.int64)).cuda()
lc = sized(lctx, lambda: lctx.matchDocsDevice(d_text.data_ptr(), d_toffs.data_ptr(), lexdocs, len(text), stream), lexdocs,
           lambda c: lctx.reserveOutput(int(c["lexems"] * 1.2) + 1024))
out["lexer"] = {"ndocs": lexdocs, "lexems": lc["lexems"]}
timed("lexer_batch_fetch_whole", lambda: lctx.batchFetch(0, lexdocs))
timed("lexer_batch_fetch_64_single_docs", lambda: [lctx.batchFetch(i, 1) for i in range(64)])

if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
