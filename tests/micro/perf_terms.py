# The index terms of a finished batch on the device (csrc/l2_terms.h) on the synthetic pipeline of bench.py's generator
# (--workload pipeline shapes: 10 000 regexes + 10 000 rules, documents of 64 KiB), the workload of
# tests/micro/perf_pattern_freq.py at a document count that fits a few seconds: all passes of a terms call by HIP events
# (lastTermsMs; the host's wait for the total between offsets and place lies inside) beside what a caller had to do without
# it -- finishedFetch() of the batch and the fetch of the text of its results (the rule set has no format strings, so the term
# value of a result is its text), then the grouping on the host (sp_match_batch_terms, the C++ twin).  THE BAR: the device
# pass takes less time than the two fetches alone; the host grouping comes on top.  The device's bytes are compared with the
# host's.
#   python tests/micro/perf_terms.py [documents of 64 KiB, default 256] [out.json]
import json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
import struspattern_amd as spa
from struspattern_amd import capi, synth

REPS = 10                   # timed calls, after two that allocate and warm up
ndocs = int(sys.argv[1]) if len(sys.argv) > 1 else 256
stream = torch.cuda.current_stream().cuda_stream


def sized(ctx, run, n, reserve):
    for _ in range(8):
        run()
        c = ctx.batchCounters()
        if c["failed_docs"] == 0:
            return c
        assert set(int(x) for x in ctx.batchStatus(n) if x) <= {2, 9}
        reserve(c)
        ctx.growArena()
    raise SystemExit("documents still failing after resizing")


vocab = synth.vocabulary(30000, 1)
pats, rules = synth.pipeline_workload(10000, 10000, vocab, seed=4)
text, offs = bench.text_corpus(ndocs * 4, 16384, vocab, seed=1000, utf8=True)
offs = np.ascontiguousarray(offs[::4])
lxi = spa.PatternLexerInstance()
synth.apply_lexer_patterns(lxi, pats)
lctx = lxi.createContext()
d_text = torch.from_numpy(text).cuda()
d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
lo = []
lc = sized(lctx, lambda: lo.append(lctx.matchDocsDevice(d_text.data_ptr(), d_offs.data_ptr(), ndocs, len(text), stream)), ndocs,
           lambda c: lctx.reserveOutput(int(c["lexems"] * 1.2) + 1024))
mi = spa.PatternMatcherInstance()
synth.apply_rules(mi, rules)
bound = mi.handleBound()
mctx = mi.createContext()
mc = sized(mctx, lambda: mctx.matchLexedDevice(lo[-1].d_lexems, lo[-1].d_doc_ranges, ndocs, int(lc["lexems"]), stream), ndocs,
           lambda c: mctx.reserveOutput(int(c["results"] * 1.2) + 1024, int(c["items"] * 1.2) + 1024))
mctx.batchFinishDevice(stream)
finish_ms = sum(mctx.lastFinishMs())
mctx.finishedTextDevice(d_text.data_ptr(), len(text), d_offs.data_ptr(), ndocs, results=True, items=False, stream=stream)
text_ms = mctx.lastTextMs()


def terms():
    mctx.finishedTermsDevice(spa.SP_TERM_TEXT, stream)
    return mctx.lastTermsMs()


terms(), terms()
samples = [terms() for _ in range(REPS)]
terms_ms = statistics.median(samples)

# the route without the call: the batch and the text of its results to the host (twice: the first call pays for the host
# allocations and page faults, the second is the figure), the grouping there
fetches = []
for _ in range(2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mb = mctx.finishedFetch()
    t1 = time.perf_counter()
    mt = mctx.finishedTextFetch()
    t2 = time.perf_counter()
    fetches.append({"finished_fetch_ms": (t1 - t0) * 1e3, "text_fetch_ms": (t2 - t1) * 1e3, "both_ms": (t2 - t0) * 1e3})
fetch_ms = min(f["both_ms"] for f in fetches)
t0 = time.perf_counter()
twin = spa.batchTerms(mb, text=mt, handle_bound=bound, flags=spa.SP_TERM_TEXT)
host_group_ms = (time.perf_counter() - t0) * 1e3

got = mctx.finishedTermsFetch()
same = all(np.array_equal(getattr(got, f), getattr(twin, f)) for f in ("records", "doc_offsets", "result_term", "status"))
assert same and not got.status.any()

nres, nrec = len(mb.results), len(got.records)
text_bytes = len(mt.result_text)
out = {"ndocs": ndocs, "text_bytes": int(len(text)), "results": nres, "results_per_document": nres / max(1, ndocs), "handle_bound": bound,
       "terms": nrec, "mean_count": nres / max(1, nrec), "term_tile": capi.lib().sp_matcher_term_tile(),
       "terms_ms_median": terms_ms, "terms_ms_all": samples, "reps": REPS,
       "fetches": fetches, "two_fetches_ms": fetch_ms, "host_grouping_ms": host_group_ms,
       "device_faster_than_the_two_fetches": bool(terms_ms < fetch_ms), "fetches_over_device": fetch_ms / terms_ms,
       "bytes_moved_by_the_fetches": 36 * nres + 8 * (nres + 1) + text_bytes + 8 * (ndocs + 1) + 36 * ndocs,
       "value_bytes": text_bytes, "mean_value_bytes": text_bytes / max(1, nres),
       "bytes_left_for_a_terms_fetch": 24 * nrec + 4 * nres + 12 * ndocs + 8,
       "working_memory_bytes": 16 * nres, "finish_ms": finish_ms, "text_ms": text_ms, "rule_stage_ms": mctx.lastKernelMs(),
       "identical_to_host": bool(same)}
print(json.dumps(out), flush=True)
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
