# The pattern frequencies of a finished batch on the device (csrc/l2_freq.h) on the synthetic pipeline of bench.py's generator,
# 2048 documents of 64 KiB, the workload of tests/micro/span_text_perf.py: all passes of a frequency call by HIP events
# (lastPatternFreqMs; the host's wait for the total between offsets and place lies inside) beside the finish and the rule stage of
# the same run, and beside the route a caller had to take without it -- finishedFetch() of the batch, then the same sums on the
# host (sp_match_batch_pattern_freq, the C++ twin).  The device's bytes are compared with the host's.
#   python tests/micro/perf_pattern_freq.py [documents of 64 KiB, default 2048] [out.json]
import json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
import struspattern_amd as spa
from struspattern_amd import capi, synth

HBM_PEAK_TBPS = 8.0         # MI355X, HBM3E
REPS = 10                   # timed calls, after two that allocate and warm up
ndocs = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
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


def frequencies():
    mctx.finishedPatternFreqDevice(stream)
    return mctx.lastPatternFreqMs()


frequencies(), frequencies()
samples = [frequencies() for _ in range(REPS)]
freq_ms = statistics.median(samples)

# the route without the call: the batch to the host, the sums there
t0 = time.perf_counter()
mb = mctx.finishedFetch()
t1 = time.perf_counter()
twin = spa.batchPatternFreq(mb, bound)
t2 = time.perf_counter()
host = {"finished_fetch_ms": (t1 - t0) * 1e3, "host_sums_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3}

got = mctx.finishedPatternFreqFetch()
same = all(np.array_equal(getattr(got, f), getattr(twin, f)) for f in ("records", "doc_offsets", "status", "handle_results", "handle_docs"))
assert same and not got.status.any()

nres, nrec = len(mb.results), len(got.records)
window = capi.lib().sp_matcher_pattern_freq_window()
windows = -(-bound // window)
# the lines of the result records under the sweeps of their handle word (the bound check, then per window: count, place,
# accumulate) and the records in the totals pass; the records zeroed and initialised, three atomics per result, two per record
read = (1 + 3 * windows) * 36 * nres + 16 * nrec
written = 2 * 16 * nrec + 12 * nres + 12 * nrec
rule_ms = mctx.lastKernelMs()
out = {"ndocs": ndocs, "text_bytes": int(len(text)), "results": nres, "handle_bound": bound, "window": window, "records": nrec,
       "result_bytes": 36 * nres, "record_bytes": 16 * nrec, "mean_count": nres / max(1, nrec),
       "pattern_freq_ms_median": freq_ms, "pattern_freq_ms_all": samples, "reps": REPS,
       "bytes_read": read, "bytes_written": written, "TBps": (read + written) / freq_ms / 1e9,
       "fraction_of_hbm_peak": (read + written) / freq_ms / 1e9 / HBM_PEAK_TBPS, "hbm_peak_TBps": HBM_PEAK_TBPS,
       "finish_ms": finish_ms, "rule_stage_ms": rule_ms, "lexer_ms": lctx.lastKernelMs(), "slower_than_rule_stage": bool(freq_ms > rule_ms),
       "host_route": host, "host_over_device": host["total_ms"] / freq_ms, "identical_to_host": bool(same)}
print(json.dumps(out), flush=True)
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
