# The matched text of a finished batch on the device (csrc/l2_text.h) on the synthetic pipeline of bench.py's generator,
# 2048 documents of 64 KiB: all passes of a text call by HIP events (lastTextMs; the host's wait for the totals between
# offsets and place lies inside) beside the route a caller had to take without it -- finishedFetch() of the batch, then a
# gather of the same spans from the host copy of the text (sp_match_batch_text, the C++ twin).  The device's bytes and
# offsets are compared with the host's.
#   python tests/micro/span_text_perf.py [documents of 64 KiB, default 2048] [out.json]
import json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
import struspattern_amd as spa
from struspattern_amd import synth

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
mctx = mi.createContext()
mc = sized(mctx, lambda: mctx.matchLexedDevice(lo[-1].d_lexems, lo[-1].d_doc_ranges, ndocs, int(lc["lexems"]), stream), ndocs,
           lambda c: mctx.reserveOutput(int(c["results"] * 1.2) + 1024, int(c["items"] * 1.2) + 1024))
mctx.batchFinishDevice(stream)
finish_ms = sum(mctx.lastFinishMs())


def gather():
    mctx.finishedTextDevice(d_text.data_ptr(), len(text), d_offs.data_ptr(), ndocs, stream=stream)
    return mctx.lastTextMs()


gather(), gather()
samples = [gather() for _ in range(REPS)]
text_ms = statistics.median(samples)

# the route without the call: the batch to the host, the spans sliced from the host text
host_text = text.tobytes()
t0 = time.perf_counter()
mb = mctx.finishedFetch()
t1 = time.perf_counter()
twin = spa.batchText(mb, host_text, offs)
t2 = time.perf_counter()
host = {"finished_fetch_ms": (t1 - t0) * 1e3, "host_gather_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3}

got = mctx.finishedTextFetch()
same = (got.result_text == twin.result_text and got.item_text == twin.item_text and np.array_equal(got.result_offsets, twin.result_offsets)
        and np.array_equal(got.item_offsets, twin.item_offsets) and np.array_equal(got.status, twin.status))
assert same and not got.status.any()

nres, nitems = len(mb.results), len(mb.items)
gathered = len(got.result_text) + len(got.item_text)
moved = 2 * gathered + 36 * nres + 28 * nitems + 8 * (nres + nitems)     # text read and written, records read, offsets written
out = {"ndocs": ndocs, "text_bytes": int(len(text)), "results": nres, "items": nitems, "result_text_bytes": len(got.result_text),
       "item_text_bytes": len(got.item_text), "mean_span_bytes": gathered / max(1, nres + nitems),
       "text_ms_median": text_ms, "text_ms_all": samples, "reps": REPS, "bytes_moved": moved, "text_TBps": moved / text_ms / 1e9,
       "fraction_of_hbm_peak": moved / text_ms / 1e9 / HBM_PEAK_TBPS, "hbm_peak_TBps": HBM_PEAK_TBPS,
       "finish_ms": finish_ms, "rule_stage_ms": mctx.lastKernelMs(), "lexer_ms": lctx.lastKernelMs(),
       "host_route": host, "host_over_device": host["total_ms"] / text_ms, "identical_to_host": bool(same)}
print(json.dumps(out), flush=True)
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
