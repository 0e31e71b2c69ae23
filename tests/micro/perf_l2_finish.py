# The device finish (csrc/l2_finish.h) on the headline batch of bench.py's pipeline workload, for the exact engine and for
# result-set mode: the three passes by HIP events (lastFinishMs) beside the yardstick, a hipMemcpyAsync device-to-device
# of the same two used byte ranges (results, items) in the same run.  Then the `exclusive` path on the larger input of
# tests/test_finish_device_gpu.py beside the wall time of batchFetch (PCIe + the host loop it replaces for device consumers).
#   python tests/micro/perf_l2_finish.py [docs of 64 KiB, default 12288] [out.json]
import ctypes, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
import struspattern_amd as spa
from struspattern_amd import capi, synth

ndocs = int(sys.argv[1]) if len(sys.argv) > 1 else 12288
out = {"ndocs": ndocs}
stream = torch.cuda.current_stream().cuda_stream
hip_memcpy = capi.lib().hipMemcpyAsync
hip_memcpy.restype, hip_memcpy.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]


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


def timed_finish(ctx, dev, c, reps=3):
    """min over reps of the passes, and of the two device-to-device copies of the same used ranges (into the finished buffers)"""
    fin = ctx.batchFinishDevice(stream)            # (allocates)
    best, copy = None, None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert hip_memcpy(fin.d_results, dev.d_results, c["results"] * 36, 3, stream) == 0
        assert hip_memcpy(fin.d_items, dev.d_items, c["items"] * 28, 3, stream) == 0
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        copy = ms if copy is None else min(copy, ms)
        fin = ctx.batchFinishDevice(stream)
        p = ctx.lastFinishMs()
        if best is None or sum(p) < sum(best):
            best = p
    return {"results": c["results"], "items": c["items"], "bytes": c["results"] * 36 + c["items"] * 28,
            "count_ms": best[0], "offsets_ms": best[1], "place_ms": best[2], "finish_ms": sum(best), "memcpy_d2d_ms": copy,
            "finish_over_memcpy": sum(best) / copy, "place_TBps": 2 * (c["results"] * 36 + c["items"] * 28) / best[2] / 1e9}


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
for name, result_sets in (("exact", False), ("result_sets", True)):
    mctx = mi.createContext(result_sets=result_sets)
    dev = []
    c = sized(mctx, lambda: dev.append(mctx.matchLexedDevice(lo[-1].d_lexems, lo[-1].d_doc_ranges, ndocs, int(lc["lexems"]), stream)), ndocs,
              lambda c: mctx.reserveOutput(int(c["results"] * 1.2) + 1024, int(c["items"] * 1.2) + 1024))
    r = timed_finish(mctx, dev[-1], c)
    r["kernel_kind"] = mctx.kernelKind()
    r["rule_stage_ms"] = mctx.lastKernelMs()
    out[name] = r
    print(name, json.dumps(r), flush=True)
    del mctx, dev
    torch.cuda.empty_cache()

# `exclusive`: the larger input of the tests
rules = synth.random_rules(400, 30, 3)
lex, offs = synth.random_documents(300, 600, 30, 4)
m = spa.PatternMatcherInstance()
m.defineOption("exclusive")
m.defineOption("maxResultSize", 30)
synth.apply_rules(m, rules)
ctx = m.createContext()
d_lex = torch.from_numpy(lex.view(np.int32)).cuda()
d_off = torch.from_numpy(offs.view(np.int64)).cuda()
c = sized(ctx, lambda: ctx.matchDocsDevice(d_lex.data_ptr(), d_off.data_ptr(), len(offs) - 1, len(lex), stream), len(offs) - 1,
          lambda c: ctx.reserveOutput(int(c["results"] * 1.2) + 1024, int(c["items"] * 1.2) + 1024))
ctx.batchFinishDevice(stream)
best = None
for _ in range(3):
    ctx.batchFinishDevice(stream)
    p = ctx.lastFinishMs()
    if best is None or sum(p) < sum(best):
        best = p
kept = len(ctx.finishedFetch().results)
host = None
for _ in range(3):
    t0 = time.perf_counter()
    b = ctx.batchFetch()
    ms = (time.perf_counter() - t0) * 1e3
    host = ms if host is None else min(host, ms)
assert len(b.results) == kept
out["exclusive"] = {"raw_results": c["results"], "kept_results": kept, "count_ms": best[0], "offsets_ms": best[1], "place_ms": best[2],
                    "finish_ms": sum(best), "batch_fetch_wall_ms": host}
print("exclusive", json.dumps(out["exclusive"]), flush=True)
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
