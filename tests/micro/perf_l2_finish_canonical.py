# The canonical device finish (SP_FINISH_CANONICAL, csrc/l2_finish.h) on the headline batch of bench.py's pipeline workload, for
# the exact engine and for result-set mode: count, offsets, sort and place by HIP events (lastFinishMs, lastFinishSortMs)
# beside the plain finish of the same batch in the same run (perf_l2_finish.py and profiles/r05_finish_perf.json are the
# yardstick for that one), and whether the two engines' canonical results and items are the same bytes.
#   python tests/micro/perf_l2_finish_canonical.py [docs of 64 KiB, default 12288] [out.json]
import ctypes, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
import struspattern_amd as spa
from struspattern_amd import capi, synth

ndocs = int(sys.argv[1]) if len(sys.argv) > 1 else 12288
REPS = 5                                           # after one finish that allocates and warms up; every sample is kept
out = {"ndocs": ndocs, "reps": REPS, "sort_tile": int(capi.lib().sp_matcher_finish_sort_tile())}
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


def timed(ctx, canonical):
    """the passes of REPS finishes: the one with the smallest sum, and the sums of all of them (the spread)"""
    ctx.batchFinishDevice(stream, canonical=canonical)
    samples = []
    for _ in range(REPS):
        ctx.batchFinishDevice(stream, canonical=canonical)
        a, b, p = ctx.lastFinishMs()
        samples.append({"count_ms": a, "offsets_ms": b, "sort_ms": ctx.lastFinishSortMs(), "place_ms": p})
    for s in samples:
        s["finish_ms"] = s["count_ms"] + s["offsets_ms"] + s["sort_ms"] + s["place_ms"]
    best = dict(min(samples, key=lambda s: s["finish_ms"]))
    best["all_finish_ms"] = [s["finish_ms"] for s in samples]
    best["all_place_ms"] = [s["place_ms"] for s in samples]
    return best


def device_copy(ptr, nbytes):
    t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert hip_memcpy(t.data_ptr(), ptr, nbytes, 3, stream) == 0
    torch.cuda.synchronize()
    return t


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
finished = {}
for name, result_sets in (("exact", False), ("result_sets", True)):
    mctx = mi.createContext(result_sets=result_sets)
    c = sized(mctx, lambda: mctx.matchLexedDevice(lo[-1].d_lexems, lo[-1].d_doc_ranges, ndocs, int(lc["lexems"]), stream), ndocs,
              lambda c: mctx.reserveOutput(int(c["results"] * 1.2) + 1024, int(c["items"] * 1.2) + 1024))
    r = {"results": c["results"], "items": c["items"], "kernel_kind": mctx.kernelKind(), "rule_stage_ms": mctx.lastKernelMs()}
    r["plain"] = timed(mctx, False)
    r["canonical"] = timed(mctx, True)
    r["canonical_over_plain"] = r["canonical"]["finish_ms"] / r["plain"]["finish_ms"]
    r["canonical_over_rule_stage"] = r["canonical"]["finish_ms"] / r["rule_stage_ms"]
    fin = mctx.batchFinishDevice(stream, canonical=True)
    finished[name] = (device_copy(fin.d_results, c["results"] * 36), device_copy(fin.d_items, c["items"] * 28))
    out[name] = r
    print(name, json.dumps(r), flush=True)
    del mctx
    torch.cuda.empty_cache()
out["same_bytes_from_both_engines"] = bool(torch.equal(finished["exact"][0], finished["result_sets"][0])
                                           and torch.equal(finished["exact"][1], finished["result_sets"][1]))
print("same bytes from both engines:", out["same_bytes_from_both_engines"], flush=True)
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
