# Lookups in the index segment of a finished batch on the device (csrc/l2_segment.h) on the workload of
# tests/micro/perf_postingblocks.py: the pipeline rule set (10 000 regexes + 10 000 rules), documents of 64 KiB, text terms.  A
# segment of the context's term blocks and posting blocks (Segment.fromContext) answers 10 000 exact queries -- drawn from its own
# entries, one in ten changed into a miss -- and 100 prefix queries of two bytes.  A lookup by HIP events (lastLookupMs: the upload
# of the queries and the five launches with the host's waits inside) and as the host sees it (the call, and the call and the wait
# for the emitting launch), the median of ten calls after two that allocate and warm up; beside them the C twin
# (sp_match_segment_lookup) on one host thread for the same queries over the fetched products.  Both sides are timed at the C
# call: the queries and the structs are marshalled once, outside.  THE BAR: the device call, upload included, takes less than the
# twin; lookupFetch plus the call takes less than fetching both block products and running the twin.  The device's arrays are
# compared with the twin's.
#   python tests/micro/perf_segment_lookup.py [documents of 64 KiB, default 256] [out.json]
import ctypes, json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
import struspattern_amd as spa
from struspattern_amd import capi, synth
from struspattern_amd import products as P

REPS = 10                   # timed calls, after two that allocate and warm up
ndocs = int(sys.argv[1]) if len(sys.argv) > 1 else 256
stream = torch.cuda.current_stream().cuda_stream
L = capi.lib()


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
mctx.finishedTextDevice(d_text.data_ptr(), len(text), d_offs.data_ptr(), ndocs, results=True, items=False, stream=stream)
mctx.finishedTermsDevice(spa.SP_TERM_TEXT, stream)
mctx.finishedDictionaryDevice(stream)
mctx.finishedDictionaryOrderDevice(stream)
mctx.finishedPostingsDevice(stream)
mctx.finishedPositionsDevice(stream)
mctx.finishedTermBlocksDevice(stream)
mctx.finishedPostingBlocksDevice(stream)
segment = spa.Segment.fromContext(mctx, stream)

# the fetches of the route without the segment (twice: the first round pays for the host allocations, the second is the figure)
fetch_rounds = []
for _ in range(2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tb, pb = mctx.finishedTermBlocksFetch(), mctx.finishedPostingBlocksFetch()
    fetch_rounds.append((time.perf_counter() - t0) * 1e3)
blocks_fetch_ms = fetch_rounds[1]

entries = tb.entries()
rng = np.random.default_rng(7)
exact = []
for k, e in enumerate(rng.integers(0, len(entries), 10000).tolist()):
    h, v = entries[e][0], entries[e][1]
    exact.append((h, v + b"\x01") if k % 10 == 9 else (h, v))                   # one in ten misses
heads = sorted({(h, v[:2]) for h, v, _, _ in entries if len(v) >= 2})
prefix = [heads[int(i)] for i in rng.integers(0, len(heads), 100).tolist()]

keep = []
c_tb, c_pb = P._to_c(tb, keep), P._to_c(pb, keep)


def measure(queries, flags):
    args, held = P._host_queries(queries)
    out = capi.SpSegmentLookupDevice()

    def device():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.sp_segment_lookup_device(segment._h, *args, flags, stream, ctypes.byref(out))
        t1 = time.perf_counter()                # the call returns behind its last wait: the emitting launch is still running
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert rc == 0
        return segment.lastLookupMs(), (t1 - t0) * 1e3, (t2 - t0) * 1e3

    def fetched():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.sp_segment_lookup_device(segment._h, *args, flags, stream, ctypes.byref(out))
        s = capi.SpSegmentLookup()
        rc2 = L.sp_segment_lookup_fetch(segment._h, ctypes.byref(s))
        t1 = time.perf_counter()
        assert rc == 0 and rc2 == 0
        L.sp_segment_lookup_free(ctypes.byref(s))
        return (t1 - t0) * 1e3

    def twin():
        s, err = capi.SpSegmentLookup(), ctypes.create_string_buffer(256)
        t0 = time.perf_counter()
        rc = L.sp_match_segment_lookup(ctypes.byref(c_tb), ctypes.byref(c_pb), *args, flags, ctypes.byref(s), err, 256)
        t1 = time.perf_counter()
        assert rc == 0, err.value
        L.sp_segment_lookup_free(ctypes.byref(s))
        return (t1 - t0) * 1e3

    device(), device()
    d = [device() for _ in range(REPS)]
    fetched()
    f = [fetched() for _ in range(REPS)]
    twin()
    w = [twin() for _ in range(REPS)]
    segment.lookupDevice(queries, prefix=bool(flags), stream=stream)
    got, want = segment.lookupFetch(), spa.segmentLookup(tb, pb, queries, prefix=bool(flags))
    same = all(getattr(got, a.attr).tobytes() == getattr(want, a.attr).tobytes() for a in P.SegmentLookup._ARRAYS)
    assert same and not got.q_status.any()
    med = statistics.median
    r = {"queries": len(queries), "nsel": int(got.totals[0]), "npostings": int(got.totals[1]), "npositions": int(got.totals[2]), "value_bytes": int(got.totals[3]),
         "lookup_ms_median": med(x[0] for x in d), "lookup_ms_min": min(x[0] for x in d), "lookup_ms_max": max(x[0] for x in d), "lookup_ms_all": [x[0] for x in d],
         "lookup_call_host_ms_median": med(x[1] for x in d), "lookup_done_host_ms_median": med(x[2] for x in d),
         "lookup_and_fetch_host_ms_median": med(f), "twin_ms_median": med(w), "twin_ms_all": w, "identical_to_twin": bool(same)}
    r["device_call_faster_than_twin"] = bool(r["lookup_done_host_ms_median"] < r["twin_ms_median"])
    r["twin_over_device_call"] = r["twin_ms_median"] / r["lookup_done_host_ms_median"]
    r["fetched_faster_than_block_fetches_and_twin"] = bool(r["lookup_and_fetch_host_ms_median"] < blocks_fetch_ms + r["twin_ms_median"])
    r["block_fetches_and_twin_over_fetched"] = (blocks_fetch_ms + r["twin_ms_median"]) / r["lookup_and_fetch_host_ms_median"]
    return r


out = {"ndocs": ndocs, "text_bytes": int(len(text)), "ndict": int(tb.ndict), "block_entries": int(tb.block_entries), "term_block_bytes": len(tb.bytes),
       "posting_block_bytes": len(pb.bytes), "position_varints": int(pb.totals[3]), "reps": REPS, "block_fetches_ms_rounds": fetch_rounds,
       "block_fetches_ms": blocks_fetch_ms, "exact": measure(exact, 0), "prefix": measure(prefix, P.SP_LOOKUP_PREFIX)}
print(json.dumps(out), flush=True)
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
