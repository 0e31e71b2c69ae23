# The order of the dictionary of a finished batch on the device (csrc/l2_dictorder.h) on the workload of
# tests/micro/perf_dictionary.py: the pipeline rule set (10 000 regexes + 10 000 rules), documents of 64 KiB, text terms.  An
# order call by HIP events (lastDictionaryOrderMs: every launch; the memsets that clear the cursor and fill the rank are
# enqueued before the first event and lie outside) beside the dictionary call, and beside the route it replaces:
# finishedTermsFetch() + finishedDictionaryFetch() + the fetch of the source bytes (finishedFetch for the document offsets,
# finishedTextFetch), then the sort on the host (sp_match_batch_dictionary_order, the C++ twin), timed on the host, the second
# of two rounds.  THE YARDSTICK is the fetches of that route alone; no fixed figure.  The device's bytes are compared with the
# host's.  Counted on the host from the fetched data: the comparisons of a merge sort that the 64-bit key does not decide.
#   python tests/micro/perf_dictorder.py [documents of 64 KiB, default 256] [out.json]
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
mctx = mi.createContext()
mc = sized(mctx, lambda: mctx.matchLexedDevice(lo[-1].d_lexems, lo[-1].d_doc_ranges, ndocs, int(lc["lexems"]), stream), ndocs,
           lambda c: mctx.reserveOutput(int(c["results"] * 1.2) + 1024, int(c["items"] * 1.2) + 1024))
mctx.batchFinishDevice(stream)
mctx.finishedTextDevice(d_text.data_ptr(), len(text), d_offs.data_ptr(), ndocs, results=True, items=False, stream=stream)
mctx.finishedTermsDevice(spa.SP_TERM_TEXT, stream)
terms_ms = mctx.lastTermsMs()
mctx.finishedDictionaryDevice(stream)
dict_ms = mctx.lastDictionaryMs()


def order():
    t0 = time.perf_counter()
    mctx.finishedDictionaryOrderDevice(stream)
    host = (time.perf_counter() - t0) * 1e3     # the call returns without waiting: what the host spends enqueueing
    return mctx.lastDictionaryOrderMs(), host


order(), order()
samples = [order() for _ in range(REPS)]
order_ms = statistics.median(s[0] for s in samples)
enqueue_ms = statistics.median(s[1] for s in samples)

# the route without the call: the terms, the dictionary and the source bytes to the host, the sort there (twice: the first round
# pays for the host allocations and page faults, the second is the figure)
rounds = []
for _ in range(2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    terms = mctx.finishedTermsFetch()
    t1 = time.perf_counter()
    d = mctx.finishedDictionaryFetch()
    t2 = time.perf_counter()
    mb, mt = mctx.finishedFetch(), mctx.finishedTextFetch()
    t3 = time.perf_counter()
    twin = spa.batchDictionaryOrder(mb, terms, d, text=mt)
    t4 = time.perf_counter()
    rounds.append({"terms_fetch_ms": (t1 - t0) * 1e3, "dictionary_fetch_ms": (t2 - t1) * 1e3, "source_fetch_ms": (t3 - t2) * 1e3,
                   "terms_and_dictionary_fetch_ms": (t2 - t0) * 1e3, "fetches_ms": (t3 - t0) * 1e3, "host_sort_ms": (t4 - t3) * 1e3, "all_ms": (t4 - t0) * 1e3})
fetches_ms, route_ms = rounds[1]["fetches_ms"], rounds[1]["all_ms"]

got = mctx.finishedDictionaryOrderFetch()
same = all(getattr(got, f).tobytes() == getattr(twin, f).tobytes() for f in ("order", "rank", "prefix_bytes", "handle_offsets"))
assert same and not terms.status.any()

# how often the key of (handle, first four bytes) ties between neighbours of the sorted order: the comparisons of the last
# merge steps between neighbours, a lower bound of the share that reads the bytes
n, ndict = len(terms.records), len(d.records)
handles = d.records[got.order, 0].astype(np.int64)
tie_neighbours = int(np.count_nonzero((handles[1:] == handles[:-1]) & (got.prefix_bytes[1:] >= 4))) if ndict > 1 else 0
lengths = d.records[:, 1]
tile = capi.lib().sp_matcher_dictionary_order_tile()
tiles = (ndict + tile - 1) // tile
levels = max(tiles - 1, 0).bit_length()
out = {"ndocs": ndocs, "text_bytes": int(len(text)), "terms": n, "ndict": ndict, "handle_bound": int(len(d.handle_terms)),
       "value_bytes_mean": float(lengths.mean()) if ndict else 0.0, "value_bytes_max": int(lengths.max()) if ndict else 0,
       "prefix_bytes_mean": float(got.prefix_bytes.mean()) if ndict else 0.0, "prefix_bytes_max": int(got.prefix_bytes.max()) if ndict else 0,
       "neighbours_that_tie_on_the_key": tie_neighbours, "share_of_neighbours_that_tie_on_the_key": tie_neighbours / max(ndict - 1, 1),
       "tile": tile, "tiles": tiles, "merge_levels": levels, "launches": 3 + (1 + levels if ndict > 1 else 0),
       "working_memory_bytes": 2 * 12 * ndict + 12 * ndict + 4,
       "order_ms_median": order_ms, "order_ms_all": [s[0] for s in samples], "order_enqueue_host_ms_median": enqueue_ms, "reps": REPS,
       "dictionary_ms": dict_ms, "terms_ms": terms_ms,
       "replaced_route_rounds": rounds, "replaced_route_fetches_ms": fetches_ms, "replaced_route_ms": route_ms,
       "device_faster_than_the_fetches_of_the_route": bool(order_ms < fetches_ms), "fetches_over_device": fetches_ms / order_ms,
       "device_faster_than_terms_and_dictionary_fetch": bool(order_ms < rounds[1]["terms_and_dictionary_fetch_ms"]),
       "route_over_device": route_ms / order_ms, "identical_to_host": bool(same)}
print(json.dumps(out), flush=True)
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
