# The positions of the postings of a finished batch on the device (csrc/l2_positions.h) on the workload of
# tests/micro/perf_postings.py: the pipeline rule set (10 000 regexes + 10 000 rules), documents of 64 KiB, text terms.  A
# positions call by HIP events (lastPositionsMs: every launch and the host's one wait between them; the memsets that clear the
# cursors, the totals and posting_positions are enqueued before the first event and lie outside), its launches summed by kind
# (lastPositionsLaunchMs, in calls of their own with an event behind every launch), the host's time in the call and in its one
# wait, beside the route it replaces: finishedFetch() + finishedTermsFetch() + finishedPostingsFetch(), then the gather on the
# host (sp_match_batch_positions, the C++ twin), timed on the host, the second of two rounds.  THE YARDSTICK is the three
# fetches alone; no fixed figure.  The device's bytes are compared with the host's.
#   python tests/micro/perf_positions.py [documents of 64 KiB, default 256] [out.json]
import json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
import struspattern_amd as spa
from struspattern_amd import capi, synth

REPS = 10                   # timed calls, after two that allocate and warm up
DIGIT_BITS = 8
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
mctx.finishedPostingsDevice(stream)
postings_ms = mctx.lastPostingsMs()
L = capi.lib()


def positions():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mctx.finishedPositionsDevice(stream)
    host = (time.perf_counter() - t0) * 1e3     # enqueueing, and the one wait for nocc and the largest position
    return mctx.lastPositionsMs(), host


positions(), positions()
samples = [positions() for _ in range(REPS)]
pos_ms = statistics.median(s[0] for s in samples)
host_ms = statistics.median(s[1] for s in samples)

# the launches by kind: calls of their own, an event behind every launch
L.sp_test_positions_launch_events(1)
kinds = []
for _ in range(REPS):
    mctx.finishedPositionsDevice(stream)
    kinds.append(mctx.lastPositionsLaunchMs())
L.sp_test_positions_launch_events(0)
launch_ms = {k: statistics.median(s[k] for s in kinds) for k in kinds[0]}
mctx.finishedPositionsDevice(stream)

# the route without the call: the finished batch, the terms and the postings to the host, the gather there (twice: the first
# round pays for the host allocations and page faults, the second is the figure)
rounds = []
for _ in range(2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mb = mctx.finishedFetch()
    t1 = time.perf_counter()
    terms = mctx.finishedTermsFetch()
    t2 = time.perf_counter()
    post = mctx.finishedPostingsFetch()
    t3 = time.perf_counter()
    twin = spa.batchPositions(mb, terms, post)
    t4 = time.perf_counter()
    rounds.append({"finished_fetch_ms": (t1 - t0) * 1e3, "terms_fetch_ms": (t2 - t1) * 1e3, "postings_fetch_ms": (t3 - t2) * 1e3,
                   "fetches_ms": (t3 - t0) * 1e3, "host_gather_ms": (t4 - t3) * 1e3, "all_ms": (t4 - t0) * 1e3})
fetches_ms, route_ms = rounds[1]["fetches_ms"], rounds[1]["all_ms"]

got = mctx.finishedPositionsFetch()
same = all(getattr(got, f).tobytes() == getattr(twin, f).tobytes() for f in ("occurrences", "posting_offsets", "posting_positions", "totals"))
assert same and not terms.status.any()

nres, n, nocc = len(mb.results), len(post.records), len(got.occurrences)
tile = L.sp_matcher_positions_tile()
tiles = (nres + tile - 1) // tile
largest = int(mb.results[:, 1].max()) if nres else 0
passes = [(largest.bit_length() + DIGIT_BITS - 1) // DIGIT_BITS, (max(n - (0 if nocc < nres else 1), 0).bit_length() + DIGIT_BITS - 1) // DIGIT_BITS]
out = {"ndocs": ndocs, "text_bytes": int(len(text)), "results": nres, "postings": n, "occurrences": nocc, "positions": int(got.totals[1]),
       "largest_ordpos": largest, "digit_bits": DIGIT_BITS, "radix_passes": passes, "tile": tile, "tiles": tiles,
       "hist_words_per_pass": 256 * tiles, "launches": 4 + 3 * sum(passes),
       "working_memory_bytes": 4 * nres + 2 * 8 * nres + 4 * 256 * tiles + 4 * 131,
       "positions_ms_median": pos_ms, "positions_ms_all": [s[0] for s in samples], "positions_host_ms_median": host_ms, "reps": REPS,
       "launch_ms_median_by_kind": launch_ms, "launch_ms_sum": sum(launch_ms.values()),
       "postings_ms": postings_ms, "dictionary_ms": dict_ms, "terms_ms": terms_ms,
       "replaced_route_rounds": rounds, "replaced_fetches_ms": fetches_ms, "replaced_route_ms": route_ms,
       "device_faster_than_the_fetches_alone": bool(pos_ms < fetches_ms), "fetches_over_device": fetches_ms / pos_ms, "route_over_device": route_ms / pos_ms,
       "identical_to_host": bool(same)}
print(json.dumps(out), flush=True)
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
