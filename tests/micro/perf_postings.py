# The postings of the dictionary of a finished batch on the device (csrc/l2_postings.h) on the workload of
# tests/micro/perf_dictionary.py: the pipeline rule set (10 000 regexes + 10 000 rules), documents of 64 KiB, text terms.  A
# postings call by HIP events (lastPostingsMs: every launch; the memset that clears the cursors is enqueued before the first
# event and lies outside) beside the dictionary call, and beside the route it replaces: finishedTermsFetch() +
# finishedDictionaryFetch(), then the inversion of term_dict on the host (sp_match_batch_postings, the C++ twin), timed on
# the host, the second of two rounds.  THE YARDSTICK is that route, fetches plus inversion; no fixed figure.  The device's
# bytes are compared with the host's.
#   python tests/micro/perf_postings.py [documents of 64 KiB, default 256] [out.json]
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


def postings():
    t0 = time.perf_counter()
    mctx.finishedPostingsDevice(stream)
    host = (time.perf_counter() - t0) * 1e3     # the call returns without waiting: what the host spends enqueueing
    return mctx.lastPostingsMs(), host


postings(), postings()
samples = [postings() for _ in range(REPS)]
post_ms = statistics.median(s[0] for s in samples)
enqueue_ms = statistics.median(s[1] for s in samples)

# the route without the call: the terms and the dictionary to the host, the inversion there (twice: the first round pays for
# the host allocations and page faults, the second is the figure)
rounds = []
for _ in range(2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    terms = mctx.finishedTermsFetch()
    t1 = time.perf_counter()
    d = mctx.finishedDictionaryFetch()
    t2 = time.perf_counter()
    twin = spa.batchPostings(terms, d)
    t3 = time.perf_counter()
    rounds.append({"terms_fetch_ms": (t1 - t0) * 1e3, "dictionary_fetch_ms": (t2 - t1) * 1e3, "host_inversion_ms": (t3 - t2) * 1e3, "all_ms": (t3 - t0) * 1e3})
route_ms = rounds[1]["all_ms"]

got = mctx.finishedPostingsFetch()
same = all(getattr(got, f).tobytes() == getattr(twin, f).tobytes() for f in ("records", "entry_offsets", "record_posting"))
assert same and not terms.status.any()

n, ndict = len(terms.records), len(d.records)
tile = capi.lib().sp_matcher_postings_tile()
tiles = (n + tile - 1) // tile
passes = (max(ndict - 1, 0).bit_length() + DIGIT_BITS - 1) // DIGIT_BITS
out = {"ndocs": ndocs, "text_bytes": int(len(text)), "terms": n, "ndict": ndict, "max_doc_freq": int(d.records[:, 4].max()) if ndict else 0,
       "digit_bits": DIGIT_BITS, "radix_passes": passes, "tile": tile, "tiles": tiles, "launches": 3 + 3 * passes,
       "working_memory_bytes": 4 * n + 2 * 8 * n + 4 * 256 * tiles + 4 * 66,
       "postings_ms_median": post_ms, "postings_ms_all": [s[0] for s in samples], "postings_enqueue_host_ms_median": enqueue_ms, "reps": REPS,
       "dictionary_ms": dict_ms, "terms_ms": terms_ms,
       "replaced_route_rounds": rounds, "replaced_route_ms": route_ms,
       "device_faster_than_the_replaced_route": bool(post_ms < route_ms), "route_over_device": route_ms / post_ms,
       "identical_to_host": bool(same)}
print(json.dumps(out), flush=True)
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
