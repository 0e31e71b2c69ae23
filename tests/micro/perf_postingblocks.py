# The posting blocks of a finished batch on the device (csrc/l2_postingblocks.h) on the workload of tests/micro/perf_termblocks.py:
# the pipeline rule set (10 000 regexes + 10 000 rules), documents of 64 KiB, text terms.  A posting-blocks call by HIP events
# (lastPostingBlocksMs: the six launches with the host's one wait inside; the memsets that clear the totals are enqueued before the
# first event and lie outside) and as the host sees it (enqueue and wait), beside the route it replaces: the fetches a host needs to
# permute and pack the lists itself -- finishedPostingsFetch() + finishedPositionsFetch() + finishedDictionaryFetch() +
# finishedDictionaryOrderFetch() --, then the coding on the host (sp_match_batch_posting_blocks, the C++ twin), timed on the host,
# the second of two rounds.  THE YARDSTICK is the fetches of that route alone; no fixed figure.  The device's bytes are compared
# with the host's.  finishedPostingBlocksFetch() is timed beside those fetches.
#   python tests/micro/perf_postingblocks.py [documents of 64 KiB, default 256] [out.json]
import json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
import struspattern_amd as spa
from struspattern_amd import synth

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
mctx.finishedDictionaryDevice(stream)
mctx.finishedDictionaryOrderDevice(stream)
mctx.finishedPostingsDevice(stream)
mctx.finishedPositionsDevice(stream)
postings_ms, positions_ms = mctx.lastPostingsMs(), mctx.lastPositionsMs()


def blocks():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mctx.finishedPostingBlocksDevice(stream)
    t1 = time.perf_counter()                    # the call returns behind its one wait: the emitting launch is still running
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return mctx.lastPostingBlocksMs(), (t1 - t0) * 1e3, (t2 - t0) * 1e3


blocks(), blocks()
samples = [blocks() for _ in range(REPS)]
blocks_ms = statistics.median(s[0] for s in samples)
call_host_ms = statistics.median(s[1] for s in samples)
done_host_ms = statistics.median(s[2] for s in samples)

# the route without the call (twice: the first round pays for the host allocations and page faults, the second is the figure)
rounds = []
for _ in range(2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    postings = mctx.finishedPostingsFetch()
    t1 = time.perf_counter()
    positions = mctx.finishedPositionsFetch()
    t2 = time.perf_counter()
    d, order = mctx.finishedDictionaryFetch(), mctx.finishedDictionaryOrderFetch()
    t3 = time.perf_counter()
    twin = spa.batchPostingBlocks(d, order, postings, positions)
    t4 = time.perf_counter()
    got = mctx.finishedPostingBlocksFetch()
    t5 = time.perf_counter()
    rounds.append({"postings_fetch_ms": (t1 - t0) * 1e3, "positions_fetch_ms": (t2 - t1) * 1e3, "dictionary_order_fetch_ms": (t3 - t2) * 1e3,
                   "fetches_ms": (t3 - t0) * 1e3, "host_twin_ms": (t4 - t3) * 1e3, "all_ms": (t4 - t0) * 1e3, "posting_blocks_fetch_ms": (t5 - t4) * 1e3})
fetches_ms, route_ms = rounds[1]["fetches_ms"], rounds[1]["all_ms"]

same = all(getattr(got, f).tobytes() == getattr(twin, f).tobytes() for f in ("bytes", "block_offsets", "totals"))
assert same
ndict, nblocks, nbytes = int(got.ndict), len(got.block_offsets) - 1, len(got.bytes)
N, nocc, npositions = len(postings.records), len(positions.occurrences), int(got.totals[3])
uncoded = 16 * N + 8 * nocc
out = {"ndocs": ndocs, "text_bytes": int(len(text)), "postings": N, "occurrences": nocc, "position_varints": npositions, "ndict": ndict,
       "block_entries": int(got.block_entries), "nblocks": nblocks, "nbytes": nbytes, "uncoded_bytes_16N_8nocc": uncoded,
       "bytes_per_posting": nbytes / max(N, 1), "bytes_per_position": nbytes / max(npositions, 1), "uncoded_over_coded": uncoded / max(nbytes, 1),
       "posting_blocks_ms_median": blocks_ms, "posting_blocks_ms_min": min(s[0] for s in samples), "posting_blocks_ms_max": max(s[0] for s in samples),
       "posting_blocks_ms_all": [s[0] for s in samples], "posting_blocks_call_host_ms_median": call_host_ms, "posting_blocks_done_host_ms_median": done_host_ms,
       "reps": REPS, "postings_ms": postings_ms, "positions_ms": positions_ms,
       "replaced_route_rounds": rounds, "replaced_route_fetches_ms": fetches_ms, "replaced_route_ms": route_ms,
       "device_faster_than_the_fetches_of_the_route": bool(done_host_ms < fetches_ms), "fetches_over_device": fetches_ms / done_host_ms,
       "route_over_device": route_ms / done_host_ms, "host_twin_ms": rounds[1]["host_twin_ms"],
       "posting_blocks_fetch_ms": rounds[1]["posting_blocks_fetch_ms"], "fetches_over_posting_blocks_fetch": fetches_ms / rounds[1]["posting_blocks_fetch_ms"],
       "identical_to_host": bool(same)}
print(json.dumps(out), flush=True)
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
