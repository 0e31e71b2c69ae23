# The dictionary of the terms of a finished batch on the device (csrc/l2_dict.h) on the workload of tests/micro/perf_terms.py:
# the pipeline rule set (10 000 regexes + 10 000 rules), documents of 64 KiB, text values.  A dictionary call by HIP events
# (lastDictionaryMs: the five launches; the host's wait for the number of entries between offsets and place lies inside, the
# memsets that clear the table and handle_terms are enqueued before the first event and lie outside) beside the route it
# replaces: finishedTermsFetch() + finishedTextFetch() + finishedFetch(), then the de-duplication on the host
# (sp_match_batch_dictionary, the C++ twin).  THE BAR: the device call takes less time than the three fetches alone; the
# host's grouping comes on top.  The device's bytes are compared with the host's.
#   python tests/micro/perf_dictionary.py [documents of 64 KiB, default 256] [out.json]
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
bound = mi.handleBound()
mctx = mi.createContext()
mc = sized(mctx, lambda: mctx.matchLexedDevice(lo[-1].d_lexems, lo[-1].d_doc_ranges, ndocs, int(lc["lexems"]), stream), ndocs,
           lambda c: mctx.reserveOutput(int(c["results"] * 1.2) + 1024, int(c["items"] * 1.2) + 1024))
mctx.batchFinishDevice(stream)
finish_ms = sum(mctx.lastFinishMs())
mctx.finishedTextDevice(d_text.data_ptr(), len(text), d_offs.data_ptr(), ndocs, results=True, items=False, stream=stream)
text_ms = mctx.lastTextMs()
mctx.finishedTermsDevice(spa.SP_TERM_TEXT, stream)
terms_ms = mctx.lastTermsMs()


def dictionary():
    mctx.finishedDictionaryDevice(stream)
    return mctx.lastDictionaryMs()


dictionary(), dictionary()
samples = [dictionary() for _ in range(REPS)]
dict_ms = statistics.median(samples)

# the route without the call: the terms, the text of the results and the batch to the host (twice: the first call pays for the
# host allocations and page faults, the second is the figure), the de-duplication there
fetches = []
for _ in range(2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    terms = mctx.finishedTermsFetch()
    t1 = time.perf_counter()
    mt = mctx.finishedTextFetch()
    t2 = time.perf_counter()
    mb = mctx.finishedFetch()
    t3 = time.perf_counter()
    fetches.append({"terms_fetch_ms": (t1 - t0) * 1e3, "text_fetch_ms": (t2 - t1) * 1e3, "finished_fetch_ms": (t3 - t2) * 1e3, "all_ms": (t3 - t0) * 1e3})
fetch_ms = min(f["all_ms"] for f in fetches)
t0 = time.perf_counter()
twin = spa.batchDictionary(mb, terms, text=mt)
host_group_ms = (time.perf_counter() - t0) * 1e3

got = mctx.finishedDictionaryFetch()
same = all(np.array_equal(getattr(got, f), getattr(twin, f)) for f in ("records", "counts", "term_dict", "doc_offsets", "handle_terms"))
assert same and not terms.status.any()

nres, nrec, ndict = len(mb.results), len(terms.records), len(got.records)
text_bytes = len(mt.result_text)
slots = min(2 * nrec, 0xFFFFFFFF)
out = {"ndocs": ndocs, "text_bytes": int(len(text)), "results": nres, "handle_bound": bound, "terms": nrec, "ndict": ndict,
       "terms_per_entry": nrec / max(1, ndict), "max_doc_freq": int(got.records[:, 4].max()) if ndict else 0,
       "dictionary_ms_median": dict_ms, "dictionary_ms_all": samples, "reps": REPS,
       "fetches": fetches, "three_fetches_ms": fetch_ms, "host_grouping_ms": host_group_ms,
       "device_faster_than_the_three_fetches": bool(dict_ms < fetch_ms), "fetches_over_device": fetch_ms / dict_ms,
       "bytes_moved_by_the_fetches": 24 * nrec + 4 * nres + 12 * ndocs + 8 + 8 * (nres + 1) + text_bytes + 36 * nres + 8 * (ndocs + 1) + 36 * ndocs,
       "bytes_of_a_dictionary_fetch": 32 * ndict + 4 * nrec + 8 * (ndocs + 1) + 4 * bound + 8,
       "working_memory_bytes": 4 * (slots + 2 * nrec) + 4 * (ndocs + 1),
       "terms_ms": terms_ms, "finish_ms": finish_ms, "text_ms": text_ms, "rule_stage_ms": mctx.lastKernelMs(),
       "identical_to_host": bool(same)}
print(json.dumps(out), flush=True)
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
