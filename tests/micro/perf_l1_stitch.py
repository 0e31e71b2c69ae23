# The segment stitch (csrc/l1_stitch.h) on the headline-shaped batch of bench.py's generator, every 64 KiB document cut into
# 16 segments of 4 KiB: the three passes by HIP events (lastStitchMs) beside the route a caller had to take without it --
# batchFetch of all lexems, the stitch on the host (tests/segments_model.py, numpy), upload of lexems, origseg and offsets --
# and beside the lexer's own time on the same batch.  The stitched batch is compared with the host's, word for word.
#   python tests/micro/perf_l1_stitch.py [documents of 64 KiB, default 12288] [out.json]
import json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
import struspattern_amd as spa
from struspattern_amd import synth
from tests import segments_model

HBM_PEAK_TBPS = 8.0         # MI355X, HBM3E
SEGS = 16
ndocs = int(sys.argv[1]) if len(sys.argv) > 1 else 12288
nseg = ndocs * SEGS
stream = torch.cuda.current_stream().cuda_stream

vocab = synth.vocabulary(30000, 1)
pats, _ = synth.pipeline_workload(10000, 10000, vocab, seed=4)
text, soffs = bench.text_corpus(nseg, 65536 // SEGS, vocab, seed=1000, utf8=True)
lxi = spa.PatternLexerInstance()
synth.apply_lexer_patterns(lxi, pats)
lctx = lxi.createContext()
d_text = torch.from_numpy(text).cuda()
d_soffs = torch.from_numpy(soffs.view(np.int64)).cuda()
for _ in range(8):
    lctx.matchDocsDevice(d_text.data_ptr(), d_soffs.data_ptr(), nseg, len(text), stream)
    lc = lctx.batchCounters()
    if lc["failed_docs"] == 0:
        break
    lctx.reserveOutput(int(lc["lexems"] * 1.2) + 1024)
    lctx.growArena()
assert lc["failed_docs"] == 0
lexer_ms = min(lctx.lastKernelMs(), *[(lctx.matchDocsDevice(d_text.data_ptr(), d_soffs.data_ptr(), nseg, len(text), stream), lctx.lastKernelMs())[1] for _ in range(2)])
nlex = int(lc["lexems"])

dso = np.arange(0, nseg + 1, SEGS, dtype=np.uint64)
d_dso = torch.from_numpy(dso.view(np.int64)).cuda()
lctx.stitchSegmentsDevice(d_dso.data_ptr(), ndocs, stream)      # (allocates)
stitch = []
for _ in range(5):
    lctx.stitchSegmentsDevice(d_dso.data_ptr(), ndocs, stream)
    stitch.append(lctx.lastStitchMs())
stitch_ms = min(stitch)

# the host route
t0 = time.perf_counter()
raw = lctx.batchFetch(0, nseg)
t1 = time.perf_counter()
hlex, hseg, hoffs, hstatus = segments_model.stitch(raw.lexems, raw.doc_offsets, raw.status, dso)
t2 = time.perf_counter()
up = [torch.from_numpy(hlex.view(np.int32)).cuda(), torch.from_numpy(hseg.view(np.int32)).cuda(), torch.from_numpy(hoffs.view(np.int64)).cuda()]
torch.cuda.synchronize()
t3 = time.perf_counter()
host = {"fetch_ms": (t1 - t0) * 1e3, "stitch_numpy_ms": (t2 - t1) * 1e3, "upload_ms": (t3 - t2) * 1e3, "total_ms": (t3 - t0) * 1e3}

lb, origseg = lctx.stitchedFetch()
assert not hstatus.any() and np.array_equal(lb.status, hstatus) and np.array_equal(lb.doc_offsets, hoffs)
assert np.array_equal(lb.lexems, hlex) and np.array_equal(origseg, hseg) and len(hlex) == nlex

moved = 36 * nlex           # per lexem: 16 B read, 16 + 4 B written
out = {"ndocs": ndocs, "segments": nseg, "text_bytes": int(len(text)), "lexems": nlex,
       "stitch_ms": stitch_ms, "stitch_ms_all": stitch, "bytes_moved": moved, "stitch_TBps": moved / stitch_ms / 1e9,
       "fraction_of_hbm_peak": moved / stitch_ms / 1e9 / HBM_PEAK_TBPS, "hbm_peak_TBps": HBM_PEAK_TBPS,
       "lexer_ms": lexer_ms, "stitch_over_lexer": stitch_ms / lexer_ms,
       "host_route": host, "host_over_device": host["total_ms"] / stitch_ms, "identical_to_host": True}
print(json.dumps(out), flush=True)
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
