"""Times the value passes (finishedValuesDevice) against the path they replace on the same batch -- finishedFetch + text
fetch + the host twin (batchValues) -- on a synthetic rule set with format strings: D documents, each N MoneyAmount-like
matches (sequence of a span and a formatted sub-pattern).  Prints one JSON line.

    python tests/micro/perf_result_values.py [D] [N] [ROUNDS]
"""
import json
import sys
import time

import numpy as np
import torch

import struspattern_amd as spa


def main():
    ndocs, per_doc, rounds = (int(x) for x in (sys.argv[1:4] + ["2000", "40", "5"][len(sys.argv) - 1:]))
    m = spa.PatternMatcherInstance()
    m.pushTerm(2); m.pushExpression("any", 1, 1, 0); m.definePattern("Currency", "EUR", True)
    m.pushTerm(1); m.attachVariable("value"); m.pushPattern("Currency"); m.attachVariable("currency")
    m.pushExpression("sequence_imm", 2, 2, 0); m.definePattern("MoneyAmount", "{currency} {value}", True)
    m.compile()
    lex, offs = [], [0]
    for d in range(ndocs):
        for k in range(per_doc):
            lex += [[1, 3 * k + 1, 10 * k, 5], [2, 3 * k + 2, 10 * k + 6, 3]]
        offs.append(len(lex))
    lex, offs = np.array(lex, np.uint32), np.array(offs, np.uint64)
    rng = np.random.default_rng(1)
    seglen = 10 * per_doc
    text = bytes(rng.integers(48, 58, ndocs * seglen, dtype=np.uint8))
    so = (np.arange(ndocs + 1, dtype=np.uint64) * seglen)
    d_text = torch.frombuffer(bytearray(text + b"\0" * 16), dtype=torch.uint8).cuda()
    d_so = torch.from_numpy(so.view(np.int64)).cuda()
    d_lex = torch.from_numpy(lex.view(np.int32).reshape(-1)).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    ctx = m.createContext()
    stream = torch.cuda.current_stream().cuda_stream
    ctx.reserveOutput(3 * ndocs * per_doc, 6 * ndocs * per_doc)
    dev_ms, host_ms = [], []
    for _ in range(rounds + 1):
        ctx.matchDocsDevice(d_lex.data_ptr(), d_offs.data_ptr(), ndocs, len(lex), stream)
        assert ctx.batchCounters()["failed_docs"] == 0
        ctx.batchFinishDevice(stream)
        ctx.finishedValuesDevice(d_text.data_ptr(), len(text), d_so.data_ptr(), ndocs, stream=stream)
        torch.cuda.synchronize()
        dev_ms.append(ctx.lastValuesMs())
        t0 = time.perf_counter()
        mb = ctx.finishedFetch()
        ctx.finishedTextDevice(d_text.data_ptr(), len(text), d_so.data_ptr(), ndocs, stream=stream)
        ctx.finishedTextFetch()
        twin = spa.batchValues(m, mb, text, so)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    got = ctx.finishedValuesFetch()
    assert got.result_values == twin.result_values and got.item_values == twin.item_values
    print(json.dumps({"ndocs": ndocs, "matches_per_doc": per_doc, "results": int(len(mb.results)), "items": int(len(mb.items)),
                      "value_bytes": [len(got.result_values), len(got.item_values)],
                      "last_values_ms_median": float(np.median(dev_ms[1:])), "last_values_ms_min": float(min(dev_ms[1:])),
                      "fetch_text_twin_ms_median": float(np.median(host_ms[1:])), "fetch_text_twin_ms_min": float(min(host_ms[1:]))}))


if __name__ == "__main__":
    main()
