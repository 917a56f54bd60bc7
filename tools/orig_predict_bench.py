#!/usr/bin/env python
"""Device time of the link queries of -orig: svils_orig_predict_links for all nodes (top-10) and svils_orig_rank_links for
8192 directed pairs at the planted n = 8192, K = 32 graph of tools/batch_bench.py, from the handle's hipEvent bracket
(svils_orig_get_query_timing).  One JSON line.

flop counts the score GEMM alone, 2 * rows * n * K (the tiles compute 16 ceil(K / 16) columns: the same at K = 32); the
yardstick is the 49.5 TFLOP/s the project measured for its f64 MFMA tiles.

  python tools/orig_predict_bench.py [--out profiles/r19a_orig_predict.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from batch_bench import planted  # noqa: E402

MFMA_TFLOPS = 49.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--topk", type=int, default=10)
    a = ap.parse_args()
    from svinet_amd import _svils
    n, k = 8192, 32
    links = planted(n, 32, 24, 4, seed=8192)
    gamma = np.random.RandomState(1).gamma(100.0, 0.01, (n, k))
    beta = np.clip(np.random.RandomState(2).randint(0, 100, size=(k, k)) / 100.0, 0.01, 0.99)
    held = links[::50]
    d = _svils.Orig(n, k, 1.0 / k)
    d.set_graph(links, np.concatenate([held, held[:, ::-1]]))
    d.set_state(gamma, beta)
    pairs = np.random.RandomState(3).randint(0, n, size=(8192, 2)).astype(np.uint32)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    out = {"workload": "planted", "n": n, "k": k, "links": int(len(links)), "topk": a.topk}
    for name, call, rows in (("predict_links", lambda: d.predict_links(a.topk), n), ("rank_links", lambda: d.rank_links(pairs), len(pairs))):
        ms = []
        for i in range(a.warmup + a.calls):
            call()
            if i >= a.warmup:
                ms.append(d.query_timing())
        flop = 2.0 * rows * n * k
        best = min(ms)
        out[name] = {"rows": int(rows), "ms": [round(x, 4) for x in ms], "best_ms": best, "median_ms": float(np.median(ms)), "flop": flop,
                     "tflops": flop / (best * 1e-3) / 1e12, "share_of_mfma_rate": flop / (best * 1e-3) / 1e12 / MFMA_TFLOPS}
    d.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
