"""Link prediction timings (svils_predict_links / svils_link_prob) against a numpy baseline.

  python tools/predict_bench.py [--mfma-tflops T] [--reps R] [--out file.jsonl] [--workloads 1,2,3]

Workloads (the flop count is 2 nq n K, the score GEMM alone):
  1  ca-AstroPh K=20, all nodes, top-10        (state after 20 sweeps)
  2  ca-AstroPh K=200, all nodes, top-10       (state after 20 sweeps)
  3  n = 1e6, K = 512 seeded random state, 8192 queries, top-100 (8.4e12 flop)
Each call is synchronous (the library synchronises its stream before returning): the time is the wall time of a warm call,
best and median of --reps.  --mfma-tflops (tools/ubench/f64mfma.hip) gives the share of the measured f64 MFMA rate.
The numpy baseline (fp64, the threads of its BLAS: OMP_NUM_THREADS) scores, masks and selects the same top-k; on workload 3
it runs 256 of the 8192 queries and is scaled by 32 (marked "extrapolated")."""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _astroph():
    src = os.path.join(ROOT, "tests", "golden", "graphs", "ca-AstroPh.csv.gz")
    tmp = tempfile.NamedTemporaryFile(delete=False, suffix=".csv")
    with gzip.open(src, "rb") as f:
        tmp.write(f.read())
    tmp.close()
    return tmp.name


def _numpy_topk(gamma, lam, nodes, topk, rowptr, col):
    P = gamma / gamma.sum(1, keepdims=True)
    beta = lam[:, 0] / (lam[:, 0] + lam[:, 1])
    out = np.empty((len(nodes), topk), dtype=np.int64)
    for b in range(0, len(nodes), 256):
        rows = nodes[b:b + 256]
        S = (P[rows] * beta) @ P.T
        for i, p in enumerate(rows):
            S[i, p] = -np.inf
            S[i, col[rowptr[p]:rowptr[p + 1]]] = -np.inf
        part = np.argpartition(-S, topk - 1, axis=1)[:, :topk]
        out[b:b + len(rows)] = np.take_along_axis(part, np.argsort(-np.take_along_axis(S, part, 1), 1), 1)
    return out


def _csr(n, links):
    a = np.concatenate([links[:, 0], links[:, 1]]).astype(np.int64)
    b = np.concatenate([links[:, 1], links[:, 0]]).astype(np.int64)
    o = np.argsort(a, kind="stable")
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, a + 1, 1)
    return np.cumsum(rowptr), b[o]


def _time(fn, reps):
    fn()   # warm: scratch, sorted rows
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts))


def run(which, reps, mfma_tflops):
    from svinet_amd import _svils
    from svinet_amd.host_api import Setup
    if which in (1, 2):
        k = 20 if which == 1 else 200
        path = _astroph()
        try:
            s = Setup(path, 17903, k)
        finally:
            os.unlink(path)
        eng = s.engine(use_validation_stop=False)
        eng.sweep(20)
        n, links, topk, nodes = s.n, s.links, 10, None
        gamma, lam, _ = eng.state()
        qn = np.arange(n)
        name = "ca-AstroPh K=%d all nodes top-%d" % (k, topk)
    else:
        n, k, topk, nq = 1000000, 512, 100, 8192
        rng = np.random.default_rng(12345)
        a, b = rng.integers(0, n, size=(2, 2 * n))
        e = np.stack([np.minimum(a, b), np.maximum(a, b)], 1)
        e = np.unique(e[e[:, 0] != e[:, 1]], axis=0)
        links = np.ascontiguousarray(e, dtype=np.uint32)
        eng = _svils.Engine(n, k, ones=len(links), ones_prob=len(links) / (n * (n - 1) / 2), use_validation_stop=False)
        eng.set_graph(links)
        gamma = rng.random((n, k)) + 0.01
        lam = rng.random((k, 2)) + 0.1
        eng.set_state(gamma, lam)
        nodes = rng.choice(n, size=nq, replace=False).astype(np.uint32)
        qn = nodes.astype(np.int64)
        name = "n=1e6 K=512 random state, 8192 queries top-100"
    nq = len(qn)
    flop = 2.0 * nq * n * k
    best, med = _time(lambda: eng.predict_links(topk, nodes), reps)
    pairs = np.stack([qn[:4096], (qn[:4096] + 1) % n], 1)
    pbest, _ = _time(lambda: eng.link_prob(pairs), reps)
    rec = {"workload": which, "name": name, "n": n, "K": k, "queries": nq, "topk": topk, "flop": flop,
           "predict_best_ms": best * 1e3, "predict_median_ms": med * 1e3, "tflops": flop / best / 1e12,
           "link_prob_4096_pairs_ms": pbest * 1e3}
    if mfma_tflops:
        rec["share_of_f64_mfma"] = rec["tflops"] / mfma_tflops
    rowptr, col = _csr(n, links)
    sub = qn if which in (1, 2) else qn[:256]
    t0 = time.perf_counter()
    ref = _numpy_topk(gamma, lam, sub, topk, rowptr, col)
    tn = (time.perf_counter() - t0) * (nq / len(sub))
    rec["numpy_ms"] = tn * 1e3
    rec["numpy_threads"] = os.environ.get("OMP_NUM_THREADS", "default")
    rec["numpy_extrapolated"] = len(sub) != nq
    rec["speedup_vs_numpy"] = tn / best
    _, sc = eng.predict_links(topk, nodes)
    P = gamma / gamma.sum(1, keepdims=True)
    beta = lam[:, 0] / (lam[:, 0] + lam[:, 1])
    want = np.sum(P[sub] * beta * P[ref[:, 0]], axis=1)   # numpy's best score (ties make the ids differ, not the scores)
    rec["top1_score_max_rel_diff"] = float(np.max(np.abs(sc[:len(sub), 0] - want) / want))
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mfma-tflops", type=float, default=0.0)
    ap.add_argument("--workloads", default="1,2,3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for w in [int(x) for x in a.workloads.split(",")]:
        rec = run(w, a.reps, a.mfma_tflops)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
