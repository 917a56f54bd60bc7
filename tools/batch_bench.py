"""-batch-gpu sweep by sweep: the hipEvent times of svils_batch_get_timing (Elogpi / Elogbeta, the pair pass, the
reductions), the kernel's own pair and round counts, and the host engine's seconds per sweep (svih_batch_sweep, one thread)
on the same box as the baseline.  Median of --sweeps sweeps after --warmup, from a state 5 sweeps in.  One JSON line per
workload.

    python tools/batch_bench.py                       # assort (n = 75, k = 4), LFR (n = 1000, k = 28), planted n = 8192 k = 32
    python tools/batch_bench.py --only lfr --host-sweeps 2
"""
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
GRAPHS = os.path.join(ROOT, "tests", "golden", "graphs")


def planted(n, blocks, deg_in, deg_out, seed):
    """links [m][2] p < q of a planted partition with about deg_in / deg_out links per node inside / across blocks, plus a ring"""
    rs = np.random.RandomState(seed)
    size = n // blocks
    p = rs.randint(0, n, n * deg_in // 2)
    q = (p // size) * size + rs.randint(0, size, p.shape[0])
    p2, q2 = rs.randint(0, n, n * deg_out // 2), rs.randint(0, n, n * deg_out // 2)
    a = np.concatenate([p, p2, np.arange(n - 1)])
    b = np.concatenate([np.minimum(q, n - 1), q2, np.arange(1, n)])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = np.unique(lo[lo < hi].astype(np.uint64) * n + hi[lo < hi].astype(np.uint64))
    return np.ascontiguousarray(np.stack([key // n, key % n], axis=1).astype(np.uint32))


def device_run(n, k, eta, links, skip, gamma, lam, sweeps, warmup):
    from svinet_amd import _svils
    d = _svils.Batch(n, k, 1.0 / k, eta)
    d.set_graph(links, skip)
    d.set_state(gamma, lam)
    d.sweep(5)
    ms, stats = [], None
    for i in range(warmup + sweeps):
        d.sweep()
        t = d.timing()
        if i >= warmup:
            ms.append(t)
            stats = d.stats()
    ms = np.array(ms)
    med = np.median(ms, axis=0)
    total = float(np.median(ms.sum(1)))
    pairs, rounds_total, rounds_max, under = stats
    w, v = _svils.batch_variant(k)
    d.close()
    return {"variant": [w, v], "dir_exp_ms": float(med[0]), "pairs_ms": float(med[1]), "reduce_ms": float(med[2]), "sweep_ms": total,
            "pairs": int(pairs), "rounds_total": int(rounds_total), "rounds_mean": rounds_total / pairs, "rounds_max": int(rounds_max),
            "underflow": int(under), "pairs_per_s": pairs / (total * 1e-3), "exp_per_s": rounds_total * 2 * k / (total * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=["assort", "lfr", "planted"])
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-sweeps", type=int, default=1, help="host engine sweeps timed as the baseline (0: none)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    from svinet_amd.host_api import BatchEngine
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        lfr = os.path.join(tmp, "lfr.txt")
        with gzip.open(os.path.join(GRAPHS, "LFR-network-n1000-k28.txt.gz"), "rb") as f, open(lfr, "wb") as g:
            g.write(f.read())
        for name, path, n, k in (("assort", os.path.join(GRAPHS, "assort-75-4.txt"), 75, 4), ("lfr", lfr, 1000, 28)):
            if a.only and a.only != name:
                continue
            e = BatchEngine(path, n, k, heldout_ratio=0.1)
            skip = sorted({tuple(int(x) for x in r) for r in e.heldout} | {tuple(int(x) for x in r) for r in e.validation})
            out = {"workload": name, "n": e.n, "k": k}
            out.update(device_run(e.n, k, e.eta, e.edges, skip, e.gamma, e.lam, a.sweeps, a.warmup))
            if a.host_sweeps:
                for _ in range(5 if name == "assort" else 0):   # the same "5 sweeps in" where that is cheap
                    e.sweep()
                t = time.perf_counter()
                for _ in range(a.host_sweeps):
                    e.sweep()
                out["host_sweep_s"] = (time.perf_counter() - t) / a.host_sweeps
                out["speedup_vs_host"] = out["host_sweep_s"] / (out["sweep_ms"] * 1e-3)
            e.close()
            lines.append(out)
        if not a.only or a.only == "planted":
            n, k = 8192, 32
            links = planted(n, 32, 24, 4, seed=8192)
            gamma = np.random.RandomState(1).gamma(100.0, 0.01, (n, k))
            out = {"workload": "planted", "n": n, "k": k, "links": int(len(links))}
            out.update(device_run(n, k, (1.0, 1.0), links, links[::50], gamma, np.tile([1.0, 1.0], (k, 1)), a.sweeps, a.warmup))
            lines.append(out)
    for out in lines:
        line = json.dumps(out)
        print(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
