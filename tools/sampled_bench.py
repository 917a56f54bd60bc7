"""-rnode / -rpair step by step: device milliseconds per step from the hipEvent bracket of svils_batch_get_timing over a chunk
of --chunk queued steps (median of --repeats chunks after one warm-up chunk), the kernels' own pair and round counts, the
number of launches per step, and the host loops' seconds per step (SampledEngine.step, one thread) on the same box.  The
mini-batches are drawn here with numpy (the start is the host engine's; the draw is not the reference's stream).  One JSON
line per workload and mode.

    python tools/sampled_bench.py                          # LFR (n = 1000, k = 28) and ca-AstroPh (n = 17903, k = 20)
    python tools/sampled_bench.py --only lfr --host-steps 20
    python tools/sampled_bench.py --only lfr --long-run 20000    # one -rnode run to the stop rule or that many iterations
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
LAUNCHES = {"rnode": 3, "rpair": 3}   # pair pass, (row pass,) tail, (Elogpi of the start node); rpair: 2 while lambda waits


def draw_pairs(rs, n, m, skip_keys):
    """m pairs p < q outside the skip set (skip_keys: p n + q), with replacement"""
    out = np.zeros((0, 2), dtype=np.int64)
    while len(out) < m:
        pq = np.sort(rs.randint(0, n, (2 * m, 2)), axis=1).astype(np.int64)
        keep = (pq[:, 0] != pq[:, 1]) & ~np.isin(pq[:, 0] * n + pq[:, 1], skip_keys)
        out = np.concatenate([out, pq[keep]])
    return np.ascontiguousarray(out[:m], dtype=np.uint32)


def device_run(e, k, mode, chunk, repeats, seed=0):
    from svinet_amd import _svils
    n = e.n
    skip = {tuple(int(x) for x in r) for r in e.heldout} | {tuple(int(x) for x in r) for r in e.validation}
    d = _svils.Batch(n, k, 1.0 / k, e.eta)
    d.set_graph(e.edges, sorted(skip))
    d.set_state(e.gamma, e.lam)
    rs = np.random.RandomState(seed)
    skip_keys = np.array(sorted(a * n + b for a, b in skip), dtype=np.int64)
    ms, stats, c = [], None, 0
    for r in range(repeats + 1):
        rg = [(1025 + (c + i) / 100.0) ** -0.5 for i in range(chunk)]
        rl = [(1026.0 + c + i) ** -0.9 for i in range(chunk)]
        if mode == "rnode":
            d.step_node(rs.randint(0, n, chunk), n / 2.0, rg, rl)
        else:
            m = n // 2
            d.step_pairs([draw_pairs(rs, n, m, skip_keys) for _ in range(chunk)], [n * (n - 1) / 2.0 / m] * chunk, rg, rl)
        c += chunk
        t = d.timing()[0]
        if r:
            ms.append(t)
            stats = d.stats()
    pairs, rounds_total, rounds_max, under = stats
    g, _ = d.state()
    d.close()
    step_ms = float(np.median(ms)) / chunk
    return {"variant": list(_svils.batch_variant(k)), "chunk": chunk, "step_ms": step_ms, "launches_per_step": LAUNCHES[mode],
            "pairs_per_step": pairs / chunk, "rounds_mean": rounds_total / max(pairs, 1), "rounds_max": int(rounds_max),
            "underflow": int(under), "step_ns_per_pair_round": step_ms * 1e6 * chunk / max(rounds_total, 1),
            "gamma_min": float(g.min())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=["lfr", "astroph"])
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=5, help="host-loop steps timed as the baseline (0: none)")
    ap.add_argument("--long-run", type=int, default=0, help="LFR only: an -rnode run on the device of at most this many iterations")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    from svinet_amd.host_api import SampledEngine
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        files = {}
        for name, gz in (("lfr", "LFR-network-n1000-k28.txt.gz"), ("astroph", "ca-AstroPh.csv.gz")):
            files[name] = os.path.join(tmp, gz[:-3])
            with gzip.open(os.path.join(GRAPHS, gz), "rb") as f, open(files[name], "wb") as g:
                g.write(f.read())
        for name, n, k in (("lfr", 1000, 28), ("astroph", 17903, 20)):
            if a.only and a.only != name:
                continue
            for mode in ("rnode", "rpair"):
                e = SampledEngine(files[name], n, k, mode, heldout_ratio=0.01)
                out = {"workload": name, "mode": mode, "n": e.n, "k": k}
                out.update(device_run(e, k, mode, a.chunk, a.repeats))
                if a.host_steps:
                    t = time.perf_counter()
                    e.step(a.host_steps)
                    out["host_step_s"] = (time.perf_counter() - t) / a.host_steps
                    out["speedup_vs_host"] = out["host_step_s"] / (out["step_ms"] * 1e-3)
                e.close()
                lines.append(out)
        if a.long_run and a.only != "astroph":
            e = SampledEngine(files["lfr"], 1000, 28, "rnode", heldout_ratio=0.01, on_device=True)
            t, stopped = time.perf_counter(), False
            while e.iter < a.long_run and not stopped:
                e.step(100)
                stopped = e.report()
            lines.append({"workload": "lfr", "mode": "rnode", "long_run": True, "iterations": int(e.iter), "stop_rule": bool(stopped),
                          "seconds": time.perf_counter() - t, "heldout_ll_at_sparsity": float(e.rows[-1, 9]),
                          "heldout_ll_at_sparsity_start": float(e.rows[0, 9])})
            e.close()
    for out in lines:
        line = json.dumps(out)
        print(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
