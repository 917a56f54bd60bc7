"""-infset step by step, with tools/sampled_bench.py's method: device milliseconds per star step from the hipEvent bracket of
svils_batch_get_timing over a chunk of --chunk queued steps (median of --repeats chunks after one warm-up chunk) -- once
as the call runs them (chains of up to 64 steps per launch) and once with the chain length forced to 1, the same lists as
one launch per step, which isolates what the single launch buys -- the kernel's own pair and round counts, and the host
loops' seconds per step (InfsetEngine.step, one thread) on the same box.  The stars are the host engine's own draw.  One
JSON line per workload.

    python tools/infset_bench.py                          # LFR (n = 1000, k = 28) and ca-AstroPh (n = 17903, k = 20)
    python tools/infset_bench.py --only lfr --long-run 200000   # one -infset run to the stop rule or that many iterations
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


def device_run(e, k, start, sched, chunk, repeats, chain):
    """the schedule from `start` = (gamma, lambda) in chunks -> median ms per step, the last chunk's counters"""
    from svinet_amd import _svils
    skip = {tuple(int(x) for x in r) for r in e.heldout} | {tuple(int(x) for x in r) for r in e.validation}
    d = _svils.Batch(e.n, k, 1.0 / k, e.eta)
    d.set_graph(e.edges, sorted(skip))
    d.set_state(*start)
    d.set_star_chain(chain)
    ms, stats = [], None
    for r in range(repeats + 1):
        d.step_star(sched[r * chunk:(r + 1) * chunk])
        t = d.timing()[0]
        if r:
            ms.append(t)
            stats = d.stats()
    g, lam = d.state()
    d.close()
    return float(np.median(ms)) / chunk, stats, g, lam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=["lfr", "astroph"])
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--long-run", type=int, default=0, help="LFR only: an -infset run on the device of at most this many iterations")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    from svinet_amd import host_api
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
            nb = os.path.join(tmp, name + "-neighbors.bin")
            t = time.perf_counter()
            host_api.preprocess(files[name], n, nb)
            out = {"workload": name, "mode": "infset", "n": n, "k": k, "preprocess_s": time.perf_counter() - t}
            e = host_api.InfsetEngine(files[name], n, k, nb, heldout_ratio=0.01)
            start = (e.gamma, e.lam)
            nsteps = a.chunk * (a.repeats + 1)
            t = time.perf_counter()
            e.step(nsteps)
            out["host_step_s"] = (time.perf_counter() - t) / nsteps
            sched = e.schedule
            chained, stats, g, lam = device_run(e, k, start, sched, a.chunk, a.repeats, 0)
            single, stats1, g1, lam1 = device_run(e, k, start, sched, a.chunk, a.repeats, 1)
            assert g.tobytes() == g1.tobytes() and lam.tobytes() == lam1.tobytes() and stats == stats1
            pairs, rounds_total, rounds_max, under = stats
            out.update({"chunk": a.chunk, "step_ms_chained": chained, "step_ms_chain_length_1": single,
                        "single_launch_gain": single / chained, "entries_per_step": pairs / a.chunk,
                        "rounds_mean": rounds_total / max(pairs, 1), "rounds_max": int(rounds_max), "underflow": int(under),
                        "speedup_vs_host": out["host_step_s"] / (chained * 1e-3),
                        "max_rel_diff_vs_host_gamma": float(np.max(np.abs(g - e.gamma) / e.gamma)), "gamma_min": float(g.min())})
            e.close()
            lines.append(out)
        if a.long_run and a.only != "astroph":
            nb = os.path.join(tmp, "lfr-neighbors.bin")
            if not os.path.exists(nb):
                host_api.preprocess(files["lfr"], 1000, nb)
            e = host_api.InfsetEngine(files["lfr"], 1000, 28, nb, heldout_ratio=0.01, on_device=True)
            t, stopped = time.perf_counter(), False
            while e.iter < a.long_run and not stopped:
                e.step(100)
                stopped = e.report()
            lines.append({"workload": "lfr", "mode": "infset", "long_run": True, "iterations": int(e.iter), "stop_rule": bool(stopped),
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
