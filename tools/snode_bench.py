"""-snode step by step, with tools/sampled_bench.py's method: device milliseconds per step from the hipEvent bracket of
svils_batch_get_timing over a chunk of --chunk queued steps (median of --repeats chunks after one warm-up chunk) -- for the
engine's own draw as it comes (both kinds mixed), for its link steps alone and for its non-link steps alone -- with the
kernel's own pair and round counts, the launches per step, and the host loops' seconds per step (StratNodeEngine.step, one
thread, all n rows moved per iteration) on the same box.  One JSON line per workload.

    python tools/snode_bench.py                          # LFR (n = 1000, k = 28) and ca-AstroPh (n = 17903, k = 20)
    python tools/snode_bench.py --only lfr --long-run 200000   # one -snode run to the stop rule or that many iterations
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


def device_run(e, k, start, steps, chunk, repeats):
    """`steps` from `start` = (gamma, lambda) in chunks -> median ms per step, the measured chunks' counters, launches per step"""
    from svinet_amd import _svils
    skip = {tuple(int(x) for x in r) for r in e.heldout} | {tuple(int(x) for x in r) for r in e.validation}
    d = _svils.Batch(e.n, k, 1.0 / k, e.eta)
    d.set_graph(e.edges, sorted(skip))
    d.set_state(*start)
    ms, pairs, rounds, rmax = [], 0, 0, 0
    for r in range(repeats + 1):
        d.step_strat(steps[r * chunk:(r + 1) * chunk])
        t = d.timing()[0]
        if r:
            ms.append(t)
            st = d.stats()
            assert st[3] == 0
            pairs, rounds, rmax = pairs + st[0], rounds + st[1], max(rmax, st[2])
    lag = d.lag()
    g, lam = d.state()
    d.close()
    measured = steps[chunk:(repeats + 1) * chunk]
    launches = sum(2 if len(s["partner"]) else 1 for s in measured) / len(measured)   # pair pass (a step with entries), tail
    return {"step_us": 1e3 * float(np.median(ms)) / chunk, "entries_per_step": pairs / len(measured), "rounds_mean": rounds / max(pairs, 1),
            "rounds_max": int(rmax), "launches_per_step": launches, "rows_behind_at_the_end": int(lag)}, g, lam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=["lfr", "astroph"])
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=20, help="host-loop steps timed as the baseline")
    ap.add_argument("--long-run", type=int, default=0, help="LFR only: a -snode run on the device of at most this many iterations")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    from svinet_amd import _svils, host_api
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
            need = a.chunk * (a.repeats + 1)
            out = {"workload": name, "mode": "snode", "n": n, "k": k, "variant": list(_svils.batch_variant(k)), "chunk": a.chunk}
            e = host_api.StratNodeEngine(files[name], n, k, heldout_ratio=0.01)
            start = (e.gamma, e.lam)
            t = time.perf_counter()
            e.step(a.host_steps)
            out["host_step_s"] = (time.perf_counter() - t) / a.host_steps
            e.close()
            # the draw never depends on the state: each kind's steps come from an engine whose chance forces that kind, the
            # mixed ones from the default chance of 1/2; the host loops run along (there is no draw without them)
            for label, eps in (("mixed", 0.5), ("link", 0.0), ("nonlink", 1.0)):
                e = host_api.StratNodeEngine(files[name], n, k, heldout_ratio=0.01, inf_epsilon=eps)
                e.step(need)
                res, g, lam = device_run(e, k, start, e.schedule(), a.chunk, a.repeats)
                res["max_rel_diff_vs_host_gamma"] = float(np.max(np.abs(g - e.gamma) / e.gamma))
                out[label] = res
                e.close()
            out["speedup_vs_host"] = out["host_step_s"] / (out["mixed"]["step_us"] * 1e-6)
            lines.append(out)
        if a.long_run and a.only != "astroph":
            e = host_api.StratNodeEngine(files["lfr"], 1000, 28, heldout_ratio=0.01, on_device=True)
            t, stopped = time.perf_counter(), False
            while e.iter < a.long_run and not stopped:
                e.sweep()
                stopped = e.report()
            lines.append({"workload": "lfr", "mode": "snode", "long_run": True, "iterations": int(e.iter), "stop_rule": bool(stopped),
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
