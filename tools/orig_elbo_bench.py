#!/usr/bin/env python
"""Device ms of one pass of the -orig lower bound (svils_orig_elbo) beside the sweep of the same state: assort-75-4 at K = 4
and LFR n = 1000 at K = 16, 28, 32, 48, 64.  One JSON line per workload.

Method: the state 5 sweeps in; hipEvent brackets of the library (svils_orig_get_elbo_timing: the pass, its
pair launches, its term launches; svils_orig_get_timing: tables, pair pass, reductions); the median of 20 after 3 warm-up
passes.  The sweep is timed from the same state every time (set_state before each), so both run the same fixed points.

  python tools/orig_elbo_bench.py --out profiles/r24a_orig_elbo_bench.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from orig_bench import lfr_path  # noqa: E402
from svinet_amd import _svils  # noqa: E402
from svinet_amd.host_api import OrigEngine  # noqa: E402


def measure(n, k, links, skip, gamma, beta, reps, warmup):
    dev = _svils.Orig(n, k, 1.0 / k)
    dev.set_graph(links, skip)
    dev.set_state(gamma, beta)
    dev.sweep(5)
    g, b = dev.state()
    el, sw = [], []
    for i in range(warmup + reps):
        parts = dev.elbo()
        if i >= warmup:
            el.append(dev.elbo_timing())
    pairs, rounds, most, _ = dev.elbo_stats()
    for i in range(warmup + reps):
        dev.set_state(g, b)
        dev.sweep(1)
        dev.state()
        if i >= warmup:
            sw.append(dev.timing())
    sweep_rounds = dev.stats()[1]
    dev.close()
    el, sw = np.median(np.array(el), axis=0), np.median(np.array(sw), axis=0)
    return {"elbo": list(parts), "pairs": pairs, "rounds": rounds, "rounds_max": most, "sweep_rounds": sweep_rounds,
            "elbo_pass_ms": float(el[0]), "elbo_pairs_ms": float(el[1]), "elbo_terms_ms": float(el[2]),
            "sweep_tables_ms": float(sw[0]), "sweep_pair_pass_ms": float(sw[1]), "sweep_reductions_ms": float(sw[2]),
            "sweep_ms": float(sw.sum()), "pass_over_sweep": float(el[0] / sw.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24a_orig_elbo_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    lfr = lfr_path()
    try:
        with open(a.out, "w") as out:
            for name, path, n, k in [("assort-75-4", os.path.join(ROOT, "tests", "golden", "graphs", "assort-75-4.txt"), 75, 4)] + \
                    [("lfr-n1000", lfr, 1000, k) for k in (16, 28, 32, 48, 64)]:
                host = OrigEngine(path, n, k, heldout_ratio=0.01, on_device=False)   # the engine's own start and held-out draw
                rec = {"record": "orig_elbo", "graph": name, "n": host.n, "k": k, "variant": list(_svils.orig_variant(k))}
                try:
                    rec.update(measure(host.n, k, host.edges, np.unique(host.heldout, axis=0), host.gamma, host.beta, a.reps, a.warmup))
                except _svils.SvilsError as exc:   # a start whose block rates leave (0, 1) within the five sweeps
                    rec["error"] = str(exc)
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
    finally:
        os.unlink(lfr)


if __name__ == "__main__":
    main()
