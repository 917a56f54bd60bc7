"""-logl on the device: the hipEvent time of a svils_batch_elbo pass beside the same handle's sweep -- its total and its
pair pass (svils_batch_get_timing) -- the pass's own pair and round counts, and the host loops' seconds per pass
(MMSBBatch::elbo, one thread) where that is affordable.  Median of --passes passes after --warmup, from a state 5 sweeps
in.  The yardstick is the ratio ELBO pass / sweep pair pass: the pass runs the same fixed point, adds 2 K logs and about
6 K multiply-adds per pair and stores almost nothing, so more than 1 + 1 / (mean rounds) is more than one extra round's
worth.  One JSON line per workload.

    python tools/elbo_bench.py                       # assort (n = 75, k = 4), LFR (n = 1000, k = 28), planted n = 8192 k = 32
    python tools/elbo_bench.py --only lfr --host-passes 0
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
GRAPHS = os.path.join(ROOT, "tests", "golden", "graphs")

from batch_bench import planted   # noqa: E402  (the same planted workload)


def device_run(n, k, eta, links, skip, gamma, lam, passes, warmup):
    from svinet_amd import _svils
    d = _svils.Batch(n, k, 1.0 / k, eta)
    d.set_graph(links, skip)
    d.set_state(gamma, lam)
    d.sweep(5)
    elbo_ms = []
    for i in range(warmup + passes):   # every pass reads the state 5 sweeps in
        parts, pairs, rounds_total = d.elbo()
        if i >= warmup:
            elbo_ms.append(d.timing()[0])
    # the next sweep runs the very fixed points the passes ran (the same state): its pair pass is the yardstick; the median
    # of the sweeps after it, whose states move on, stands beside it
    sweep_ms = []
    for i in range(passes):
        d.sweep()
        sweep_ms.append(d.timing())
        if i == 0:
            sweep_pairs, sweep_rounds = d.stats()[:2]
    sweep_ms = np.array(sweep_ms)
    w, v = _svils.batch_variant(k)
    d.close()
    pair_pass = float(sweep_ms[0, 1])
    elbo = float(np.median(elbo_ms))
    mean_rounds = rounds_total / pairs
    assert (sweep_pairs, sweep_rounds) == (pairs, rounds_total)   # the same pairs, the same rounds
    return {"variant": [w, v], "elbo_ms": elbo, "elbo_ms_min": float(np.min(elbo_ms)), "sweep_ms": float(sweep_ms[0].sum()),
            "sweep_pairs_ms": pair_pass, "sweep_ms_median_later": float(np.median(sweep_ms.sum(1))),
            "sweep_pairs_ms_median_later": float(np.median(sweep_ms[:, 1])),
            "elbo_over_pair_pass": elbo / pair_pass, "one_extra_round": 1.0 + 1.0 / mean_rounds,
            "pairs": int(pairs), "rounds_mean": mean_rounds,
            "elbo": float(parts[0]), "G": float(parts[1]), "P": float(parts[2]), "N": float(parts[3])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=["assort", "lfr", "planted"])
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-passes", type=int, default=1, help="host-loop passes timed as the baseline (0: none)")
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
            out.update(device_run(e.n, k, e.eta, e.edges, skip, e.gamma, e.lam, a.passes, a.warmup))
            if a.host_passes:
                for _ in range(5):   # the same "5 sweeps in"
                    e.sweep()
                t = time.perf_counter()
                for _ in range(a.host_passes):
                    e.elbo()
                out["host_elbo_s"] = (time.perf_counter() - t) / a.host_passes
                out["speedup_vs_host"] = out["host_elbo_s"] / (out["elbo_ms"] * 1e-3)
            e.close()
            lines.append(out)
        if not a.only or a.only == "planted":
            n, k = 8192, 32
            links = planted(n, 32, 24, 4, seed=8192)
            gamma = np.random.RandomState(1).gamma(100.0, 0.01, (n, k))
            out = {"workload": "planted", "n": n, "k": k, "links": int(len(links))}
            out.update(device_run(n, k, (1.0, 1.0), links, links[::50], gamma, np.tile([1.0, 1.0], (k, 1)), a.passes, a.warmup))
            lines.append(out)
    for out in lines:
        line = json.dumps(out)
        print(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
