#!/usr/bin/env python
"""ms per sweep of the -orig engine (the full K x K blockmodel): the device against -host-loops on assort-75-4 at K = 4 and
on LFR n = 1000 at K = 28, and a K scan 4 .. 64 of the device on the LFR graph.  One JSON line per record.

The pair pass's f64 rate counts 2 K^2 FMAs per side per round (the L0 and the L1 product of a tile that holds links and
non-links) from the exact round total of the sweep: flop = rounds * 2 sides * 2 K^2 FMAs * 2; `useful_tflops` counts the K^2
FMAs per side a pair needs.  The yardstick is the 49.5 TFLOP/s the project measured for its f64 MFMA tiles.

  python tools/orig_bench.py --out profiles/r18a_orig_bench.jsonl
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
from svinet_amd import _svils  # noqa: E402
from svinet_amd.host_api import OrigEngine  # noqa: E402

MFMA_TFLOPS = 49.5


def lfr_path():
    src = os.path.join(ROOT, "tests", "golden", "graphs", "LFR-network-n1000-k28.txt.gz")
    tmp = tempfile.NamedTemporaryFile(delete=False, suffix=".txt")
    with gzip.open(src, "rb") as f:
        tmp.write(f.read())
    tmp.close()
    return tmp.name


def device_sweeps(n, k, links, skip, gamma, beta, sweeps, warmup):
    """median device ms of a sweep's three phases and its wall ms, and the counters of one sweep"""
    dev = _svils.Orig(n, k, 1.0 / k)
    dev.set_graph(links, skip)
    dev.set_state(gamma, beta)
    ms, wall = [], []
    for i in range(warmup + sweeps):
        t0 = time.perf_counter()
        dev.sweep(1)
        dev.state()
        t1 = time.perf_counter()
        if i >= warmup:
            ms.append(dev.timing())
            wall.append(1e3 * (t1 - t0))
    pairs, rounds, most, bad_norm, bad_beta = dev.stats()
    dev.close()
    ms = np.median(np.array(ms), axis=0)
    rec = {"tables_ms": float(ms[0]), "pair_pass_ms": float(ms[1]), "reductions_ms": float(ms[2]), "wall_ms": float(np.median(wall)),
           "pairs": pairs, "rounds_last_sweep": rounds, "rounds_max": most}
    rec["mfma_tflops"] = rounds * 2 * 2 * k * k * 2 / (ms[1] * 1e-3) / 1e12
    rec["useful_tflops"] = rec["mfma_tflops"] / 2
    rec["fraction_of_mfma_peak"] = rec["mfma_tflops"] / MFMA_TFLOPS
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18a_orig_bench.jsonl"))
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-host", action="store_true", help="leave the -host-loops runs out")
    a = ap.parse_args()
    lfr = lfr_path()
    out = open(a.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    try:
        for name, path, n, k in (("assort-75-4", os.path.join(ROOT, "tests", "golden", "graphs", "assort-75-4.txt"), 75, 4),
                                 ("lfr-n1000", lfr, 1000, 28)):
            host = OrigEngine(path, n, k, heldout_ratio=0.01, on_device=False)
            gamma, beta, skip = host.gamma, host.beta, np.unique(host.heldout, axis=0)   # a pair may be drawn twice
            rec = {"record": "engine", "graph": name, "n": host.n, "k": k}
            rec.update(device_sweeps(host.n, k, host.edges, skip, gamma, beta, a.sweeps, a.warmup))
            if not a.no_host:
                times = []
                for i in range(a.warmup + a.sweeps):   # the same sweeps as the device ran: the rounds fall as the fit settles
                    t0 = time.perf_counter()
                    host.sweep()
                    if i >= a.warmup:
                        times.append(1e3 * (time.perf_counter() - t0))
                rec["host_loops_ms"] = float(np.median(times))
                rec["host_rounds_last_sweep"] = host.rounds_total
                rec["speedup_wall"] = rec["host_loops_ms"] / rec["wall_ms"]
            emit(rec)
        host = OrigEngine(lfr, 1000, 4, heldout_ratio=0.01, on_device=False)
        rs = np.random.RandomState(18)
        for k in (4, 8, 16, 17, 28, 32, 33, 48, 49, 64):
            gamma = rs.gamma(100.0, 0.01, size=(host.n, k))
            beta = np.clip(rs.randint(0, 100, size=(k, k)) / 100.0, 0.01, 0.99)
            rec = {"record": "k_scan", "graph": "lfr-n1000", "n": host.n, "k": k, "variant": list(_svils.orig_variant(k))}
            rec.update(device_sweeps(host.n, k, host.edges, np.unique(host.heldout, axis=0), gamma, beta, a.sweeps, a.warmup))
            emit(rec)
    finally:
        out.close()
        os.unlink(lfr)


if __name__ == "__main__":
    main()
