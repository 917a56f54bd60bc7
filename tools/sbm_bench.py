"""The -single engine on the device: device milliseconds per E-step pass and per whole iteration from
the hipEvent brackets of svils_sbm_get_timing, for the blocked chain (B consecutive nodes gather at once) and the plain chain
(B = 1) on the same handle, alternating, the median of --repeats runs after one warm-up run each; the time of one chain launch
at the nodes-per-launch cap; the device ms of a bound pass of -single-logl (svils_sbmelbo) and the wall ms
of the whole call beside an E-pass, the median of --repeats passes after a warm-up; and, on LFR, the seconds per pass of the host loops (-host-loops: one iteration through the host
library, over its passes; on ca-AstroPh they are not run).  One JSON line per workload:

    LFR (n = 1 000) at K = 28, ca-AstroPh (n = 17 903) at K = 20

The start is the reference's (Gamma(100 * 100 / K, 0.01) rows); the skip list is 1 % of the links and as many non-links.  Both
chains are checked to leave the same bits.

    python tools/sbm_bench.py [--only lfr astroph] [--out file]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sparse_graph_bench import Graph, golden_links   # noqa: E402


def start(n, k, rs):
    v = 100.0 / k
    phi = rs.gamma(100 * v, 0.01, (n, k))
    return phi / phi.sum(axis=1, keepdims=True), rs.gamma(100 * v, 0.01, k), rs.gamma(100.0, 0.01, (k + 1, 2))


def run(name, gz, k, a):
    from svinet_amd import _svils
    rs = np.random.RandomState(7)
    n, links = golden_links(gz)
    g = Graph(n, links, rs)
    skip = np.sort(g.skip, axis=1).astype(np.uint32)
    state = start(n, k, rs)
    eta = np.ones((k + 1, 2))
    eta[k] = (0.0001, 1.0)
    h = _svils.Sbm(n, k, 0.5, eta)
    h.set_graph(links, skip)
    out = {"workload": name, "n": n, "k": k, "links": int(len(links)), "skip_pairs": int(len(skip)), "variant": list(_svils.sbm_variant(k)),
           "repeats": a.repeats, "launch_nodes": a.launch_nodes or 2048}
    h.set_launch_nodes(a.launch_nodes)
    res, bits = {"blocked": [], "plain": []}, {}
    for r in range(a.repeats + 1):
        for form in ("blocked", "plain"):                  # alternating
            h.set_plain_chain(form == "plain")
            h.set_state(*state)
            h.sweep(1)
            ms = h.timing()
            passes = h.stats()[0]
            bits[form] = b"".join(x.tobytes() for x in h.state())
            if r:
                res[form].append((ms[0], ms[1], ms[2], passes))
    for form, rows in res.items():
        rows = np.array(rows)
        med = np.median(rows, axis=0)
        out[form] = {"iteration_ms": med[0], "chain_ms": med[1], "mstep_ms": med[2], "passes": int(med[3]),
                     "ms_per_pass": med[1] / max(med[3], 1), "iteration_ms_min_max": [rows[:, 0].min(), rows[:, 0].max()]}
    out["same_bits"] = bits["blocked"] == bits["plain"]
    out["plain_over_blocked_per_pass"] = out["plain"]["ms_per_pass"] / out["blocked"]["ms_per_pass"]
    # one launch at the cap: a single pass cut into launches, its chain time over the number of launches
    h.set_plain_chain(False)
    h.set_state(*state)
    h.estep(1)
    cap = a.launch_nodes or 2048
    out["launch_ms_at_cap"] = h.timing()[1] / -(-n // cap)
    # the bound pass of -single-logl (svils_sbmelbo) beside an E-pass: device ms of its four kernels and
    # the wall ms of the whole call (with the copies back and the host's lnGamma terms), on the state the E-pass left
    h.elbo()
    ems, wall, vals = [], [], set()
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        vals.add(h.elbo())
        wall.append((time.perf_counter() - t0) * 1e3)
        ems.append(h.elbo_timing())
    out["elbo"] = {"device_ms": float(np.median(ems)), "device_ms_min_max": [min(ems), max(ems)], "call_wall_ms": float(np.median(wall)),
                   "same_bits": len(vals) == 1, "over_e_pass": float(np.median(ems)) / out["blocked"]["ms_per_pass"]}
    h.close()
    if a.host and name == "lfr":
        from svinet_amd.host_api import SbmEngine
        import gzip
        import tempfile
        with tempfile.NamedTemporaryFile(suffix=".txt", delete=False) as f:
            f.write(gzip.open(os.path.join(ROOT, "tests", "golden", "graphs", gz), "rb").read())
        e = SbmEngine(f.name, n, k, seed=6, on_device=False)
        t0 = time.perf_counter()
        e.sweep()
        out["host_loops_s_per_pass"] = (time.perf_counter() - t0) / (e.passes + 0.5)   # (the M-step is about half a pass)
        e.close()
        os.unlink(f.name)
    else:
        out["host_loops_s_per_pass"] = "not run"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None, choices=["lfr", "astroph"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launch-nodes", type=int, default=0)
    ap.add_argument("--no-host", dest="host", action="store_false")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    for name, gz, k in (("lfr", "LFR-network-n1000-k28.txt.gz", 28), ("astroph", "ca-AstroPh.csv.gz", 20)):
        if a.only and name not in a.only:
            continue
        line = json.dumps(run(name, gz, k, a))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
