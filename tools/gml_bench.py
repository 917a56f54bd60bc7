"""-gml / -lcstats on the device, pass by pass: the hipEvent times of the node pass, the link pass (with the band recheck)
and the counts (with the GML list) from svils_lc_get_timing, the number of links rechecked in the reference's order, and
the CLI end to end: the tutorial's chain `-link-sampling -max-iterations 1` (which writes gamma.txt / lambda.txt), then
`-gml` in its output directory, timed as a whole.  One JSON line.

    python tools/gml_bench.py --graph mmsb:1000000:512     # config 5 (svinet_amd/mmsbgen_sparse.py, mean degree 24)
    python tools/gml_bench.py --graph mmsb:200000:512 --restate
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")


def model(n, k, seed=7):
    """the generator's graph and a gamma / lambda near its planted memberships"""
    from svinet_amd import mmsbgen_sparse
    pairs, (comm, w, beta) = mmsbgen_sparse.generate(n, k, 24, return_truth=True)
    rng = np.random.default_rng(seed)
    gamma = np.full((n, k), 0.01) + rng.gamma(0.05, 0.1, size=(n, k))
    np.add.at(gamma, (np.repeat(np.arange(n), comm.shape[1]), comm.reshape(-1)), 100.0 * w.reshape(-1))
    lam = np.stack([beta * 100 + 1e-3, (1 - beta) * 100 + 1e-3], axis=1)
    return pairs, gamma, lam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="mmsb:1000000:512")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--restate", action="store_true", help="also compare the arrays with tools/restate_gml.py")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    from svinet_amd import mmsbgen_sparse
    from svinet_amd.host_api import LinkCommunities
    _, sn, sk = a.graph.split(":")
    n, k = int(sn), int(sk)
    pairs, gamma, lam = model(n, k)
    links = np.asarray(pairs, np.uint32)
    out = {"graph": a.graph, "n": n, "k": k, "links": int(len(links))}
    runs = []
    for _ in range(a.reps):
        t = time.perf_counter()
        r = LinkCommunities(links, gamma, lam)
        runs.append(dict(r["timing_ms"], wall_ms=1e3 * (time.perf_counter() - t)))
    for key in ("node", "link", "count", "wall_ms"):
        out[key + ("" if key == "wall_ms" else "_ms")] = float(np.median([x[key] for x in runs]))
    out["device_ms"] = out["node_ms"] + out["link_ms"] + out["count_ms"]
    out.update(unlikely=r["unlikely"], gml_edges=int(len(r["gml_edges"])), rechecked=r["n_rechecked"])
    out["gather_gb"] = 2 * 8 * k * len(links) / 1e9
    out["link_pass_gb_per_s"] = out["gather_gb"] / (out["link_ms"] * 1e-3)
    if a.restate:
        import restate_gml as R
        t = time.perf_counter()
        ref = R.link_communities(links, gamma, lam)
        out["restate_s"] = time.perf_counter() - t
        out["restate_equal"] = bool(all(np.array_equal(r[x], ref[x]) for x in ("group", "colour", "join", "gml", "deg_c",
                                                                                  "memberships", "influence"))
                                    and np.array_equal(r["bridgeness"].view(np.int64), ref["bridgeness"].view(np.int64)))
    del r
    if not a.no_cli:
        with tempfile.TemporaryDirectory() as tmp:
            net = os.path.join(tmp, "net.txt")
            mmsbgen_sparse.write_pairs(net, pairs)
            t = time.perf_counter()
            subprocess.run([SVINET, "-file", net, "-n", str(n), "-k", str(k), "-link-sampling", "-max-iterations", "1"], cwd=tmp,
                           stdout=subprocess.DEVNULL, check=True)
            out["cli_fit_s"] = time.perf_counter() - t
            fit = [os.path.join(tmp, d) for d in os.listdir(tmp) if d.endswith("-linksampling")][0]
            env = dict(os.environ, SVINET_TIMING_FILE=os.path.join(tmp, "timing.json"))
            t = time.perf_counter()
            subprocess.run([SVINET, "-file", net, "-n", str(n), "-k", str(k), "-gml"], cwd=fit, stdout=subprocess.DEVNULL, check=True,
                           env=env)
            out["cli_gml_s"] = time.perf_counter() - t
            out["cli_gml_device"] = json.load(open(os.path.join(tmp, "timing.json")))
            out["cli_gml_bytes"] = {f: os.path.getsize(os.path.join(fit, "gml", f)) for f in sorted(os.listdir(os.path.join(fit, "gml")))
                                    if f.endswith((".txt", ".gml"))}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
