"""Posterior predictive replicates on the device, phase by phase: the hipEvent times of the draw (tile kernel and link
count), of the list / CSR build and of the statistics from svils_ppc_get_timing, per replicate, for a planted model of
svinet_amd/mmsbgen_sparse.py (top-4 memberships; beta scaled so that a replicate has the mean degree asked for), beside the
observed side (svils_ppc_set_links + svils_ppc_stats of the generator's own graph).  The draw is held against its flop
model: n (n - 1) / 2 pairs x 2 K flop on the fp64 MFMA.  One JSON line per model.

    python tools/ppc_bench.py                                  # the three shapes of DESIGN.md section 4l
    python tools/ppc_bench.py --model 1000:28 --restate        # also time tools/restate_ppc.py's loops and compare
    python tools/ppc_bench.py --orig                           # the K x K kind beside the assortative one

--orig: after the assortative replicates, the same handle draws as many under svils_ppc_set_params_orig with
B = diag(beta) / 2 + one off-diagonal rate that carries the other half of the links, so both kinds see lists of about
the same length; the orig_* keys stand beside the assortative ones of the same run.  k_ppc_aq runs inside
svils_ppc_set_params_orig, outside the draw's bracket: orig_set_params_wall_ms is its wall time, upload included.
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

ORIG_SHAPES = ("32768:64", "18772:20")           # the K x K kind's largest shape, and ca-AstroPh's
SHAPES = ("1000:28", "18772:20", "32768:256")    # LFR, ca-AstroPh (its node count and the K of the headline run), the handle's largest n
MFMA_F64_TFLOPS = 49.5                           # measured, DESIGN.md section 4a


def model(n, k, mean_deg):
    from svinet_amd import mmsbgen_sparse
    pairs, (comm, w, beta) = mmsbgen_sparse.generate(n, k, mean_deg, return_truth=True)
    pi = np.zeros((n, k))
    np.add.at(pi, (np.repeat(np.arange(n), comm.shape[1]), comm.reshape(-1)), w.reshape(-1))
    pi /= pi.sum(1)[:, None]
    mass = pi.sum(0)
    beta = np.clip(beta * (n * mean_deg / 2.0) / float((beta * mass * mass / 2.0).sum()), 0.0, 1.0)
    return np.asarray(pairs, np.uint32), pi, beta


def run(shape, a):
    from svinet_amd.host_api import PPC
    n, k = (int(x) for x in shape.split(":"))
    links, pi, beta = model(n, k, a.mean_deg)
    ppc = PPC(n, k, max_links=max(8 * len(links), 1 << 16))
    ppc.set_params(pi, beta)
    rows, wall = [], []
    for r in range(a.warmup + a.reps):
        t = time.perf_counter()
        ppc.draw(seed=a.seed, r=r)
        s = ppc.stats()
        if r >= a.warmup:
            wall.append(1e3 * (time.perf_counter() - t))
            rows.append(dict(s["timing_ms"], ones=s["ones"], rechecked=s["rechecked"], triangles=s["triangles"]))
    out = {"model": shape, "n": n, "k": k, "replicates": a.reps}
    for key in ("draw", "csr", "stats"):
        out[key + "_ms"] = float(np.median([x[key] for x in rows]))
    out["device_ms"] = out["draw_ms"] + out["csr_ms"] + out["stats_ms"]
    out["wall_ms"] = float(np.median(wall))
    out["ones_mean"] = float(np.mean([x["ones"] for x in rows]))
    out["rechecked_total"] = int(sum(x["rechecked"] for x in rows))
    pairs = n * (n - 1) / 2
    out["draw_tflops"] = pairs * 2 * k / (out["draw_ms"] * 1e-3) / 1e12
    out["draw_mfma_fraction"] = out["draw_tflops"] / MFMA_F64_TFLOPS
    out["draw_gpairs_per_s"] = pairs / (out["draw_ms"] * 1e-3) / 1e9
    ppc.observe(links)
    o = ppc.stats()
    out.update(observed_links=int(len(links)), observed_csr_ms=o["timing_ms"]["csr"], observed_stats_ms=o["timing_ms"]["stats"],
               observed_triangles=o["triangles"])
    if a.orig:
        mass = pi.sum(0)
        cross = (mass.sum() ** 2 - float((mass * mass).sum())) / 2.0          # sum over g != h of mass_g mass_h / 2
        B = np.full((k, k), min(1.0, (out["ones_mean"] / 2.0) / cross))
        B[np.arange(k), np.arange(k)] = beta / 2.0
        t = time.perf_counter()
        ppc.set_params_orig(pi, B)
        out["orig_set_params_wall_ms"] = 1e3 * (time.perf_counter() - t)
        rows = []
        for r in range(a.warmup + a.reps):
            ppc.draw(seed=a.seed, r=r)
            s = ppc.stats()
            if r >= a.warmup:
                rows.append(dict(s["timing_ms"], ones=s["ones"], rechecked=s["rechecked"], offdiag=s["offdiag_share"]))
        for key in ("draw", "csr", "stats"):
            out["orig_" + key + "_ms"] = float(np.median([x[key] for x in rows]))
        out["orig_ones_mean"] = float(np.mean([x["ones"] for x in rows]))
        out["orig_rechecked_total"] = int(sum(x["rechecked"] for x in rows))
        out["orig_offdiag_share_mean"] = float(np.mean([x["offdiag"] for x in rows]))
        out["orig_stats_us_per_link"] = 1e3 * out["orig_stats_ms"] / out["orig_ones_mean"]
        out["stats_us_per_link"] = 1e3 * out["stats_ms"] / out["ones_mean"]
    if a.restate:
        import restate_ppc as R
        t = time.perf_counter()
        want = R.draw_loops(pi, beta, a.seed, 0)
        out["restate_loops_s"] = time.perf_counter() - t
        out["restate_equal"] = bool(np.array_equal(ppc.draw(pi, beta, seed=a.seed, r=0).astype(np.int64), want))
    ppc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", action="append", help="n:k (default: %s)" % " ".join(SHAPES))
    ap.add_argument("--mean-deg", type=float, default=24.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--restate", action="store_true", help="also run the restatement's double loop once and compare the links")
    ap.add_argument("--orig", action="store_true", help="also the K x K kind at the same n and K (default shapes: %s)" % " ".join(ORIG_SHAPES))
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    for shape in a.model or (ORIG_SHAPES if a.orig else SHAPES):
        line = json.dumps(run(shape, a))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
