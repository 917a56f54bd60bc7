"""The hop plot of posterior predictive replicates on the device: the hipEvent time of svils_ppc_hops per replicate
(svils_ppc_get_hop_timing), its launches and levels, for the planted models of tools/ppc_bench.py (the three shapes of
DESIGN.md section 4l, beta scaled to the mean degree asked for), beside the replicate's own device time (draw, list / CSR,
statistics).  The gather is held against its byte model: per pass and level that does work, 2 links column ids of 4 B
and 2 links x W frontier words of 8 B.  One JSON line per model and hop batch.

    python tools/hops_bench.py                                  # the three shapes at the default batch
    python tools/hops_bench.py --words 1 2 4 8 --chunk 4 8 16   # the A/B of the hop batch
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ppc_bench  # noqa: E402


def run(shape, a):
    from svinet_amd.host_api import PPC
    n, k = (int(x) for x in shape.split(":"))
    links, pi, beta = ppc_bench.model(n, k, a.mean_deg)
    ppc = PPC(n, k, max_links=max(8 * len(links), 1 << 16))
    ppc.set_params(pi, beta)
    for words in a.words:
        for chunk in a.chunk:
            ppc.set_hop_batch(words, chunk)
            w = words or 8
            rows = []
            for r in range(a.warmup + a.reps):
                ppc.draw(seed=a.seed, r=r)
                s = ppc.stats()
                h = ppc.hops()
                ms, launches = ppc.hop_timing()
                if r < a.warmup:
                    continue
                # the levels that do work in a pass: up to the first empty one, the largest ecc of its sources + 1
                work = sum(int(h["ecc"][s0:s0 + 64 * w].max()) + 1 for s0 in range(0, n, 64 * w))
                rows.append(dict(ms=ms, launches=launches, work=work, levels=len(h["D"]), ones=s["ones"], effdiam=h["effdiam"],
                                 components=h["components"], largest=h["largest"], replicate_ms=sum(s["timing_ms"].values())))
            med = lambda key: float(np.median([x[key] for x in rows]))  # noqa: E731
            out = {"model": shape, "n": n, "k": k, "replicates": a.reps, "words": w, "levels_per_chunk": chunk or 8,
                   "passes": -(-n // (64 * w)), "hops_ms": med("ms"), "launches": med("launches"), "working_levels": med("work"),
                   "levels": med("levels"), "ones_mean": float(np.mean([x["ones"] for x in rows])), "effdiam": med("effdiam"),
                   "components": med("components"), "largest": med("largest"), "replicate_device_ms": med("replicate_ms")}
            model_bytes = np.median([x["work"] * 2.0 * x["ones"] * (4 + 8 * w) for x in rows])
            out["gather_model_gb"] = float(model_bytes) / 1e9
            out["gather_gb_per_s"] = float(model_bytes) / (out["hops_ms"] * 1e-3) / 1e9
            out["hops_over_replicate"] = out["hops_ms"] / out["replicate_device_ms"]
            line = json.dumps(out)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
    ppc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", action="append", help="n:k (default: %s)" % " ".join(ppc_bench.SHAPES))
    ap.add_argument("--mean-deg", type=float, default=24.0)
    ap.add_argument("--words", type=int, nargs="+", default=[0], help="hop batches to time (0: the default)")
    ap.add_argument("--chunk", type=int, nargs="+", default=[0], help="levels per chunk to time (0: the default)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    for shape in a.model or ppc_bench.SHAPES:
        run(shape, a)


if __name__ == "__main__":
    main()
