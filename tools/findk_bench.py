"""-findk on the device, phase by phase: per iteration the hipEvent times of the count (+ top 5), apply (set_gamma +
estimate_all_pi), likelihoods and groups (svils_findk_get_timing), the host time of the padding draws and the number of
padded nodes, the whole step's wall time -- and the numpy restatement's time on the same input (tools/restate_findk.py).
One JSON line per graph.

    python tools/findk_bench.py --graph astroph            # tests/golden/graphs/ca-AstroPh (n = 17903)
    python tools/findk_bench.py --graph mmsb:1000000:512    # the config-5 graph (svinet_amd/mmsbgen_sparse.py, mean degree 24)
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


def graph_file(spec, tmp):
    if spec == "astroph":
        dst = os.path.join(tmp, "ca-AstroPh.csv")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "graphs", "ca-AstroPh.csv.gz"), "rb") as f, open(dst, "wb") as g:
            g.write(f.read())
        return dst, 17903, 20
    _, sn, sk = spec.split(":")
    from svinet_amd import mmsbgen_sparse
    dst = os.path.join(tmp, "mmsb.txt")
    mmsbgen_sparse.write_pairs(dst, mmsbgen_sparse.generate(int(sn), int(sk), 24))
    return dst, int(sn), int(sk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="astroph")
    ap.add_argument("--no-restate", action="store_true")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    from svinet_amd.host_api import FindK
    with tempfile.TemporaryDirectory() as tmp:
        path, n, k = graph_file(a.graph, tmp)
        t0 = time.perf_counter()
        fk = FindK(path, n, k)
        setup_s = time.perf_counter() - t0
        iters = []
        while True:
            t = time.perf_counter()
            r = fk.step()
            wall = time.perf_counter() - t
            if r == FindK.STEP_DONE:
                break
            rec = fk.timing()
            rec.update({"iter": fk.iter, "step_wall_ms": 1e3 * wall, "unlikely": fk.unlikely, "stopped": r == FindK.STEP_STOPPED})
            iters.append(rec)
            if r == FindK.STEP_STOPPED:
                break
        lab, val, masks = fk.state()
        fk.close()
        out = {"graph": a.graph, "n": n, "k": k, "setup_s": setup_s, "iterations": iters,
               "device_ms_per_iter": float(np.mean([i["count_ms"] + i["apply_ms"] + i["likelihood_ms"] + i["groups_ms"] for i in iters])),
               "pad_host_ms_per_iter": float(np.mean([i["pad_host_ms"] for i in iters])),
               "step_wall_ms_per_iter": float(np.mean([i["step_wall_ms"] for i in iters]))}
        out["pad_share_of_step"] = out["pad_host_ms_per_iter"] / out["step_wall_ms_per_iter"]
        if not a.no_restate:
            import restate_findk as R
            t = time.perf_counter()
            edges, seq2id = R.read_graph(path, n)
            ref = R.FindK(edges, seq2id, len(seq2id), k).run()
            out["restate_s"] = time.perf_counter() - t
            out["restate_equal_state"] = bool(np.array_equal(ref.labels, lab.astype(np.int64)) and np.array_equal(ref.values, val))
            out["restate_pad_s"] = float(sum(ref.pad_seconds))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
