"""svils_rank_links: its time against svils_predict_links(topk = 10) on the same handle, and what it measures on fitted models.

  python tools/rank_bench.py [--reps R] [--out file.jsonl] [--workloads time,lfr,astroph] [--baselines]

  time     n = 1e6, K = 512 seeded random state (that of tools/predict_bench.py's workload 3): 8192 directed pairs (p, q), one
           per query node, through rank_links, and the same 8192 nodes through predict_links(topk = 10); same handle, same
           process.  Each call is synchronous; the time is the wall time of a warm call, best and median of --reps.
  lfr      LFR n = 1000, K = 28 fitted to the stop rule: the held-out links of the validation set, both directions, ranked;
           per-link AUC, MRR and hits@k as link-ranks-summary.txt defines them
  astroph  the same for ca-AstroPh, K = 20 (at most 6400 sweeps; "stopped" says whether the stop rule fired)

  --baselines  the model-free baselines beside the model (svils_nbr_rank).  `time` then runs on the
           config-5 graph (svinet_amd/mmsbgen_sparse.py: n = 1e6, mean degree 24) instead of the sparser random one and
           adds a warm nbr_rank(AA) and nbr_score(AA) call for the same 8192 pairs, with the sizes of the queries'
           two-hop walks; lfr / astroph add the summary of the same pairs ranked by cn, aa and ra and a warm
           nbr_rank(AA) call beside a warm rank_links call."""
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

GRAPHS = {"lfr": ("LFR-network-n1000-k28.txt.gz", 1000, 28), "astroph": ("ca-AstroPh.csv.gz", 17903, 20)}


def _time(fn, reps):
    fn()   # warm: scratch, sorted rows
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, float(np.median(ts)) * 1e3


def _summary(above, tied, ncand):
    mid = above + 0.5 * tied
    ahead = above.astype(np.int64) + tied
    return {"auc": float(np.mean(1.0 - mid / ncand)), "mrr": float(np.mean(1.0 / (mid + 1.0))),
            "hits1": float(np.mean(ahead < 1)), "hits10": float(np.mean(ahead < 10)), "hits100": float(np.mean(ahead < 100)),
            "chance10": float(np.mean(10.0 / ncand)), "tied_pairs": int(np.sum(tied > 0))}


def run_time(reps, baselines=False):
    from svinet_amd import _svils
    n, k, nq = 1000000, 512, 8192
    rng = np.random.default_rng(12345)
    if baselines:
        from svinet_amd import mmsbgen_sparse as G
        e = np.asarray(G.generate(n, k, 24), dtype=np.int64)
    else:
        a, b = rng.integers(0, n, size=(2, 2 * n))
        e = np.stack([np.minimum(a, b), np.maximum(a, b)], 1)
    e = np.stack([e.min(1), e.max(1)], 1)
    e = np.unique(e[e[:, 0] != e[:, 1]], axis=0)
    links = np.ascontiguousarray(e, dtype=np.uint32)
    eng = _svils.Engine(n, k, ones=len(links), ones_prob=len(links) / (n * (n - 1) / 2), use_validation_stop=False)
    eng.set_graph(links)
    eng.set_state(rng.random((n, k)) + 0.01, rng.random((k, 2)) + 0.1)
    nodes = rng.choice(n, size=nq, replace=False).astype(np.uint32)
    pairs = np.stack([nodes, (nodes + 1 + rng.integers(0, n - 1, size=nq)) % n], 1).astype(np.uint32)
    rbest, rmed = _time(lambda: eng.rank_links(pairs), reps)
    pbest, pmed = _time(lambda: eng.predict_links(10, nodes), reps)
    flop = 2.0 * nq * n * k
    rec = {"workload": "time", "name": "n=1e6 K=512 random state, 8192 query rows", "n": n, "K": k, "rows": nq, "flop": flop,
           "links": len(links), "rank_links_best_ms": rbest, "rank_links_median_ms": rmed, "predict_links_top10_best_ms": pbest,
           "predict_links_top10_median_ms": pmed, "rank_tflops": flop / rbest / 1e9, "predict_tflops": flop / pbest / 1e9,
           "rank_over_predict": rbest / pbest}
    if baselines:
        nbest, nmed = _time(lambda: eng.nbr_rank(_svils.NBR_AA, pairs), reps)
        sbest, smed = _time(lambda: eng.nbr_score(_svils.NBR_AA, pairs), reps)
        deg = np.bincount(links.ravel(), minlength=n)
        walk = np.zeros(n, dtype=np.int64)                  # entries the two-hop walk of a query node reads: sum of deg z, z in N(p)
        np.add.at(walk, links[:, 0], deg[links[:, 1]])
        np.add.at(walk, links[:, 1], deg[links[:, 0]])
        w = walk[nodes]
        rec.update({"name": "n=1e6 K=512 config-5 graph, 8192 directed pairs", "nbr_rank_aa_best_ms": nbest,
                    "nbr_rank_aa_median_ms": nmed, "nbr_score_aa_best_ms": sbest, "nbr_score_aa_median_ms": smed,
                    "nbr_rank_over_rank_links": nbest / rbest, "max_degree": int(deg.max()),
                    "two_hop_entries_mean": float(w.mean()), "two_hop_entries_max": int(w.max())})
    eng.close()
    return rec


def run_quality(which, baselines=False):
    from svinet_amd.host_api import Setup
    fname, n, k = GRAPHS[which]
    tmp = tempfile.NamedTemporaryFile(delete=False, suffix=".txt")
    with gzip.open(os.path.join(ROOT, "tests", "golden", "graphs", fname), "rb") as f:
        tmp.write(f.read())
    tmp.close()
    try:
        s = Setup(tmp.name, n, k)
    finally:
        os.unlink(tmp.name)
    eng = s.engine(use_validation_stop=True)
    for _ in range(100):
        eng.sweep(64)
        if eng.control().stopped:
            break
    c = eng.control()
    v1 = s.validation_accept[s.validation_accept[:, 2] == 1][:, :2]
    pairs = np.ascontiguousarray(np.stack([v1, v1[:, ::-1]], 1).reshape(-1, 2), dtype=np.uint32)
    t0 = time.perf_counter()
    above, tied, ncand, _ = eng.rank_links(pairs)
    ms = (time.perf_counter() - t0) * 1e3
    rec = {"workload": which, "n": s.n, "K": k, "stopped": bool(c.stopped), "iterations": int(c.iter), "directed_pairs": len(pairs)}
    rec.update(_summary(above, tied, ncand))
    rec["rank_links_first_call_ms"] = ms
    if baselines:
        from svinet_amd import _svils
        for name, m in (("cn", _svils.NBR_CN), ("aa", _svils.NBR_AA), ("ra", _svils.NBR_RA)):
            a, t, nc, _ = eng.nbr_rank(m, pairs)
            rec[name] = _summary(a, t, nc)
        rec["rank_links_warm_best_ms"], rec["rank_links_warm_median_ms"] = _time(lambda: eng.rank_links(pairs), 5)
        rec["nbr_rank_aa_warm_best_ms"], rec["nbr_rank_aa_warm_median_ms"] = _time(lambda: eng.nbr_rank(_svils.NBR_AA, pairs), 5)
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default="time,lfr,astroph")
    ap.add_argument("--out", default=None)
    ap.add_argument("--baselines", action="store_true")
    a = ap.parse_args()
    for w in a.workloads.split(","):
        rec = run_time(a.reps, a.baselines) if w == "time" else run_quality(w, a.baselines)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
