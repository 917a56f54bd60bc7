"""The hop plot and the components of an undirected simple graph, restated from DESIGN.md section 4o in plain Python: one
queue BFS per source over sorted adjacency lists, no bit tricks.  The device (svils_ppc_hops, `svinet -ppc -ppc-hops`) is
held to this, integer for integer and text for text (tests/test_gpu_hops.py).

    d(s, v)   the BFS distance; infinite across components; d(s, s) = 0
    D[h]      ordered pairs (s, v) with d(s, v) = h (D[0] = n, D[1] = 2 links); levels = len(D) = the largest finite d + 1
    ecc[s]    the largest finite d(s, .), 0 for an isolated node;  comp[v]: the smallest node id of v's component
"""
import math
from collections import deque

import numpy as np


def adjacency(links, n):
    adj = [[] for _ in range(n)]
    for p, q in np.asarray(links, np.int64).reshape(-1, 2).tolist():
        adj[p].append(q)
        adj[q].append(p)
    for row in adj:
        row.sort()
    return adj


def hops(links, n):
    """{D [levels], ecc [n], comp [n], deg [n]} of the graph of links [E][2] on n nodes"""
    adj = adjacency(links, n)
    D = [0] * n
    ecc = [0] * n
    comp = [-1] * n
    for s in range(n):
        dist = [-1] * n
        dist[s] = 0
        queue = deque([s])
        while queue:
            u = queue.popleft()
            du = dist[u]
            D[du] += 1
            if du > ecc[s]:
                ecc[s] = du
            if comp[u] < 0:          # sources ascend: the first one to reach u is the smallest id of its component
                comp[u] = s
            for v in adj[u]:
                if dist[v] < 0:
                    dist[v] = du + 1
                    queue.append(v)
    levels = max(h for h in range(n) if D[h]) + 1
    return {"D": np.array(D[:levels], np.uint64), "ecc": np.array(ecc, np.uint32), "comp": np.array(comp, np.uint32),
            "deg": np.array([len(r) for r in adj], np.uint32)}


def effdiam(D):
    """the 90th percentile of the hop plot, linearly interpolated (SNAP's CalcEffDiam), in the definition's order"""
    C, run = [], 0
    for d in D:
        run += int(d)
        C.append(run)
    t = 0.9 * float(C[-1])
    hs = 0
    while float(C[hs]) < t:
        hs += 1
    if hs == 0:
        return 0.0
    return float(hs - 1) + (t - float(C[hs - 1])) / float(C[hs] - C[hs - 1])


def summary(D, deg, comp):
    D = [int(d) for d in D]
    n = len(comp)
    total = sum(D)
    reachable = total - n
    far = sum(h * d for h, d in enumerate(D))
    comp = np.asarray(comp, np.int64)
    return {"reachable": reachable, "diameter": len(D) - 1, "levels": len(D),
            "components": int(np.count_nonzero(comp == np.arange(n))), "largest": int(np.bincount(comp, minlength=n).max()),
            "isolated": int(np.count_nonzero(np.asarray(deg) == 0)),
            "meandist": float(far) / float(reachable) if reachable else math.nan, "effdiam": effdiam(D)}


def all_of(links, n):
    """hops() and summary() in one dict"""
    h = hops(links, n)
    h.update(summary(h["D"], h["deg"], h["comp"]))
    return h


# ---- the five files of `svinet -ppc -ppc-hops` ----

STATISTICS = ("effdiam", "diameter", "meandist", "components", "largest", "isolated")


def fx(x, digits=5):
    return "nan" if math.isnan(x) else "%.*f" % (digits, x)


def obs_hops_text(D):
    out, run = "", 0
    for h, d in enumerate(D):
        run += int(d)
        out += "%d\t%d\t%d\n" % (h, int(d), run)
    return out


def rep_hops_text(reps):
    return "".join("%d\t%s\t%d\t%s\t%d\t%d\t%d\n" % (r, fx(s["effdiam"]), s["diameter"], fx(s["meandist"]), s["components"], s["largest"],
                                                     s["isolated"]) for r, s in enumerate(reps))


def summary_text(obs, reps):
    """the columns of ppc/summary.txt: statistic, observed, replicate mean, deviation, two-sided p (restate_ppc.moments)"""
    import restate_ppc
    out = ""
    for name in STATISTICS:
        m = restate_ppc.moments([float(s[name]) for s in reps], float(obs[name]))
        out += "%s\t%s\t%s\t%s\t%s\n" % (name, fx(float(obs[name])), fx(m[0]), fx(m[1]), fx(m[3]))
    return out


def hops_texts(obs, reps):
    """{path relative to the working directory: text} from the all_of() of the observed network and of every replicate"""
    return {"obs-hop.txt": fx(obs["effdiam"]) + "\n", "ppc/ppc-hop.txt": "".join(fx(s["effdiam"]) + "\n" for s in reps),
            "ppc/obs-hops.txt": obs_hops_text(obs["D"]), "ppc/rep-hops.txt": rep_hops_text(reps),
            "ppc/hops-summary.txt": summary_text(obs, reps)}


def ppc_hops_texts(links, gam, lam, draws, seed, mean):
    """the five files of `svinet -ppc -ppc-hops` for a fitted model: the replicates are restate_ppc's"""
    import restate_ppc as R
    gam = np.asarray(gam, np.float64)
    n = gam.shape[0]
    pim, betam = R.mean_params(gam, lam)
    reps = []
    for r in range(draws):
        pi, beta = (pim, betam) if mean else (R.dirichlet_rows(gam, seed, r), R.beta_draws(lam, seed, r))
        reps.append(all_of(R.draw(pi, beta, seed, r), n))
    return hops_texts(all_of(links, n), reps)
