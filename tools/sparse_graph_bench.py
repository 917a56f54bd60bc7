"""The two graph forms of the svils_batch handle side by side: device milliseconds per step from the
hipEvent bracket of svils_batch_get_timing over a chunk of --chunk queued steps (median of --repeats chunks after one
warm-up chunk, tools/sampled_bench.py's method) for the four step kinds -- node steps, pair steps of n / 2 random pairs,
star steps (a node's links and 100 random non-links) and strat steps (a node's links, or n / 10 random non-links, in
turn) -- on one drawn list of steps per workload:

    dense and sparse form    ca-AstroPh (n = 17 903) at K = 20, LFR (n = 1 000) at K = 28
    sparse form alone        svinet_amd/mmsbgen_sparse.py graphs of n = 10^5 and 10^6 at K = 64, with the device memory in use after a chunk

One JSON line per workload; where both forms run, their final states are compared as bits.

    python tools/sparse_graph_bench.py                       # all four workloads
    python tools/sparse_graph_bench.py --only astroph lfr    # the side-by-side ones
    python tools/sparse_graph_bench.py --dense-only          # the dense form alone: also runs on a build without the sparse form,
                                                             # the yardstick of the dense numbers (from that build's tree)
"""
import argparse
import gzip
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GRAPHS = os.path.join(ROOT, "tests", "golden", "graphs")
KINDS = ("node", "pairs", "star", "strat")


def golden_links(gz):
    """the links of a golden graph file, nodes renumbered 0 .. n - 1 -> n, links [m][2] (p < q, unique)"""
    with gzip.open(os.path.join(GRAPHS, gz), "rt") as f:
        ids = np.array([[int(x) for x in line.replace(",", " ").split()[:2]] for line in f if line.strip() and line[0].isdigit()], dtype=np.int64)
    names, flat = np.unique(ids, return_inverse=True)
    return len(names), unique_pairs(flat.reshape(-1, 2), len(names))


def unique_pairs(pairs, n):
    lo, hi = np.minimum(pairs[:, 0], pairs[:, 1]).astype(np.int64), np.maximum(pairs[:, 0], pairs[:, 1]).astype(np.int64)
    key = np.unique((lo * n + hi)[lo != hi])
    return np.stack([key // n, key % n], axis=1).astype(np.uint32)


class Graph:
    def __init__(self, n, links, rs):
        self.n, self.links = n, links
        ends = np.concatenate([links, links[:, ::-1]]).astype(np.int64)
        order = np.argsort(ends[:, 0] * n + ends[:, 1])
        self.col = ends[order, 1]
        self.row = np.concatenate([[0], np.cumsum(np.bincount(ends[:, 0], minlength=n))])
        # the skip set: 1 % of the links and as many random non-links, as the engines hold out
        m = max(2, len(links) // 100)
        zeros = unique_pairs(rs.randint(0, n, (2 * m, 2)), n)
        zeros = zeros[~np.isin(self.keys(zeros), self.keys(links))][:m]
        self.skip = np.concatenate([links[rs.choice(len(links), m, replace=False)], zeros])
        self.skipkeys = np.sort(self.keys(self.skip))

    def keys(self, pairs):
        return pairs[:, 0].astype(np.int64) * self.n + pairs[:, 1].astype(np.int64)

    def nbrs(self, a):
        return self.col[self.row[a]:self.row[a + 1]]

    def star(self, a, partner, rs):
        partner = np.unique(partner[partner != a])
        keep = ~np.isin(np.minimum(a, partner) * self.n + np.maximum(a, partner), self.skipkeys)
        partner = partner[keep][rs.permutation(int(keep.sum()))]
        return dict(start=int(a), partner=partner.astype(np.uint32), y=np.isin(partner, self.nbrs(a)).astype(np.uint8))

    def draw(self, rs, count):
        """count steps of every kind: the step sizes of iteration 1000 on, the scales of the engines"""
        n, out = self.n, {}
        rg = [(1024.0 + 1 + (1000 + c) / 100.0) ** -0.5 for c in range(count)]
        rl = [(1024.0 + 1 + 1000 + c) ** -0.9 for c in range(count)]
        out["node"] = dict(nodes=rs.randint(0, n, count), scale=n / 2.0, rho_gamma=rg, rho_lambda=rl)
        lists = []
        for _ in range(count):
            p = unique_pairs(rs.randint(0, n, (n // 2, 2)), n)
            lists.append(p[~np.isin(self.keys(p), self.skipkeys)])
        out["pairs"] = dict(lists=lists, scale=[(n * (n - 1) / 2.0) / max(len(l), 1) for l in lists], rho_gamma=rg, rho_lambda=rl)
        stars, strat = [], []
        for c in range(count):
            a = int(rs.randint(0, n))
            s = self.star(a, np.concatenate([self.nbrs(a), rs.randint(0, n, 100)]), rs)
            s.update(rho_partner=np.full(len(s["partner"]), rg[c]), rho_start=rg[c], scale=n / 2.0, rho_lambda=rl[c])
            stars.append(s)
            a = int(rs.randint(0, n))
            if c % 2 == 0:
                s = self.star(a, self.nbrs(a), rs)
            else:
                cand = rs.randint(0, n, n // 10 + n // 50)
                s = self.star(a, cand[~np.isin(cand, self.nbrs(a))], rs)
                s["partner"], s["y"] = s["partner"][: n // 10], s["y"][: n // 10]
            s.update(rho_gamma=rg[c], scale=float(n) if c % 2 == 0 else 10.0 * n, rho_lambda=rl[c])
            strat.append(s)
        out["star"], out["strat"] = stars, strat
        return out


def run_form(g, k, sparse, steps, chunk, repeats, state):
    """-> {kind: ms per step}, the final state, the most device memory in use after a chunk: bytes above what was in use
    before the handle was made (hipMemGetInfo through torch, so torch's own context is in it; what set_graph holds for a
    moment while it builds is not)"""
    import torch
    from svinet_amd import _svils
    used = lambda: torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0]
    base, peak = used(), 0
    d = _svils.Batch(g.n, k, 1.0 / k, (1.0, 1.0), **({"sparse": True} if sparse else {}))
    d.set_graph(g.links, g.skip)
    d.set_state(*state)
    out = {}
    for kind in KINDS:
        ms, s = [], steps[kind]
        for r in range(repeats + 1):
            lo, hi = r * chunk, (r + 1) * chunk
            if kind == "node":
                d.step_node(s["nodes"][lo:hi], s["scale"], s["rho_gamma"][lo:hi], s["rho_lambda"][lo:hi])
            elif kind == "pairs":
                d.step_pairs(s["lists"][lo:hi], s["scale"][lo:hi], s["rho_gamma"][lo:hi], s["rho_lambda"][lo:hi])
            elif kind == "star":
                d.step_star(s[lo:hi])
            else:
                d.step_strat(s[lo:hi])
            t = d.timing()[0]
            peak = max(peak, used() - base)
            assert d.stats()[3] == 0
            if r:
                ms.append(t)
        out[kind] = float(np.median(ms)) / chunk
    final = d.state()
    d.close()
    return out, final, peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None, choices=["astroph", "lfr", "gen1e5", "gen1e6"])
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dense-only", action="store_true", help="the side-by-side workloads in dense form alone")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    from svinet_amd import _svils, mmsbgen_sparse
    for name, k, both in (("astroph", 20, True), ("lfr", 28, True), ("gen1e5", 64, False), ("gen1e6", 64, False)):
        if (a.only and name not in a.only) or (a.dense_only and not both):
            continue
        t0 = time.perf_counter()
        rs = np.random.RandomState(7)
        if name == "astroph":
            n, links = golden_links("ca-AstroPh.csv.gz")
        elif name == "lfr":
            n, links = golden_links("LFR-network-n1000-k28.txt.gz")
        else:
            n = 10 ** 5 if name == "gen1e5" else 10 ** 6
            links = unique_pairs(mmsbgen_sparse.generate(n, k), n)
        g = Graph(n, links, rs)
        chunk = a.chunk if n < 500000 else max(2, a.chunk // 4)
        steps = g.draw(rs, chunk * (a.repeats + 1))
        state = (rs.gamma(100.0, 0.01, (n, k)), 1.0 + rs.gamma(100.0, 0.01, (k, 2)))
        out = {"workload": name, "n": n, "k": k, "links": int(len(links)), "skip_pairs": int(len(g.skip)), "variant": list(_svils.batch_variant(k)),
               "chunk": chunk, "repeats": a.repeats, "max_degree": int(np.diff(g.row).max())}
        if a.dense_only:
            out["dense_ms_per_step"], fd, _ = run_form(g, k, False, steps, chunk, a.repeats, state)
        else:
            out["sparse_ms_per_step"], fs, peak = run_form(g, k, True, steps, chunk, a.repeats, state)
            out["sparse_device_bytes_in_use_after_a_chunk"] = int(peak)
        if both and not a.dense_only:
            out["dense_ms_per_step"], fd, _ = run_form(g, k, False, steps, chunk, a.repeats, state)
            out["sparse_over_dense"] = {kind: out["sparse_ms_per_step"][kind] / out["dense_ms_per_step"][kind] for kind in KINDS}
            out["final_states_equal_as_bits"] = bool(fs[0].tobytes() == fd[0].tobytes() and fs[1].tobytes() == fd[1].tobytes())
        out["wall_s"] = time.perf_counter() - t0
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
