"""An INDEPENDENT numpy restatement of `svinet -findk` (FastInit::batch_infer, src/fastinit.cc:240-289) -- TEST
INFRASTRUCTURE.  Written from the reference text, not from svinet_amd/host/findk.cc or svils_findk.hip, with the
arithmetic made different where the result does not depend on it:

  * numpy's MT19937 (legacy seeding = GSL's init_genrand, default seed 4357) instead of host/rng.hh;
  * the count as np.unique over 64-bit (node, label) keys, the top 5 by np.lexsort, instead of per-node sorts / hashes;
  * the 25 slot pairs of edge_likelihood / compute_and_log_groups as whole-array passes (k1 outer, k2 inner, the
    reference's summation order: an unmatched pair adds 0.0, which changes no sum);
  * communities from np.unique over (label, external id) keys instead of membership masks.

Only the padding draws of set_gamma are a Python loop (a data-dependent sequential draw stream).  The held-out sums
are sequential (np.cumsum), the reference's order.

    python tools/restate_findk.py <edge list> <n> <k> <outdir> [-link-thresh t] [-heldout-ratio r]
"""
import os
import sys
import time

import numpy as np

S = 5
SENTINEL = 65535


class Mt:
    """gsl_rng_default = mt19937 with the default seed (FastInit never calls gsl_rng_set)"""

    def __init__(self):
        self.bg = np.random.MT19937()
        self.bg._legacy_seeding(4357)

    def raw(self, m=None):
        return self.bg.random_raw(m)

    def uniform(self, m):                      # gsl_rng_uniform: get() / 2^32
        return self.raw(m).astype(np.float64) / 4294967296.0

    def uniform_int(self, n):                  # gsl_rng_uniform_int: scale = 0xffffffff / n, redrawn while k >= n
        scale = 0xFFFFFFFF // n
        while True:
            k = int(self.raw()) // scale
            if k < n:
                return k


def read_graph(path, n):
    """Network::read (src/network.cc:10-116) for files that name at most n ids: sequence ids by first appearance (first
    column before second), self pairs and repeated pairs dropped.  Returns links [E][2] (p < q, file order) and seq2id."""
    raw = np.loadtxt(path, dtype=np.int64, ndmin=2, usecols=(0, 1)) if os.path.getsize(path) < (1 << 20) else \
        np.fromstring(open(path).read(), dtype=np.int64, sep=" ").reshape(-1, 2)
    flat = raw.reshape(-1)
    ids, first = np.unique(flat, return_index=True)
    if len(ids) > n:
        raise ValueError("the file names %d ids, more than n = %d (not restated)" % (len(ids), n))
    order = np.argsort(first, kind="stable")
    seq2id = ids[order]
    seq_of = np.empty(len(ids), np.int64)
    seq_of[order] = np.arange(len(ids))
    pq = seq_of[np.searchsorted(ids, flat)].reshape(-1, 2)
    lo, hi = np.minimum(pq[:, 0], pq[:, 1]), np.maximum(pq[:, 0], pq[:, 1])
    keep = lo != hi
    key = (lo << 32) | hi
    _, firstk = np.unique(key[keep], return_index=True)
    rows = np.nonzero(keep)[0][np.sort(firstk)]
    return np.stack([lo[rows], hi[rows]], axis=1), seq2id


def heldout_sample(edges, n, ratio, r, accuracy=False):
    """init_heldout / set_heldout_sample / get_random_edge (src/fastinit.cc:467-508, fastinit.hh:478-512): the pairs
    {(p, q): y} in the std::map's (p, q) order"""
    E = len(edges)
    eset = set(map(tuple, edges.tolist()))
    s = int(ratio * E)
    half = s // 2
    hmap = {}
    c0 = c1 = 0
    if not accuracy:
        while c0 < half or c1 < half:
            if c0 == half:
                while True:
                    e = tuple(edges[r.uniform_int(E)].tolist())
                    if e not in hmap:
                        break
            else:
                while True:
                    a, b = r.uniform_int(n), r.uniform_int(n)
                    e = (a, b) if a < b else (b, a)
                    if a != b and e not in hmap:
                        break
            y = 1 if e in eset else 0
            if y == 0 and c0 < half:
                c0 += 1
                hmap[e] = 0
            if y == 1 and c1 < half:
                c1 += 1
                hmap[e] = 1
    keys = sorted(hmap)
    return np.array([(p, q, hmap[(p, q)]) for p, q in keys], dtype=np.int64).reshape(-1, 3)


def count_top(n, src, lab):
    """the count of one iteration (src/fastinit.cc:258-271) and set_gamma's order (:213-220): per node the distinct
    labels sorted by count descending, ties by ascending label (the stable qsort over the std::map's order).
    Returns top labels [n][5] (-1 past the distinct ones), their counts, and the distinct count per node."""
    key = (src.astype(np.int64) << 32) | lab.astype(np.int64)
    uk, cnt = np.unique(key, return_counts=True)
    node, label = uk >> 32, uk & 0xFFFFFFFF
    o = np.lexsort((label, -cnt, node))
    node, label, cnt = node[o], label[o], cnt[o]
    d = np.bincount(node, minlength=n)
    start = np.concatenate([[0], np.cumsum(d)[:-1]])
    rank = np.arange(len(node)) - start[node]
    top_lab = np.full((n, S), -1, np.int64)
    top_cnt = np.zeros((n, S), np.int64)
    m = rank < S
    top_lab[node[m], rank[m]] = label[m]
    top_cnt[node[m], rank[m]] = cnt[m]
    return top_lab, top_cnt, d


def set_gamma(labels, values, top_lab, top_cnt, d, alpha, draw_int, n):
    """set_gamma (:200-236): nodes without a count keep their slots; otherwise counted slots (label, count + alpha), then
    pads (5 - d of them, in draw order) with value 2 alpha, drawn in node order by draw_int(n), redrawn when the draw is
    one of the node's counted labels (earlier pads are not checked: duplicates stay)"""
    labels, values = labels.copy(), values.copy()
    has = d > 0
    full = np.minimum(d, S)
    for j in range(S):
        m = has & (j < full)
        labels[m, j] = top_lab[m, j]
        values[m, j] = top_cnt[m, j].astype(np.float64) + alpha
    for i in np.nonzero(has & (d < S))[0].tolist():
        counted = set(top_lab[i, :d[i]].tolist())
        for j in range(int(d[i]), S):
            while True:
                k = draw_int(n)
                if k not in counted:
                    break
            labels[i, j] = k
            values[i, j] = alpha + alpha
    return labels, values


def estimate_pi(values, n, alpha):
    """estimate_all_pi (src/fastinit.hh:460-476): (n - 5) in uint32 arithmetic"""
    s = values[:, 0] + values[:, 1] + values[:, 2] + values[:, 3] + values[:, 4]
    s = s + float((n - S) & 0xFFFFFFFF) * alpha
    return values / s[:, None]


def edge_ll(labels, pi, p, q, y):
    """edge_likelihood (src/fastinit.cc:416-446) of pairs p[m], q[m] with y[m]"""
    Lp, Lq, Pp, Pq = labels[p], labels[q], pi[p], pi[q]
    s = np.zeros(len(p))
    one = y == 1
    for k1 in range(S):
        for k2 in range(S):
            eq = Lp[:, k1] == Lq[:, k2]
            s += np.where(eq == one, Pp[:, k1] * Pq[:, k2], 0.0)
    return np.log(np.maximum(s, 1e-30))


def groups(labels, pi, edges, link_thresh):
    """compute_and_log_groups (src/fastinit.cc:291-414) over both directions of every link: (unlikely count,
    [(label, sequence id)] memberships as a sorted unique int64 key array label << 32 | node)"""
    i = np.concatenate([edges[:, 0], edges[:, 1]])
    m = np.concatenate([edges[:, 1], edges[:, 0]])
    Li, Lm, Pi, Pm = labels[i], labels[m], pi[i], pi[m]
    mx = np.zeros(len(i))
    sm = np.zeros(len(i))
    max_k = np.full(len(i), SENTINEL, np.int64)
    for k1 in range(S):
        for k2 in range(S):
            eq = Li[:, k1] == Lm[:, k2]
            u = np.where(eq, Pi[:, k1] * Pm[:, k2], 0.0)
            sm += u
            better = eq & (u > mx)
            mx = np.where(better, u, mx)
            max_k = np.where(better, Li[:, k1], max_k)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(sm > 0, mx / np.where(sm > 0, sm, 1.0), 0.0)
    bad = ratio < link_thresh
    ok = ~bad & (max_k != SENTINEL)
    mem = np.unique(np.concatenate([(max_k[ok] << 32) | i[ok], (max_k[ok] << 32) | m[ok]]))
    return int(bad.sum()), mem


def fmt9(v):
    """printf("%.9f") as glibc writes it; the only NaN here is 0 / 0 of an empty held-out set, whose sign bit x86 sets"""
    if np.isnan(v):
        return "-nan"
    return "%.9f" % v


class FindK:
    def __init__(self, edges, seq2id, n, k, heldout_ratio=0.01, link_thresh=0.5, accuracy=False):
        self.edges, self.seq2id, self.n = edges, seq2id, n
        self.alpha = 1.0 / k
        self.link_thresh = link_thresh
        E = len(edges)
        total_pairs = ((n * (n - 1)) & 0xFFFFFFFF) // 2                 # uint32 product, src/fastinit.cc:41-45
        self.ones_prob = E / total_pairs
        self.zeros_prob = 1.0 - self.ones_prob
        self.r = Mt()
        u = self.r.uniform(S * n).reshape(n, S)                          # init_gamma, :178-190
        self.labels = (np.arange(n)[:, None] + np.arange(S)[None, :]) % n
        self.values = u.copy()
        self.values[:, 0] = 1.0 + u[:, 0]
        self.held = heldout_sample(edges, n, heldout_ratio, self.r, accuracy)
        hkey = set((p << 32) | q for p, q, y in self.held.tolist() if y == 1)
        ekey = (edges[:, 0] << 32) | edges[:, 1]
        self.train = ~np.isin(ekey, np.array(sorted(hkey), dtype=np.int64)) if hkey else np.ones(E, bool)
        self.iter = 0
        self.prev_h = self.max_h = -2147483647.0
        self.nh = 0
        self.rows, self.communities, self.sizes, self.unlikely, self.training_ll = [], [], [], [], []
        self.pad_seconds = []

    def step(self):
        """0: an iteration with groups, 1: the stop rule fired, 2: the loop is over"""
        n = self.n
        if self.iter > np.log10(n):
            return 2
        tr = self.edges[self.train]
        maxg = self.labels[:, 0]
        src = np.concatenate([tr[:, 0], tr[:, 1]])
        lab = np.concatenate([maxg[tr[:, 1]], maxg[tr[:, 0]]])
        top_lab, top_cnt, d = count_top(n, src, lab)
        t0 = time.perf_counter()
        self.labels, self.values = set_gamma(self.labels, self.values, top_lab, top_cnt, d, self.alpha, self.r.uniform_int, n)
        self.pad_seconds.append(time.perf_counter() - t0)
        self.pi = estimate_pi(self.values, n, self.alpha)
        one = np.ones(len(self.edges), np.int64)
        self.training_ll.append(float(np.mean(edge_ll(self.labels, self.pi, self.edges[:, 0], self.edges[:, 1], one))))
        self.iter += 1
        if self.heldout_row():
            return 1
        bad, mem = groups(self.labels, self.pi, self.edges, self.link_thresh)
        self.unlikely.append(bad)
        lab_of, node = mem >> 32, mem & 0xFFFFFFFF
        key = np.unique((lab_of << 32) | self.seq2id[node])     # ids ascending within each label
        lab_of, ids = key >> 32, key & 0xFFFFFFFF
        cuts = np.nonzero(np.diff(lab_of))[0] + 1
        comm, size = [], []
        for L, part in zip(lab_of[np.concatenate([[0], cuts])] if len(key) else [], np.split(ids, cuts) if len(key) else []):
            comm.append("".join("%d " % v for v in part.tolist()) + "\n")
            size.append("%d\t%d\n" % (L, len(part)))
        self.communities.append("".join(comm))
        self.sizes.append("".join(size))
        return 0

    def heldout_row(self):
        """heldout_likelihood (:511-567): the row and the stop rule (True: stop)"""
        h = self.held
        k = len(h)
        u = edge_ll(self.labels, self.pi, h[:, 0], h[:, 1], h[:, 2]) if k else np.zeros(0)
        y = h[:, 2] if k else np.zeros(0, np.int64)
        seq = lambda v: float(np.cumsum(v)[-1]) if len(v) else 0.0
        s, sz, so = seq(u), seq(u[y == 0]), seq(u[y == 1])
        kz, ko = int((y == 0).sum()), int((y == 1).sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            div = lambda a, b: np.float64(a) / np.float64(b)
            z, o = self.zeros_prob * div(sz, kz), self.ones_prob * div(so, ko)
            a = z + o
            self.rows.append((self.iter, div(s, k), k, div(sz, kz), kz, div(so, ko), ko, z, o, a))
        stop = False
        if a > self.prev_h and self.prev_h != 0 and abs((a - self.prev_h) / self.prev_h) < 0.00001:
            stop = True
        elif a < self.prev_h:
            self.nh += 1
        elif a > self.prev_h:
            self.nh = 0
        self.max_h = max(self.max_h, a) if not np.isnan(a) else self.max_h
        if self.nh > 10:
            stop = True
        self.prev_h = a
        return stop

    def run(self):
        while self.step() == 0:
            pass
        return self

    def heldout_text(self, seconds=0):
        out = []
        for r in self.rows:
            it, sk, k, szk, kz, sok, ko, z, o, a = r
            out.append("%d\t%d\t%s\t%d\t%s\t%d\t%s\t%d\t%s\t%s\t%s\n" % (it, seconds, fmt9(sk), k, fmt9(szk), kz, fmt9(sok), ko,
                                                                         fmt9(z), fmt9(o), fmt9(a)))
        return "".join(out)

    def write(self, outdir):
        os.makedirs(outdir, exist_ok=True)
        files = {"heldout.txt": self.heldout_text(), "uncolored-links.txt": "".join("%d\n" % u for u in self.unlikely),
                 "communities.txt": self.communities[-1] if self.communities else None,
                 "communities_size.txt": self.sizes[-1] if self.sizes else None}
        for name, text in files.items():
            if text is not None:
                with open(os.path.join(outdir, name), "w") as f:
                    f.write(text)


def main(argv):
    path, n, k, outdir = argv[1], int(argv[2]), int(argv[3]), argv[4]
    kw = {}
    if "-link-thresh" in argv:
        kw["link_thresh"] = float(argv[argv.index("-link-thresh") + 1])
    if "-heldout-ratio" in argv:
        kw["heldout_ratio"] = float(argv[argv.index("-heldout-ratio") + 1])
    t0 = time.perf_counter()
    edges, seq2id = read_graph(path, n)
    n = len(seq2id)
    fk = FindK(edges, seq2id, n, k, **kw).run()
    fk.write(outdir)
    print("restate_findk: n=%d links=%d iterations=%d communities=%d in %.2f s" %
          (n, len(edges), fk.iter, fk.communities[-1].count("\n") if fk.communities else 0, time.perf_counter() - t0))


if __name__ == "__main__":
    main(sys.argv)
