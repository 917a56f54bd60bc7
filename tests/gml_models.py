"""Models and graphs for the -gml / -lcstats tests (test infrastructure): links [E][2] (p < q), gamma [n][k], lam [k][2]."""
import numpy as np


def _unique_links(p, q):
    lo, hi = np.minimum(p, q), np.maximum(p, q)
    keep = lo != hi
    key = np.unique((lo[keep].astype(np.int64) << 32) | hi[keep])
    return np.stack([key >> 32, key & 0xFFFFFFFF], axis=1)


def near_threshold(K, count, seed=0, uniform=8):
    """`count` nodes whose rows put max(pi) / sum(pi) within a few ulps of 0.5 (even nodes) or 0.9 (odd nodes), each linked
    to one of `uniform` nodes with a flat row at the end.  K is a power of two and beta = 1, so every x_k of a link is
    pi_p[k] / K exactly and the link's ratio is the row's own."""
    assert K & (K - 1) == 0
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.5, 1.5, size=(count, K - 1))
    s = np.zeros(count)
    for c in range(K - 1):
        s = s + r[:, c]
    t = np.where(np.arange(count) % 2 == 0, 0.5, 0.9)
    a = s * (t / (1 - t)) * (1 + rng.integers(-8, 9, size=count) * 2.0 ** -52)
    gamma = np.vstack([np.hstack([a[:, None], r]), np.ones((uniform, K))])
    links = np.stack([np.arange(count), count + np.arange(count) % uniform], axis=1)
    lam = np.tile([1.0, 0.0], (K, 1))
    return links, gamma, lam


def mixed(K=8, seed=1):
    """near-threshold links on the lower half of the columns, plus ties in x and in pi, links with x = 0 everywhere (a NaN
    ratio) and empty communities (the upper half carries no mass)"""
    h = K // 2
    links, g0, lam0 = near_threshold(h, 2000, seed)
    gamma = np.hstack([g0, np.zeros((g0.shape[0], K - h))])
    n = gamma.shape[0]
    tie = np.zeros((40, K))
    tie[:, :h] = 1.0
    tie[:, 1] = tie[:, 2] = 5.0                    # two equal maxima
    only = np.zeros((40, K))
    only[np.arange(40), np.arange(40) % h] = 1.0   # one column each: pairs on different columns have x = 0
    gamma = np.vstack([gamma, tie, only])
    a = n + np.arange(40)
    b = n + 40 + np.arange(40)
    extra = np.concatenate([np.stack([a, b], axis=1), np.stack([b[:-1], b[1:]], axis=1), np.stack([a[:-1], a[1:]], axis=1)])
    lam = np.vstack([lam0, np.tile([2.0, 3.0], (K - h, 1))])
    return np.vstack([links, extra]), gamma, lam


def random_model(n, K, E, seed=2):
    rng = np.random.default_rng(seed)
    links = _unique_links(rng.integers(0, n, E), rng.integers(0, n, E))
    used = np.zeros(n, bool)
    used[links.reshape(-1)] = True
    remap = np.cumsum(used) - 1                    # every node has a link (the reader's n counts no singletons)
    links = remap[links]
    n = int(used.sum())
    gamma = rng.gamma(0.2, 1.0, size=(n, K)) + 1e-3
    lam = np.stack([rng.uniform(0.5, 50, K), rng.uniform(0.5, 50, K)], axis=1)
    return links, gamma, lam


def hub_model(n_leaf=30000, K=16, seed=4):
    """node 0 linked to every leaf, the leaves in a ring of pairs"""
    rng = np.random.default_rng(seed)
    hub = np.stack([np.zeros(n_leaf, np.int64), np.arange(1, n_leaf + 1)], axis=1)
    ring = np.stack([np.arange(1, n_leaf, 2), np.arange(2, n_leaf + 1, 2)], axis=1)
    gamma = rng.gamma(0.3, 1.0, size=(n_leaf + 1, K)) + 1e-4
    gamma[0] = 1.0
    lam = np.stack([rng.uniform(1, 20, K), rng.uniform(1, 20, K)], axis=1)
    return np.vstack([hub, ring]), gamma, lam


def write_model(d, gamma, lam, seq2id):
    """gamma.txt / lambda.txt as the fit writes them ("%d\\t%d" then "%.5f" columns; "%d" then "%.5f" columns)"""
    import os
    with open(os.path.join(d, "gamma.txt"), "w") as f:
        for i in range(gamma.shape[0]):
            f.write("%d\t%d\t" % (i, seq2id[i]) + "\t".join("%.5f" % v for v in gamma[i]) + "\n")
    with open(os.path.join(d, "lambda.txt"), "w") as f:
        for k in range(lam.shape[0]):
            f.write("%d\t%.5f\t%.5f\n" % (k, lam[k, 0], lam[k, 1]))
