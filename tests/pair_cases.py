"""Helpers the -m gpu tests of the pair queries share (test infrastructure): test_gpu_predict.py, test_gpu_rank.py and
test_gpu_nbr.py.  Graphs are links [E][2] (p < q, sorted), states gamma [n][k] and lam [k][2]; everything random is drawn
from the caller's generator, so a test's seed fixes its case."""
import numpy as np

NONE = 0xFFFFFFFF


def _pb(gamma, lam):
    return gamma / gamma.sum(1, keepdims=True), lam[:, 0] / (lam[:, 0] + lam[:, 1])


def _nbrs(n, links):
    nb = [[] for _ in range(n)]
    for p, q in np.asarray(links).tolist():
        nb[p].append(q)
        nb[q].append(p)
    return [np.array(sorted(set(x)), dtype=np.int64) for x in nb]


def _random_links(rng, n, m):
    """the first m of the distinct links drawn, in sorted order (test_gpu_nbr.py has its own: a random m of them)"""
    a = rng.integers(0, n, size=3 * m)
    b = rng.integers(0, n, size=3 * m)
    e = np.stack([np.minimum(a, b), np.maximum(a, b)], 1)
    e = e[e[:, 0] != e[:, 1]]
    e = np.unique(e, axis=0)[:m]
    return np.ascontiguousarray(e[np.lexsort((e[:, 1], e[:, 0]))], dtype=np.uint32)


def _random_pairs(rng, n, m):
    p = rng.integers(0, n, size=m)
    q = (p + 1 + rng.integers(0, n - 1, size=m)) % n
    return np.stack([p, q], 1).astype(np.uint32)


def _lfr_setup(graph_files, k=28):
    from svinet_amd.host_api import Setup
    return Setup(graph_files["lfr"], 1000, k)


def _state_bits(eng):
    g, lam, conv = eng.state()
    c = eng.control()
    ctl = (c.iter, c.annealing, c.write_comm, c.nh, c.prev_h, c.max_h, c.stopped, c.why, c.sweeps_done, c.rows)
    return g.view(np.uint64).copy(), lam.view(np.uint64).copy(), conv, eng.rows().view(np.uint64).copy(), ctl


def _same(a, b):
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def _bits(res):
    return [np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else x.dtype).copy() for x in res]
