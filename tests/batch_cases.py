"""What tests/test_gpu_batch.py and tests/test_batch_device_abi.py share: seeded planted graphs, the start state of the
-batch engine, and a copy of oracle/batch_oracle.py::phis that also records every pair's exit round (the oracle itself
stays as it is)."""
import numpy as np

from oracle import batch_oracle as B


def planted_links(n, blocks, p_in, p_out, seed):
    """links [m][2] uint32, p < q, of a planted-partition graph on n nodes (numpy.random.RandomState(seed)); a ring keeps
    every node linked, so the reader drops none of them"""
    rs = np.random.RandomState(seed)
    group = np.arange(n) * blocks // n
    iu = np.triu_indices(n, 1)
    prob = np.where(group[iu[0]] == group[iu[1]], p_in, p_out)
    keep = rs.random_sample(prob.shape[0]) < prob
    ring = (iu[1] - iu[0] == 1) | ((iu[0] == 0) & (iu[1] == n - 1))
    keep |= ring
    return np.ascontiguousarray(np.stack([iu[0][keep], iu[1][keep]], axis=1).astype(np.uint32))


def write_graph(path, links):
    with open(path, "w") as f:
        for p, q in links:
            f.write("%d\t%d\n" % (p, q))
    return str(path)


def adjacency(n, edges):
    adj = np.zeros((n, n), dtype=np.int64)
    adj[edges[:, 0], edges[:, 1]] = adj[edges[:, 1], edges[:, 0]] = 1
    return adj


def heldout_row(u, y, ones_prob):
    """oracle/batch_oracle.py::heldout_row from per-pair log-likelihoods u (pairs in sorted order)"""
    u, y = np.asarray(u), np.asarray(y)
    m0, m1 = u[y == 0].mean(), u[y == 1].mean()
    z = 1 - ones_prob
    return [u.mean(), len(u), m0, int((y == 0).sum()), m1, int((y == 1).sum()), z * m0, ones_prob * m1, z * m0 + ones_prob * m1]


def phis_rounds(elogpi, elogbeta, p, q, y):
    """B.phis with the number of update rounds every pair ran (its exit round + 1) -> phi1, phi2, rounds"""
    npairs, K = p.shape[0], elogpi.shape[1]
    yk = y[:, None].astype(np.float64)
    elogf = elogbeta[None, :, 0] * yk + elogbeta[None, :, 1] * (1 - yk)
    logeps = np.log(B.EPSILON)
    phi1 = np.full((npairs, K), 1.0 / K)
    phi2 = np.full((npairs, K), 1.0 / K)
    old1 = np.zeros((npairs, K))
    old2 = np.zeros((npairs, K))
    live = np.ones(npairs, dtype=bool)
    rounds = np.zeros(npairs, dtype=np.int64)

    def update(b, c):
        a = np.exp(elogpi[c] + elogf * b + np.where(yk == 1, (1 - b) * logeps, 0.0))
        s = a.sum(1, keepdims=True)
        assert np.all(s > 0)
        return a / s

    for i in range(B.ONLINE_ITERATIONS):
        if i % 2 == 0:
            old1[live] = phi1[live]
            old2[live] = phi2[live]
        n1 = update(phi2, p)
        n2 = update(phi1, q)
        v1 = np.abs(n1 - old1).mean(1)
        v2 = np.abs(n2 - old2).mean(1)
        phi1[live] = n1[live]
        phi2[live] = n2[live]
        rounds[live] = i + 1
        if i % 2 == 0:
            continue
        live &= ~((v1 < B.MEAN_CHANGE_THRESH) & (v2 < B.MEAN_CHANGE_THRESH))
        if not live.any():
            break
    return phi1, phi2, rounds


def sweep_rounds(gamma, lam, adj, skip):
    """the exit rounds of every trained pair of one sweep from (gamma, lambda)"""
    n = gamma.shape[0]
    elogpi, elogbeta = B.dir_exp(gamma), B.dir_exp(lam)
    iu = np.triu_indices(n, 1)
    keep = np.array([(a, b) not in skip for a, b in zip(*iu)])
    p, q = iu[0][keep], iu[1][keep]
    return phis_rounds(elogpi, elogbeta, p, q, adj[p, q])[2]
