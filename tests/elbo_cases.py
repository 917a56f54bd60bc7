"""What tests/test_elbo.py and tests/test_gpu_elbo.py share: an independent numpy restatement of the reference's
approx_log_likelihood (src/mmsbinfer.cc:1948-2056), s = G + P + N, on top of oracle/batch_oracle.py (dir_exp),
batch_cases.phis_rounds (the fixed point, with every pair's round count) and scipy's gammaln; a second, literal
scalar-loop version with the g != h double loop for tiny n; and the conditions a test state has to meet.

One departure from the reference, the engines' own: an entry of phi that has underflowed to exactly 0 adds 0 to the
entropy terms (log(phi) * phi is NaN there)."""
import math

import numpy as np
from scipy.special import gammaln

import batch_cases as BC
import sampled_cases as SC
from oracle import batch_oracle as B

RTOL = 1e-9   # the bound the project holds its likelihood rows to on the HIP path


def trained_pairs(n, skip):
    iu = np.triu_indices(n, 1)
    keep = np.array([(int(a), int(b)) not in skip for a, b in zip(*iu)], dtype=bool)
    return iu[0][keep], iu[1][keep]


def _xlogx(p):
    out = np.zeros_like(p)
    pos = p > 0
    out[pos] = p[pos] * np.log(p[pos])
    return out


class Elbo:
    """the restated lower bound of a state: G, P, N, total, the round count of every trained pair, and what
    check_conditions looks at (the per-pair and per-node terms, phi)"""

    def __init__(self, gamma, lam, adj, skip, alpha, eta, epsilon=B.EPSILON):
        gamma, lam = np.asarray(gamma, dtype=np.float64), np.asarray(lam, dtype=np.float64)
        n, K = gamma.shape
        elogpi, elogbeta = B.dir_exp(gamma), B.dir_exp(lam)
        eta = np.asarray(eta, dtype=np.float64)
        # G (:1962-1982)
        g = gammaln(eta.sum()) - gammaln(eta).sum() + ((eta - 1)[None, :] * elogbeta).sum(1)
        g = g - (gammaln(lam.sum(1)) - gammaln(lam).sum(1)) - ((lam - 1) * elogbeta).sum(1)
        self.g_terms = g
        self.G = float(g.sum())
        # P (:1984-2029)
        self.p, self.q = trained_pairs(n, skip)
        y = adj[self.p, self.q]
        assert epsilon == B.EPSILON
        phi1, phi2, self.rounds = BC.phis_rounds(elogpi, elogbeta, self.p, self.q, y)   # (asserts every normaliser > 0)
        yk = y[:, None].astype(np.float64)
        elogf = elogbeta[None, :, 0] * yk + elogbeta[None, :, 1] * (1 - yk)
        pp = phi1 * phi2
        t = (pp * elogf).sum(1)
        t = t + np.where(y == 1, math.log(epsilon) * (phi1.sum(1) * phi2.sum(1) - pp.sum(1)), 0.0)
        t = t + (phi1 * elogpi[self.p]).sum(1) + (phi2 * elogpi[self.q]).sum(1)
        t = t - _xlogx(phi1).sum(1) - _xlogx(phi2).sum(1)
        self.pair_terms = t
        self.P = float(t.sum())
        self.phi_min = float(min(phi1.min(), phi2.min())) if len(t) else 1.0
        # N (:2031-2056)
        alpha = float(alpha)
        nt = gammaln(K * alpha) - K * gammaln(alpha) + (alpha - 1) * elogpi.sum(1)
        nt = nt - (gammaln(gamma.sum(1)) - gammaln(np.maximum(gamma, 1e-30)).sum(1)) - ((gamma - 1) * elogpi).sum(1)
        self.node_terms = nt
        self.N = float(nt.sum())
        self.total = self.G + self.P + self.N
        self.parts = np.array([self.total, self.G, self.P, self.N])
        self.rounds_total = int(self.rounds.sum())
        self._state = (gamma, lam, adj)

    def assert_exits_are_clear(self):
        gamma, lam, adj = self._state
        SC.assert_exits_are_clear(gamma, lam, adj, self.p, self.q)


def literal(gamma, lam, adj, skip, alpha, eta, epsilon=B.EPSILON):
    """the reference's loops one scalar at a time (tiny n only) -> G, P, N"""
    gamma, lam = np.asarray(gamma, dtype=np.float64), np.asarray(lam, dtype=np.float64)
    n, K = gamma.shape
    elogpi, elogbeta = B.dir_exp(gamma), B.dir_exp(lam)
    logeps = math.log(epsilon)
    G = 0.0
    for k in range(K):
        G += math.lgamma(eta[0] + eta[1]) - (math.lgamma(eta[0]) + math.lgamma(eta[1]))
        G += sum((eta[t] - 1) * elogbeta[k, t] for t in range(2))
        G -= math.lgamma(lam[k, 0] + lam[k, 1]) - (math.lgamma(lam[k, 0]) + math.lgamma(lam[k, 1]))
        G -= sum((lam[k, t] - 1) * elogbeta[k, t] for t in range(2))
    P = 0.0
    for p in range(n):
        for q in range(p + 1, n):
            if (p, q) in skip:
                continue
            y = int(adj[p, q])
            phi1, phi2 = B.phis(elogpi, elogbeta, np.array([p]), np.array([q]), np.array([y]))
            phi1, phi2 = phi1[0], phi2[0]
            for k in range(K):
                P += phi1[k] * phi2[k] * (elogbeta[k, 0] * y + elogbeta[k, 1] * (1 - y))
            if y == 1:
                for g in range(K):
                    for h in range(K):
                        if g != h:
                            P += phi1[g] * phi2[h] * logeps
            for k in range(K):
                P += phi1[k] * elogpi[p, k]
                P += phi2[k] * elogpi[q, k]
            for k in range(K):
                if phi1[k] > 0:
                    P -= math.log(phi1[k]) * phi1[k]
                if phi2[k] > 0:
                    P -= math.log(phi2[k]) * phi2[k]
    N = 0.0
    for p in range(n):
        N += math.lgamma(K * alpha) - K * math.lgamma(alpha)
        N += sum((alpha - 1) * elogpi[p, k] for k in range(K))
        N -= math.lgamma(gamma[p].sum()) - sum(math.lgamma(max(gamma[p, k], 1e-30)) for k in range(K))
        N -= sum((gamma[p, k] - 1) * elogpi[p, k] for k in range(K))
    return G, P, N


def graph_case(n, seed):
    """links [m][2] and the skip set of a test graph on n nodes: two planted blocks; node 5 without a link and node 7 with
    every pair skipped (n > 8); skipped pairs at rows and columns 63 / 64 (n > 64), else at the last rows and columns"""
    if n == 3:
        return np.array([(0, 1)], dtype=np.uint32), {(0, 2)}
    links = BC.planted_links(n, 2, 0.5, 0.08, seed)
    links = links[(links[:, 0] != 5) & (links[:, 1] != 5)]
    skip = {(min(i, 7), max(i, 7)) for i in range(n) if i != 7}
    hi = 64 if n > 65 else n - 2
    skip |= {(hi - 1, hi), (hi - 2, hi - 1), (10, hi - 1), (10, hi), (hi - 1, hi + 1), (hi, hi + 1), (0, 1), (0, n - 1)}
    assert all(0 <= a < b < n for a, b in skip)
    return np.ascontiguousarray(links), skip


def state_case(n, k, kind, adj, skip, seed, sweeps=2):
    """gamma [n][k], lambda [k][2] of a test state.  "plain": a Gamma(100, 0.01) start after two sweeps of the oracle;
    "peaked": gamma = Gamma(0.3, 1) + 0.02 and a lambda that favours links inside a community; "zeros": gamma entries of
    1e-3 beside entries of 50, which drives some phi to exactly 0 while every normaliser stays > 0"""
    rs = np.random.RandomState(seed)
    if kind == "plain":
        gamma, lam = rs.gamma(100.0, 0.01, size=(n, k)), np.tile([1.0, 1.0], (k, 1))
        for _ in range(sweeps):
            gamma, lam = B.sweep(gamma, lam, adj, skip, 1.0 / k, (1.0, 1.0))
        if n > 8:
            gamma[7] = rs.gamma(100.0, 0.01, size=k)   # (a sweep leaves the node whose pairs are all skipped at the prior: term 0)
        else:
            lam = lam + rs.gamma(2.0, 1.0, size=(k, 2))   # (two or three pairs leave lambda at eta: G would be rounding noise)
        return gamma, lam
    lam = np.stack([rs.gamma(2.0, 1.0, size=k) + 0.5, rs.gamma(6.0, 1.0, size=k) + 0.5], axis=1)
    if kind == "peaked":
        return rs.gamma(0.3, 1.0, size=(n, k)) + 0.02, lam
    assert kind == "zeros"
    gamma = np.where(rs.random_sample((n, k)) < 0.5, 1e-3, 50.0)
    gamma[:, 0] = 50.0
    return gamma, lam


# cases whose first seed gives fewer than three distinct exit rounds, or an exit test within 1e-4 of the threshold
# (check_conditions / assert_exits_are_clear, in numpy): the seed is stepped this many times
SEED_STEPS = {(37, 256, "plain"): 1, (96, 9, "plain"): 1, (96, 17, "plain"): 1, (96, 17, "peaked"): 2, (96, 65, "peaked"): 1,
              (96, 128, "peaked"): 1}
_graphs = {}


def case(n, k, kind):
    """links, skip set, adjacency, gamma, lambda of the test case (n, k, kind); alpha = 1 / k, eta = (1, 1)"""
    if n not in _graphs:
        links, skip = graph_case(n, 500 + n)
        _graphs[n] = links, skip, BC.adjacency(n, links)
    links, skip, adj = _graphs[n]
    gamma, lam = state_case(n, k, kind, adj, skip, 1000 * n + k + 7919 * SEED_STEPS.get((n, k, kind), 0))
    return links, skip, adj, gamma, lam


def check_conditions(e, exact_zeros=False, min_exit_rounds=3):
    """from the restatement alone: the state exercises what the tests are about.  Pairs leave at >= 3 distinct rounds (a
    state with fewer trained pairs than that cannot: min_exit_rounds); every normaliser is > 0 (phis_rounds asserted it);
    every pair term and every node term is < 0 and G < -1e-4, so that G, P and N cannot cancel and none of them is the
    rounding noise of its summands; every phi entry is > 0, except in the
    state built for exact zeros, which must hold some"""
    assert len(np.unique(e.rounds)) >= min_exit_rounds, np.unique(e.rounds)
    assert np.all(np.isfinite(e.pair_terms)) and np.all(e.pair_terms < 0), e.pair_terms.max()
    assert np.all(np.isfinite(e.node_terms)) and np.all(e.node_terms < 0), e.node_terms.max()
    assert e.G < -1e-4, e.G   # (K <= 256 terms with summands of order 1 round at 1e-13: below 1e-9 of a G this far from 0)
    if exact_zeros:
        assert e.phi_min == 0.0
    else:
        assert e.phi_min > 0.0


def assert_parts(got, e, rtol=RTOL):
    """total, G, P, N each within rtol of the restatement"""
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)), got
    np.testing.assert_allclose(got, e.parts, rtol=rtol, atol=0)
