"""What tests/test_sampled.py and tests/test_gpu_sampled.py share: a numpy restatement of ONE sampled-pair step of the
reference's MMSBInfer::infer (src/mmsbinfer.cc:513-642, process() :1092-1190), on top of oracle/batch_oracle.py (dir_exp,
phis -- imported, the oracle stays as it is) and batch_cases.phis_rounds; the step sizes; and the guard that makes the
round counters comparable."""
import numpy as np

import batch_cases as BC
from oracle import batch_oracle as B

TAU0, KAPPA, NODETAU0, NODEKAPPA = 1024.0, 0.9, 1024.0, 0.5   # src/env.hh:405-408


def rho_gamma(c, nodetau0=NODETAU0, nodekappa=NODEKAPPA):
    """:584 with :18 -- c the iteration count"""
    return (nodetau0 + 1 + c / 100.0) ** (-nodekappa)


def rho_lambda(it, lambda_start_iter, tau0=TAU0, kappa=KAPPA):
    """:622"""
    return (tau0 + 1 + it - lambda_start_iter + 1) ** (-kappa)


def node_pairs(n, a, skip):
    """get_randomnode_edges (:1867-1876): every pair (a, j), j != a, outside the skip set -> p, q (p < q)"""
    js = [j for j in range(n) if j != a and (min(a, j), max(a, j)) not in skip]
    p = np.array([min(a, j) for j in js], dtype=np.int64)
    q = np.array([max(a, j) for j in js], dtype=np.int64)
    return p, q


def step(gamma, lam, adj, p, q, alpha, eta, scale, rho_g, rho_l):
    """one step from (gamma, lambda) on the mini-batch (p[i], q[i]) -> new gamma, new lambda, the rounds of every pair.
    rho_l < 0: lambda is returned as it came (the delayed learning of :613)"""
    n, K = gamma.shape
    p, q = np.asarray(p, dtype=np.int64), np.asarray(q, dtype=np.int64)
    gammat, lambdat = np.zeros((n, K)), np.zeros((K, 2))
    rounds = np.zeros(0, dtype=np.int64)
    if len(p):
        y = adj[p, q]
        elogpi, elogbeta = B.dir_exp(gamma), B.dir_exp(lam)
        phi1, phi2, rounds = BC.phis_rounds(elogpi, elogbeta, p, q, y)
        check1, check2 = B.phis(elogpi, elogbeta, p, q, y)
        assert np.array_equal(check1, phi1) and np.array_equal(check2, phi2)
        np.add.at(gammat, p, phi1)
        np.add.at(gammat, q, phi2)
        pp = phi1 * phi2
        lambdat[:, 0] = (pp * (y[:, None] == 1)).sum(0)
        lambdat[:, 1] = (pp * (y[:, None] == 0)).sum(0)
    g = (1 - rho_g) * gamma + rho_g * (alpha + scale * gammat)
    if rho_l < 0:
        return g, lam.copy(), rounds
    l = (1 - rho_l) * lam + rho_l * (np.asarray(eta, dtype=np.float64)[None, :] + scale * lambdat)
    return g, l, rounds


def exit_margins(gamma, lam, adj, p, q):
    """for every pair the mean changes (both sides) at its exit test and at the last test it failed: [npairs][4], NaN where
    there is no such test (a pair that left at its first test failed none; one that ran into the cap passed none)"""
    p, q = np.asarray(p, dtype=np.int64), np.asarray(q, dtype=np.int64)
    elogpi, elogbeta = B.dir_exp(gamma), B.dir_exp(lam)
    y = adj[p, q]
    npairs, K = p.shape[0], elogpi.shape[1]
    yk = y[:, None].astype(np.float64)
    elogf = elogbeta[None, :, 0] * yk + elogbeta[None, :, 1] * (1 - yk)
    logeps = np.log(B.EPSILON)
    phi1 = np.full((npairs, K), 1.0 / K)
    phi2 = np.full((npairs, K), 1.0 / K)
    old1, old2 = np.zeros((npairs, K)), np.zeros((npairs, K))
    live = np.ones(npairs, dtype=bool)
    out = np.full((npairs, 4), np.nan)

    def update(b, c):
        a = np.exp(elogpi[c] + elogf * b + np.where(yk == 1, (1 - b) * logeps, 0.0))
        return a / a.sum(1, keepdims=True)

    for i in range(B.ONLINE_ITERATIONS):
        if i % 2 == 0:
            old1[live], old2[live] = phi1[live], phi2[live]
        n1, n2 = update(phi2, p), update(phi1, q)
        v1, v2 = np.abs(n1 - old1).mean(1), np.abs(n2 - old2).mean(1)
        phi1[live], phi2[live] = n1[live], n2[live]
        if i % 2 == 0:
            continue
        leave = live & (v1 < B.MEAN_CHANGE_THRESH) & (v2 < B.MEAN_CHANGE_THRESH)
        stay = live & ~leave
        out[leave, 0], out[leave, 1] = v1[leave], v2[leave]
        out[stay, 2], out[stay, 3] = v1[stay], v2[stay]
        live = stay
        if not live.any():
            break
    return out


def assert_exits_are_clear(gamma, lam, adj, p, q):
    """no mean change at a pair's exit test, nor at the last test it failed, within a relative 1e-4 of the threshold: the
    tolerance of the comparisons admits input differences of 1e-7, which then cannot move an exit by a round"""
    if not len(p):
        return
    m = exit_margins(gamma, lam, adj, p, q)
    rel = np.abs(m - B.MEAN_CHANGE_THRESH) / B.MEAN_CHANGE_THRESH
    assert not np.any(rel <= 1e-4), "a pair's exit test is within 1e-4 of the threshold: pick another seed"
