"""What tests/test_orig_elbo.py and tests/test_gpu_orig_elbo.py share: a numpy restatement of the lower bound of -orig
(the reference's MMSBInferOrig::approx_log_likelihood, src/mmsbinferorig.cc:624-726, of the CURRENT
state over the pairs a sweep visits), on orig_cases.fixed_point / dir_exp and scipy.special.gammaln, a literal scalar-loop
form of the same sums, and the conditions a test state must meet.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np
from scipy.special import gammaln

import orig_cases as OC

EPS = 1e-10   # log(fd[g][h] + 1e-10) (:654)


def xlogx(v):
    """v log v with 0 log 0 = 0 (the reference's log(phi) * phi is NaN at an exact 0)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(v > 0, v * np.log(np.where(v > 0, v, 1.0)), 0.0)


def node_terms(gamma, elogpi, alpha):
    """:668-688, one value per node"""
    K = gamma.shape[1]
    return (gammaln(K * alpha) - K * gammaln(alpha) + (alpha - 1.0) * elogpi.sum(1)
            - (gammaln(gamma.sum(1)) - gammaln(np.maximum(gamma, 1e-30)).sum(1)) - ((gamma - 1.0) * elogpi).sum(1))


def elbo(gamma, beta, adj, skip, alpha):
    """-> dict: total, P, N, pair (the term of every visited pair), node, rounds, bad, and the three magnitudes of
    check_conditions (sums of |bilinear|, |cross|, |entropy| over the pairs)"""
    n = gamma.shape[0]
    p, q = OC.ordered_pairs(n, skip)
    y = adj[p, q]
    elogpi = OC.dir_exp(gamma)
    phi1, phi2, rounds, bad = OC.fixed_point(elogpi, beta, p, q, y)
    t = (np.log((1.0 - beta) + EPS), np.log(beta + EPS))
    link = (y == 1)[:, None]
    bil = (phi1 * np.where(link, phi2 @ t[1].T, phi2 @ t[0].T)).sum(1)   # sum_g phi1[g] sum_h T_y[g][h] phi2[h]
    cross = (phi1 * elogpi[p]).sum(1) + (phi2 * elogpi[q]).sum(1)
    ent = xlogx(phi1).sum(1) + xlogx(phi2).sum(1)
    pair = bil + cross - ent
    node = node_terms(gamma, elogpi, alpha)
    P, N = float(pair.sum()), float(node.sum())
    return dict(total=P + N, P=P, N=N, pair=pair, node=node, rounds=rounds, bad=bad, phi1=phi1, phi2=phi2,
                mag=(float(np.abs(bil).sum()), float(np.abs(cross).sum()), float(np.abs(ent).sum())))


def elbo_loops(gamma, beta, adj, skip, alpha):
    """the literal form: the loops of :635-688 over scalars, the fixed point written out pair by pair -> total, P, N, rounds"""
    n, K = gamma.shape
    skip = set((int(a), int(b)) for a, b in skip)
    elogpi = OC.dir_exp(gamma)
    P, rounds_total = 0.0, 0
    for p in range(n):
        for q in range(n):
            if p == q or (p, q) in skip:
                continue
            y = int(adj[p, q])
            f = beta if y else 1.0 - beta
            lf = np.log(f)
            phi1, phi2 = [1.0 / K] * K, [1.0 / K] * K
            old1, old2 = [0.0] * K, [0.0] * K
            for i in range(OC.ONLINE_ITERATIONS):
                if i % 2 == 0:
                    old1, old2 = list(phi1), list(phi2)
                n1 = [math.exp(elogpi[p, g] + sum(lf[g, h] * phi2[h] for h in range(K))) for g in range(K)]
                n2 = [math.exp(elogpi[q, g] + sum(lf[g, h] * phi1[h] for h in range(K))) for g in range(K)]
                s1, s2 = sum(n1), sum(n2)
                phi1, phi2 = [v / s1 for v in n1], [v / s2 for v in n2]
                rounds_total += 1
                if i % 2 == 1:
                    v1 = sum(abs(a - b) for a, b in zip(phi1, old1)) / K
                    v2 = sum(abs(a - b) for a, b in zip(phi2, old2)) / K
                    if v1 < OC.MEAN_CHANGE_THRESH and v2 < OC.MEAN_CHANGE_THRESH:
                        break
            s = 0.0
            for g in range(K):
                for h in range(K):
                    s += phi1[g] * phi2[h] * math.log(f[g, h] + EPS)
            for k in range(K):
                s += phi1[k] * elogpi[p, k]
                s += phi2[k] * elogpi[q, k]
            for k in range(K):
                s -= math.log(phi1[k]) * phi1[k] if phi1[k] > 0 else 0.0
                s -= math.log(phi2[k]) * phi2[k] if phi2[k] > 0 else 0.0
            P += s
    N = 0.0
    for p in range(n):
        v = sum(math.lgamma(alpha) for _ in range(K))
        s = math.lgamma(K * alpha) - v
        s += sum((alpha - 1.0) * elogpi[p, k] for k in range(K))
        v = sum(math.lgamma(max(gamma[p, k], 1e-30)) for k in range(K))
        s -= math.lgamma(sum(gamma[p, k] for k in range(K))) - v
        s -= sum((gamma[p, k] - 1.0) * elogpi[p, k] for k in range(K))
        N += s
    return P + N, P, N, rounds_total


def check_conditions(r, beta, peaked=True):
    """what lets a relative tolerance on total, P and N mean something: every pair term < 0 and every node term < 0 (no sum
    cancels), and the magnitudes of the three kinds of pair terms together stay below 50 |P|.  peaked: the state also meets
    orig_cases.check_conditions (exits at many rounds, a pair at the cap)"""
    if peaked:
        OC.check_conditions(r["rounds"], r["bad"], beta)
    assert not r["bad"].any() and np.all((beta > 0) & (beta < 1))
    assert np.all(r["pair"] < 0), float(r["pair"].max())
    assert np.all(r["node"] < 0), float(r["node"].max())
    assert sum(r["mag"]) / abs(r["P"]) < 50, sum(r["mag"]) / abs(r["P"])
    assert np.isfinite(r["total"])
