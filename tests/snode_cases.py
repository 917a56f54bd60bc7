"""What tests/test_snode.py and tests/test_gpu_snode.py share: a numpy restatement of ONE eager step of the reference's
FastAMM2::infer (src/fastamm2.cc:565-640 with opt_process / opt_process_noninf, :933-1165) -- every one of the n rows of
gamma moves -- on top of oracle/batch_oracle.py (dir_exp, phis -- imported, the oracle stays as it is) and
batch_cases.phis_rounds; the step sizes and scales; and the partner lists of a draw."""
import numpy as np

import batch_cases as BC
from oracle import batch_oracle as B

TAU0, KAPPA, NODETAU0, NODEKAPPA = 1024.0, 0.9, 1024.0, 0.5   # src/env.hh:405-408
INF_EPSILON, SETS = 0.5, 10                                   # _inf_epsilon, _m (src/fastamm2.cc:15-16)


def rho_gamma(it, nodetau0=NODETAU0, nodekappa=NODEKAPPA):
    """:606 -- _nodec[i] is incremented for every i at every iteration: one step size for all rows"""
    return (nodetau0 + 1 + it) ** (-nodekappa)


def rho_lambda(it, tau0=TAU0, kappa=KAPPA):
    """:627; _lambda_start_iter = 0"""
    return (tau0 + 1 + it + 1) ** (-kappa)


def scale_of(kind, n, inf_epsilon=INF_EPSILON):
    """:591-592"""
    return n / (2 * (1 - inf_epsilon)) if kind == 0 else (float(n) * SETS) / (2 * inf_epsilon)


def setsize(n):
    return n // SETS


def star(start, partner, adj, rho_gamma, scale, rho_lambda):
    partner = np.asarray(partner, dtype=np.int64).reshape(-1)
    return dict(start=int(start), partner=partner, y=adj[start, partner].astype(np.uint8) if len(partner) else np.zeros(0, np.uint8),
                rho_gamma=float(rho_gamma), scale=float(scale), rho_lambda=float(rho_lambda))


def pairs_of(s):
    a, j = s["start"], np.asarray(s["partner"], dtype=np.int64)
    return np.minimum(a, j), np.maximum(a, j)


def step(gamma, lam, adj, s, alpha, eta):
    """one eager step from (gamma, lambda) -> new gamma, new lambda, the rounds of every pair.  EVERY row moves: the rows of
    the star towards alpha + scale gammat, every other row towards alpha (:605-620); rho_lambda < 0 returns lambda as it came"""
    a, j = s["start"], np.asarray(s["partner"], dtype=np.int64)
    p, q = pairs_of(s)
    n, K = gamma.shape
    gammat, lambdat = np.zeros((n, K)), np.zeros((K, 2))
    rounds = np.zeros(0, dtype=np.int64)
    if len(j):
        assert len(set(j.tolist())) == len(j) and a not in set(j.tolist())
        y = adj[p, q]
        assert np.array_equal(y, np.asarray(s["y"], dtype=np.int64))
        elogpi, elogbeta = B.dir_exp(gamma), B.dir_exp(lam)
        phi1, phi2, rounds = BC.phis_rounds(elogpi, elogbeta, p, q, y)
        check1, check2 = B.phis(elogpi, elogbeta, p, q, y)
        assert np.array_equal(check1, phi1) and np.array_equal(check2, phi2)
        first = (p == a)[:, None]
        gammat[a] = np.where(first, phi1, phi2).sum(0)
        gammat[j] = np.where(first, phi2, phi1)
        pp = phi1 * phi2
        lambdat[:, 0] = (pp * (y[:, None] == 1)).sum(0)
        lambdat[:, 1] = (pp * (y[:, None] == 0)).sum(0)
    rho = s["rho_gamma"]
    named = np.zeros(n, dtype=bool)
    named[a] = True
    named[j] = True
    g = np.where(named[:, None], (1 - rho) * gamma + rho * (alpha + s["scale"] * gammat), (1 - rho) * gamma + rho * alpha)
    rl = s["rho_lambda"]
    if rl < 0:
        return g, lam.copy(), rounds
    return g, (1 - rl) * lam + rl * (np.asarray(eta, dtype=np.float64)[None, :] + s["scale"] * lambdat), rounds


def run(gamma, lam, adj, steps, alpha, eta, guard=None):
    """the restated chain -> gamma, lambda, all rounds; guard(g, lam, p, q) is called before every step"""
    rounds = []
    for s in steps:
        if guard is not None:
            guard(gamma, lam, *pairs_of(s))
        gamma, lam, r = step(gamma, lam, adj, s, alpha, eta)
        rounds.append(r)
    return gamma, lam, np.concatenate(rounds) if rounds else np.zeros(0, dtype=np.int64)


def expected_partners(kind, start, block_start, shuffled, nbrs, skip):
    """the partner list the reference's loops make: kind 0 the links of start outside the skip set, in link order; kind 1
    the walk through the shuffled order from block_start, wrapping, skipping start, taking the nodes with y = 0 outside the
    skip set until n // 10 are taken (the walk ends after one lap)"""
    a, n = start, len(shuffled)
    ok = lambda j: (min(a, j), max(a, j)) not in skip
    if kind == 0:
        return [j for j in nbrs[a] if ok(j)]
    mine = set(nbrs[a])
    walk = [int(shuffled[(block_start + x) % n]) for x in range(n)]
    return [j for j in walk if j != a and j not in mine and ok(j)][:setsize(n)]


def block_starts(n):
    """every value floor(u / setsize) * setsize can take for u in [0, n)"""
    return sorted({(u // setsize(n)) * setsize(n) for u in range(n)})
