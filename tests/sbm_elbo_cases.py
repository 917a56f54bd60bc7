"""TEST INFRASTRUCTURE: an independent numpy restatement of the variational lower bound of the single-membership stochastic
blockmodel (-single-logl; the written definition is svils_sbmelbo's in include/svils.h; the reference's
SBM::approx_log_likelihood, src/sbm.cc:1133-1239).

Every sum is formed DIRECTLY over the trained pairs of sbm_cases.masks, with scipy's gammaln and xlogy.  It never uses the split
into column sums and link / skip corrections that the device computes with: that algebra is what the tests hold to it.

Beside the bound it returns A, the sum of the absolute values of all addends of the total.  An fp64 sum of m addends in any order
stays within about m 2^-53 A of the exact one; at the sizes of the tests (n K <= 130 * 256) that is 4e-12 A, and every comparison
with this restatement uses 1e-9 A: about 250 times the bound, and many orders of magnitude below a wrong or a missing term.
"""
import math

import numpy as np
from scipy.special import gammaln, xlogy

import sbm_cases as S

RTOL_A = 1e-9          # times A: every comparison with the restatement


def elbo(phi, gamma, lam, eta, T, Y, alpha=S.ALPHA):
    """-> (total, P, N, G, A) of the state (phi, gamma, lambda) with the Elogpi / Elogbeta of gamma and lambda"""
    n, K = phi.shape
    elogpi, elogbeta = S.elog(gamma, lam)
    i, j = np.nonzero(np.triu(T, 1))
    t = np.where(Y[i, j], 0, 1)                          # column of Elogbeta: 0 for a link, 1 for a non-link
    V = phi[i] * phi[j]                                  # [pairs][K]
    pk = V * elogbeta[:K][:, t].T                        # the terms of the K groups
    pr = (1.0 - V.sum(axis=1)) * elogbeta[K, t]          # the proper 1 - sum_k
    P = pk.sum() + pr.sum()
    A = np.abs(pk).sum() + np.abs(pr).sum()
    ne, nh = phi * elogpi, -xlogy(phi, phi)              # an exact 0 of phi adds 0
    N = ne.sum() + nh.sum()
    A += np.abs(ne).sum() + np.abs(nh).sum()
    g = []                                               # the addends of G
    for par, sign in ((eta, 1.0), (lam, -1.0)):
        g += [sign * gammaln(par.sum(axis=1)), -sign * gammaln(par[:, 0]), -sign * gammaln(par[:, 1]),
              sign * (par[:, 0] - 1.0) * elogbeta[:, 0], sign * (par[:, 1] - 1.0) * elogbeta[:, 1]]
    g += [np.array([gammaln(K * alpha)]), np.full(K, -gammaln(alpha)), (alpha - 1.0) * elogpi,
          np.array([-gammaln(gamma.sum())]), gammaln(np.maximum(gamma, 1e-30)), -(gamma - 1.0) * elogpi]
    g = np.concatenate(g)
    G = g.sum()
    A += np.abs(g).sum()
    return P + N + G, P, N, G, A


def elbo_prefix(phi, gamma, lam, eta, links, skip, alpha=S.ALPHA):
    """-> (total, P, N, G, A) as elbo returns them, for sizes the masks cannot reach: the pair part from the direct pair sums of
    sbm_cases.pair_sums_prefix (np.longdouble), N and G as above.  phi_ik phi_jk >= 0, 1 - sum_k phi_ik phi_jk >= 0 and
    Elogbeta < 0, so all addends of P are <= 0: their absolute values sum to -P"""
    n, K = phi.shape
    elogpi, elogbeta = S.elog(gamma, lam)
    a, b, n1, n0 = S.pair_sums_prefix(phi, links, skip)
    P = float((a * elogbeta[:K, 0]).sum() + (b * elogbeta[:K, 1]).sum() + (n1 - a.sum()) * elogbeta[K, 0] + (n0 - b.sum()) * elogbeta[K, 1])
    assert np.all(elogbeta < 0) and np.all(a >= 0) and np.all(b >= 0) and n1 >= a.sum() and n0 >= b.sum()
    ne, nh = phi * elogpi, -xlogy(phi, phi)
    N = ne.sum() + nh.sum()
    g = []
    for par, sign in ((eta, 1.0), (lam, -1.0)):
        g += [sign * gammaln(par.sum(axis=1)), -sign * gammaln(par[:, 0]), -sign * gammaln(par[:, 1]),
              sign * (par[:, 0] - 1.0) * elogbeta[:, 0], sign * (par[:, 1] - 1.0) * elogbeta[:, 1]]
    g += [np.array([gammaln(K * alpha)]), np.full(K, -gammaln(alpha)), (alpha - 1.0) * elogpi,
          np.array([-gammaln(gamma.sum())]), gammaln(np.maximum(gamma, 1e-30)), -(gamma - 1.0) * elogpi]
    g = np.concatenate(g)
    G = g.sum()
    return P + N + G, P, N, G, -P + np.abs(ne).sum() + np.abs(nh).sum() + np.abs(g).sum()


def entropy(phi):
    """the entropy part of N alone: - sum phi log phi"""
    return -xlogy(phi, phi).sum()


def case_elbo(case, state=None):
    """the bound of a case of sbm_cases in its own state, or in `state` = (phi, gamma, lambda)"""
    T, Y = case.masks()
    phi, gamma, lam = state if state is not None else (case.phi, case.gamma, case.lam)
    return elbo(phi, gamma, lam, case.eta, T, Y)


def literal_elbo(phi, gamma, lam, eta, T, Y, alpha=S.ALPHA):
    """the scalar loops of src/sbm.cc:1133-1239 as written there (math.lgamma, math.log), one addition at a time -> (s, A)"""
    n, K = phi.shape
    elogpi, elogbeta = S.elog(gamma, lam)
    s, A = 0.0, 0.0

    def add(v):
        nonlocal s, A
        s += v
        A += abs(v)

    for k in range(K + 1):
        for par, sign in ((eta, 1.0), (lam, -1.0)):
            add(sign * math.lgamma(par[k, 0] + par[k, 1]))
            for t in range(2):
                add(-sign * math.lgamma(par[k, t]))
                add(sign * (par[k, t] - 1) * elogbeta[k, t])
    for p in range(n):
        for q in range(n):
            if p >= q or not T[p, q]:
                continue
            y = 1 if Y[p, q] else 0
            sm = 0.0
            for k in range(K):
                sm += phi[p, k] * phi[q, k]
                add(phi[p, k] * phi[q, k] * (y * elogbeta[k, 0] + (1 - y) * elogbeta[k, 1]))
            add((1 - sm) * (y * elogbeta[K, 0] + (1 - y) * elogbeta[K, 1]))
    for i in range(n):
        for k in range(K):
            add(phi[i, k] * elogpi[k])
            if phi[i, k] > 0:
                add(-phi[i, k] * math.log(phi[i, k]))
    add(math.lgamma(K * alpha))
    for k in range(K):
        add(-math.lgamma(alpha))
        add((alpha - 1) * elogpi[k])
    add(-math.lgamma(gamma.sum()))
    for k in range(K):
        add(math.lgamma(max(gamma[k], 1e-30)))
        add(-(gamma[k] - 1) * elogpi[k])
    return s, A


def one_hot_state(n, K):
    """phi exactly 0 and 1 on the planted groups, with the gamma and lambda of the peaked state"""
    _, gamma, lam = S.peaked_state(n, K)
    phi = np.zeros((n, K))
    phi[np.arange(n), S.groups_of(n, K)] = 1.0
    return phi, gamma, lam
