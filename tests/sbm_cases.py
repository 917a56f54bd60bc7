"""TEST INFRASTRUCTURE: an independent numpy restatement of one iteration of the single-membership stochastic blockmodel
(-single; the written definition is the svils_sbm section of include/svils.h), and the cases the SBM tests share.

The restatement forms every sum DIRECTLY over the trained pairs -- a node's E-step sum walks all its trained partners, the
M-step all trained pairs i < j -- with scipy's digamma and logsumexp.  It never uses the split into column sums and
corrections that the device engine computes with: that algebra is what the tests hold to it.
"""
import functools

import numpy as np
from scipy.special import digamma, logsumexp

ALPHA = 0.5          # sbm_alpha
MAX_PASSES = 10
THRESH = 0.01


def eta_of(K, eta0=1.0, eta1=1.0):
    eta = np.empty((K + 1, 2))
    eta[:K] = (eta0, eta1)
    eta[K] = (0.0001, 1.0)
    return eta


def elog(gamma, lam):
    return digamma(gamma) - digamma(gamma.sum()), digamma(lam) - digamma(lam.sum(1))[:, None]


def masks(n, links, skip):
    """T [n][n]: the pair is trained; Y [n][n]: the pair is a link"""
    Y = np.zeros((n, n), dtype=bool)
    T = ~np.eye(n, dtype=bool)
    for p, q in np.asarray(links, dtype=np.int64).reshape(-1, 2):
        Y[p, q] = Y[q, p] = True
    for p, q in np.asarray(skip, dtype=np.int64).reshape(-1, 2):
        T[p, q] = T[q, p] = False
    return T, Y


def estep(phi, gamma, lam, T, Y, max_passes=MAX_PASSES):
    """-> (phi after the E-step, passes, msum of every pass); Gauss-Seidel: node p reads the rows 0 .. p - 1 of the same pass"""
    n, K = phi.shape
    phi = phi.copy()
    elogpi, elogbeta = elog(gamma, lam)
    msums = []
    for _ in range(max_passes):
        msum = 0.0
        for p in range(n):
            q = np.flatnonzero(T[p])
            t = np.where(Y[p, q], 0, 1)                  # column of Elogbeta: 0 for a link, 1 for a non-link
            P = phi[q]                                   # [m][K]
            a = elogpi + ((1.0 - P) * elogbeta[K, t][:, None] + P * elogbeta[:K][:, t].T).sum(axis=0)
            new = np.exp(a - logsumexp(a))
            msum += np.abs(phi[p] - new).sum()
            phi[p] = new
        msums.append(msum)
        if msum < THRESH:
            break
    return phi, len(msums), np.array(msums)


def mstep(phi, eta, T, Y, alpha=ALPHA):
    """-> (gamma, lambda) of phi"""
    n, K = phi.shape
    gamma = alpha + phi.sum(axis=0)
    i, j = np.nonzero(np.triu(T, 1))
    y = Y[i, j]
    G = phi[i] * phi[j]                                  # [pairs][K]
    lam = eta.copy()
    lam[:K, 0] += G[y].sum(axis=0)
    lam[:K, 1] += G[~y].sum(axis=0)
    lam[K, 0] += (1.0 - G[y]).sum()                      # summed over k as well (src/sbm.cc:512-515)
    lam[K, 1] += (1.0 - G[~y]).sum()
    return gamma, lam


def iterate(phi, gamma, lam, eta, T, Y, niter):
    """niter whole iterations -> (phi, gamma, lambda, [passes of every E-step], [msums of every E-step])"""
    passes, msums = [], []
    for _ in range(niter):
        phi, np_, ms = estep(phi, gamma, lam, T, Y)
        gamma, lam = mstep(phi, eta, T, Y)
        passes.append(np_)
        msums.append(ms)
    return phi, gamma, lam, passes, msums


def pair_loglik(phi, lam, pairs, y):
    K = phi.shape[1]
    r = lam[:, 0] / lam.sum(axis=1)
    out = []
    for (p, q), yy in zip(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), y):
        v = phi[p] * phi[q]
        f = r if yy else 1.0 - r
        s = (v * f[:K]).sum() + (1.0 - v.sum()) * f[K]
        out.append(np.log(max(s, 1e-30)))
    return np.array(out)


# ---- graphs ------------------------------------------------------------------------------------------------------------
def groups_of(n, K):
    return np.arange(n) % min(K, 4)


def planted(n, K, seed, p_in=0.5, p_out=0.03):
    """-> (links [m][2] p < q, skip [s][2] p < q): planted groups, and about n / 2 skipped pairs of both y values"""
    rng = np.random.RandomState(1000 + seed)
    g = groups_of(n, K)
    i, j = np.triu_indices(n, 1)
    y = rng.random_sample(i.shape[0]) < np.where(g[i] == g[j], p_in, p_out)
    links = np.stack([i[y], j[y]], axis=1).astype(np.uint32)
    non = np.stack([i[~y], j[~y]], axis=1).astype(np.uint32)
    h = n // 4
    s1 = links[rng.choice(links.shape[0], min(h, links.shape[0]), replace=False)] if links.shape[0] else links
    s0 = non[rng.choice(non.shape[0], min(h, non.shape[0]), replace=False)] if non.shape[0] else non
    return links, np.concatenate([s1, s0]).astype(np.uint32).reshape(-1, 2)


def path_graph(n):
    """0 - 1 - 2 - ...: every node has an earlier and a later neighbour in its own block"""
    return np.stack([np.arange(n - 1), np.arange(1, n)], axis=1).astype(np.uint32)


def star_graph(n, centre):
    return np.array([(min(centre, q), max(centre, q)) for q in range(n) if q != centre], dtype=np.uint32)


# ---- states ------------------------------------------------------------------------------------------------------------
def plain_state(n, K, seed):
    """the reference's starts: Gamma(100 * 100 / K, 0.01) for gamma and the rows of phi, Gamma(100, 0.01) for lambda"""
    rng = np.random.RandomState(2000 + seed)
    v, vl = 100.0 / K, (1.0 if K <= 100 else 100.0 / K)
    gamma = rng.gamma(100 * v, 0.01, K)
    lam = rng.gamma(100 * vl, 0.01, (K + 1, 2))
    phi = rng.gamma(100 * v, 0.01, (n, K))
    return phi / phi.sum(axis=1, keepdims=True), gamma, lam


def peaked_state(n, K, seed=0):
    """planted groups: phi 0.9 on the planted group, lambda favouring links inside groups"""
    g = groups_of(n, K)
    phi = np.full((n, K), 0.1 / (K - 1))
    phi[np.arange(n), g] = 0.9
    gamma = ALPHA + phi.sum(axis=0)
    lam = np.empty((K + 1, 2))
    lam[:K] = (6.0, 4.0)
    lam[K] = (1.0, 30.0)
    return phi / phi.sum(axis=1, keepdims=True), gamma, lam


# ---- the cases every SBM test draws from ----------------------------------------------------------------------------------
class Case:
    def __init__(self, name, n, K, links, skip, state):
        self.name, self.n, self.K = name, n, K
        self.links = np.asarray(links, dtype=np.uint32).reshape(-1, 2)
        self.skip = np.asarray(skip, dtype=np.uint32).reshape(-1, 2)
        self.phi, self.gamma, self.lam = state
        self.eta = eta_of(K)

    @functools.lru_cache(maxsize=None)
    def masks(self):
        return masks(self.n, self.links, self.skip)

    @functools.lru_cache(maxsize=None)
    def estep(self, max_passes=MAX_PASSES):
        """the restatement's E-step from the case's state, computed once and shared: (phi, passes, msums)"""
        T, Y = self.masks()
        return estep(self.phi, self.gamma, self.lam, T, Y, max_passes)

    @functools.lru_cache(maxsize=None)
    def iterate(self, niter):
        T, Y = self.masks()
        return iterate(self.phi, self.gamma, self.lam, self.eta, T, Y, niter)

    def y_of(self, pairs):
        _, Y = self.masks()
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        return Y[pairs[:, 0], pairs[:, 1]].astype(np.uint8)


@functools.lru_cache(maxsize=None)     # one object per case: its reference results are computed once per process
def planted_case(n, K, seed, state="plain"):
    links, skip = planted(n, K, seed)
    st = plain_state(n, K, seed) if state == "plain" else peaked_state(n, K, seed)
    return Case("planted-n%d-k%d-s%d-%s" % (n, K, seed, state), n, K, links, skip, st)


@functools.lru_cache(maxsize=None)
def block_cases(B):
    """the smallest shapes where the look-ahead of a block of B nodes can go wrong (K = 4, n = 2 B + 3)"""
    n, K = 2 * B + 3, 4
    mid = B // 2
    out = []
    # a path: every node has an earlier and a later neighbour in its own block
    out.append(Case("path", n, K, path_graph(n), [], plain_state(n, K, 11)))
    # a star centred mid-block: the centre reads the block's earlier rows from the block, the later ones as they were
    out.append(Case("star", n, K, star_graph(n, mid), [], plain_state(n, K, 12)))
    # node B + 1 has no links; the rest is a path
    lonely = np.array([(a, b) for a, b in path_graph(n) if B + 1 not in (a, b)], dtype=np.uint32)
    out.append(Case("lonely", n, K, lonely, [], plain_state(n, K, 13)))
    # skipped pairs of both y values inside one block (0-1 a link, 0-2 none) and across a block edge (B-1 - B a link, B-2 - B+1 none)
    skip = [(0, 1), (0, 2), (B - 1, B), (B - 2, B + 1)] if B >= 3 else [(0, 1), (0, 2)]
    out.append(Case("skips", n, K, path_graph(n), skip, plain_state(n, K, 14)))
    return out


ESTEP_K = (2, 3, 7, 64, 65, 256)        # at n = 61
ITER_CASES = ((61, 7, 1), (130, 4, 2), (61, 65, 1))   # (n, K, seed) of the whole-iteration cases
EARLY = (61, 4, 1)                      # peaked: the E-step ends after 2 passes
# The seed of the engine runs on the LFR golden graph (n = 1000, K = 28, two iterations).  With seeds 0 .. 5 the restatement's
# first E-step ends after three passes and the last pass of the second has msum = 0.0090: inside the band the case conditions
# exclude.  With seed 6 the E-steps take 9 and 4 passes and no msum comes within 10 % of 0.01 (tests/test_sbm.py asserts it)
LFR_SEED = 6


def estep_cases(B):
    """every E-step case of the device tests: K over ESTEP_K at n = 61; n over the block edges at K = 4 and K = 65"""
    out = [planted_case(61, K, 1) for K in ESTEP_K]
    for K in (4, 65):
        out += [planted_case(n, K, 2) for n in (2, 3, B - 1, B, B + 1, 2 * B + 1, 130)]
    return out


def all_cases(B):
    """every case any SBM test uses (the case conditions of tests/test_sbm.py are asserted on all of them)"""
    return (estep_cases(B) + block_cases(B) + [planted_case(n, K, s) for n, K, s in ITER_CASES] +
            [planted_case(*EARLY, state="peaked")] + [planted_case(n, K, s) for n, K, s in ((61, 4, 1), (97, 7, 2), (130, 3, 3))])
