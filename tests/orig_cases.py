"""What tests/test_orig.py and tests/test_gpu_orig.py share: an independent numpy restatement of one sweep of the reference's
MMSBInferOrig::batch_infer (src/mmsbinferorig.cc:212-294; PhiComp2::update_phis_until_conv, src/mmsbinferorig.hh:120-226),
vectorised over the pairs, and the states and graphs the tests run it on.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
from scipy.special import digamma

ONLINE_ITERATIONS = 50          # src/env.hh: online_iterations
MEAN_CHANGE_THRESH = 0.00001    # src/env.hh: meanchangethresh


def dir_exp(gamma):
    """set_dir_exp (src/mmsbinferorig.cc:601-622): psi(max(g, 1e-30)) - psi(row sum of g)"""
    return digamma(np.maximum(gamma, 1e-30)) - digamma(gamma.sum(1, keepdims=True))


def adjacency(n, links):
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    adj = np.zeros((n, n), dtype=np.int64)
    adj[links[:, 0], links[:, 1]] = adj[links[:, 1], links[:, 0]] = 1
    return adj


def ordered_pairs(n, skip=()):
    """every ordered pair (p, q), p != q, in the order of the loops at :221-235, without the pairs of `skip` in exactly
    that orientation"""
    p, q = np.divmod(np.arange(n * n), n)
    keep = p != q
    for a, b in skip:
        keep[a * n + b] = False
    return p[keep], q[keep]


def fixed_point(elogpi, beta, p, q, y):
    """update_phis_until_conv for every pair -> phi1, phi2, rounds (exit round + 1), bad (a normaliser was not > 0).
    Both sides use the OLD vectors and both use L_y[g][h] (:129-137: fd[g][h] with b the other side's vector -- not
    transposed for the second side); plain-sum normalisation (:141-148); the old vectors are saved at even i (:187-190),
    the exit is tested at odd i (:210-219)."""
    m, K = p.shape[0], elogpi.shape[1]
    logf = (np.log(1.0 - beta), np.log(beta))   # compute_f (:159-172) gives exactly 1 - beta or beta
    phi1 = np.full((m, K), 1.0 / K)
    phi2 = np.full((m, K), 1.0 / K)
    old1 = np.zeros((m, K))
    old2 = np.zeros((m, K))
    live = np.ones(m, dtype=bool)
    rounds = np.zeros(m, dtype=np.int64)
    bad = np.zeros(m, dtype=bool)
    for i in range(ONLINE_ITERATIONS):
        idx = np.flatnonzero(live)
        if idx.size == 0:
            break
        if i % 2 == 0:
            old1[idx] = phi1[idx]
            old2[idx] = phi2[idx]
        link = (y[idx] == 1)[:, None]

        def update(b, c):
            u = elogpi[c] + np.where(link, b @ logf[1].T, b @ logf[0].T)
            a = np.exp(u)
            s = a.sum(1)
            with np.errstate(invalid="ignore", divide="ignore"):
                return a / s[:, None], s

        n1, s1 = update(phi2[idx], p[idx])
        n2, s2 = update(phi1[idx], q[idx])
        bad[idx] |= ~(s1 > 0) | ~(s2 > 0)
        v1 = np.abs(n1 - old1[idx]).mean(1)
        v2 = np.abs(n2 - old2[idx]).mean(1)
        phi1[idx] = n1
        phi2[idx] = n2
        rounds[idx] = i + 1
        if i % 2 == 1:
            live[idx[(v1 < MEAN_CHANGE_THRESH) & (v2 < MEAN_CHANGE_THRESH)]] = False
    return phi1, phi2, rounds, bad


def sweep(gamma, beta, adj, skip, alpha):
    """one pass of :217-269 -> gamma, beta, rounds of every visited pair, bad normalisers"""
    n = gamma.shape[0]
    p, q = ordered_pairs(n, skip)
    y = adj[p, q]
    phi1, phi2, rounds, bad = fixed_point(dir_exp(gamma), beta, p, q, y)
    gnext = np.full_like(gamma, alpha)
    np.add.at(gnext, p, phi1)
    np.add.at(gnext, q, phi2)
    tot = phi1.T @ phi2
    num = (phi1 * y[:, None]).T @ phi2
    with np.errstate(invalid="ignore", divide="ignore"):
        return gnext, num / tot, rounds, bad


def pair_loglik(gamma, beta, pairs, y):
    """edge_likelihood (:563-587): log sum_g sum_h pi_p[g] pi_q[h] (y ? beta_gh : 1 - beta_gh), no clamp"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    pi = gamma / gamma.sum(1, keepdims=True)
    out = np.empty(pairs.shape[0])
    for x, ((a, b), yy) in enumerate(zip(pairs, y)):
        out[x] = np.log(pi[a] @ (beta if yy else 1.0 - beta) @ pi[b])
    return out


def init_beta1(rs, k):
    """init_beta1 (:167-186) from numpy draws: uniform_int(100) / 100 clamped to [0.01, 0.99]"""
    return np.clip(rs.randint(0, 100, size=(k, k)) / 100.0, 0.01, 0.99)


def random_links(n, density, rs):
    """links [m][2] uint32, p < q: the upper triangle of rand(n, n) < density"""
    iu = np.triu_indices(n, 1)
    keep = rs.rand(n, n)[iu] < density
    return np.ascontiguousarray(np.stack([iu[0][keep], iu[1][keep]], axis=1).astype(np.uint32))


def plain_state(seed, n, k, density=0.15):
    """links, gamma ~ Gamma(100, 0.01) (init_gamma, :157-164), beta as init_beta1"""
    rs = np.random.RandomState(seed)
    links = random_links(n, density, rs)
    return links, rs.gamma(100.0, 0.01, size=(n, k)), init_beta1(rs, k)


def peaked_state(seed, n, k):
    """a state whose pairs leave the fixed point at many different rounds, some only at the cap: links = the upper
    triangle of rand(n, n) < 0.15, gamma = gamma(0.3, 1.0) + 0.02, beta in {0.01, 0.99} with equal chance, then 30 % of
    the entries set to 0.5"""
    rs = np.random.RandomState(seed)
    links = random_links(n, 0.15, rs)
    gamma = rs.gamma(0.3, 1.0, size=(n, k)) + 0.02
    beta = np.where(rs.rand(k, k) < 0.5, 0.01, 0.99)
    beta[rs.rand(k, k) < 0.3] = 0.5
    return links, gamma, beta


def check_conditions(rounds, bad, beta):
    """what a test state must meet by the restatement alone: exits at >= 5 distinct rounds, a pair at the cap, no
    normaliser <= 0, beta inside (0, 1)"""
    assert len(set(rounds[rounds < ONLINE_ITERATIONS].tolist())) >= 5, sorted(set(rounds.tolist()))
    assert (rounds == ONLINE_ITERATIONS).sum() >= 1
    assert not bad.any()
    assert np.all((beta > 0) & (beta < 1))
