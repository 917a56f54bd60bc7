"""Helpers of the link-query tests of -orig (test infrastructure): tests/test_gpu_orig_predict.py.

The reference is a numpy fp64 restatement written here from the definitions of include/svils.h:
score(p, c) = pi_p^T beta pi_c with P = gamma / rowsum, S[p] = (P[p] @ beta) @ P.T, and the candidates of p = every node
c != p except those where {p, c} is a link and neither (p, c) nor (c, p) is in the skip list."""
import numpy as np

from pair_cases import NONE, _random_links, _random_pairs

EPS = 1e-12


def hub_links(rng, n, m, hub):
    """random links plus a hub adjacent to ids 0, n - 1 and every third id: its neighbours span all the 64-candidate tiles
    (the construction of test_gpu_rank.py's _hub_links)"""
    extra = [(min(hub, x), max(hub, x)) for x in sorted({0, n - 1} | set(range(1, n, 3))) if x != hub]
    e = np.unique(np.concatenate([_random_links(rng, n, m), np.array(extra, dtype=np.uint32)]), axis=0)
    return np.ascontiguousarray(e[np.lexsort((e[:, 1], e[:, 0]))], dtype=np.uint32)


def mixed_skip(rng, n, links):
    """a skip list that uses every case of the candidate rule: of a tenth of the links a third is skipped as (p, c) only, a
    third as (c, p) only and a third in both orientations; and a few non-links are skipped too (they change nothing)"""
    pick = links[rng.choice(len(links), size=max(3, len(links) // 10), replace=False)].astype(np.int64)
    skip = []
    for i, (p, c) in enumerate(pick.tolist()):
        skip += [[(p, c)], [(c, p)], [(p, c), (c, p)]][i % 3]
    have = {tuple(x) for x in links.tolist()}
    for p, c in _random_pairs(rng, n, 8).tolist():
        if (min(p, c), max(p, c)) not in have and (p, c) not in skip:
            skip.append((p, c))
    return np.array(skip, dtype=np.uint32).reshape(-1, 2)


def random_state(n, k, m, seed, ties=False, hub=None):
    """links, skip, gamma, beta: gamma = U(0,1) + 0.01 and beta = clip(U(0,1), 0.01, 0.99), or (ties) gamma entries in
    {1, 2, 3} and beta entries in {1/4, 1/2, 3/4}: many nodes share a row of pi, so scores tie exactly"""
    rng = np.random.default_rng(seed)
    links = _random_links(rng, n, m) if hub is None else hub_links(rng, n, m, hub)
    skip = mixed_skip(rng, n, links)
    if ties:
        gamma = rng.integers(1, 4, size=(n, k)).astype(np.float64)
        beta = rng.integers(1, 4, size=(k, k)).astype(np.float64) / 4.0
    else:
        gamma = rng.random((n, k)) + 0.01
        beta = np.clip(rng.random((k, k)), 0.01, 0.99)
    return links, skip, gamma, beta


def device(n, k, links, skip, gamma, beta):
    from svinet_amd import _svils
    d = _svils.Orig(n, k, 1.0 / k)
    d.set_graph(links, skip)
    d.set_state(gamma, beta)
    return d


def excluded(n, links, skip):
    """ex[p, c]: c is NOT a candidate of p because {p, c} is a training link"""
    adj = np.zeros((n, n), dtype=bool)
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    adj[links[:, 0], links[:, 1]] = adj[links[:, 1], links[:, 0]] = True
    sk = np.zeros((n, n), dtype=bool)
    skip = np.asarray(skip, dtype=np.int64).reshape(-1, 2)
    sk[skip[:, 0], skip[:, 1]] = True
    return adj & ~(sk | sk.T)


def pi_of(gamma):
    return gamma / gamma.sum(1, keepdims=True)


def score_rows(P, beta, p):
    """S[p, :] for the nodes p"""
    return (P[p] @ beta) @ P.T


def rank_ref(P, beta, ex, pairs, eps=EPS):
    """per directed pair: lo, hi (the interval the device's above and above + tied must lie in), ncand and numpy's score"""
    n = P.shape[0]
    out = np.zeros((len(pairs), 3), dtype=np.int64)
    sc = np.zeros(len(pairs))
    for i, (p, q) in enumerate(np.asarray(pairs, dtype=np.int64).tolist()):
        S = score_rows(P, beta, p)
        cand = ~ex[p]
        cand[p] = False
        cand[q] = False
        s = S[q]
        out[i] = np.sum(S[cand] > s * (1 + eps)), np.sum(S[cand] >= s * (1 - eps)), cand.sum()
        sc[i] = s
    return out[:, 0], out[:, 1], out[:, 2], sc


def check_against_numpy(res, ref, sharp=True, rtol=1e-12):
    above, tied, ncand, score = res
    lo, hi, nc, sc = ref
    assert np.array_equal(ncand, nc)
    print("max relative score error %.3g" % np.abs(score / sc - 1).max())
    np.testing.assert_allclose(score, sc, rtol=rtol, atol=0)
    a, at = above.astype(np.int64), above.astype(np.int64) + tied
    assert np.all(lo <= a) and np.all(at <= hi), (lo, a, at, hi)
    share = np.mean(lo == hi)
    print("rank vs numpy: %d pairs, lo == hi for %.4f" % (len(lo), share))
    if sharp:
        assert share >= 0.99, share


def check_against_topk(dev, n, ex, nodes, topk=25):
    """the library's own lists as the reference: scores bitwise, above <= j <= above + tied, equality where the next score is
    strictly lower, ncand = n - 2 - training degree.  Returns (ranked entries tied with another, strict steps)"""
    ids, sc = dev.predict_links(topk, nodes)
    rows, cols = np.nonzero(ids != NONE)
    pairs = np.stack([nodes[rows], ids[rows, cols]], 1)
    assert not ex[pairs[:, 0], pairs[:, 1]].any() and np.all(pairs[:, 0] != pairs[:, 1])
    above, tied, ncand, score = dev.rank_links(pairs)
    assert np.array_equal(score.view(np.uint64), sc[rows, cols].view(np.uint64))
    assert np.array_equal(dev.link_prob(pairs).view(np.uint64), score.view(np.uint64))
    assert np.all(above <= cols) and np.all(cols <= above.astype(np.int64) + tied)
    assert np.array_equal(ncand, n - 2 - ex[nodes[rows]].sum(1))
    nxt = np.full(ids.shape, np.inf)
    nxt[:, :-1] = sc[:, 1:]
    strict = (cols < topk - 1) & (sc[rows, cols] > nxt[rows, cols])
    assert np.array_equal((above.astype(np.int64) + tied)[strict], cols[strict])
    return int(np.sum(tied > 0)), int(np.sum(strict))


def topk_ref(P, beta, ex, p, topk, eps=EPS):
    """numpy's list of p: ids by (score descending, id ascending) among the candidates, and their scores"""
    S = score_rows(P, beta, p)
    cand = ~ex[p]
    cand[p] = False
    ids = np.nonzero(cand)[0]
    order = np.lexsort((ids, -S[ids]))[:topk]
    return ids[order], S[ids[order]]


def planted_two_groups(path, n=200, p_across=0.2, p_within=0.01, seed=5):
    """a disassortative graph: two groups of n / 2, links across the groups at p_across and within at p_within; written as
    "id<TAB>id" lines, ids 1 .. n.  Returns the links (0-based, p < q)"""
    rng = np.random.default_rng(seed)
    g = np.arange(n) % 2
    iu = np.triu_indices(n, 1)
    prob = np.where(g[iu[0]] != g[iu[1]], p_across, p_within)
    keep = rng.random(len(prob)) < prob
    links = np.stack([iu[0][keep], iu[1][keep]], 1)
    with open(path, "w") as f:
        for a, b in links.tolist():
            f.write("%d\t%d\n" % (a + 1, b + 1))
    return links
