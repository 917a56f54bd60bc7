"""-m gpu: the sparse form of the svils_batch handle (svils_batch_create_sparse, -sparse-graph).

1. Under the cap the two forms take the same calls and agree bit for bit after every one of them: the step kernels are
   the same code, instantiated once per lookup (DenseGraph: two word reads, SparseGraph: a search in a sorted row).
2. Above the cap (n = 33 025) the sparse form is held to the restatements the dense form is held to -- tests/sampled_cases.py,
   infset_cases.py, snode_cases.py, imported as they are -- at their rtol 1e-7 after sampled_cases.assert_exits_are_clear,
   with equal round totals.  The restatements index adj[p, q]: PairAdj answers that from the sorted pairs, not an n x n array.
   Seeds were chosen on the host so that every restated step runs clean (exit margins clear, no underflow).
3. The contract of the sparse form: the refusals of the step calls with the dense form's wording and an untouched state,
   the all-pairs passes SVILS_ERR_UNSUPPORTED, set_graph twice.
4. The command line: each engine with and without -sparse-graph on assort-75-4 writes the same files; -infset / -snode
   with -sparse-graph above the cap agree with the engines of host_api driven through the same iterations."""
import subprocess

import numpy as np
import pytest

import infset_cases as IC
import sampled_cases as SC
import snode_cases as NC
from svinet_amd import _svils, host_api
from svinet_amd.host_api import InfsetEngine, SampledEngine, StratNodeEngine
from test_gpu_batch import RTOL, SVINET

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -4


# ---------------------------------------------------------------------------------------------------------------------
# 1. the two forms agree bit for bit under the cap
# ---------------------------------------------------------------------------------------------------------------------
HUB, ISOLATED, ALL_SKIPPED = 3, 5, 7


class Small:
    """a random graph of density 0.2 with, where n allows (n >= 33), a hub, an isolated node, partners at 31 / 32 / 63 / 64,
    and a skip set of links and non-links with the whole row of one node"""

    def __init__(self, n, k, seed):
        self.n, self.k, self.alpha, self.eta = n, k, 1.0 / k, (1.0, 1.0)
        rs = np.random.RandomState(seed)
        iu = np.triu_indices(n, 1)
        keep = rs.random_sample(iu[0].shape[0]) < 0.2
        pairs = {(int(p), int(q)) for p, q in zip(iu[0][keep], iu[1][keep])} | {(0, n - 1)}
        self.special = n >= 33
        if self.special:
            pairs |= {(min(HUB, j), max(HUB, j)) for j in range(n) if j != HUB}
            pairs |= {(1, q) for q in (31, 32, 63, 64) if q < n}
            pairs = {e for e in pairs if ISOLATED not in e}
        self.links = np.array(sorted(pairs), dtype=np.uint32).reshape(-1, 2)
        self.linkset = pairs
        skip = set()
        if self.special:
            non = [(int(p), int(q)) for p, q in zip(*iu) if (int(p), int(q)) not in pairs]
            skip |= {tuple(self.links[i]) for i in rs.choice(len(self.links), 6, replace=False)}
            skip |= {non[i] for i in rs.choice(len(non), 6, replace=False)}
            skip |= {(min(ALL_SKIPPED, j), max(ALL_SKIPPED, j)) for j in range(n) if j != ALL_SKIPPED}
            skip |= {(1, 32)}
        self.skip = {(int(p), int(q)) for p, q in skip} - {(0, n - 1)}                  # (the pair steps list that pair)
        self.gamma = rs.gamma(100.0, 0.01, (n, k))
        self.lam = np.tile(np.asarray(self.eta), (k, 1)) + rs.gamma(100.0, 0.01, (k, 2))
        self.rs = rs

    def handle(self, sparse):
        d = _svils.Batch(self.n, self.k, self.alpha, self.eta, sparse=sparse)
        order = self.rs.permutation(len(self.links))               # the lists may come in any order
        d.set_graph(self.links[order], sorted(self.skip)[::-1])
        d.set_state(self.gamma, self.lam)
        return d

    def y(self, a, j):
        return 1 if (min(a, j), max(a, j)) in self.linkset else 0

    def free(self, a):
        return [j for j in range(self.n) if j != a and (min(a, j), max(a, j)) not in self.skip]

    def star(self, a, m, it):
        free = self.free(a)
        partner = [free[i] for i in self.rs.permutation(len(free))[:m]]
        return dict(start=a, partner=np.array(partner, dtype=np.uint32), y=np.array([self.y(a, j) for j in partner], dtype=np.uint8),
                    rho_partner=np.array([IC.rho_node(c, nodetau0=3.0) for c in range(len(partner))]), rho_start=IC.rho_node(it, nodetau0=3.0),
                    rho_gamma=NC.rho_gamma(it, nodetau0=3.0), scale=self.n / 2.0, rho_lambda=IC.rho_lambda(it, tau0=10.0))


def _same_bits(dense, sparse, what):
    for name, (a, b) in (("state", (dense.state(), sparse.state())), ("expectations", (dense.expectations(), sparse.expectations()))):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), (what, name)
    assert dense.stats() == sparse.stats(), what
    assert dense.lag() == sparse.lag(), what


FORM_KS = [2, 5, 13, 20, 40, 67, 200]   # one K per W of svils_batch_variant: 2, 5, 20, 67, 200 reach W = 1, 2, 8, 32, 64; 13 and 40 add W = 4 and 16


@pytest.mark.parametrize("k", FORM_KS)
@pytest.mark.parametrize("n", [2, 33, 65, 130])
def test_the_two_forms_agree_bit_for_bit(n, k):
    """the same calls to a dense and to a sparse handle, interleaved: node steps at the hub, the isolated node and the node
    whose pairs are all skipped, pair steps with a repeated pair and an empty list, a star chain of five steps with an empty
    star cut at two different lengths, four strat steps; after every call the state, the expectations, the counters and the
    lag are equal as bits and integers, and so are the pair likelihoods of 200 pairs"""
    assert {_svils.batch_variant(x)[0] for x in FORM_KS} == {_svils.batch_variant(x)[0] for x in range(2, _svils.BATCH_MAX_K + 1)}
    w = Small(n, k, seed=100 * n + k)
    dense, sparse = w.handle(False), w.handle(True)
    both = (dense, sparse)
    _same_bits(dense, sparse, "start")
    nodes = [HUB, ISOLATED, ALL_SKIPPED, n - 1] if w.special else [0, n - 1]
    for c, a in enumerate(nodes):                                   # node steps, one call each; the last leaves lambda alone
        for d in both:
            d.step_node([a], n / 2.0, [SC.rho_gamma(c)], [SC.rho_lambda(c, 0) if c + 1 < len(nodes) else -1.0])
        _same_bits(dense, sparse, "node step at %d" % a)
    iu = np.triu_indices(n, 1)
    ok = np.array([(int(p), int(q)) not in w.skip for p, q in zip(*iu)])
    allp = np.stack([iu[0][ok], iu[1][ok]], axis=1)
    m = max(1, min(len(allp), n // 2))
    lst = allp[w.rs.choice(len(allp), m, replace=len(allp) < m)]
    lst = np.concatenate([lst, lst[:1], np.array([[0, n - 1]])])    # a repeated pair, and the pair (0, n - 1)
    lists = [lst, np.zeros((0, 2), dtype=np.uint32), lst[::-1][: max(1, m // 2)]]
    for d in both:
        d.step_pairs(lists, [50.0, 50.0, 70.0], [0.05, 0.04, 0.03], [0.02, -1.0, 0.01])
    _same_bits(dense, sparse, "pair steps")
    starts = [nodes[0], n - 1, 0, nodes[0], 1 % n]
    stars = [w.star(a, 0 if c == 2 else min(n - 1, 9 + 60 * (c % 2)), c) for c, a in enumerate(starts)]
    assert len(stars[2]["partner"]) == 0
    for d, chain in zip(both, (2, 3)):                              # the chain cut at two different lengths
        d.set_star_chain(chain)
        d.step_star(stars)
    _same_bits(dense, sparse, "star chain")
    strat = [dict(s, scale=NC.scale_of(c % 2, n)) for c, s in enumerate(stars[:4])]
    for d in both:
        d.step_strat(strat)
    assert dense.lag() == sparse.lag() and (n == 2 or dense.lag() > 0)
    _same_bits(dense, sparse, "strat steps")
    pairs = np.stack([w.rs.randint(0, n, 200), w.rs.randint(0, n, 200)], axis=1)
    pairs[pairs[:, 0] == pairs[:, 1], 1] = (pairs[pairs[:, 0] == pairs[:, 1], 0] + 1) % n
    y = w.rs.randint(0, 2, 200)
    assert dense.pair_loglik(pairs, y).tobytes() == sparse.pair_loglik(pairs, y).tobytes()
    assert np.all(np.isfinite(dense.state()[0]))
    for d in both:
        d.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. above the cap, against the restatements
# ---------------------------------------------------------------------------------------------------------------------
BIG_N, BIG_HUB, BIG_LAST, BIG_SKIPPED = 33025, 100, 33024, 200


class PairAdj:
    """adj[p, q] of the restatements from the sorted pairs: 1 where (p, q) or (q, p) is a link"""

    def __init__(self, n, links):
        self.n = n
        self.keys = np.sort(links[:, 0].astype(np.int64) * n + links[:, 1].astype(np.int64))

    def __getitem__(self, idx):
        p, q = np.broadcast_arrays(np.asarray(idx[0], dtype=np.int64), np.asarray(idx[1], dtype=np.int64))
        key = np.minimum(p, q) * self.n + np.maximum(p, q)
        at = np.minimum(np.searchsorted(self.keys, key), len(self.keys) - 1)
        return (self.keys[at] == key).astype(np.int64)


class Big:
    """n = 33 025, mean degree 8, a hub of degree 5 000, links and skip pairs with both ends >= 32 768"""

    def __init__(self, seed=1):
        n = self.n = BIG_N
        rs = self.rs = np.random.RandomState(seed)
        a, b = rs.randint(0, n, 4 * n), rs.randint(0, n, 4 * n)
        pairs = {(int(min(p, q)), int(max(p, q))) for p, q in zip(a, b) if p != q and BIG_HUB not in (p, q)}
        hub = rs.choice(np.setdiff1d(np.arange(n), [BIG_HUB]), 5000, replace=False)
        pairs |= {(int(min(BIG_HUB, j)), int(max(BIG_HUB, j))) for j in hub} | {(BIG_HUB, 32768), (BIG_HUB, BIG_LAST)}
        pairs |= {(32768, BIG_LAST), (32770, 33000), (32769, 32771), (31, BIG_LAST), (0, n - 1)}
        self.links = np.array(sorted(pairs), dtype=np.uint32)
        self.linkset = pairs
        self.adj = PairAdj(n, self.links)
        mine = [int(j) for j in np.unique(self.links[np.any(self.links == BIG_SKIPPED, axis=1)]) if j != BIG_SKIPPED]
        skip = {(32770, 33000), (32769, 33001), (BIG_HUB, 32768), (BIG_LAST - 1, BIG_LAST)}       # links and non-links past 32 768
        skip |= {(min(BIG_SKIPPED, j), max(BIG_SKIPPED, j)) for j in mine[:3] + [0, 31, 32, 64, 32767, 32768, BIG_LAST]}
        self.skip = skip
        self.degree = np.bincount(self.links.reshape(-1), minlength=n)
        assert self.degree[BIG_HUB] >= 5000 and 7.5 < self.degree.mean() < 8.5

    def handle(self, k, seed):
        """The state: every row one of four seeded rows times (1 + 1e-3 u), u uniform in [-1, 1) per cell.  A step of
        33 024 independent rows has a few pairs within 1e-4 of the exit threshold whatever the seed (a pair's mean change
        falls by a factor of ten or so per test: about 1e-4 of all pairs sit that close), and the standing of the
        restatements could not be asserted; with four kinds of row the pairs of a step come in a few narrow bands, which a
        seed can keep clear of the threshold -- while a row read from the wrong node is still 1e-3 off, 10^4 times the
        tolerance"""
        rs = np.random.RandomState(seed)
        self.k, self.alpha, self.eta = k, 1.0 / k, (1.0, 1.0)
        kinds = rs.gamma(100.0, 0.01, (4, k)) * (1.0 + 3.0 * (rs.random_sample((4, k)) < 0.3))
        self.gamma = kinds[rs.randint(0, 4, self.n)] * (1.0 + 1e-3 * (2.0 * rs.random_sample((self.n, k)) - 1.0))
        self.lam = np.tile(np.asarray(self.eta), (k, 1)) + rs.gamma(100.0, 0.01, (k, 2))
        d = _svils.Batch(self.n, k, self.alpha, self.eta, sparse=True)
        d.set_graph(self.links[rs.permutation(len(self.links))], sorted(self.skip))
        d.set_state(self.gamma, self.lam)
        return d, rs

    def reset(self, d):
        """every group of steps starts from the seeded state: the kinds of row do not multiply from group to group"""
        d.set_state(self.gamma, self.lam)
        return self.gamma, self.lam

    def star(self, a, partner, it):
        partner = np.array([j for j in dict.fromkeys(partner) if j != a and (min(a, j), max(a, j)) not in self.skip], dtype=np.int64)
        return IC.star(a, partner, self.adj, [IC.rho_node(c % 7, nodetau0=3.0) for c in range(len(partner))], IC.rho_node(it, nodetau0=3.0),
                       self.n / 2.0, IC.rho_lambda(it, tau0=10.0))

    def neighbours(self, a):
        rows = self.links[np.any(self.links == a, axis=1)].astype(np.int64)
        return [int(j) for j in np.unique(rows) if j != a]


BIG_SEEDS = {3: 0, 20: 0}   # chosen on the host: every restated step below runs with clear exit margins and no underflow


@pytest.fixture(scope="module")
def big():
    return Big()


def _totals(d, rounds):
    pairs_done, rounds_total, rounds_max, underflow = d.stats()
    assert (pairs_done, rounds_total, underflow) == (len(rounds), int(rounds.sum()), 0)
    assert rounds_max == (int(rounds.max()) if len(rounds) else 0)


def _close(d, g, lam):
    dg, dl = d.state()
    np.testing.assert_allclose(dg, g, rtol=RTOL)
    np.testing.assert_allclose(dl, lam, rtol=RTOL)
    return dg, dl


@pytest.mark.parametrize("k", [3, 20])
def test_above_the_cap_the_steps_match_the_restatements(big, k):
    w, n = big, BIG_N
    d, rs = w.handle(k, seed=BIG_SEEDS[k])
    with pytest.raises(_svils.SvilsError) as ei:                    # the dense form stops at the cap
        _svils.Batch(n, k, w.alpha, w.eta)
    assert ei.value.code == ERR_UNSUPPORTED and "SVILS_BATCH_MAX_N" in str(ei.value)
    # node steps: the hub, the last node, a node with skipped pairs
    for c, a in enumerate((BIG_HUB, BIG_LAST, BIG_SKIPPED)):
        g, lam = w.reset(d)
        p, q = SC.node_pairs(n, a, w.skip)
        assert len(p) == n - 1 - sum(a in e for e in w.skip)
        SC.assert_exits_are_clear(g, lam, w.adj, p, q)
        rg, rl = SC.rho_gamma(c), SC.rho_lambda(c, 0)
        d.step_node([a], n / 2.0, [rg], [rl])
        g, lam, rounds = SC.step(g, lam, w.adj, p, q, w.alpha, w.eta, n / 2.0, rg, rl)
        _totals(d, rounds)
        _close(d, g, lam)
    # a pair step of n // 2 pairs: random ones, a hub's links, pairs past 32 768
    m = n // 2
    lst = {(int(min(p, q)), int(max(p, q))) for p, q in zip(rs.randint(0, n, m), rs.randint(0, n, m)) if p != q}
    lst |= {tuple(int(x) for x in e) for e in w.links[np.any(w.links == BIG_HUB, axis=1)][:300]} | {(32768, BIG_LAST), (32769, 32771), (32800, 33010)}
    lst = np.array(sorted(lst - w.skip)[:m], dtype=np.int64)
    lst = lst[rs.permutation(len(lst))]
    assert len(lst) == m and w.adj[lst[:, 0], lst[:, 1]].sum() >= 300
    g, lam = w.reset(d)
    SC.assert_exits_are_clear(g, lam, w.adj, lst[:, 0], lst[:, 1])
    scale = (n * (n - 1) / 2.0) / m
    d.step_pairs([lst], [scale], [0.03], [0.02])
    g, lam, rounds = SC.step(g, lam, w.adj, lst[:, 0], lst[:, 1], w.alpha, w.eta, scale, 0.03, 0.02)
    _totals(d, rounds)
    _close(d, g, lam)
    # a star chain: the hub with its links and some non-links, a start past 32 768, an empty star, partners past 32 768
    far = [32768, 32769, 33000, BIG_LAST, 5, 31, 32, 64]
    stars = [w.star(BIG_HUB, w.neighbours(BIG_HUB)[:700] + far, 0), w.star(32770, w.neighbours(32770) + far, 1),
             w.star(BIG_LAST, [], 2), w.star(BIG_SKIPPED, w.neighbours(BIG_SKIPPED) + far, 3)]
    assert any(int(j) >= 32768 for s in stars for j in s["partner"]) and stars[0]["y"].sum() >= 690
    g, lam = w.reset(d)
    g0, rounds = g, []
    for s in stars:
        SC.assert_exits_are_clear(g, lam, w.adj, *IC.pairs_of(s))
        g, lam, r = IC.step(g, lam, w.adj, s, w.alpha, w.eta)
        rounds.append(r)
    d.step_star(stars)
    _totals(d, np.concatenate(rounds))
    dg, dl = _close(d, g, lam)
    named = np.unique(np.concatenate([s["partner"] for s in stars] + [[s["start"] for s in stars]]).astype(np.int64))
    rest = np.setdiff1d(np.arange(n), named)
    assert len(rest) > n - 2000 and dg[rest].tobytes() == g0[rest].tobytes()     # a star step leaves every unlisted row bit for bit
    g, lam = w.reset(d)
    # strat steps: the links of the hub, a block of n // 10 non-links with nodes past 32 768
    block = [int(j) for j in rs.permutation(n) if j != 32770 and not w.adj[32770, j]][: NC.setsize(n) - 2] + [33001, BIG_LAST]
    strat = []
    for it, (a, partner, kind) in enumerate(((BIG_HUB, w.neighbours(BIG_HUB), 0), (32770, block, 1), (BIG_LAST, w.neighbours(BIG_LAST), 0))):
        partner = [j for j in dict.fromkeys(partner) if (min(a, j), max(a, j)) not in w.skip]
        strat.append(NC.star(a, partner, w.adj, NC.rho_gamma(it, nodetau0=3.0), NC.scale_of(kind, n), NC.rho_lambda(it, tau0=10.0)))
    assert len(strat[1]["partner"]) >= NC.setsize(n) - 2 and not strat[1]["y"].any() and strat[0]["y"].all()
    d.step_strat(strat)
    assert d.lag() == n - 1 - len(strat[-1]["partner"])
    g, lam, rounds = NC.run(g, lam, w.adj, strat, w.alpha, w.eta, guard=lambda g_, l_, p, q: SC.assert_exits_are_clear(g_, l_, w.adj, p, q))
    _totals(d, rounds)
    _close(d, g, lam)
    d.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the contract of the sparse form
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_keep_their_wording_and_the_state():
    w = Small(65, 5, seed=9)
    d = w.handle(True)
    non = next((p, q) for p in range(10, 20) for q in range(40, 60) if (p, q) not in w.linkset and (p, q) not in w.skip)
    lnk = next(e for e in sorted(w.linkset) if e not in w.skip and HUB not in e)
    skipped = sorted(w.skip)[0]
    good = w.star(HUB, 10, 0)

    def bad(**kw):
        return dict(good, **kw)

    flipped = bad(start=non[0], partner=np.array([non[1]], dtype=np.uint32), y=np.array([1], dtype=np.uint8), rho_partner=np.array([0.5]))
    flipped1 = bad(start=lnk[0], partner=np.array([lnk[1]], dtype=np.uint32), y=np.array([0], dtype=np.uint8), rho_partner=np.array([0.5]))
    inskip = bad(start=skipped[1], partner=np.array([skipped[0]], dtype=np.uint32), y=np.array([w.y(*skipped)], dtype=np.uint8),
                 rho_partner=np.array([0.5]))
    twice = bad(partner=np.append(good["partner"][:3], good["partner"][0]), y=np.append(good["y"][:3], good["y"][0]), rho_partner=np.full(4, 0.5))
    for step, text in ((flipped, "has y = 1, the graph says otherwise"), (flipped1, "has y = 0, the graph says otherwise"),
                       (inskip, "is in the skip set"), (twice, "lists partner %u twice" % good["partner"][0])):
        for call in (d.step_star, d.step_strat):
            with pytest.raises(_svils.SvilsError) as ei:
                call([good, step])
            assert ei.value.code == ERR_ARG and text in str(ei.value) and "entry" in str(ei.value) and "of step 1" in str(ei.value), str(ei.value)
    with pytest.raises(_svils.SvilsError) as ei:
        d.step_pairs([[lnk], [lnk, skipped]], [1.0, 1.0], [0.5, 0.5], [0.5, 0.5])
    assert ei.value.code == ERR_ARG and "pair 1 of step 1 (%u, %u) is in the skip set" % skipped in str(ei.value)
    # set_graph: the refusals of the dense form in its order -- a repeat before a later entry that is no pair, and the other way round
    dense = _svils.Batch(w.n, w.k, w.alpha, w.eta)
    for links, skip, text in (([(1, 2), (3, 4), (1, 2), (5, 5)], [], "link 2 (1, 2) is repeated"),
                              ([(1, 2), (5, 5), (3, 4), (1, 2)], [], "link 1 (5, 5) is not a pair p < q < n = 65"),
                              ([(1, 2), (2, 1)], [], "link 1 (2, 1) is not a pair"), ([(1, 65)], [], "link 0 (1, 65) is not a pair"),
                              ([(9, 8)], [(1, 2), (1, 2)], "link 0 (9, 8) is not a pair"),
                              ([(1, 2)], [(4, 9), (3, 4), (4, 9), (4, 9)], "skipped pair 2 (4, 9) is repeated")):
        for h in (dense, d):
            with pytest.raises(_svils.SvilsError) as ei:
                h.set_graph(links, skip)
            assert ei.value.code == ERR_ARG and text in str(ei.value), (text, str(ei.value))
    dense.close()
    g, lam = d.state()
    assert g.tobytes() == w.gamma.tobytes() and lam.tobytes() == w.lam.tobytes() and d.lag() == 0
    d.step_star([good])                                             # the graph is still the one set before the refused set_graph calls
    assert d.stats()[0] == 10
    d.close()


def test_the_all_pairs_passes_are_refused_and_change_nothing():
    w = Small(65, 5, seed=11)
    d, ref = w.handle(True), w.handle(True)
    L = _svils.load()
    for call in (lambda: d.sweep(), lambda: d.elbo(), lambda: d.set_elbo_tiles(4)):
        with pytest.raises(_svils.SvilsError) as ei:
            call()
        assert ei.value.code == ERR_UNSUPPORTED and "need the dense form" in str(ei.value)
    assert L.svils_batch_sweep(d._h, 0) == ERR_UNSUPPORTED
    assert d.stats() == ref.stats() and d.timing()[0] == -1
    for h in (d, ref):
        h.step_node([HUB], w.n / 2.0, [0.03], [0.02])
    with pytest.raises(_svils.SvilsError):
        d.sweep()
    assert d.stats() == ref.stats()
    for x, y in zip(d.state() + d.expectations(), ref.state() + ref.expectations()):
        assert x.tobytes() == y.tobytes()
    d.close()
    ref.close()


def test_set_graph_twice_agrees_with_a_fresh_handle():
    w, small = Small(130, 5, seed=13), Small(130, 5, seed=14)
    small.links = small.links[::5]                                  # a smaller graph the second time
    small.linkset = {tuple(int(x) for x in e) for e in small.links}
    small.skip = set(sorted(small.skip)[:4])
    d = w.handle(True)
    d.step_node([HUB], w.n / 2.0, [0.03], [0.02])
    d.set_graph(small.links, sorted(small.skip))
    d.set_state(small.gamma, small.lam)
    fresh = small.handle(True)
    stars = [small.star(a, 20, c) for c, a in enumerate((HUB, 9, 129))]
    lst = np.array([e for e in sorted(small.linkset) if e not in small.skip][:40])
    for h in (d, fresh):
        h.step_node([HUB, 64], small.n / 2.0, [0.03, 0.03], [0.02, 0.02])
        h.step_pairs([lst], [40.0], [0.05], [0.02])
        h.step_star(stars)
    _same_bits(d, fresh, "after the second set_graph")
    d.close()
    fresh.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the command line
# ---------------------------------------------------------------------------------------------------------------------
def _run(args, out, cwd=None, timeout=300):
    out.mkdir(exist_ok=True)
    r = subprocess.run([SVINET] + args + ["-outdir", str(out)], capture_output=True, text=True, timeout=timeout, cwd=cwd)
    assert r.returncode == 0, (args, r.stderr[-2000:])
    dirs = [p for p in out.iterdir() if p.is_dir()]
    assert len(dirs) == 1
    return dirs[0]


def _same_run(da, db):
    """two runs of one seed: the models and lists byte for byte, the report files without their wall-clock column"""
    for name in ("gamma.txt", "lambda.txt", "groups.txt", "communities.txt", "summary.txt"):
        assert (da / name).read_bytes() == (db / name).read_bytes(), name
    lists = sorted(p.name for p in da.iterdir() if p.name.startswith(("heldout-", "validation-")))
    assert len(lists) == 2
    for name in lists:
        assert (da / name).read_bytes() == (db / name).read_bytes(), name
    for name in ("heldout.txt", "validation.txt", "max.txt"):
        va, vb = np.atleast_2d(np.loadtxt(da / name)), np.atleast_2d(np.loadtxt(db / name))
        assert va.shape == vb.shape and np.array_equal(np.delete(va, 1, axis=1), np.delete(vb, 1, axis=1)), name   # column 1: seconds


@pytest.mark.parametrize("engine", [["-rnode"], ["-rpair"], ["-rpair", "-stratified"], ["-infset", "-rfreq", "50"], ["-snode"]])
def test_cli_writes_the_same_files_with_and_without_the_flag(graph_files, tmp_path, engine):
    work = tmp_path / "work"
    work.mkdir()
    host_api.preprocess(graph_files["assort"], 75, str(work / "neighbors.bin"))
    common = ["-file", graph_files["assort"], "-n", "75", "-k", "4", "-seed", "3", "-heldout-ratio", "0.1", "-no-stop", "-max-iterations", "149"]
    da = _run(common + engine, tmp_path / "dense", cwd=str(work))
    db = _run(common + engine + ["-sparse-graph"], tmp_path / "sparse", cwd=str(work))
    assert da.name == db.name and len(np.loadtxt(da / "heldout.txt")) >= 2
    _same_run(da, db)


def test_cli_above_the_cap_agrees_with_the_engines(big, tmp_path):
    """-preprocess, then -infset and -snode with -sparse-graph on the n = 33 025 graph: 300 iterations, three reports; the
    files print the states the engines of host_api reach with sparse_graph=True through the same iterations"""
    n, k, iters = BIG_N, 4, 300
    graph = tmp_path / "big.txt"
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n], axis=1)            # every node is seen, in order: ids are sequence numbers
    with open(graph, "w") as f:
        for p, q in np.concatenate([ring, big.links.astype(np.int64)]):
            f.write("%d\t%d\n" % (p, q))
    common = ["-file", str(graph), "-n", str(n), "-k", str(k), "-seed", "2"]
    pre = _run(common + ["-preprocess"], tmp_path / "pre")
    assert (pre / "neighbors.bin").stat().st_size > 12 * n
    r = subprocess.run([SVINET] + common + ["-snode", "-outdir", str(tmp_path / "none")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "32768" in r.stderr and not (tmp_path / "none").exists()
    for name, flags, make in (("infset", ["-infset", "-rfreq", "100"], lambda: InfsetEngine(str(graph), n, k, str(pre / "neighbors.bin"), on_device=True, seed=2, sparse_graph=True)),
                              ("snode", ["-snode"], lambda: StratNodeEngine(str(graph), n, k, on_device=True, seed=2, sparse_graph=True))):
        run = _run(common + flags + ["-sparse-graph", "-no-stop", "-max-iterations", str(iters - 1)], tmp_path / name, cwd=str(pre), timeout=600)
        assert list(np.loadtxt(run / "heldout.txt")[:, 0]) == [0, 100, 200, 300]
        fg, fl = np.loadtxt(run / "gamma.txt")[:, 2:], np.loadtxt(run / "lambda.txt")[:, 1:]
        assert fg.shape == (n, k) and np.all(fg > 0)
        e = make()
        assert e.n == n
        for _ in range(iters // 100):
            e.step(100)
            assert not e.report()
        assert np.all(np.abs(fg - e.gamma) <= 0.5e-5 * (1 + 1e-6)) and np.all(np.abs(fl - e.lam) <= 0.5e-5 * (1 + 1e-6)), name
        e.close()


def test_sampled_engine_takes_the_flag(graph_files):
    a = SampledEngine(graph_files["assort"], 75, 4, "rnode", on_device=True, heldout_ratio=0.1, seed=5)
    b = SampledEngine(graph_files["assort"], 75, 4, "rnode", on_device=True, heldout_ratio=0.1, seed=5, sparse_graph=True)
    for e in (a, b):
        e.step(20)
    assert a.gamma.tobytes() == b.gamma.tobytes() and a.lam.tobytes() == b.lam.tobytes()
    a.close()
    b.close()
