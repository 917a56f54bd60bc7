"""-m gpu: link queries of a fitted -orig state (svils_orig_link_prob / _predict_links / _rank_links, csrc/svils_orig_predict.hip;
-orig -clean-holdout -predict-pairs / -recommend / -rank-pairs / -rank-heldout).

Two references, as in test_gpu_rank.py.  The exact one is the library's own top-k list: a node at place j of p's list must
have the list's score bitwise, above <= j <= above + tied, and above + tied == j where the next score is strictly lower.
The independent one is the numpy fp64 restatement of tests/orig_pair_cases.py: scores at rtol 1e-12 (two dot products of at
most 64 positive terms: a relative error below 2 * 64 * 2^-53 = 1.4e-14), counts inside the interval
lo = #{S > s (1 + 1e-12)} <= above, above + tied <= hi = #{S >= s (1 - 1e-12)}, with lo == hi for at least 99 % of a
shape's pairs so that the interval cannot hide a wrong count, and ncand exact."""
import functools
import glob
import os
import subprocess

import numpy as np
import pytest

import orig_cases as OC
import orig_pair_cases as PC
from conftest import GOLDEN
from pair_cases import NONE, _bits, _random_pairs
from svinet_amd import _svils
from svinet_amd.host_api import OrigEngine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
ASSORT = os.path.join(GOLDEN, "graphs", "assort-75-4.txt")
ERR_ARG, ERR_UNSUPPORTED = -1, -4
RTOL = 1e-7

# (n, K, hub): the smallest K; an odd K with two 16-column chunks (a row of gamma is not 16-byte aligned) and a hub whose
# exclusions fall in every tile; three chunks, many tiles and several candidate chunks; the largest K.  No n is a multiple of 64
SHAPES = [(65, 2, None), (530, 17, 200), (2000, 37, None), (1100, 64, None)]


@functools.lru_cache(maxsize=None)
def _case(n, k, hub, ties=False):
    """the state, its numpy side and 600 random pairs (with the hub: pairs from it and to it first): computed once, shared,
    never written to"""
    links, skip, gamma, beta = PC.random_state(n, k, 4 * n, seed=100 * k + n, ties=ties, hub=hub)
    pairs = _random_pairs(np.random.default_rng(n), n, 600)
    if hub is not None:
        others = np.array([0, n - 1, 1, 2, 3, 4, 5, 6, 63, 64, 65, 127, 128, 129, 255, 256], dtype=np.uint32)
        h = np.full(len(others), hub, dtype=np.uint32)
        pairs = np.concatenate([np.stack([h, others], 1), np.stack([others, h], 1), pairs[:600 - 2 * len(others)]])
    ex, P = PC.excluded(n, links, skip), PC.pi_of(gamma)
    for a in (links, skip, gamma, beta, pairs, ex, P):
        a.setflags(write=False)
    return links, skip, gamma, beta, pairs, ex, P


@pytest.mark.parametrize("n,k,hub", SHAPES)
def test_scores_and_ranks_match_numpy(n, k, hub):
    links, skip, gamma, beta, pairs, ex, P = _case(n, k, hub)
    assert len(pairs) == 600
    if hub is not None:
        assert ex[hub, 0] and ex[hub, n - 1] and all(ex[hub, t:t + 64].any() for t in range(0, n, 64))   # exclusions in every tile
    dev = PC.device(n, k, links, skip, gamma, beta)
    ref = PC.rank_ref(P, beta, ex, pairs)
    res = dev.rank_links(pairs)
    PC.check_against_numpy(res, ref)
    prob = dev.link_prob(pairs)
    np.testing.assert_allclose(prob, ref[3], rtol=1e-12, atol=0)
    assert np.array_equal(prob.view(np.uint64), res[3].view(np.uint64))


@pytest.mark.parametrize("n,k,hub", SHAPES)
def test_ranks_agree_exactly_with_the_topk_lists(n, k, hub):
    links, skip, gamma, beta, _, ex, _ = _case(n, k, hub)
    dev = PC.device(n, k, links, skip, gamma, beta)
    nodes = np.random.default_rng(7).choice(n, size=min(300, n), replace=False).astype(np.uint32)
    if hub is not None:
        nodes[0] = hub if hub not in nodes else nodes[0]
    ntied, nstrict = PC.check_against_topk(dev, n, ex, nodes, topk=25)
    print("rank vs top-k: %d ranked entries tied with another, %d strict steps" % (ntied, nstrict))
    assert nstrict > 0


@pytest.mark.parametrize("n,strict", [(300, True), (3000, False)])
def test_exact_ties_agree_with_the_topk_lists(n, strict):
    """gamma entries in {1, 2, 3}, beta entries in {1/4, 1/2, 3/4}, K = 3: a few dozen distinct rows of pi, so a query's scores
    tie exactly in large groups -- the numpy interval says nothing here (lo != hi everywhere), the lists say everything"""
    links, skip, gamma, beta, _, ex, _ = _case(n, 3, None, ties=True)
    dev = PC.device(n, 3, links, skip, gamma, beta)
    nodes = np.random.default_rng(7).choice(n, size=300, replace=False).astype(np.uint32)
    ntied, nstrict = PC.check_against_topk(dev, n, ex, nodes, topk=25)
    print("rank vs top-k: %d ranked entries tied with another, %d strict steps" % (ntied, nstrict))
    assert ntied > 0
    assert nstrict > 0 or not strict


def test_the_score_is_not_symmetric():
    """beta far from symmetric: score(p, q) and score(q, p) differ, each matches numpy, and neither matches numpy with beta
    transposed"""
    n, k = 130, 5
    links, skip, gamma, _ = PC.random_state(n, k, 400, seed=3)
    beta = np.clip(np.triu(np.full((k, k), 0.9)) + 0.02, 0.01, 0.99)   # 0.92 on and above the diagonal, 0.02 below
    assert np.abs(beta - beta.T).max() > 0.8
    dev = PC.device(n, k, links, skip, gamma, beta)
    pq = _random_pairs(np.random.default_rng(1), n, 200)
    qp = np.ascontiguousarray(pq[:, ::-1])
    P = PC.pi_of(gamma)
    fwd, bwd = dev.link_prob(pq), dev.link_prob(qp)
    want_f = np.einsum("ig,gh,ih->i", P[pq[:, 0]], beta, P[pq[:, 1]])
    want_b = np.einsum("ig,gh,ih->i", P[pq[:, 1]], beta, P[pq[:, 0]])
    np.testing.assert_allclose(fwd, want_f, rtol=1e-12, atol=0)
    np.testing.assert_allclose(bwd, want_b, rtol=1e-12, atol=0)
    assert np.all(np.abs(fwd / bwd - 1) > 1e-6)
    assert np.all(np.abs(fwd / want_b - 1) > 1e-6)      # the transposed beta is another answer, everywhere
    ex = PC.excluded(n, links, skip)
    PC.check_against_numpy(dev.rank_links(qp), PC.rank_ref(P, beta, ex, qp))
    with pytest.raises(AssertionError):
        PC.check_against_numpy(dev.rank_links(qp), PC.rank_ref(P, beta.T.copy(), ex, qp))


def test_candidate_rule():
    """a link skipped only as (p, c), only as (c, p), or in both orientations is a candidate of both ends; an unskipped link
    is not; a skipped non-link changes nothing"""
    n, k = 70, 3
    rng = np.random.default_rng(5)
    gamma, beta = rng.random((n, k)) + 0.01, np.clip(rng.random((k, k)), 0.01, 0.99)
    links = np.array([(1, 2), (3, 4), (5, 6), (7, 8), (9, 10)], dtype=np.uint32)
    skip = [(1, 2), (4, 3), (5, 6), (6, 5), (11, 12)]   # (7, 8) and (9, 10) are trained on; (11, 12) is no link
    dev = PC.device(n, k, links, skip, gamma, beta)
    ids, _ = dev.predict_links(n, np.arange(n, dtype=np.uint32))
    lists = [set(r[r != NONE].tolist()) for r in ids]
    for a, b in ((1, 2), (3, 4), (5, 6), (11, 12)):
        assert b in lists[a] and a in lists[b], (a, b)
    for a, b in ((7, 8), (9, 10)):
        assert b not in lists[a] and a not in lists[b], (a, b)
    for p in range(n):
        gone = {p} | ({8} if p == 7 else {7} if p == 8 else {10} if p == 9 else {9} if p == 10 else set())
        assert lists[p] == set(range(n)) - gone
    plain = PC.device(n, k, links, [(1, 2), (4, 3), (5, 6), (6, 5)], gamma, beta)   # without the skipped non-link
    for a, b in zip(_bits(dev.predict_links(10)), _bits(plain.predict_links(10))):
        assert np.array_equal(a, b)
    pairs = np.array([(1, 2), (2, 1), (7, 8), (8, 7), (11, 12), (20, 21)], dtype=np.uint32)
    ncand = dev.rank_links(pairs)[2]
    assert ncand.tolist() == [n - 2, n - 2, n - 2, n - 2, n - 2, n - 2]   # q is never counted; 7 and 8 lose only each other
    assert dev.rank_links([(7, 20)])[2][0] == n - 3
    PC.check_against_numpy(dev.rank_links(pairs), PC.rank_ref(PC.pi_of(gamma), beta, PC.excluded(n, links, skip), pairs))


def test_topk_edges():
    """topk = 1 and 256; n = 65 with topk = 256 (the filled slots); nodes = NULL; batches of 1, 63, 64 and 65 query nodes; a row
    is the same bits alone and among others; the same call twice gives the same bits"""
    n, k, hub = SHAPES[1]
    links, skip, gamma, beta, _, ex, P = _case(n, k, hub)
    dev = PC.device(n, k, links, skip, gamma, beta)
    all_ids, all_sc = dev.predict_links(256)                       # nodes = NULL
    assert all_ids.shape == (n, 256)
    for a, b in zip(_bits(dev.predict_links(256)), _bits((all_ids, all_sc))):
        assert np.array_equal(a, b)
    for p in (0, hub, n - 1):
        want_ids, want_sc = PC.topk_ref(P, beta, ex, p, 256)
        np.testing.assert_allclose(all_sc[p], want_sc, rtol=1e-12, atol=0)
        clear = np.abs(np.diff(want_sc)) > 1e-11 * want_sc[:-1]    # places numpy's own order is sure of
        ok = np.concatenate([[True], clear]) & np.concatenate([clear, [True]])
        assert np.array_equal(all_ids[p][ok], want_ids[ok])
    one_ids, one_sc = dev.predict_links(1)
    assert np.array_equal(one_ids[:, 0], all_ids[:, 0]) and np.array_equal(one_sc[:, 0].view(np.uint64), all_sc[:, 0].view(np.uint64))
    rng = np.random.default_rng(9)
    for m in (1, 63, 64, 65):
        nodes = rng.choice(n, size=m, replace=False).astype(np.uint32)
        ids, sc = dev.predict_links(256, nodes)
        assert np.array_equal(ids, all_ids[nodes]) and np.array_equal(sc.view(np.uint64), all_sc[nodes].view(np.uint64))
    # fewer candidates than slots
    n2, k2, _ = SHAPES[0]
    links2, skip2, gamma2, beta2, _, ex2, P2 = _case(n2, k2, None)
    small = PC.device(n2, k2, links2, skip2, gamma2, beta2)
    ids, sc = small.predict_links(256)
    for p in range(n2):
        cnt = n2 - 1 - int(ex2[p].sum())
        assert np.all(ids[p, :cnt] != NONE) and np.all(ids[p, cnt:] == NONE) and np.all(sc[p, cnt:] == -1.0)
        assert set(ids[p, :cnt].tolist()) == set(np.nonzero(~ex2[p])[0].tolist()) - {p}
        assert np.all(np.diff(sc[p, :cnt]) <= 0)
        np.testing.assert_allclose(sc[p, :cnt], PC.topk_ref(P2, beta2, ex2, p, 256)[1], rtol=1e-12, atol=0)


def test_a_pair_does_not_depend_on_the_rest_of_the_call():
    n, k, hub = SHAPES[2]
    links, skip, gamma, beta, pairs, _, _ = _case(n, k, hub)
    dev = PC.device(n, k, links, skip, gamma, beta)
    rng = np.random.default_rng(4)
    mine = pairs[:70]
    alone = _bits(dev.rank_links(mine))
    crowd = np.concatenate([mine, _random_pairs(rng, n, 9000)])          # more than one internal batch
    perm = rng.permutation(len(crowd))
    inside = _bits(dev.rank_links(crowd[perm]))
    where = np.argsort(perm)[:70]
    for a, b in zip(alone, inside):
        assert np.array_equal(a, b[where])
    assert np.array_equal(dev.link_prob(crowd[perm])[where].view(np.uint64), alone[3])


def _peaked_device():
    """a state that sweeps without a degenerate block (tests/test_gpu_orig.py sweeps it five times)"""
    k, n, seed = 4, 89, 22
    links, gamma, beta = OC.peaked_state(seed, n, k)
    skip = [(int(a), int(b)) for a, b in links[:6]] + [(int(b), int(a)) for a, b in links[3:9]]
    return n, k, links, skip, PC.device(n, k, links, skip, gamma, beta)


def test_queries_follow_the_state():
    """query, sweep, query again: the second answer is that of the new state; the same after svils_orig_set_state"""
    n, k, links, skip, dev = _peaked_device()
    ex = PC.excluded(n, links, skip)
    pairs = _random_pairs(np.random.default_rng(2), n, 200)
    nodes = np.arange(n, dtype=np.uint32)

    def ask():
        g, b = dev.state()
        res, prob, (ids, sc) = dev.rank_links(pairs), dev.link_prob(pairs), dev.predict_links(5, nodes)
        PC.check_against_numpy(res, PC.rank_ref(PC.pi_of(g), b, ex, pairs))
        np.testing.assert_allclose(prob, res[3], rtol=0, atol=0)
        np.testing.assert_allclose(sc[0], PC.topk_ref(PC.pi_of(g), b, ex, 0, 5)[1], rtol=1e-12, atol=0)
        return _bits(res) + _bits((ids, sc))

    first = ask()
    dev.sweep(1)
    second = ask()
    assert not np.array_equal(first[3], second[3]) and not np.array_equal(first[5], second[5])
    rng = np.random.default_rng(8)
    dev.set_state(rng.random((n, k)) + 0.01, np.clip(rng.random((k, k)), 0.01, 0.99))
    third = ask()
    assert not np.array_equal(second[3], third[3]) and not np.array_equal(second[5], third[5])


def test_queries_do_not_disturb_the_sweeps():
    n, k, links, skip, a = _peaked_device()
    _, _, _, _, b = _peaked_device()
    a.sweep(1)
    before = _bits(a.state())
    a.rank_links([(0, 1), (5, 2)])
    a.predict_links(3)
    a.link_prob([(4, 3)])
    for x, y in zip(before, _bits(a.state())):
        assert np.array_equal(x, y)
    a.sweep(2)
    b.sweep(3)
    for x, y in zip(_bits(a.state()), _bits(b.state())):
        assert np.array_equal(x, y)


def test_errors():
    n, k, hub = SHAPES[0]
    links, skip, gamma, beta, _, _, _ = _case(n, k, hub)
    dev = PC.device(n, k, links, skip, gamma, beta)
    L, h = _svils.load(), dev._h
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
    out, ids, cnt = np.zeros(4), np.zeros((n, 256), dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    sc = np.zeros((n, 256))
    for bad in ([(4, 4)], [(0, n)], [(n, 0)]):
        pr = u32(bad)
        assert L.svils_orig_link_prob(h, pr.ctypes.data, 1, out.ctypes.data) == ERR_ARG
        assert L.svils_orig_rank_links(h, pr.ctypes.data, 1, cnt.ctypes.data, None, None, None) == ERR_ARG
    assert b"p == q" in L.svils_last_error() or b">= n" in L.svils_last_error()
    for topk in (0, 257):
        assert L.svils_orig_predict_links(h, None, 0, topk, ids.ctypes.data, sc.ctypes.data) == ERR_ARG
    nodes = u32([0, n])
    assert L.svils_orig_predict_links(h, nodes.ctypes.data, 2, 3, ids.ctypes.data, sc.ctypes.data) == ERR_ARG
    assert L.svils_orig_predict_links(h, None, 5, 3, ids.ctypes.data, sc.ctypes.data) == ERR_ARG   # NULL means all n
    assert L.svils_orig_predict_links(h, None, 0, 3, None, None) == ERR_ARG
    null = (L.svils_orig_link_prob(None, None, 0, None), L.svils_orig_predict_links(None, None, 0, 1, None, None),
            L.svils_orig_rank_links(None, None, 0, None, None, None, None))
    assert null == (ERR_ARG,) * 3
    pr = u32([(0, 1), (2, 3)])
    assert L.svils_orig_link_prob(h, pr.ctypes.data, 2, None) == ERR_ARG
    assert L.svils_orig_rank_links(h, pr.ctypes.data, 2, None, None, None, None) == 0      # any output may be NULL
    only = np.zeros(2, dtype=np.uint32)
    assert L.svils_orig_rank_links(h, pr.ctypes.data, 2, None, only.ctypes.data, None, None) == 0
    assert np.array_equal(only, dev.rank_links(pr)[1])
    assert L.svils_orig_rank_links(h, None, 0, None, None, None, None) == 0
    assert all(len(x) == 0 for x in dev.rank_links(np.zeros((0, 2), dtype=np.uint32)))
    bare = _svils.Orig(n, k, 1.0 / k)                        # no graph, no state
    nostate = _svils.Orig(n, k, 1.0 / k)
    nostate.set_graph(links, skip)
    for d in (bare, nostate):
        for call in (lambda: d.link_prob(pr), lambda: d.predict_links(3), lambda: d.rank_links(pr)):
            with pytest.raises(_svils.SvilsError) as ei:
                call()
            assert ei.value.code == ERR_ARG
    g, b = dev.state()
    assert np.array_equal(g, gamma) and np.array_equal(b, beta)


def test_a_degenerate_state_is_refused_and_left_alone():
    """the complete graph of tests/test_gpu_orig.py: every beta is exactly 1 after one sweep and the flag is up"""
    n, k = 6, 3
    links = np.array([(a, b) for a in range(n) for b in range(a + 1, n)], dtype=np.uint32)
    rs = np.random.RandomState(63)
    gamma, beta = rs.gamma(100.0, 0.01, size=(n, k)), OC.init_beta1(rs, k)
    dev = PC.device(n, k, links, (), gamma, beta)
    assert dev.rank_links([(0, 1)])[2][0] == 0               # all five others are training neighbours of 0
    dev.sweep(1)
    before = _bits(dev.state(check=False))
    for call in (lambda: dev.link_prob([(0, 1)]), lambda: dev.predict_links(2), lambda: dev.rank_links([(0, 1)])):
        with pytest.raises(_svils.SvilsError) as ei:
            call()
        assert ei.value.code == ERR_UNSUPPORTED and "left (0, 1)" in str(ei.value)
    for x, y in zip(before, _bits(dev.state(check=False))):
        assert np.array_equal(x, y)


def _directed(pairs):
    pairs = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    return np.ascontiguousarray(np.stack([pairs, pairs[:, ::-1]], 1).reshape(-1, 2))


def _held_links(e):
    """the y = 1 lines of heldout-edges.txt, then of validation-edges.txt, as listed"""
    adj = OC.adjacency(e.n, e.edges)
    both = np.concatenate([e.heldout, e.validation])
    return both[adj[both[:, 0], both[:, 1]] == 1]


def _run(args, cwd):
    r = subprocess.run([SVINET] + args, capture_output=True, text=True, timeout=300, cwd=str(cwd))
    assert r.returncode == 0, r.stderr
    d = glob.glob(os.path.join(str(cwd), "n*-k*"))
    assert len(d) == 1
    return d[0]


def _rank_lines(e, pairs, ids):
    """the lines of a rank file for `pairs`, formatted from the engine's answers"""
    above, tied, ncand, score = e.rank_links(_directed(pairs))
    adj = OC.adjacency(e.n, e.edges)
    out = []
    for i, (p, q) in enumerate(np.asarray(pairs).tolist()):
        f = ["%d" % ids[p], "%d" % ids[q], "%d" % adj[p, q], "%.9e" % score[2 * i]]
        for d in (2 * i, 2 * i + 1):
            f += ["%.3f" % (above[d] + 0.5 * tied[d] + 1.0), "%d" % ncand[d]]
        out.append("\t".join(f))
    return out


def test_cli_clean_holdout_queries(tmp_path):
    base = ["-file", ASSORT, "-n", "75", "-k", "4", "-orig", "-max-iterations", "3", "-heldout-ratio", "0.1"]
    for w in ("dev", "host", "plain"):
        (tmp_path / w).mkdir()
    pf = tmp_path / "pairs.txt"
    d = _run(base + ["-clean-holdout", "-recommend", "5", "-rank-heldout"], tmp_path / "dev")
    e = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, clean_holdout=True)
    for _ in range(3):
        e.sweep()
    gt = np.loadtxt(os.path.join(d, "gamma.txt"))
    ids = gt[:, 1].astype(np.int64)
    # heldout-ranks.txt: every line is the engine's answer
    held = _held_links(e)
    lines = open(os.path.join(d, "heldout-ranks.txt")).read().splitlines()
    assert len(held) > 0 and lines == _rank_lines(e, held, ids)
    head, vals = [l.split("\t") for l in open(os.path.join(d, "link-ranks-summary.txt")).read().splitlines()]
    assert head == ["pairs", "auc", "mrr", "hits1", "hits10", "hits100", "chance10"] and int(vals[0]) == 2 * len(held)
    # recommendations.txt: one line per node in groups.txt order, id then (id, score) x 5
    rec = [l.split("\t") for l in open(os.path.join(d, "recommendations.txt")).read().splitlines()]
    rid, rsc = e.predict_links(5)
    assert len(rec) == 75 and all(len(r) == 11 for r in rec)
    for p, r in enumerate(rec):
        assert int(r[0]) == ids[p]
        assert [int(x) for x in r[1::2]] == ids[rid[p]].tolist() and r[2::2] == ["%.9e" % s for s in rsc[p]]
    assert not os.path.exists(os.path.join(d, "link-prob.txt")) and not os.path.exists(os.path.join(d, "link-ranks.txt"))
    # -predict-pairs / -rank-pairs: the same run again with a pair file (external ids, both orientations of a few pairs)
    some = np.concatenate([held[:5], held[:5, ::-1], np.array([(0, 1), (1, 0), (10, 50)])])
    pf.write_text("".join("%d\t%d\n" % (ids[p], ids[q]) for p, q in some.tolist()))
    d2 = _run(base + ["-clean-holdout", "-predict-pairs", str(pf), "-rank-pairs", str(pf)], tmp_path / "dev")
    assert d2 == d
    assert open(os.path.join(d, "link-ranks.txt")).read().splitlines() == _rank_lines(e, some, ids)
    adj = OC.adjacency(e.n, e.edges)
    want = ["%d\t%d\t%d\t%.9e" % (ids[p], ids[q], adj[p, q], s) for (p, q), s in zip(some.tolist(), e.link_prob(some))]
    assert open(os.path.join(d, "link-prob.txt")).read().splitlines() == want
    # gamma / beta against the host loops with the same hold-out
    hd = _run(base + ["-clean-holdout", "-host-loops"], tmp_path / "host")
    for f in ("gamma.txt", "beta.txt"):
        np.testing.assert_allclose(np.loadtxt(os.path.join(d, f)), np.loadtxt(os.path.join(hd, f)), rtol=RTOL)
    # without the flag the run is the one it always was: the files of the engine without clean hold-out, to the last digit
    pd = _run(base, tmp_path / "plain")
    o = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, clean_holdout=False)
    for _ in range(3):
        o.sweep()
    got_g = [l.split("\t")[2:] for l in open(os.path.join(pd, "gamma.txt")).read().splitlines()]
    assert got_g == [["%.5f" % x for x in row] for row in o.gamma]
    got_b = [l.split("\t") for l in open(os.path.join(pd, "beta.txt")).read().splitlines()]
    assert got_b == [["%.12g" % x for x in row] for row in o.beta]
    assert not np.array_equal(o.beta, e.beta)                # and the flag does change what is trained on
    assert not [f for f in os.listdir(pd) if "rank" in f or "recommend" in f or "link-prob" in f]


def test_engine_clean_holdout_skips_both_orientations_of_both_sets():
    e = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, clean_holdout=True)
    plain = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, clean_holdout=False)
    assert np.array_equal(e.heldout, plain.heldout) and np.array_equal(e.validation, plain.validation)
    assert np.array_equal(e.gamma, plain.gamma) and np.array_equal(e.beta, plain.beta)
    adj = OC.adjacency(e.n, e.edges)
    both = np.concatenate([e.heldout, e.validation]).astype(np.int64)
    skip = sorted({(p, q) for p, q in both.tolist()} | {(q, p) for p, q in both.tolist()})
    g, b, _, bad = OC.sweep(e.gamma, e.beta, adj, skip, 0.25)
    assert not bad.any()
    e.sweep()
    np.testing.assert_allclose(e.gamma, g, rtol=RTOL)
    np.testing.assert_allclose(e.beta, b, rtol=RTOL)
    # every held-out link is a candidate of both its ends, a training link of neither
    ids, _ = e.predict_links(74)
    lists = [set(r[r != NONE].tolist()) for r in ids]
    for p, q in _held_links(e).tolist():
        assert q in lists[p] and p in lists[q]
    held = {(p, q) for p, q in skip}
    train = [(int(p), int(q)) for p, q in e.edges if (int(p), int(q)) not in held]
    assert train and all(q not in lists[p] and p not in lists[q] for p, q in train)
    host = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, clean_holdout=True, on_device=False)
    with pytest.raises(_svils.SvilsError):
        host.rank_links([(0, 1)])


def test_disassortative_demonstration(tmp_path):
    """a planted two-group graph with links ACROSS the groups: the K x K model ranks its held-out links from the block rates.
    Prints the mean per-link AUC of the command line's summary; asserts only that the device's ranks are numpy's on the
    fetched state"""
    gf = tmp_path / "two-groups.txt"
    PC.planted_two_groups(str(gf))
    d = _run(["-file", str(gf), "-n", "200", "-k", "2", "-orig", "-clean-holdout", "-max-iterations", "20", "-heldout-ratio", "0.1",
              "-rank-heldout"], tmp_path)
    head, vals = [l.split("\t") for l in open(os.path.join(d, "link-ranks-summary.txt")).read().splitlines()]
    print("planted two groups, n = 200, K = 2, 20 sweeps, clean hold-out: %s directed held-out links, mean per-link AUC %.4f, "
          "MRR %.4f, hits@10 %.4f (chance %.4f)" % (vals[0], float(vals[1]), float(vals[2]), float(vals[4]), float(vals[6])))
    e = OrigEngine(str(gf), 200, 2, heldout_ratio=0.1, clean_holdout=True)
    for _ in range(20):
        e.sweep()
    pairs = _directed(_held_links(e))
    both = np.concatenate([e.heldout, e.validation]).astype(np.int64)
    skip = sorted({(p, q) for p, q in both.tolist()} | {(q, p) for p, q in both.tolist()})
    ex = PC.excluded(e.n, e.edges, skip)
    PC.check_against_numpy(e.rank_links(pairs), PC.rank_ref(PC.pi_of(e.gamma), e.beta, ex, pairs))
    print("beta of the fitted state:\n%s" % e.beta)
