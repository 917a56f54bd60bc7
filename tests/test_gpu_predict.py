"""-m gpu: link prediction from a fitted state (svils_link_prob / svils_predict_links, -predict-pairs / -recommend).

The reference here is a numpy fp64 restatement written in this file: P = gamma / gamma.sum(1), beta = l0 / (l0 + l1),
link_prob(p, q) = sum_z P_pz P_qz beta_z (src/linksampling.hh:240-256); the top-k check is tie-aware."""
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pair_cases import NONE, _lfr_setup, _nbrs, _pb, _random_links, _same, _state_bits

pytestmark = pytest.mark.gpu

SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")


def _pair_ref(P, beta, pairs):
    return np.sum(P[pairs[:, 0]] * P[pairs[:, 1]] * beta, axis=1)


def _check_topk(ids, sc, P, beta, nodes, k, nbrs):
    """ids distinct, neither self nor training neighbours, scores non-increasing (ties by ascending id) and equal to numpy's
    at the returned ids, and the returned set equals numpy's top k up to ids whose score lies within 1e-12 max of the k-th"""
    n = P.shape[0]
    assert ids.shape == (len(nodes), k) and sc.shape == (len(nodes), k)
    for r0 in range(0, len(nodes), 256):
        rows = np.asarray(nodes[r0:r0 + 256])
        S = (P[rows] * beta) @ P.T
        for i, p in enumerate(rows):
            row_ids, row_sc = ids[r0 + i], sc[r0 + i]
            cand = np.ones(n, bool)
            cand[p] = False
            cand[nbrs[p]] = False
            ncand = int(cand.sum())
            nv = min(k, ncand)
            assert np.all(row_ids[:nv] != NONE) and np.all(row_ids[nv:] == NONE) and np.all(row_sc[nv:] == -1.0), p
            got = row_ids[:nv].astype(np.int64)
            assert len(set(got.tolist())) == nv and cand[got].all(), p
            gs = row_sc[:nv]
            assert np.all(np.diff(gs) <= 0), p
            tie = np.diff(gs) == 0
            assert np.all(np.diff(got)[tie] > 0), p
            np.testing.assert_allclose(gs, S[i, got], rtol=1e-12, atol=1e-300)
            cid = np.nonzero(cand)[0]
            order = cid[np.lexsort((cid, -S[i, cid]))][:nv]
            if nv == 0:
                continue
            kth = S[i, order[-1]]
            tol = 1e-12 * max(S[i, cid].max(), 1e-300)
            for q in set(got.tolist()) ^ set(order.tolist()):
                assert abs(S[i, q] - kth) <= tol, (p, q, S[i, q], kth)


def _random_engine(n, k, m, seed, ties=False):
    from svinet_amd import _svils
    rng = np.random.default_rng(seed)
    links = _random_links(rng, n, m)
    eng = _svils.Engine(n, k, ones=len(links), ones_prob=len(links) / (n * (n - 1) / 2), use_validation_stop=False)
    eng.set_graph(links)
    gamma = rng.integers(1, 4, size=(n, k)).astype(np.float64) if ties else rng.random((n, k)) + 0.01
    lam = rng.random((k, 2)) + 0.1
    eng.set_state(gamma, lam)
    return eng, links, gamma, lam


def test_pair_scores_match_numpy_and_the_likelihood(graph_files):
    s = _lfr_setup(graph_files)
    eng = s.engine(use_validation_stop=False)
    eng.sweep(20)
    g, lam, _ = eng.state()
    P, beta = _pb(g, lam)
    rng = np.random.default_rng(1)
    pairs = rng.integers(0, s.n, size=(100000, 2))
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    vs = s.validation_sorted
    allp = np.concatenate([pairs, vs[:, :2].astype(np.int64)])
    prob = eng.link_prob(allp)
    np.testing.assert_allclose(prob, _pair_ref(P, beta, allp), rtol=1e-13, atol=0)
    assert np.array_equal(prob, eng.link_prob(allp))                      # bitwise repeatable
    ones = vs[vs[:, 2] == 1]
    lp = eng.link_prob(ones[:, :2])
    row = eng.validation_row()
    assert abs(np.mean(np.log(np.maximum(lp, 1e-30))) - row[5]) <= 1e-12   # column mean1 of the held-out likelihood


def test_topk_lfr_all_nodes(graph_files):
    s = _lfr_setup(graph_files)
    eng = s.engine(use_validation_stop=False)
    eng.sweep(20)
    g, lam, _ = eng.state()
    P, beta = _pb(g, lam)
    ids, sc = eng.predict_links(10)
    _check_topk(ids, sc, P, beta, np.arange(s.n), 10, _nbrs(s.n, s.links))
    ids2, sc2 = eng.predict_links(10)
    assert np.array_equal(ids, ids2) and np.array_equal(sc.view(np.uint64), sc2.view(np.uint64))   # two calls: bitwise equal
    sub = np.array([17, 3, 999, 3, 0, 512], dtype=np.uint32)                                         # duplicates, any order
    si, ss = eng.predict_links(10, sub)
    assert np.array_equal(si, ids[sub]) and np.array_equal(ss.view(np.uint64), sc[sub].view(np.uint64))
    assert np.array_equal(si[1], si[3])


@pytest.mark.parametrize("k,nq,topk", [(20, 512, 100), (200, None, 50)])
def test_topk_astroph(graph_files, k, nq, topk):
    from svinet_amd.host_api import Setup
    s = Setup(graph_files["astroph"], 17903, k)
    eng = s.engine(use_validation_stop=False)
    eng.sweep(5)
    g, lam, _ = eng.state()
    P, beta = _pb(g, lam)
    rng = np.random.default_rng(k)
    nodes = rng.choice(s.n, size=512, replace=False).astype(np.uint32)
    if nq is None:
        nodes[:4] = [0, 1, 2, 3]     # the hubs: ca-AstroPh numbers them first (the degree-504 node among them)
    ids, sc = eng.predict_links(topk, nodes)
    _check_topk(ids, sc, P, beta, nodes, topk, _nbrs(s.n, s.links))


@pytest.mark.parametrize("n,k,m,nq,topk,ties", [(3000, 3, 12000, 300, 10, True), (2000, 37, 8000, 200, 25, False),
                                                 (600, 2048, 2400, 64, 256, False)])
def test_topk_random_states(n, k, m, nq, topk, ties):
    eng, links, gamma, lam = _random_engine(n, k, m, seed=k, ties=ties)
    P, beta = _pb(gamma, lam)
    nodes = np.random.default_rng(7).choice(n, size=nq, replace=False).astype(np.uint32)
    ids, sc = eng.predict_links(topk, nodes)
    _check_topk(ids, sc, P, beta, nodes, topk, _nbrs(n, links))
    pr = eng.link_prob(np.stack([np.repeat(nodes[:8], 1), ids[:8, 0]], 1))
    np.testing.assert_allclose(pr, sc[:8, 0], rtol=1e-13)


# (n, K, links, query nodes, topk), the tile-edge shapes of test_gpu_rank.SHAPES: n = 64 / 65 one candidate tile and one
# node more; K = 1, 4, 16, 17 the padding to 16 columns; 1, 63, 64, 65 query nodes the edge of the query tile; topk = 70 is
# more than the 64 candidates there can be, so the (NONE, -1.0) fill is checked
@pytest.mark.parametrize("n,k,m,nq,topk", [(64, 4, 100, 63, 10), (65, 1, 100, 64, 70), (65, 16, 120, 65, 25), (300, 17, 900, 1, 10)])
def test_topk_tile_edges(n, k, m, nq, topk):
    eng, links, gamma, lam = _random_engine(n, k, m, seed=1000 + n + k)
    P, beta = _pb(gamma, lam)
    nodes = np.random.default_rng(nq).choice(n, size=nq, replace=False).astype(np.uint32)
    ids, sc = eng.predict_links(topk, nodes)
    _check_topk(ids, sc, P, beta, nodes, topk, _nbrs(n, links))


def test_topk_many_chunks():
    n, k = 200000, 512
    eng, links, gamma, lam = _random_engine(n, k, 4 * n, seed=5)
    P, beta = _pb(gamma, lam)
    nodes = np.random.default_rng(9).choice(n, size=256, replace=False).astype(np.uint32)
    ids, sc = eng.predict_links(20, nodes)
    _check_topk(ids, sc, P, beta, nodes, 20, _nbrs(n, links))


def test_sentinel_fill_and_held_out_candidates(graph_files):
    from svinet_amd.host_api import Setup
    s = Setup(graph_files["assort"], 75, 4)
    eng = s.engine(use_validation_stop=False)
    eng.sweep(10)
    g, lam, _ = eng.state()
    P, beta = _pb(g, lam)
    ids, sc = eng.predict_links(80)
    assert np.any(ids == NONE) and np.all(sc[ids == NONE] == -1.0)
    _check_topk(ids, sc, P, beta, np.arange(s.n), 80, _nbrs(s.n, s.links))
    # every candidate appears (80 > n - 1): so do the validation links, which are not training links
    v1 = s.validation_sorted[s.validation_sorted[:, 2] == 1]
    assert len(v1)
    for p, q, _ in v1:
        assert q in ids[p] and p in ids[q]


def test_prediction_does_not_disturb_the_sweeps(graph_files):
    s = _lfr_setup(graph_files)
    a, b = s.engine(use_validation_stop=False), s.engine(use_validation_stop=False)
    pairs = s.validation_sorted[:, :2]
    a.sweep(10)
    a.predict_links(10)
    a.link_prob(pairs)
    a.sweep(10)
    b.sweep(10)
    b.sweep(10)
    _same(_state_bits(a), _state_bits(b))


def test_prediction_on_a_stopped_handle(graph_files):
    s = _lfr_setup(graph_files)
    eng = s.engine(use_validation_stop=True)
    for _ in range(100):
        eng.sweep(64)
        if eng.control().stopped:
            break
    assert eng.control().stopped
    before = _state_bits(eng)
    ids, sc = eng.predict_links(10)
    eng.link_prob(s.validation_sorted[:, :2])
    eng.sweep(4)                                       # no-ops after the stop
    _same(before, _state_bits(eng))
    g, lam, _ = eng.state()
    P, beta = _pb(g, lam)
    _check_topk(ids, sc, P, beta, np.arange(s.n), 10, _nbrs(s.n, s.links))


def test_prediction_on_a_minibatch_handle(graph_files):
    s = _lfr_setup(graph_files)
    a, b = s.engine(use_validation_stop=False), s.engine(use_validation_stop=False)
    for e in (a, b):
        e.set_stochastic(batch_nodes=100, tau0=1.0, kappa=0.5)
        e.step(10)
    ids, sc = a.predict_links(10)
    a.link_prob(s.validation_sorted[:, :2])
    a.step(10)
    b.step(10)
    _same(_state_bits(a), _state_bits(b))
    b2 = s.engine(use_validation_stop=False)
    b2.set_stochastic(batch_nodes=100, tau0=1.0, kappa=0.5)
    b2.step(10)
    g, lam, _ = b2.state()
    P, beta = _pb(g, lam)
    _check_topk(ids, sc, P, beta, np.arange(s.n), 10, _nbrs(s.n, s.links))


def test_refusals(graph_files):
    from svinet_amd import _svils
    from svinet_amd.host_api import Setup
    s = _lfr_setup(graph_files)
    ksh = _svils.Engine(s.n, 28, ones=s.ones, ones_prob=s.ones_prob, eta=s.eta, use_validation_stop=False, k_slice=(0, 28))
    ksh.set_graph(s.links)
    for call in (lambda: ksh.predict_links(5), lambda: ksh.link_prob([[0, 1]])):
        with pytest.raises(_svils.SvilsError) as ei:
            call()
        assert ei.value.code == -4 and "K-sharded" in str(ei.value)
    rng = np.random.default_rng(3)
    t = Setup(n=20, k=2100, pairs=_random_links(rng, 20, 80).astype(np.int32) + 1, heldout_ratio=0.05)
    tiled = t.engine(use_validation_stop=False)
    with pytest.raises(_svils.SvilsError) as ei:
        tiled.predict_links(5)
    assert ei.value.code == -4 and "column-tiled" in str(ei.value)
    eng = s.engine(use_validation_stop=False)
    for call in (lambda: eng.predict_links(5, [s.n]), lambda: eng.link_prob([[0, s.n]]), lambda: eng.link_prob([[4, 4]]),
                 lambda: eng.predict_links(0), lambda: eng.predict_links(257)):
        with pytest.raises(_svils.SvilsError) as ei:
            call()
        assert ei.value.code == -1
    bare = _svils.Engine(s.n, 28, ones=s.ones, ones_prob=s.ones_prob)
    with pytest.raises(_svils.SvilsError) as ei:
        bare.predict_links(5)
    assert ei.value.code == -1


def test_usefulness_on_lfr(graph_files):
    """fitted to the stop rule, link_prob ranks held-out links above held-out non-links, and the top-10 lists find held-out
    links far more often than chance"""
    s = _lfr_setup(graph_files)
    eng = s.engine(use_validation_stop=True)
    for _ in range(100):
        eng.sweep(64)
        if eng.control().stopped:
            break
    vs = s.validation_sorted
    prob = eng.link_prob(vs[:, :2])
    y = vs[:, 2] == 1
    pos, neg = prob[y], prob[~y]
    auc = (np.sum(pos[:, None] > neg[None, :]) + 0.5 * np.sum(pos[:, None] == neg[None, :])) / (len(pos) * len(neg))
    ids, _ = eng.predict_links(10)
    nb = _nbrs(s.n, s.links)
    hit, rate = [], []
    for p, q, _ in vs[y]:
        for a, b in ((p, q), (q, p)):
            hit.append(b in ids[a])
            rate.append(10.0 / (s.n - 1 - len(nb[a])))
    print("usefulness: AUC %.4f, held-out links in top-10 %.4f, random rate %.5f" % (auc, np.mean(hit), np.mean(rate)))
    assert auc >= 0.8
    assert np.mean(hit) >= 10 * np.mean(rate)


def _cli_predict(graph_files, tmp_path, extra):
    from svinet_amd.host_api import Setup
    s = Setup(graph_files["lfr"], 1000, 28)
    rng = np.random.default_rng(2)
    pp = [(s.seq2id[p], s.seq2id[q]) for p, q, _ in s.validation_sorted[:40]]
    for _ in range(40):
        p, q = rng.choice(s.n, size=2, replace=False)
        pp.append((s.seq2id[p], s.seq2id[q]))
    f = tmp_path / "pairs.txt"
    f.write_text("".join("%d\t%d\n" % x for x in pp))
    r = subprocess.run([SVINET, "-file", graph_files["lfr"], "-n", "1000", "-k", "28", "-link-sampling", "-no-stop",
                        "-max-iterations", "20", "-recommend", "5", "-predict-pairs", str(f)] + extra, cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    d = glob.glob(str(tmp_path / "n1000-k28-*"))
    assert len(d) == 1
    d = d[0]
    gt = np.loadtxt(os.path.join(d, "gamma.txt"))
    lt = np.loadtxt(os.path.join(d, "lambda.txt"))
    ext = gt[:, 1].astype(np.int64)
    P, beta = _pb(gt[:, 2:], lt[:, 1:3])
    seq = {int(e): i for i, e in enumerate(ext)}
    edges = set()
    for line in open(graph_files["lfr"]):
        a = line.split()
        if len(a) >= 2 and not a[0].startswith("#"):
            edges.add((int(a[0]), int(a[1])))
            edges.add((int(a[1]), int(a[0])))
    held = set()
    for row in np.loadtxt(os.path.join(d, "validation-edges.txt"), dtype=np.int64).reshape(-1, 3):
        held.add((int(row[0]), int(row[1])))
        held.add((int(row[1]), int(row[0])))
    lp = [l.split("\t") for l in open(os.path.join(d, "link-prob.txt")).read().splitlines()]
    assert len(lp) == len(pp)
    for (a, b), row in zip(pp, lp):
        assert (int(row[0]), int(row[1])) == (int(a), int(b))
        assert int(row[2]) == (1 if (int(a), int(b)) in edges else 0)
        want = float(np.sum(P[seq[int(a)]] * P[seq[int(b)]] * beta))
        assert abs(float(row[3]) - want) <= 1e-4 * want
    rec = [l.split("\t") for l in open(os.path.join(d, "recommendations.txt")).read().splitlines()]
    assert len(rec) == s.n
    for i, row in enumerate(rec):
        assert int(row[0]) == ext[i] and len(row) == 1 + 2 * 5
        qs = [int(x) for x in row[1::2]]
        sc = np.array([float(x) for x in row[2::2]])
        assert np.all(np.diff(sc) <= 0)
        want = (P[i] * beta) @ P[[seq[q] for q in qs]].T
        assert np.all(np.abs(sc - want) <= 1e-4 * np.abs(want).max())
        for q in qs:
            assert q != ext[i] and ((ext[i], q) not in edges or (ext[i], q) in held), (ext[i], q)


def test_cli_predict_files(graph_files, tmp_path):
    _cli_predict(graph_files, tmp_path, [])


def test_cli_predict_files_minibatch(graph_files, tmp_path):
    _cli_predict(graph_files, tmp_path, ["-minibatch", "100"])
