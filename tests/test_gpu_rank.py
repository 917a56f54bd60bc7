"""-m gpu: where given links stand among their nodes' candidates (svils_rank_links, -rank-pairs / -rank-heldout).

Two references.  The exact one is the library's own top-k list: a node at place j of p's list must have the list's score
bitwise, above <= j <= above + tied, and above + tied == j where the next score is strictly lower -- this holds with any
number of exact ties.  The independent one is a numpy fp64 restatement written in this file from the definitions
(S = P diag(beta) P^T, candidates of p = every node but p and p's training neighbours): device and numpy scores differ by
rounding, so a count is required to lie between lo = #{S[p,c] > S[p,q] (1 + 1e-12)} and hi = #{S[p,c] >= S[p,q] (1 - 1e-12)},
and the test asserts that lo == hi for at least 99 % of a shape's pairs, so that the interval cannot hide a wrong count.
K = 1 is the one shape where that share cannot hold: pi = 1 for every node, all scores are beta_0 in exact arithmetic, so
lo = 0 and hi = ncand whatever the seed.  That shape keeps the interval and ncand checks and is ALSO run through the exact
check against the top-k lists, which is the stronger of the two."""
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pair_cases import NONE, _bits, _lfr_setup, _nbrs, _pb, _random_links, _random_pairs, _same, _state_bits

pytestmark = pytest.mark.gpu

SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
EPS = 1e-12


def _hub_links(rng, n, m, hub):
    """random links plus a hub adjacent to ids 0, n - 1 and every third id: its neighbours span all the 64-candidate tiles"""
    extra = [(min(hub, x), max(hub, x)) for x in sorted({0, n - 1} | set(range(1, n, 3))) if x != hub]
    e = np.unique(np.concatenate([_random_links(rng, n, m), np.array(extra, dtype=np.uint32)]), axis=0)
    return np.ascontiguousarray(e[np.lexsort((e[:, 1], e[:, 0]))], dtype=np.uint32)


def _random_state(n, k, m, seed, ties=False, hub=None):
    rng = np.random.default_rng(seed)
    links = _random_links(rng, n, m) if hub is None else _hub_links(rng, n, m, hub)
    gamma = rng.integers(1, 4, size=(n, k)).astype(np.float64) if ties else rng.random((n, k)) + 0.01
    lam = rng.random((k, 2)) + 0.1
    return links, gamma, lam


def _engine(n, k, links, gamma, lam):
    from svinet_amd import _svils
    eng = _svils.Engine(n, k, ones=len(links), ones_prob=len(links) / (n * (n - 1) / 2), use_validation_stop=False)
    eng.set_graph(links)
    eng.set_state(gamma, lam)
    return eng


def _rank_ref(P, beta, nbrs, pairs, eps=EPS):
    """per pair: lo, hi (the interval the device's above and above + tied must lie in), ncand and numpy's score"""
    n = P.shape[0]
    out = np.zeros((len(pairs), 3), dtype=np.int64)
    sc = np.zeros(len(pairs))
    for i, (p, q) in enumerate(np.asarray(pairs, dtype=np.int64).tolist()):
        S = (P[p] * beta) @ P.T
        cand = np.ones(n, bool)
        cand[p] = False
        cand[nbrs[p]] = False
        cand[q] = False
        s = S[q]
        out[i] = np.sum(S[cand] > s * (1 + eps)), np.sum(S[cand] >= s * (1 - eps)), cand.sum()
        sc[i] = s
    return out[:, 0], out[:, 1], out[:, 2], sc


def _check_against_numpy(res, ref, sharp=True, rtol=1e-12):
    above, tied, ncand, score = res
    lo, hi, nc, sc = ref
    assert np.array_equal(ncand, nc)
    np.testing.assert_allclose(score, sc, rtol=rtol, atol=0)
    a, at = above.astype(np.int64), above.astype(np.int64) + tied
    assert np.all(lo <= a) and np.all(at <= hi), (lo, a, at, hi)
    share = np.mean(lo == hi)
    print("rank vs numpy: %d pairs, lo == hi for %.4f" % (len(lo), share))
    if sharp:
        assert share >= 0.99, share


def _check_against_topk(eng, n, nbrs, nodes, topk=25):
    ids, sc = eng.predict_links(topk, nodes)
    rows, cols = np.nonzero(ids != NONE)
    pairs = np.stack([nodes[rows], ids[rows, cols]], 1)
    above, tied, ncand, score = eng.rank_links(pairs)
    assert np.array_equal(score.view(np.uint64), sc[rows, cols].view(np.uint64))
    assert np.all(above <= cols) and np.all(cols <= above.astype(np.int64) + tied)
    deg = np.array([len(nbrs[p]) for p in nodes[rows]])
    assert np.array_equal(ncand, n - 2 - deg)
    nxt = np.full(ids.shape, np.inf)
    nxt[:, :-1] = sc[:, 1:]
    strict = (cols < topk - 1) & (sc[rows, cols] > nxt[rows, cols])
    assert np.array_equal((above.astype(np.int64) + tied)[strict], cols[strict])
    return int(np.sum(tied > 0)), int(np.sum(strict))


# ties / strict: whether exact ties / strictly lower next scores occur within the 25-entry lists of the case (counted with
# numpy beforehand).  n = 3000 with integer gamma in 1..3 and K = 3 has a few dozen distinct scores per query, each shared by
# far more than 25 candidates: its lists are all ties, no strict step.  n = 300 with the same gamma has both.  K = 1: all
# scores are equal up to rounding, neither is required.
@pytest.mark.parametrize("n,k,m,gties,ties,strict", [(3000, 3, 12000, True, True, False), (300, 3, 1200, True, True, True),
                                                     (2000, 37, 8000, False, False, True), (65, 1, 100, False, False, False)])
def test_ranks_agree_exactly_with_the_topk_lists(n, k, m, gties, ties, strict):
    links, gamma, lam = _random_state(n, k, m, seed=k, ties=gties)
    eng = _engine(n, k, links, gamma, lam)
    nodes = np.random.default_rng(7).choice(n, size=min(300, n), replace=False).astype(np.uint32)
    ntied, nstrict = _check_against_topk(eng, n, _nbrs(n, links), nodes, topk=25)
    print("rank vs top-k: %d ranked entries tied with another, %d strict steps" % (ntied, nstrict))
    assert ntied > 0 or not ties      # the case is there for its exact ties
    assert nstrict > 0 or not strict  # ... or for the places that are then fixed exactly


# (n, K, links, pairs, hub): n = 64 / 65 one candidate tile and one node more; K = 1, 4, 16, 17 the padding to 16 columns;
# 1, 63, 64, 65 pairs the edge of the query tile; (200000, 4 n) many candidate chunks; a hub whose neighbours span the tiles
SHAPES = [(64, 4, 100, 63, None), (65, 1, 100, 64, None), (65, 16, 120, 65, None), (300, 17, 900, 1, None),
          (200000, 16, 800000, 65, None), (400, 5, 800, 64, 200)]


def _shape_case(n, k, m, npairs, hub):
    links, gamma, lam = _random_state(n, k, m, seed=1000 + n + k, hub=hub)
    rng = np.random.default_rng(npairs)
    pairs = _random_pairs(rng, n, npairs)
    if hub is not None:      # from the hub and to the hub: neighbours (ids 0 and n - 1 among them) and strangers
        others = np.array([0, n - 1, 1, 2, 3, 4, 5, 6, 63, 64, 65, 127, 128, 129, 255, 256], dtype=np.uint32)
        others = others[others != hub]
        h = np.full(len(others), hub, dtype=np.uint32)
        pairs = np.concatenate([np.stack([h, others], 1), np.stack([others, h], 1), pairs[:npairs - 2 * len(others)]])
    return links, gamma, lam, pairs


@pytest.mark.parametrize("n,k,m,npairs,hub", SHAPES)
def test_ranks_match_numpy(n, k, m, npairs, hub):
    links, gamma, lam, pairs = _shape_case(n, k, m, npairs, hub)
    assert len(pairs) == npairs
    P, beta = _pb(gamma, lam)
    eng = _engine(n, k, links, gamma, lam)
    _check_against_numpy(eng.rank_links(pairs), _rank_ref(P, beta, _nbrs(n, links), pairs), sharp=k > 1)


def test_ranks_match_numpy_fitted_assort(graph_files):
    from svinet_amd.host_api import Setup
    s = Setup(graph_files["assort"], 75, 4)
    eng = s.engine(use_validation_stop=False)
    eng.sweep(10)
    g, lam, _ = eng.state()
    P, beta = _pb(g, lam)
    pp = np.array([(p, q) for p in range(s.n) for q in range(s.n) if p != q], dtype=np.uint32)
    _check_against_numpy(eng.rank_links(pp), _rank_ref(P, beta, _nbrs(s.n, s.links), pp))


def test_candidates_and_arguments():
    from svinet_amd import _svils
    n, k = 300, 6
    links, gamma, lam = _random_state(n, k, 900, seed=11)
    P, beta = _pb(gamma, lam)
    nb = _nbrs(n, links)
    eng = _engine(n, k, links, gamma, lam)
    p = int(np.argmax([len(x) for x in nb]))
    qn = int(nb[p][0])                                                   # a training neighbour of p
    qs = int(next(x for x in range(n) if x != p and x not in set(nb[p].tolist())))   # and a stranger
    pairs = np.array([[p, qn], [p, qs]], dtype=np.uint32)
    res = eng.rank_links(pairs)
    _check_against_numpy(res, _rank_ref(P, beta, nb, pairs))
    assert res[2][0] == res[2][1] + 1 == n - 1 - len(nb[p])
    for bad in ([[4, 4]], [[0, n]], [[n, 0]]):
        with pytest.raises(_svils.SvilsError) as ei:
            eng.rank_links(bad)
        assert ei.value.code == -1
    lib = _svils.load()
    assert lib.svils_rank_links(eng._h, pairs.ctypes.data, 2, None, None, None, None) == 0
    only = np.zeros(2, dtype=np.uint32)
    assert lib.svils_rank_links(eng._h, pairs.ctypes.data, 2, None, only.ctypes.data, None, None) == 0
    assert np.array_equal(only, res[1])
    assert lib.svils_rank_links(eng._h, None, 0, None, None, None, None) == 0
    assert all(len(x) == 0 for x in eng.rank_links(np.zeros((0, 2), dtype=np.uint32)))
    bare = _svils.Engine(n, k, ones=len(links), ones_prob=0.01)
    with pytest.raises(_svils.SvilsError) as ei:
        bare.rank_links(pairs)
    assert ei.value.code == -1


def test_a_pair_does_not_depend_on_the_rest_of_the_call():
    n, k = 2000, 37
    links, gamma, lam = _random_state(n, k, 8000, seed=k)
    eng = _engine(n, k, links, gamma, lam)
    rng = np.random.default_rng(4)
    mine = _random_pairs(rng, n, 70)
    alone = _bits(eng.rank_links(mine))
    crowd = np.concatenate([mine, _random_pairs(rng, n, 9000)])          # more than one internal batch
    perm = rng.permutation(len(crowd))
    inside = _bits(eng.rank_links(crowd[perm]))
    where = np.argsort(perm)[:70]
    for a, b in zip(alone, inside):
        assert np.array_equal(a, b[where])
    for a, b in zip(alone, _bits(eng.rank_links(mine))):
        assert np.array_equal(a, b)


def _heldout_directed(s):
    v1 = s.validation_accept[s.validation_accept[:, 2] == 1][:, :2]
    return np.ascontiguousarray(np.stack([v1, v1[:, ::-1]], 1).reshape(-1, 2), dtype=np.uint32)   # p -> q, q -> p, ...


def test_ranking_does_not_disturb_the_sweeps(graph_files):
    s = _lfr_setup(graph_files)
    a, b = s.engine(use_validation_stop=False), s.engine(use_validation_stop=False)
    a.sweep(10)
    before = _state_bits(a)
    a.rank_links(_heldout_directed(s))
    _same(before, _state_bits(a))
    a.sweep(10)
    b.sweep(10)
    b.sweep(10)
    _same(_state_bits(a), _state_bits(b))


def _fit_to_the_stop_rule(s):
    eng = s.engine(use_validation_stop=True)
    for _ in range(100):
        eng.sweep(64)
        if eng.control().stopped:
            break
    assert eng.control().stopped
    return eng


def _summary(above, tied, ncand):
    """the columns of link-ranks-summary.txt, from the definitions: sequential double sums in the given order"""
    auc = mrr = chance = 0.0
    h = [0, 0, 0]
    for a, t, c in zip(above.tolist(), tied.tolist(), ncand.tolist()):
        mid = a + 0.5 * t
        auc += 1.0 - mid / c
        mrr += 1.0 / (mid + 1.0)
        chance += 10.0 / c
        for j, lim in enumerate((1, 10, 100)):
            h[j] += a + t < lim
    m = float(len(above))
    return [len(above), auc / m, mrr / m, h[0] / m, h[1] / m, h[2] / m, chance / m]


def test_usefulness_on_a_stopped_lfr_handle(graph_files):
    """fitted to the stop rule (the call works on a stopped handle and leaves it alone): the summary of the device's counts
    equals the summary of numpy's own counts on the same state, held-out links rank far above the middle of their nodes'
    candidates, and they are among the first ten far more often than chance"""
    s = _lfr_setup(graph_files)
    eng = _fit_to_the_stop_rule(s)
    before = _state_bits(eng)
    pairs = _heldout_directed(s)
    above, tied, ncand, score = eng.rank_links(pairs)
    eng.sweep(4)                                       # no-ops after the stop
    _same(before, _state_bits(eng))
    g, lam, _ = eng.state()
    P, beta = _pb(g, lam)
    lo, hi, nc, sc = _rank_ref(P, beta, _nbrs(s.n, s.links), pairs, eps=0.0)   # eps = 0: numpy's own above, above + tied
    got, want = _summary(above, tied, ncand), _summary(lo, hi - lo, nc)
    print("LFR K = 28, %d directed held-out links: AUC %.4f MRR %.4f hits@1 %.4f hits@10 %.4f hits@100 %.4f chance@10 %.5f"
          % tuple(got))
    assert got[0] == want[0] and abs(got[1] - want[1]) <= 1e-12
    assert got[3:6] == want[3:6]
    assert got[1] > 0.5
    assert got[4] > 10 * got[6]


def test_ranking_on_a_minibatch_handle(graph_files):
    s = _lfr_setup(graph_files)
    a, b = s.engine(use_validation_stop=False), s.engine(use_validation_stop=False)
    for e in (a, b):
        e.set_stochastic(batch_nodes=100, tau0=1.0, kappa=0.5)
        e.step(10)
    pairs = _heldout_directed(s)
    res = a.rank_links(pairs)
    g, lam, _ = a.state()
    a.step(10)
    b.step(10)
    _same(_state_bits(a), _state_bits(b))
    P, beta = _pb(g, lam)
    _check_against_numpy(res, _rank_ref(P, beta, _nbrs(s.n, s.links), pairs))


def test_refusals(graph_files):
    from svinet_amd import _svils
    from svinet_amd.host_api import Setup
    s = _lfr_setup(graph_files)
    ksh = _svils.Engine(s.n, 28, ones=s.ones, ones_prob=s.ones_prob, eta=s.eta, use_validation_stop=False, k_slice=(0, 28))
    ksh.set_graph(s.links)
    rng = np.random.default_rng(3)
    t = Setup(n=20, k=2100, pairs=_random_links(rng, 20, 80).astype(np.int32) + 1, heldout_ratio=0.05)
    tiled = t.engine(use_validation_stop=False)
    block = s.engine(use_validation_stop=False, node_block=(250, 700))
    for eng, needle in ((ksh, "K-sharded"), (tiled, "column-tiled"), (block, "node-block")):
        with pytest.raises(_svils.SvilsError) as ei:
            eng.rank_links([[0, 1]])
        assert ei.value.code == -4 and needle in str(ei.value) and "svils_rank_links" in str(ei.value)


def _cli_ranks(graph_files, tmp_path, extra):
    from svinet_amd import _svils
    from svinet_amd.host_api import Setup
    s = Setup(graph_files["lfr"], 1000, 28)
    rng = np.random.default_rng(2)
    pp = [(s.seq2id[p], s.seq2id[q]) for p, q, _ in s.validation_sorted[:40]]
    pp += [(s.seq2id[p], s.seq2id[q]) for p, q in s.links[:10]]          # training links: y = 1, not in the summary
    for _ in range(30):
        p, q = rng.choice(s.n, size=2, replace=False)
        pp.append((s.seq2id[p], s.seq2id[q]))
    f = tmp_path / "pairs.txt"
    f.write_text("".join("%d\t%d\n" % x for x in pp))

    def run(flags):
        r = subprocess.run([SVINET, "-file", graph_files["lfr"], "-n", "1000", "-k", "28", "-link-sampling", "-no-stop",
                            "-max-iterations", "20"] + flags + extra, cwd=str(tmp_path), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=900)
        assert r.returncode == 0, r.stderr

    run(["-rank-heldout", "-rank-pairs", str(f)])
    d = glob.glob(str(tmp_path / "n1000-k28-*"))
    assert len(d) == 1
    d = d[0]
    gt = np.loadtxt(os.path.join(d, "gamma.txt"))
    lt = np.loadtxt(os.path.join(d, "lambda.txt"))
    ext = gt[:, 1].astype(np.int64)
    gamma, lam = np.ascontiguousarray(gt[:, 2:]), np.ascontiguousarray(lt[:, 1:3])
    seq = {int(e): i for i, e in enumerate(ext)}
    edges = set()
    for line in open(graph_files["lfr"]):
        a = line.split()
        if len(a) >= 2 and not a[0].startswith("#"):
            edges.add((int(a[0]), int(a[1])))
            edges.add((int(a[1]), int(a[0])))
    val = np.loadtxt(os.path.join(d, "validation-edges.txt"), dtype=np.int64).reshape(-1, 3)
    held = {(int(a), int(b)) for a, b, _ in val} | {(int(b), int(a)) for a, b, _ in val}
    train = np.array(sorted({(min(seq[a], seq[b]), max(seq[a], seq[b])) for a, b in edges if (a, b) not in held}), dtype=np.uint32)
    n = len(ext)
    nb = _nbrs(n, train)
    P, beta = _pb(gamma, lam)
    eng = _engine(n, 28, train, gamma, lam)

    def check(name, want_pairs):
        rows = [l.split("\t") for l in open(os.path.join(d, name)).read().splitlines()]
        assert len(rows) == len(want_pairs) and all(len(r) == 8 for r in rows)
        directed, mids, ncs, counted = [], [], [], []
        for (a, b), row in zip(want_pairs, rows):
            assert (int(row[0]), int(row[1])) == (int(a), int(b))
            y = 1 if (int(a), int(b)) in edges else 0
            assert int(row[2]) == y
            directed += [(seq[int(a)], seq[int(b)]), (seq[int(b)], seq[int(a)])]
            mids += [float(row[4]), float(row[6])]
            ncs += [int(row[5]), int(row[7])]
            counted += [y == 1 and (int(a), int(b)) in held] * 2
        directed = np.array(directed, dtype=np.uint32).reshape(-1, 2)
        mids, ncs, counted = np.array(mids), np.array(ncs), np.array(counted, dtype=bool)
        # the reloaded model has five decimals: the file's ranks against numpy's interval at 1e-4, its counts exactly
        lo, hi, nc, sc = _rank_ref(P, beta, nb, directed, eps=1e-4)
        assert np.array_equal(ncs, nc)
        fs = np.array([float(r[3]) for r in rows])
        assert np.all(np.abs(fs - sc[0::2]) <= 1e-4 * sc[0::2])
        assert np.all(lo + 1 <= mids) and np.all(mids <= hi + 1), (lo, mids, hi)
        above, tied, ncand, score = eng.rank_links(directed)              # and against the library on that model
        assert np.array_equal(ncand, ncs)
        assert np.all(lo <= above) and np.all(above.astype(np.int64) + tied <= hi)
        assert np.all(np.abs(score[0::2] - fs) <= 1e-4 * fs)
        return mids[counted], ncs[counted]

    def check_summary(mids, ncs):
        head, vals = [l.split("\t") for l in open(os.path.join(d, "link-ranks-summary.txt")).read().splitlines()]
        assert head == ["pairs", "auc", "mrr", "hits1", "hits10", "hits100", "chance10"]
        # no ties in a continuous fitted state: every mid-rank is whole, so above + tied = mid-rank - 1
        assert np.all(mids == np.floor(mids))
        want = _summary((mids - 1).astype(np.int64), np.zeros(len(mids), dtype=np.int64), ncs)
        assert int(vals[0]) == want[0] and want[0] > 0
        np.testing.assert_allclose([float(x) for x in vals[1:]], want[1:], rtol=1e-12, atol=0)

    v1 = [(int(a), int(b)) for a, b, y in val if y == 1]
    check("link-ranks.txt", pp)
    check_summary(*check("heldout-ranks.txt", v1))                         # both flags: the summary is the held-out file's
    assert len(v1) > 0
    for name in ("link-ranks.txt", "heldout-ranks.txt", "link-ranks-summary.txt"):
        os.rename(os.path.join(d, name), os.path.join(d, name + ".both"))
    run(["-rank-pairs", str(f)])                                           # the same run again, into the same directory
    assert not os.path.exists(os.path.join(d, "heldout-ranks.txt"))
    mids, ncs = check("link-ranks.txt", pp)
    assert len(mids) == 2 * 40 - 2 * int(np.sum(s.validation_sorted[:40, 2] == 0))
    check_summary(mids, ncs)


def test_cli_rank_files(graph_files, tmp_path):
    _cli_ranks(graph_files, tmp_path, [])


def test_cli_rank_files_minibatch(graph_files, tmp_path):
    _cli_ranks(graph_files, tmp_path, ["-minibatch", "100"])
