"""-m gpu: the sampled-pair steps of -rnode / -rpair on the device (svils_batch_step_node, svils_batch_step_pairs,
csrc/svils_batch.hip).

The reference is tests/sampled_cases.py, a restatement of one step on top of oracle/batch_oracle.py; every step is compared
from the device's own state before it.  Tolerance: rtol 1e-7 on gamma, lambda and the heldout row, the one
tests/test_gpu_batch.py holds this fixed point to.  sampled_cases.assert_exits_are_clear is asserted for the pairs of
every compared step, and with it the device's round counters equal the restated ones exactly."""
import math

import numpy as np
import pytest

import batch_cases as BC
import sampled_cases as SC
from oracle import batch_oracle as B
from svinet_amd import _svils
from svinet_amd.host_api import SampledEngine
from test_gpu_batch import RTOL, Start, _cli, _free_bytes, _variant_ks

pytestmark = pytest.mark.gpu


def _check(s, g0, l0, p, q, scale, rg, rl):
    """the device's state and counters after one step against the restatement of that step from (g0, l0)"""
    SC.assert_exits_are_clear(g0, l0, s.adj, p, q)
    g, lam, rounds = SC.step(g0, l0, s.adj, p, q, s.alpha, s.eta, scale, rg, rl)
    dg, dl = s.dev.state()
    np.testing.assert_allclose(dg, g, rtol=RTOL)
    np.testing.assert_allclose(dl, lam, rtol=RTOL)
    if rl < 0:
        assert dl.tobytes() == l0.tobytes()
    pairs_done, rounds_total, rounds_max, underflow = s.dev.stats()
    assert (pairs_done, rounds_total, underflow) == (len(p), int(rounds.sum()), 0)
    assert rounds_max == (int(rounds.max()) if len(p) else 0)
    return dg, dl


def _node_step(s, a, c, rl=None):
    g0, l0 = s.dev.state()
    p, q = SC.node_pairs(s.n, a, s.skip)
    rg = SC.rho_gamma(c)
    rl = SC.rho_lambda(c, 0) if rl is None else rl
    s.dev.step_node([a], s.n / 2.0, [rg], [rl])
    return _check(s, g0, l0, p, q, s.n / 2.0, rg, rl)


def _pair_step(s, pairs, c, scale=None, rl=None):
    g0, l0 = s.dev.state()
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    scale = s.n * (s.n - 1) / 2.0 / len(pairs) if scale is None else scale
    rg = SC.rho_gamma(c)
    rl = SC.rho_lambda(c, 0) if rl is None else rl
    s.dev.step_pairs([pairs], [scale], [rg], [rl])
    return _check(s, g0, l0, pairs[:, 0], pairs[:, 1], scale, rg, rl)


def _draw_pairs(s, m, seed):
    """m pairs outside the skip set, drawn with replacement"""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < m:
        a, b = sorted(int(x) for x in rs.randint(0, s.n, 2))
        if a != b and (a, b) not in s.skip:
            out.append((a, b))
    return out


@pytest.mark.parametrize("k", _variant_ks())
def test_steps_match_the_restatement_for_every_variant(graph_files, k):
    s = Start(graph_files["assort"], 75, k)
    hub = int(np.argmax(s.adj.sum(1)))
    for c, a in enumerate((0, 74, hub)):
        _node_step(s, a, c)
    for c in (3, 4):
        _pair_step(s, _draw_pairs(s, 37, 10 * k + c), c)


@pytest.mark.parametrize("k", _variant_ks())
def test_sweep_and_step_paths_run_the_same_rounds(graph_files, k):
    """one fixed point behind both paths: from one start state a sweep, and on a second handle ONE pair step that lists every
    trained pair (rho_gamma = 1, rho_lambda < 0: lambda and Elogbeta stay the start's), run each pair's fixed point from the
    same Elogpi / Elogbeta.  The round counters are integers and are compared without a tolerance: a last-bit drift between
    two copies of the loop moves a pair's exit, and these, before it shows at rtol 1e-7"""
    s = Start(graph_files["assort"], 75, k)
    s.dev.sweep()
    swept = s.dev.stats()
    pairs = np.array([(p, q) for p in range(s.n) for q in range(p + 1, s.n) if (p, q) not in s.skip], dtype=np.uint32)
    assert len(pairs) == s.trained
    d = _svils.Batch(s.n, k, s.alpha, s.eta)
    d.set_graph(s.edges, sorted(s.skip))
    d.set_state(s.gamma, s.lam)
    d.step_pairs([pairs], [1.0], [1.0], [-1.0])
    stepped = d.stats()
    d.close()
    assert stepped[0] == swept[0] == s.trained
    assert stepped[1] == swept[1] and stepped[2] == swept[2]
    assert stepped[3] == swept[3] == 0


@pytest.mark.parametrize("k", [4, 5])
@pytest.mark.parametrize("n", [10, 64, 65, 256, 257, 258])
def test_steps_at_lane_group_and_workgroup_edges(tmp_path, n, k):
    """at k = 4 a wavefront holds 64 pairs and a workgroup 256: n - 1 pairs of a node step and lists of 1, 64, 65 and 257
    pairs on either side of both"""
    links = BC.planted_links(n, 2, 0.0 if n == 10 else 0.3, 0.0 if n == 10 else 0.03, seed=200 + n)
    s = Start(BC.write_graph(tmp_path / "g.txt", links), n, k)
    assert s.n == n
    for c, a in enumerate((0, n // 2, n - 1)):
        _node_step(s, a, c)
    for c, m in enumerate((1, 64, 65, 257), start=3):
        _pair_step(s, _draw_pairs(s, m, 1000 * n + m), c)


def test_skipped_pairs_of_a_node_step(graph_files):
    """a start node with four more skipped pairs: their far ends move towards alpha with phi = 0, and so does a node whose
    only pair with the start node is skipped; the counter is the restated count"""
    extra = [(5, 9), (5, 40), (2, 5), (5, 74)]
    s = Start(graph_files["assort"], 75, 4, skip_extra=extra)
    g0, _ = s.dev.state()
    p, _ = SC.node_pairs(75, 5, s.skip)
    assert len(p) <= 74 - len(extra)
    dg, _ = _node_step(s, 5, 0)
    rg = SC.rho_gamma(0)
    for j in (9, 40, 2, 74):
        np.testing.assert_allclose(dg[j], (1 - rg) * g0[j] + rg * s.alpha, rtol=1e-14)
    assert s.dev.stats()[0] == len(p)
    _node_step(s, 9, 1)


def test_pair_lists_repeats_hubs_families_and_refusals(graph_files):
    s = Start(graph_files["assort"], 75, 4)
    free = [e for e in _draw_pairs(s, 200, 4)]
    one = free[0]
    _pair_step(s, [one, free[1], one, free[2], one], 0)                       # one pair three times
    hub = [(min(7, j), max(7, j)) for j in range(75) if j != 7 and (min(7, j), max(7, j)) not in s.skip][:20]
    _pair_step(s, hub + free[3:10], 1)                                        # a hub in 20 pairs
    both = [(a, 10) for a in (1, 3, 8) if (a, 10) not in s.skip] + [(10, b) for b in (20, 30, 50) if (10, b) not in s.skip]
    assert any(q == 10 for _, q in both) and any(p == 10 for p, _ in both)
    _pair_step(s, both, 2)                                                    # a node as p and as q
    # a stratified pair of steps: non-links with zeros_prob, links with ones_prob (src/mmsbinfer.hh:722-748)
    total, mb = 75 * 74 / 2.0, 37
    zeros = [e for e in free if s.adj[e] == 0][:mb]
    ones = [tuple(int(x) for x in e) for e in s.edges if tuple(int(x) for x in e) not in s.skip][:mb]
    assert len(zeros) == len(ones) == mb and all(s.adj[e] == 1 for e in ones)
    _pair_step(s, zeros, 3, scale=total * (1 - s.ones_prob) / mb)
    _pair_step(s, ones, 4, scale=total * s.ones_prob / mb)
    # a listed pair of the skip set, a self pair, p > q, a node >= n: refused before anything is enqueued
    g0, l0 = s.dev.state()
    for bad in (sorted(s.skip)[0], (4, 4), (9, 3), (3, 75)):
        with pytest.raises(_svils.SvilsError) as ei:
            s.dev.step_pairs([free[:5], free[5:8] + [bad]], [1.0, 1.0], [0.03, 0.03], [0.01, 0.01])
        assert ei.value.code == -1
    g1, l1 = s.dev.state()
    assert g1.tobytes() == g0.tobytes() and l1.tobytes() == l0.tobytes()


@pytest.mark.parametrize("kind", ["node", "pairs"])
def test_delayed_lambda_stays_bit_identical(graph_files, kind):
    """rho_lambda < 0 leaves lambda bit for bit while gamma moves (_check asserts both); the next step learns it"""
    s = Start(graph_files["assort"], 75, 5)
    for c, rl in ((0, -1.0), (1, -1.0), (2, None)):
        g0, l0 = s.dev.state()
        if kind == "node":
            dg, dl = _node_step(s, 11 * c + 1, c, rl=rl)
        else:
            dg, dl = _pair_step(s, _draw_pairs(s, 37, 50 + c), c, rl=rl)
        assert not np.array_equal(dg, g0)
        assert (dl.tobytes() == l0.tobytes()) == (rl is not None)


@pytest.mark.parametrize("kind", ["node", "pairs"])
def test_steps_are_bitwise_reproducible_and_conserve_mass(kind):
    """no oracle at n = 2000, k = 8: 7 steps in one call, in 7 calls and on a second handle agree bit for bit.
    Mass: every trained pair adds scale to each endpoint's gammat, so a step takes S = sum(gamma) to
    (1 - rho) S + rho (n k alpha + 2 scale P).  Rounding of one step: the blend of a cell is 4 operations, at most 4 eps of
    the cell, 4 eps S' over the cells; a phi vector sums to 1 within (k + 4) eps (k - 1 additions, a reciprocal of 2 ulp,
    a product), 2 P (k + 4) eps over the step; the gammat of the cells hold 2 P units in sums of at most n terms, at most 2 n P eps;
    the last two scaled by rho scale.  Evaluating the recurrence below costs a few eps S' more (taken as another 4).  The
    bound is twice the sum of these, carried through the steps by the same recurrence."""
    n, k, nsteps = 2000, 8, 7
    links = BC.planted_links(n, 8, 0.05, 0.002, seed=n)
    rs = np.random.RandomState(n + 1)
    gamma = rs.gamma(100.0, 0.01, (n, k))
    lam = np.tile([1.0, 1.0], (k, 1))
    skip = links[::97][:50]
    skipset = {tuple(int(x) for x in e) for e in skip}
    alpha = 1.0 / k
    rg = [SC.rho_gamma(c) for c in range(nsteps)]
    rl = [-1.0, -1.0] + [SC.rho_lambda(c, 2) for c in range(2, nsteps)]
    if kind == "node":
        nodes = [0, n - 1, int(skip[0][0]), 1000, 63, 64, int(skip[0][0])]
        scale = [n / 2.0] * nsteps
        npairs = [n - 1 - sum(1 for e in skipset if a in e) for a in nodes]
    else:
        lists = []
        for c in range(nsteps):
            m = 1000 - 7 * c
            pq = np.sort(rs.randint(0, n, (3 * m, 2)), axis=1)
            pq = [tuple(int(x) for x in e) for e in pq if e[0] != e[1] and tuple(int(x) for x in e) not in skipset][:m]
            assert len(pq) == m
            lists.append(np.array(pq + pq[:5], dtype=np.uint32))             # five pairs twice
        scale = [n * (n - 1) / 2.0 / len(l) for l in lists]
        npairs = [len(l) for l in lists]

    def run(cuts):
        d = _svils.Batch(n, k, alpha, (1.0, 1.0))
        d.set_graph(links, skip)
        d.set_state(gamma, lam)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            if kind == "node":
                d.step_node(nodes[lo:hi], scale[0], rg[lo:hi], rl[lo:hi])
            else:
                d.step_pairs(lists[lo:hi], scale[lo:hi], rg[lo:hi], rl[lo:hi])
        out = d.state() + (d.stats(),)
        d.close()
        return out

    one, again, cut = run([0, nsteps]), run([0, nsteps]), run(list(range(nsteps + 1)))
    for other in (again, cut):
        assert other[0].tobytes() == one[0].tobytes() and other[1].tobytes() == one[1].tobytes()
    assert one[2] == again[2] and one[2][0] == sum(npairs) and one[2][3] == 0 and cut[2][0] == npairs[-1]
    eps = np.finfo(float).eps
    mass, bound = math.fsum(gamma.ravel()), 0.0
    for c in range(nsteps):
        mass = (1 - rg[c]) * mass + rg[c] * (n * k * alpha + 2 * scale[c] * npairs[c])
        bound = (1 - rg[c]) * bound + 2 * eps * (8 * mass + rg[c] * scale[c] * npairs[c] * (2 * (k + 4) + 2 * n))
    assert abs(math.fsum(one[0].ravel()) - mass) <= bound
    assert bound < 1e-9 * mass
    assert np.all(one[0] > 0) and np.all(one[1] > 0) and not np.array_equal(one[1], lam)


def test_sweeps_and_steps_mixed_on_one_handle(graph_files):
    s = Start(graph_files["assort"], 75, 5)
    g, lam = B.sweep(s.gamma, s.lam, s.adj, s.skip, s.alpha, s.eta)
    s.dev.sweep()
    dg, dl = s.dev.state()
    np.testing.assert_allclose(dg, g, rtol=RTOL)
    _node_step(s, 17, 0)
    _pair_step(s, _draw_pairs(s, 37, 7), 1)
    _node_step(s, 60, 2)
    g0, l0 = s.dev.state()
    g, lam = B.sweep(g0, l0, s.adj, s.skip, s.alpha, s.eta)
    s.dev.sweep()
    dg, dl = s.dev.state()
    np.testing.assert_allclose(dg, g, rtol=RTOL)
    np.testing.assert_allclose(dl, lam, rtol=RTOL)
    assert s.dev.stats()[0] == s.trained
    y = s.heldout_y()
    np.testing.assert_allclose(BC.heldout_row(s.dev.pair_loglik(s.hsorted, y), y, s.ones_prob),
                               B.heldout_row(g, lam, s.hsorted, s.adj, s.ones_prob), rtol=RTOL)
    s.dev.set_state(s.gamma, s.lam)                                           # a step after set_state sees the new state
    _node_step(s, 3, 0)


def test_scopes_destroy_with_steps_in_flight():
    """the style of test_gpu_batch.py::test_scopes_set_graph_twice_and_destroy_in_flight: after a warm-up cycle, handles
    destroyed with a chunk of node steps and a chunk of pair steps still queued leave the free memory where it was"""
    n, k = 1500, 16
    links = BC.planted_links(n, 4, 0.05, 0.002, seed=1)
    rs = np.random.RandomState(3)
    gamma = rs.gamma(100.0, 0.01, (n, k))
    lam = np.tile([1.0, 1.0], (k, 1))
    skipset = {tuple(int(x) for x in e) for e in links[:40]}
    lists = []
    for _ in range(20):
        pq = np.sort(rs.randint(0, n, (900, 2)), axis=1)
        lists.append(np.array([e for e in pq if e[0] != e[1] and (int(e[0]), int(e[1])) not in skipset][:750], dtype=np.uint32))
    nodes = rs.randint(0, n, 60)

    def cycle():
        d = _svils.Batch(n, k, 1.0 / k, (1.0, 1.0))
        d.set_graph(links, links[:40])
        d.set_state(gamma, lam)
        d.step_node(nodes, n / 2.0, [0.03] * 60, [0.002] * 60)
        d.step_pairs(lists, [1500.0] * 20, [0.03] * 20, [0.002] * 20)
        d.step_pairs(lists[:3], [1500.0] * 3, [0.03] * 3, [-1.0] * 3)
        d.close()                            # enqueued, not waited for

    cycle()
    warm = _free_bytes()
    for _ in range(2):
        cycle()
        assert _free_bytes() >= warm - (2 << 20)


def test_null_arrays_are_refused(graph_files):
    s = Start(graph_files["assort"], 75, 4)
    L, h = _svils.load(), s.dev._h
    one, node = np.ones(1), np.zeros(1, dtype=np.uint32)
    off, pair = np.array([0, 1], dtype=np.uint64), np.array([[0, 1]], dtype=np.uint32)
    assert L.svils_batch_step_node(h, 1, None, 37.5, one.ctypes.data, one.ctypes.data) == -1
    assert L.svils_batch_step_node(h, 1, node.ctypes.data, 37.5, None, one.ctypes.data) == -1
    assert L.svils_batch_step_node(h, 1, node.ctypes.data, 0.0, one.ctypes.data, one.ctypes.data) == -1
    assert L.svils_batch_step_pairs(h, 1, None, pair.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data) == -1
    assert L.svils_batch_step_pairs(h, 1, off.ctypes.data, None, one.ctypes.data, one.ctypes.data, one.ctypes.data) == -1
    assert L.svils_batch_step_pairs(h, 1, off.ctypes.data, pair.ctypes.data, one.ctypes.data, one.ctypes.data, None) == -1
    node[0] = 75
    assert L.svils_batch_step_node(h, 1, node.ctypes.data, 37.5, one.ctypes.data, one.ctypes.data) == -1
    g, lam = s.dev.state()
    assert g.tobytes() == s.gamma.tobytes() and lam.tobytes() == s.lam.tobytes()


@pytest.mark.parametrize("mode", ["rnode", "rpair", "rpair-stratified"])
def test_host_engine_with_both_backends(graph_files, mode):
    """the same schedule on the host loops and on the device; the guard is asserted for the host side's states"""
    kw = dict(heldout_ratio=0.1, eta_type="fromdata", nodelay=True, seed=1)   # (seed 0 puts an -rpair exit within 1e-4 of the threshold)
    a = SampledEngine(graph_files["assort"], 75, 4, mode, **kw)
    b = SampledEngine(graph_files["assort"], 75, 4, mode, on_device=True, **kw)
    assert np.array_equal(a.heldout, b.heldout) and np.array_equal(a.validation, b.validation)
    adj = BC.adjacency(a.n, a.edges)
    for s in range(5):
        g, lam = a.gamma, a.lam
        a.step(1)
        d = a.schedule[s]
        SC.assert_exits_are_clear(g, lam, adj, d["pairs"][:, 0].astype(np.int64), d["pairs"][:, 1].astype(np.int64))
    b.step(5)
    for x, y in zip(a.schedule, b.schedule):
        assert np.array_equal(x["pairs"], y["pairs"])
        assert (x["node"], x["family"], x["scale"], x["rho_gamma"], x["rho_lambda"]) == (y["node"], y["family"], y["scale"], y["rho_gamma"], y["rho_lambda"])
    assert not a.report() and not b.report()
    assert a.iter == b.iter == 5 and a.rows.shape == b.rows.shape == (2, 10)
    np.testing.assert_allclose(b.rows, a.rows, rtol=RTOL)
    np.testing.assert_allclose(b.gamma, a.gamma, rtol=RTOL)
    np.testing.assert_allclose(b.lam, a.lam, rtol=RTOL)


@pytest.mark.parametrize("flags,name", [(["-rnode"], "Urnode"), (["-rpair", "-stratified"], "SUrpair")])
def test_cli_runs_on_the_device(graph_files, tmp_path, flags, name):
    common = ["-file", graph_files["assort"], "-n", "75", "-k", "4", "-heldout-ratio", "0.1"]
    (tmp_path / "gpu").mkdir()
    (tmp_path / "host").mkdir()
    r = _cli(common + flags + ["-max-iterations", "250"], tmp_path / "gpu")
    assert r.returncode == 0, r.stderr
    d = tmp_path / "gpu" / ("n75-k4-mmsb-" + name)
    for f in ("param.txt", "heldout-edges.txt", "validation-edges.txt", "heldout.txt", "validation.txt", "max.txt",
              "gamma.txt", "lambda.txt", "groups.txt", "communities.txt", "summary.txt"):
        assert (d / f).exists(), f
    rows = np.loadtxt(d / "heldout.txt")
    assert rows.shape == (3, 11) and list(rows[:, 0]) == [0, 100, 200]
    gam = np.loadtxt(d / "gamma.txt")
    assert gam.shape == (75, 6) and np.all(gam[:, 2:] > 0)
    assert np.loadtxt(d / "lambda.txt").shape == (4, 3)
    h = _cli(common + ["-batch", "-max-iterations", "1"], tmp_path / "host")
    assert h.returncode == 0, h.stderr
    for f in ("heldout-edges.txt", "validation-edges.txt"):
        assert (d / f).read_bytes() == (tmp_path / "host" / "n75-k4-mmsb-batch" / f).read_bytes(), f


def test_timing_and_stats_name_the_last_timed_call(tmp_path):
    """sweep, step call, elbo(), step call, sweep on one handle: timing() is (all three >= 0) after a sweep and
    (>= 0, -1, -1) after a step call and after elbo(); stats() are those of the last sweep or step call, which elbo()
    leaves alone.  A step call and elbo() both read (>= 0, -1, -1): what this pins is that neither is taken for a sweep, and,
    by the last sweep, that neither state sticks"""
    n, k = 70, 5
    s = Start(BC.write_graph(tmp_path / "g.txt", BC.planted_links(n, 2, 0.3, 0.03, seed=70)), n, k)
    assert s.n == n

    def stepped(pairs_done):
        ms = s.dev.timing()
        assert ms[0] >= 0 and ms[1] == ms[2] == -1
        assert s.dev.stats()[0] == pairs_done

    def swept():
        assert np.all(s.dev.timing() >= 0)
        assert s.dev.stats()[0] == s.trained

    s.dev.sweep()
    swept()
    s.dev.step_node([7], n / 2.0, [SC.rho_gamma(0)], [SC.rho_lambda(0, 0)])
    in_node_step = len(SC.node_pairs(n, 7, s.skip)[0])
    stepped(in_node_step)
    parts, pairs_done, _ = s.dev.elbo()
    assert pairs_done == s.trained and math.isfinite(parts[0])
    stepped(in_node_step)
    s.dev.step_pairs([_draw_pairs(s, 37, 70)], [n * (n - 1) / 2.0 / 37], [SC.rho_gamma(1)], [SC.rho_lambda(1, 0)])
    stepped(37)
    s.dev.sweep()
    swept()


def test_cli_refuses_k_above_the_limit(graph_files, tmp_path):
    r = _cli(["-file", graph_files["assort"], "-n", "75", "-k", "300", "-rnode"], tmp_path, timeout=60)
    assert r.returncode == 2 and "256" in r.stderr
    assert not list(tmp_path.iterdir())
