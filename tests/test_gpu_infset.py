"""-m gpu: the informative-set steps of -infset on the device (svils_batch_step_star, k_batch_star_chain in
csrc/svils_batch.hip).

The reference is tests/infset_cases.py, a restatement of one star step on top of oracle/batch_oracle.py.  Tolerance: rtol
1e-7 on gamma and lambda, the one tests/test_gpu_batch.py holds this fixed point to.  sampled_cases.assert_exits_are_clear
is asserted for the pairs of every restated step, and with it the device's round counters equal the restated ones exactly.
Graphs: random sparse ones of at most 400 nodes (batch_cases.planted_links), the state a seeded gamma draw."""
import math
import os
import subprocess

import numpy as np
import pytest

import batch_cases as BC
import infset_cases as IC
import sampled_cases as SC
from oracle import batch_oracle as B
from svinet_amd import _svils
from svinet_amd.host_api import InfsetEngine
from test_gpu_batch import RTOL, SVINET

pytestmark = pytest.mark.gpu

STAR_WAVES = 8   # wavefronts of the chain's workgroup (STAR_THREADS / 64, csrc/svils_batch.hip)


class World:
    """a planted graph, a skip set, a seeded state and a device handle holding them"""

    def __init__(self, n, k, seed, blocks=4, p_in=0.08, p_out=0.01, eta=(1.0, 1.0)):
        self.n, self.k, self.alpha, self.eta = n, k, 1.0 / k, eta
        self.links = BC.planted_links(n, blocks, p_in, p_out, seed=seed)
        self.adj = BC.adjacency(n, self.links)
        rs = np.random.RandomState(seed + 1)
        self.gamma = rs.gamma(100.0, 0.01, (n, k))
        self.lam = np.tile(np.asarray(eta), (k, 1)) + rs.gamma(100.0, 0.01, (k, 2))
        self.skiplist = np.concatenate([self.links[::7][:12], np.array([(1, 5), (2, n - 1)], dtype=np.uint32)])
        self.skip = {tuple(int(x) for x in e) for e in self.skiplist}
        self.rs = rs
        self.dev = self.handle()

    def handle(self):
        d = _svils.Batch(self.n, self.k, self.alpha, self.eta)
        d.set_graph(self.links, sorted(self.skip))
        d.set_state(self.gamma, self.lam)
        return d

    def free(self, a):
        return [j for j in range(self.n) if j != a and (min(a, j), max(a, j)) not in self.skip]

    def star(self, a, m, c, scale=None, rho_lambda=None, only_zeros=False):
        """a star of m entries around a: its links outside the skip set first (as opt_process lists them), then non-links"""
        free = self.free(a)
        ones = [j for j in free if self.adj[a, j]] if not only_zeros else []
        zeros = [j for j in free if not self.adj[a, j]]
        self.rs.shuffle(zeros)
        partner = (ones + zeros)[:m]
        assert len(partner) == m
        rho = [IC.rho_node(int(x), nodetau0=3.0) for x in self.rs.randint(0, 40, m)]
        return IC.star(a, partner, self.adj, rho, IC.rho_node(c, nodetau0=3.0), self.n / 2.0 if scale is None else scale,
                       IC.rho_lambda(c, tau0=10.0) if rho_lambda is None else rho_lambda)


def _restate(w, g, lam, stars):
    """the restated chain from (g, lam), the guard asserted for every step -> gamma, lambda, all rounds"""
    rounds = []
    for s in stars:
        p, q = IC.pairs_of(s)
        SC.assert_exits_are_clear(g, lam, w.adj, p, q)
        g, lam, r = IC.step(g, lam, w.adj, s, w.alpha, w.eta)
        rounds.append(r)
    return g, lam, np.concatenate(rounds) if rounds else np.zeros(0, dtype=np.int64)


ELOG_ATOL = 1e-12   # Elogpi / Elogbeta against the oracle's: two digammas of magnitude < 20 each within 2e-15 relative on
                    # the device (svils_devutil.h) and a few ulp in the oracle, 1e-13 in all; ten times that


def _run_and_check(w, stars):
    g0, l0 = w.dev.state()
    e0, b0 = w.dev.expectations()                                              # the pre-step dir_exp, as the device forms it
    w.dev.step_star(stars)
    g, lam, rounds = _restate(w, g0, l0, stars)
    dg, dl = w.dev.state()
    np.testing.assert_allclose(dg, g, rtol=RTOL)
    np.testing.assert_allclose(dl, lam, rtol=RTOL)
    pairs_done, rounds_total, rounds_max, underflow = w.dev.stats()
    assert (pairs_done, rounds_total, underflow) == (len(rounds), int(rounds.sum()), 0)
    assert rounds_max == (int(rounds.max()) if len(rounds) else 0)
    named = set()
    for s in stars:
        named |= {s["start"]} | {int(j) for j in s["partner"]}
    rest = np.setdiff1d(np.arange(w.n), sorted(named))
    assert len(rest) and dg[rest].tobytes() == g0[rest].tobytes()             # rows no step names: bit for bit
    e1, b1 = w.dev.expectations()
    assert e1[rest].tobytes() == e0[rest].tobytes()                            # ... of gamma and of Elogpi
    np.testing.assert_allclose(e1, B.dir_exp(dg), rtol=0, atol=ELOG_ATOL)      # and the named rows are those of the new gamma
    np.testing.assert_allclose(b1, B.dir_exp(dl), rtol=0, atol=ELOG_ATOL)
    if all(s["rho_lambda"] < 0 for s in stars):
        assert b1.tobytes() == b0.tobytes()
    return dg, dl


@pytest.mark.parametrize("k", [3, 7, 13, 29, 61, 100, 200, 256])
def test_chains_match_the_restatement_for_every_variant(k):
    """one K per W of the (W, V) table, none filling its W x V lanes, and the largest K; chains of 12 steps in one launch"""
    assert {_svils.batch_variant(x)[0] for x in (3, 7, 13, 29, 61, 100, 200)} == {1, 2, 4, 8, 16, 32, 64}
    w = World(200, k, seed=10 + k)
    starts = w.rs.randint(0, w.n, 12)
    stars = [w.star(int(a), int(m), c) for c, (a, m) in enumerate(zip(starts, w.rs.randint(5, 60, 12)))]
    _run_and_check(w, stars)


def test_entry_counts_around_the_pass_size():
    """K = 13: W = 4, a pass holds P = 8 x 16 = 128 entries: 0, 1, P - 1, P, P + 1 and 3 P + 2 entries, in one chain"""
    k = 13
    wd, _ = _svils.batch_variant(k)
    P = STAR_WAVES * 64 // wd
    assert P == 128
    w = World(400, k, seed=80)
    counts = [0, 1, P - 1, P, P + 1, 3 * P + 2]
    stars = [w.star(int(a), m, c) for c, (a, m) in enumerate(zip(w.rs.randint(20, w.n, len(counts)), counts))]
    _run_and_check(w, stars)
    for s in stars:                                                             # and each alone in its own launch
        _run_and_check(w, [s])


def _with_partner(w, s, j):
    """the star s with node j among its partners"""
    partner = [int(x) for x in s["partner"]]
    if j not in partner:
        partner[-1] = j
    return IC.star(s["start"], partner, w.adj, s["rho_partner"], s["rho_start"], s["scale"], s["rho_lambda"])


def test_steps_that_depend_on_the_step_before():
    w = World(300, 7, seed=5)
    a, b = 17, 42
    assert (a, b) not in w.skip
    s3 = w.star(b, 33, 3)
    c = int(s3["partner"][0])
    big = IC.scale_of(1, w.n)
    stars = [w.star(a, 25, 0), w.star(a, 40, 1),                                # the same start node twice in a row
             _with_partner(w, w.star(a, 30, 2), b), s3,                         # a start node that was a partner just before
             _with_partner(w, w.star(c, 20, 4), b),                             # ... and a partner that was the start node
             # a step of only non-links at the large scale of a non-informative step, then link steps
             w.star(90, 200, 5, scale=big, only_zeros=True), w.star(90, 30, 6), w.star(91, 30, 7)]
    assert b in stars[2]["partner"] and b in stars[4]["partner"] and stars[4]["start"] in s3["partner"]
    assert not stars[5]["y"].any() and stars[6]["y"].any()
    _run_and_check(w, stars)
    # rho_lambda < 0 leaves lambda (and with it Elogbeta: the next step agrees with the restatement) bit for bit
    _, l0 = w.dev.state()
    _, l1 = _run_and_check(w, [w.star(11, 30, 8, rho_lambda=-1.0), w.star(12, 0, 9, rho_lambda=-1.0)])
    assert l1.tobytes() == l0.tobytes()
    _, l2 = _run_and_check(w, [w.star(11, 30, 10)])
    assert l2.tobytes() != l1.tobytes()


def test_chains_are_bitwise_reproducible_and_conserve_mass():
    """12 steps in one call, in 12 calls, with the chain cut at every length from 1 to 12 and on a second handle agree bit
    for bit.  Mass: a step adds scale to gammat of each end of every pair, so it takes the sum S_i of row i to
    (1 - rho_i) S_i + rho_i (k alpha + scale t_i), t_i = 1 for a partner and m for the start node -- the closed form of
    the blends, evaluated per row.  Rounding, as test_steps_are_bitwise_reproducible_and_conserve_mass derives it: the
    blend of a cell is 4 operations, 4 eps of the cell, 4 eps S' over a row; a phi vector sums to 1 within (k + 4) eps,
    m of them added for the start node add m eps more; both scaled by rho scale; evaluating the recurrence costs another
    4 eps S'.  The bound is twice the sum, carried through the steps by the same recurrence."""
    n, k, nsteps = 400, 29, 12
    w = World(n, k, seed=3)
    stars = [w.star(int(a), int(m), c) for c, (a, m) in enumerate(zip(w.rs.randint(0, n, nsteps), w.rs.randint(0, 150, nsteps)))]
    stars[4] = w.star(stars[3]["start"], 70, 4)

    def run(cuts, chain=0):
        d = w.handle()
        d.set_star_chain(chain)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            d.step_star(stars[lo:hi])
        out = d.state() + (d.stats(),)
        d.close()
        return out

    one = run([0, nsteps])
    for other in [run([0, nsteps]), run(list(range(nsteps + 1)))] + [run([0, nsteps], chain=c) for c in range(1, nsteps + 1)]:
        assert other[0].tobytes() == one[0].tobytes() and other[1].tobytes() == one[1].tobytes()
    assert one[2][0] == sum(len(s["partner"]) for s in stars) and one[2][3] == 0
    assert run([0, nsteps], chain=5)[2] == one[2]                              # the counters cover the whole call
    eps = np.finfo(float).eps
    mass = np.array([math.fsum(r) for r in w.gamma])
    bound = np.zeros(n)
    for s in stars:
        m = len(s["partner"])
        rows = [s["start"]] + [int(j) for j in s["partner"]]
        rho = np.array([s["rho_start"]] + list(s["rho_partner"]))
        t = np.array([float(m)] + [1.0] * m)
        mass[rows] = (1 - rho) * mass[rows] + rho * (k * w.alpha + s["scale"] * t)
        bound[rows] = (1 - rho) * bound[rows] + 2 * eps * (8 * mass[rows] + rho * s["scale"] * t * (k + 4 + m))
    got = np.array([math.fsum(r) for r in one[0]])
    assert np.all(np.abs(got - mass) <= bound) and np.all(bound < 1e-9 * mass)
    assert np.all(one[0] > 0) and np.all(one[1] > 0)


def test_sweeps_star_steps_and_node_steps_mixed_on_one_handle():
    """Elogpi / Elogbeta have to be those of the state across the three kinds of work (elog_fresh)"""
    w = World(120, 5, seed=8)
    g, lam = B.sweep(w.gamma, w.lam, w.adj, w.skip, w.alpha, w.eta)
    w.dev.sweep()
    dg, dl = w.dev.state()
    np.testing.assert_allclose(dg, g, rtol=RTOL)
    _run_and_check(w, [w.star(7, 30, 0), w.star(50, 20, 1)])
    g0, l0 = w.dev.state()                                                      # an -rnode step on what the stars left
    p, q = SC.node_pairs(w.n, 33, w.skip)
    SC.assert_exits_are_clear(g0, l0, w.adj, p, q)
    rg, rl = SC.rho_gamma(0), SC.rho_lambda(0, 0)
    w.dev.step_node([33], w.n / 2.0, [rg], [rl])
    g, lam, _ = SC.step(g0, l0, w.adj, p, q, w.alpha, w.eta, w.n / 2.0, rg, rl)
    dg, dl = w.dev.state()
    np.testing.assert_allclose(dg, g, rtol=RTOL)
    np.testing.assert_allclose(dl, lam, rtol=RTOL)
    _run_and_check(w, [w.star(33, 25, 2)])
    g0, l0 = w.dev.state()
    g, lam = B.sweep(g0, l0, w.adj, w.skip, w.alpha, w.eta)
    w.dev.sweep()
    dg, dl = w.dev.state()
    np.testing.assert_allclose(dg, g, rtol=RTOL)
    np.testing.assert_allclose(dl, lam, rtol=RTOL)
    w.dev.set_state(w.gamma, w.lam)                                             # a star after set_state sees the new state
    _run_and_check(w, [w.star(3, 10, 0)])


def test_argument_errors_leave_the_state_untouched():
    w = World(100, 4, seed=2)
    good = w.star(10, 12, 0)
    skipped = sorted(w.skip)[0]

    def bad(**kw):
        s = dict(w.star(20, 6, 1))
        s.update(kw)
        return s

    base = w.star(20, 6, 1)
    cases = [
        bad(start=100),                                                                          # a node >= n
        bad(partner=np.append(base["partner"][:5], 100), y=base["y"], rho_partner=base["rho_partner"]),
        bad(partner=np.append(base["partner"][:5], 20)),                                         # a partner equal to the start
        bad(partner=np.append(base["partner"][:5], base["partner"][0]), y=np.append(base["y"][:5], base["y"][0])),   # listed twice
        dict(IC.star(skipped[0], [skipped[1]], w.adj, [0.5], 0.5, 50.0, 0.1)),                   # a pair of the skip set
        bad(y=1 - base["y"]),                                                                    # y against the graph
        bad(rho_partner=np.append(base["rho_partner"][:5], 0.0)),                                # rho outside (0, 1]
        bad(rho_partner=np.append(base["rho_partner"][:5], 1.5)),
        bad(rho_start=0.0), bad(rho_start=1.0001), bad(rho_lambda=1.5), bad(scale=0.0), bad(scale=float("inf")),
    ]
    for s in cases:
        with pytest.raises(_svils.SvilsError) as ei:
            w.dev.step_star([good, s])
        assert ei.value.code == -1, s
    g, lam = w.dev.state()
    assert g.tobytes() == w.gamma.tobytes() and lam.tobytes() == w.lam.tobytes()
    L, h = _svils.load(), w.dev._h
    one, node, y, off = np.ones(1) * 0.5, np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint8), np.array([0, 0], dtype=np.uint64)
    assert L.svils_batch_step_star(h, 1, None, off.ctypes.data, None, None, None, one.ctypes.data, one.ctypes.data, one.ctypes.data) == -1
    assert L.svils_batch_step_star(h, 1, node.ctypes.data, None, None, None, None, one.ctypes.data, one.ctypes.data, one.ctypes.data) == -1
    off[1] = 1
    assert L.svils_batch_step_star(h, 1, node.ctypes.data, off.ctypes.data, None, y.ctypes.data, one.ctypes.data, one.ctypes.data,
                                   one.ctypes.data, one.ctypes.data) == -1
    assert w.dev.state()[0].tobytes() == w.gamma.tobytes()
    with pytest.raises(_svils.SvilsError) as ei:                                # a chain longer than the documented most
        w.dev.set_star_chain(_svils.BATCH_STAR_CHAIN_MAX + 1)
    assert ei.value.code == -1
    w.dev.set_star_chain(_svils.BATCH_STAR_CHAIN_MAX)
    w.dev.step_star([good])                                                     # and the handle still works
    assert w.dev.stats()[0] == 12


def _files_agree(fa, fb, ub):
    """two printed arrays (five decimals) of states within rtol 1e-7 of each other: every cell at rtol 1e-7, except where
    the rounding to five decimals falls between the two unrounded values -- such a cell is exactly one unit of the last
    decimal apart and the unrounded value `ub` lies within its rtol 1e-7 of a rounding boundary.  Returns their number"""
    out = ~np.isclose(fa, fb, rtol=RTOL, atol=0)
    assert np.all(np.abs(fa[out] - fb[out]) <= 1e-5 * (1 + 1e-9))
    x = ub[out] * 1e5
    assert np.all(np.abs(x - np.floor(x) - 0.5) <= RTOL * x + 1e-9 * x)
    return int(out.sum())


def test_cli_and_both_engine_backends_on_lfr(graph_files, tmp_path):
    """-preprocess, then -infset on the device against -host-loops of the same seed: 300 iterations with -no-stop, three
    report intervals of 100 steps, each two launches of the chain.  gamma.txt / lambda.txt agree at rtol 1e-7 (_files_agree
    says what a five-decimal file may do at a rounding boundary); the unrounded states of the same 300 iterations, through
    both InfsetEngine backends, agree at rtol 1e-7 alone and are what the files print"""
    common = ["-file", graph_files["lfr"], "-n", "1000", "-k", "28", "-seed", "2"]
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([SVINET] + common + ["-preprocess", "-outdir", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    os.replace(tmp_path / "n1000-k28-mmsb-seed2-infset" / "neighbors.bin", work / "neighbors.bin")
    out = {}
    for name, extra in (("gpu", []), ("host", ["-host-loops"])):
        (tmp_path / name).mkdir()
        r = subprocess.run([SVINET] + common + ["-infset", "-rfreq", "100", "-no-stop", "-max-iterations", "299", "-outdir", str(tmp_path / name)]
                           + extra, capture_output=True, text=True, timeout=300, cwd=str(work))
        assert r.returncode == 0, r.stderr
        d = tmp_path / name / "n1000-k28-mmsb-seed2-infset"
        assert list(np.loadtxt(d / "heldout.txt")[:, 0]) == [0, 100, 200, 300]
        out[name] = (np.loadtxt(d / "gamma.txt")[:, 2:], np.loadtxt(d / "lambda.txt")[:, 1:], (d / "heldout-pairs.txt").read_bytes())
    assert out["gpu"][2] == out["host"][2]
    assert out["gpu"][0].shape == (1000, 28) and np.all(out["gpu"][0] > 0)
    # the same 300 iterations in the library: the CLI's calls, a report interval per call
    eng = {}
    for name, on_device in (("gpu", True), ("host", False)):
        e = InfsetEngine(graph_files["lfr"], 1000, 28, str(work / "neighbors.bin"), on_device=on_device, seed=2)
        for _ in range(3):
            e.step(100)
            assert not e.report()
        eng[name] = (e.gamma, e.lam)
        for x, printed in zip(eng[name], out[name][:2]):                        # the files print these states
            assert np.all(np.abs(printed - x) <= 0.5e-5 * (1 + 1e-6))
        e.close()
    np.testing.assert_allclose(eng["gpu"][0], eng["host"][0], rtol=RTOL)
    np.testing.assert_allclose(eng["gpu"][1], eng["host"][1], rtol=RTOL)
    flipped = _files_agree(out["gpu"][0], out["host"][0], eng["host"][0]) + _files_agree(out["gpu"][1], out["host"][1], eng["host"][1])
    print("cells printed one unit apart at a rounding boundary: %d of %d" % (flipped, out["gpu"][0].size + out["gpu"][1].size))
    # both kinds of step on both backends
    kw = dict(seed=2, inf_epsilon=0.05)
    a = InfsetEngine(graph_files["lfr"], 1000, 28, str(work / "neighbors.bin"), **kw)
    b = InfsetEngine(graph_files["lfr"], 1000, 28, str(work / "neighbors.bin"), on_device=True, **kw)
    assert np.array_equal(a.heldout, b.heldout) and np.array_equal(a.shuffled, b.shuffled)
    a.step(60)
    b.step(60)
    assert {d["kind"] for d in a.schedule} == {0, 1}
    for x, y in zip(a.schedule, b.schedule):
        assert np.array_equal(x["partner"], y["partner"]) and np.array_equal(x["rho_partner"], y["rho_partner"])
        assert (x["start"], x["kind"], x["scale"], x["rho_start"], x["rho_lambda"]) == (y["start"], y["kind"], y["scale"], y["rho_start"], y["rho_lambda"])
    assert not a.report() and not b.report() and a.iter == b.iter == 60
    np.testing.assert_allclose(b.rows, a.rows, rtol=RTOL)
    np.testing.assert_allclose(b.gamma, a.gamma, rtol=RTOL)
    np.testing.assert_allclose(b.lam, a.lam, rtol=RTOL)
