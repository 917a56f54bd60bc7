"""-m gpu: the stratified random node steps of -snode on the device (svils_batch_step_strat: k_batch_strat_pairs,
k_batch_strat_tail and the lazy decay with k_batch_catch_up in csrc/svils_batch.hip).

The reference is tests/snode_cases.py, a restatement of one EAGER step (all n rows move) on top of oracle/batch_oracle.py.
Tolerance: rtol 1e-7 on gamma and lambda, the one tests/sampled_cases.py and tests/infset_cases.py hold this fixed point
to.  sampled_cases.assert_exits_are_clear is asserted for the pairs of every restated step, and with it the device's round
counters equal the restated ones exactly.  Graphs: random sparse ones of at most 300 nodes (batch_cases.planted_links),
the state a seeded gamma draw.  Every input below lets the restatement itself run clean (no normaliser underflow, the exit
margins clear, every block of non-links complete): the seeds were chosen so, on the host."""
import math
import os
import subprocess

import numpy as np
import pytest

import batch_cases as BC
import sampled_cases as SC
import snode_cases as NC
from oracle import batch_oracle as B
from svinet_amd import _svils
from svinet_amd.host_api import StratNodeEngine
from test_gpu_batch import RTOL, SVINET

pytestmark = pytest.mark.gpu

ELOG_ATOL = 1e-12   # as tests/test_gpu_infset.py: two digammas of magnitude < 20, 1e-13 in all; ten times that


class World:
    """a planted graph, a skip set, a seeded state and (on first use) a device handle holding them"""

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
        self._dev = None

    @property
    def dev(self):
        if self._dev is None:
            self._dev = self.handle()
        return self._dev

    def handle(self):
        d = _svils.Batch(self.n, self.k, self.alpha, self.eta)
        d.set_graph(self.links, sorted(self.skip))
        d.set_state(self.gamma, self.lam)
        return d

    def handle_ll(self, g, lam, y):
        """the pair likelihoods of the skip list from a fresh handle holding (g, lam): no step has run on it"""
        d = self.handle()
        d.set_state(g, lam)
        out = d.pair_loglik(self.skiplist, y)
        d.close()
        return out

    def free(self, a, avoid=()):
        return [j for j in range(self.n) if j != a and j not in avoid and (min(a, j), max(a, j)) not in self.skip]

    def star(self, a, it, kind=None, m=None, avoid=(), rho_gamma=None, rho_lambda=None):
        """kind 0: the links of a outside the skip set (or the first m), at the scale of a link step; kind 1: m (default
        n // 10) shuffled non-links of a, at the scale of a non-link step; kind None: m entries, links first.  The step
        sizes are those of iteration `it` with nodetau0 = 3 and tau0 = 10, so that rows move visibly"""
        free = self.free(a, avoid)
        ones, zeros = [j for j in free if self.adj[a, j]], [j for j in free if not self.adj[a, j]]
        self.rs.shuffle(zeros)
        if kind == 0:
            partner = ones if m is None else ones[:m]
        elif kind == 1:
            partner = zeros[:NC.setsize(self.n) if m is None else m]
        else:
            partner = (ones + zeros)[:m]
        assert m is None or len(partner) == m
        return NC.star(a, partner, self.adj, NC.rho_gamma(it, nodetau0=3.0) if rho_gamma is None else rho_gamma,
                       NC.scale_of(1 if kind == 1 else 0, self.n), NC.rho_lambda(it, tau0=10.0) if rho_lambda is None else rho_lambda)

    def mixed(self, nsteps, it0=0, avoid=()):
        """steps of both kinds at random start nodes"""
        starts = [int(a) for a in self.rs.randint(0, self.n, 4 * nsteps) if a not in avoid][:nsteps]
        return [self.star(a, it0 + c, kind=int(kd), avoid=avoid) for c, (a, kd) in enumerate(zip(starts, self.rs.randint(0, 2, nsteps)))]

    def guard(self, g, lam, p, q):
        SC.assert_exits_are_clear(g, lam, self.adj, p, q)

    def restate(self, g, lam, steps):
        return NC.run(g, lam, self.adj, steps, self.alpha, self.eta, guard=self.guard)


def _run_and_check(w, steps):
    g0, l0 = w.dev.state()
    w.dev.step_strat(steps)
    assert w.dev.lag() == w.n - 1 - len(steps[-1]["partner"])                   # all rows but those of the last step are behind
    g, lam, rounds = w.restate(g0, l0, steps)
    pairs_done, rounds_total, rounds_max, underflow = w.dev.stats()
    assert (pairs_done, rounds_total, underflow) == (len(rounds), int(rounds.sum()), 0)
    assert rounds_max == (int(rounds.max()) if len(rounds) else 0)
    assert w.dev.timing()[0] > 0
    dg, dl = w.dev.state()
    assert w.dev.lag() == 0
    np.testing.assert_allclose(dg, g, rtol=RTOL)
    np.testing.assert_allclose(dl, lam, rtol=RTOL)
    e1, b1 = w.dev.expectations()                                               # the step maintains no Elogpi: renewed here
    np.testing.assert_allclose(e1, B.dir_exp(dg), rtol=0, atol=ELOG_ATOL)
    np.testing.assert_allclose(b1, B.dir_exp(dl), rtol=0, atol=ELOG_ATOL)
    return dg, dl


def variant_case(k):
    w = World(130, k, seed=10 + k)
    return w, w.mixed(12)


@pytest.mark.parametrize("k", [3, 7, 13, 29, 61, 100, 200, 256])
def test_steps_match_the_restatement_for_every_variant(k):
    """one K per W of the (W, V) table, none filling its W x V lanes, and the largest K; n = 130: a block of 13 non-links;
    12 steps of both kinds in one call"""
    assert {_svils.batch_variant(x)[0] for x in (3, 7, 13, 29, 61, 100, 200)} == {1, 2, 4, 8, 16, 32, 64}
    w, steps = variant_case(k)
    assert {len(s["partner"]) == 13 and not s["y"].any() for s in steps} == {True, False}
    _run_and_check(w, steps)


def entry_case(k):
    wd, _ = _svils.batch_variant(k)
    G = 64 // wd
    w = World(300, k, seed=80 + k)
    counts = sorted({0, 1, G - 1, G, G + 1, 4 * G, 4 * G + 1})
    return w, G, [w.star(int(a), c, m=m) for c, (a, m) in enumerate(zip(w.rs.randint(20, w.n, len(counts)), counts))]


@pytest.mark.parametrize("k", [3, 256])
def test_entry_counts_around_the_group_and_workgroup_sizes(k):
    """W = 1 (G = 64 groups per wavefront) and W = 64 (G = 1): 0, 1, G - 1, G, G + 1, 4 G (a full workgroup) and 4 G + 1
    entries, in one call and each alone"""
    w, G, steps = entry_case(k)
    assert G == (64 if k == 3 else 1) and [len(s["partner"]) for s in steps][-1] == 4 * G + 1
    _run_and_check(w, steps)
    for s in steps:
        _run_and_check(w, [s])


def decay_case():
    """40 steps: none names row r; row t is named first at step 30 (a partner) and is the start node of step 31"""
    w = World(200, 7, seed=21)
    r, t = 150, 60
    steps = w.mixed(30, avoid=(r, t))
    s30 = w.star(17, 30, m=20, avoid=(r, t))
    s30 = NC.star(17, np.append(s30["partner"][:19], t), w.adj, s30["rho_gamma"], s30["scale"], s30["rho_lambda"])
    steps += [s30, w.star(t, 31, kind=0, avoid=(r,))] + w.mixed(8, it0=32, avoid=(r,))
    return w, r, t, steps


def test_decay_of_untouched_rows_and_of_rows_touched_late():
    """A row no step names equals alpha + (gamma0 - alpha) prod (1 - rho_s): the forty log1p and the one exp are each within
    a few ulp, the forty additions into c within 40 eps |c| / 2 with |c| < 15, so the factor is within 1e-13; rtol 1e-12.
    A row first read after 30 untouched steps equals the restatement"""
    w, r, t, steps = decay_case()
    assert len(steps) == 40 and all(r != s["start"] and r not in s["partner"] for s in steps)
    assert all(t != s["start"] and t not in s["partner"] for s in steps[:30]) and t in steps[30]["partner"] and steps[31]["start"] == t
    dg, _ = _run_and_check(w, steps)
    f = np.prod([1 - s["rho_gamma"] for s in steps])
    np.testing.assert_allclose(dg[r], w.alpha + (w.gamma[r] - w.alpha) * f, rtol=1e-12)
    assert 1e-6 < f < 1e-4 and abs(math.log(f)) < 15


def underflow_case():
    w = World(100, 5, seed=33)
    steps = [w.star(c % 10, c, m=3, avoid=range(40, 100), rho_gamma=0.999) for c in range(300)]
    return w, steps


def test_a_decay_factor_that_underflows_leaves_alpha():
    """rho_gamma = 0.999 for 300 steps: c = 300 log1p(-0.999) = -2072 and exp(c) is 0.  The rows no step names are then
    exactly alpha, nothing is NaN, and the named rows are the restatement's"""
    w, steps = underflow_case()
    assert math.exp(sum(math.log1p(-s["rho_gamma"]) for s in steps)) == 0.0
    dg, dl = _run_and_check(w, steps)
    named = sorted({s["start"] for s in steps} | {int(j) for s in steps for j in s["partner"]})
    rest = np.setdiff1d(np.arange(w.n), named)
    assert len(rest) >= 60 and np.all(dg[rest] == w.alpha)
    assert not np.all(dg[named] == w.alpha)                                    # (a named row decays too once the steps leave it alone)
    assert np.all(np.isfinite(dg)) and np.all(np.isfinite(dl))


def test_lag_counts_the_rows_behind():
    w = World(130, 7, seed=4)
    assert w.dev.lag() == 0
    steps = w.mixed(3)
    w.dev.step_strat(steps)
    behind = w.n - 1 - len(steps[-1]["partner"])
    assert w.dev.lag() == behind
    bad = dict(steps[0], rho_gamma=1.0)
    with pytest.raises(_svils.SvilsError) as ei:
        w.dev.step_strat([steps[1], bad])
    assert ei.value.code == -1 and w.dev.lag() == behind                       # a refused call changes nothing
    w.dev.state()
    assert w.dev.lag() == 0
    w.dev.step_strat([w.star(5, 3, m=0)])                                       # a step without entries: only its start node is current
    assert w.dev.lag() == w.n - 1
    w.dev.set_state(w.gamma, w.lam)
    assert w.dev.lag() == 0


def repro_case():
    w = World(130, 29, seed=3)
    steps = w.mixed(12)
    steps[4] = w.star(steps[3]["start"], 4, kind=0)                             # the same start node twice in a row
    return w, steps


def test_steps_are_bitwise_reproducible_however_they_are_cut():
    """12 steps in one call, in 12 calls, cut in two at every length and on a second handle agree bit for bit at the final
    get_state: the factors depend on the running c and the rows' c_i alone, never on the calls.  A get_state after step 6
    brings every row to its true value there -- a rounding of the rows that were behind -- so that run agrees with the
    restatement at rtol 1e-7 and with the uninterrupted run to rounding; the largest relative difference is printed (DESIGN.md
    section 4m quotes it), there is no bound of its own to assert"""
    w, steps = repro_case()
    n = len(steps)

    def run(cuts, look=False):
        d = w.handle()
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            d.step_strat(steps[lo:hi])
            if look:
                d.state()
        out = d.state() + (d.stats(),)
        d.close()
        return out

    one = run([0, n])
    for other in [run([0, n]), run(list(range(n + 1)))] + [run([0, c, n]) for c in range(1, n)]:
        assert other[0].tobytes() == one[0].tobytes() and other[1].tobytes() == one[1].tobytes()
    assert one[2][0] == sum(len(s["partner"]) for s in steps) and one[2][3] == 0
    g, lam, _ = w.restate(w.gamma, w.lam, steps)
    looked = run([0, 6, n], look=True)
    np.testing.assert_allclose(looked[0], g, rtol=RTOL)
    np.testing.assert_allclose(looked[1], lam, rtol=RTOL)
    print("largest relative difference of gamma after a get_state at step 6: %.3g" % np.max(np.abs(looked[0] - one[0]) / one[0]))


def test_row_sums_follow_the_closed_form():
    """A step takes the sum S_i of row i to (1 - rho) S_i + rho (k alpha + scale t_i), t_i = m for the start node, 1 for a
    partner and 0 for every other row.  Rounding, as test_gpu_sampled.py::test_steps_are_bitwise_reproducible_and_conserve_mass
    derives it and test_gpu_infset.py carries it per row: the blend of a cell is 4 operations, 4 eps S' over a row; a phi
    vector sums to 1 within (k + 4) eps, m of them added for the start node add m eps more, both scaled by rho scale;
    evaluating the recurrence costs another 4 eps S'.  The decay adds its factor exp(c - c_i): c within eps |c| / 2 per
    addition, log1p and exp within an ulp each, here (|c| + 2) eps S' per step.  The bound is twice the sum, carried through
    the steps by the same recurrence"""
    w, steps = repro_case()
    w.dev.step_strat(steps)
    dg, dl = w.dev.state()
    eps, k = np.finfo(float).eps, w.k
    mass = np.array([math.fsum(r) for r in w.gamma])
    bound, c = np.zeros(w.n), 0.0
    for s in steps:
        m, rho = len(s["partner"]), s["rho_gamma"]
        t = np.zeros(w.n)
        t[s["partner"]] = 1.0
        t[s["start"]] = float(m)
        c += math.log1p(-rho)
        mass = (1 - rho) * mass + rho * (k * w.alpha + s["scale"] * t)
        bound = (1 - rho) * bound + 2 * eps * ((8 + abs(c) + 2) * mass + rho * s["scale"] * t * (k + 4 + m))
    got = np.array([math.fsum(r) for r in dg])
    assert np.all(np.abs(got - mass) <= bound) and np.all(bound < 1e-9 * mass)
    assert np.all(dg > 0) and np.all(dl > 0)


def mixed_case():
    w = World(120, 5, seed=8)
    return w, w.mixed(3), w.mixed(3, it0=3)


def test_sweeps_strat_steps_node_steps_and_star_steps_mixed_on_one_handle():
    """every other entry point catches the rows up first, and Elogpi / Elogbeta are those of the state across all kinds of work"""
    import infset_cases as IC
    w, first, second = mixed_case()
    g, lam = B.sweep(w.gamma, w.lam, w.adj, w.skip, w.alpha, w.eta)
    w.dev.sweep()
    w.dev.step_strat(first)                                                     # on what the sweep left, and not looked at:
    g, lam, _ = w.restate(g, lam, first)
    p, q = SC.node_pairs(w.n, 33, w.skip)                                       # the node step has to catch the rows up itself
    SC.assert_exits_are_clear(g, lam, w.adj, p, q)
    rg, rl = SC.rho_gamma(0), SC.rho_lambda(0, 0)
    assert w.dev.lag() > 0
    w.dev.step_node([33], w.n / 2.0, [rg], [rl])
    assert w.dev.lag() == 0
    g, lam, _ = SC.step(g, lam, w.adj, p, q, w.alpha, w.eta, w.n / 2.0, rg, rl)
    dg, dl = w.dev.state()
    np.testing.assert_allclose(dg, g, rtol=RTOL)
    np.testing.assert_allclose(dl, lam, rtol=RTOL)
    w.dev.step_strat(second[:1])
    g, lam, _ = w.restate(g, lam, second[:1])
    free = w.free(40)[:25]                                                      # a star step on rows that are behind
    s = IC.star(40, free, w.adj, [0.3] * 25, 0.4, w.n / 2.0, 0.1)
    SC.assert_exits_are_clear(g, lam, w.adj, *IC.pairs_of(s))
    w.dev.step_star([s])
    g, lam, _ = IC.step(g, lam, w.adj, s, w.alpha, w.eta)
    _, l0 = w.dev.state()
    np.testing.assert_allclose(l0, lam, rtol=RTOL)
    w.dev.step_strat(second[1:])
    g, lam, _ = w.restate(g, lam, second[1:])
    y = w.adj[w.skiplist[:, 0], w.skiplist[:, 1]].astype(np.uint8)              # the pair likelihoods read caught-up rows
    ll = w.dev.pair_loglik(w.skiplist, y)
    assert w.dev.lag() == 0
    dg, dl = w.dev.state()
    np.testing.assert_allclose(dg, g, rtol=RTOL)
    np.testing.assert_allclose(dl, lam, rtol=RTOL)
    np.testing.assert_allclose(ll, w.handle_ll(dg, dl, y), rtol=RTOL)
    w.dev.step_strat(first[:1])                                                 # ... and so does a sweep
    g, lam, _ = w.restate(dg, dl, first[:1])
    g, lam = B.sweep(g, lam, w.adj, w.skip, w.alpha, w.eta)
    w.dev.sweep()
    dg, dl = w.dev.state()
    np.testing.assert_allclose(dg, g, rtol=RTOL)
    np.testing.assert_allclose(dl, lam, rtol=RTOL)


def test_argument_errors_leave_the_state_and_the_lag_untouched():
    w = World(100, 4, seed=2)
    good = w.star(10, 0, m=12)
    skipped = sorted(w.skip)[0]
    base = w.star(20, 1, m=6)

    def bad(**kw):
        s = dict(base)
        s.update(kw)
        return s

    cases = [
        bad(start=100),                                                                          # a node >= n
        bad(partner=np.append(base["partner"][:5], 100)),
        bad(partner=np.append(base["partner"][:5], 20)),                                         # a partner equal to the start
        bad(partner=np.append(base["partner"][:5], base["partner"][0]), y=np.append(base["y"][:5], base["y"][0])),   # listed twice
        dict(NC.star(skipped[0], [skipped[1]], w.adj, 0.5, 50.0, 0.1)),                          # a pair of the skip set
        bad(y=1 - base["y"]),                                                                    # y against the graph
        bad(rho_gamma=0.0), bad(rho_gamma=1.0), bad(rho_gamma=1.0001), bad(rho_gamma=float("nan")),   # outside (0, 1)
        bad(rho_lambda=1.5), bad(scale=0.0), bad(scale=float("inf")),
    ]
    for s in cases:
        with pytest.raises(_svils.SvilsError) as ei:
            w.dev.step_strat([good, s])
        assert ei.value.code == -1, s
    assert w.dev.lag() == 0
    g, lam = w.dev.state()
    assert g.tobytes() == w.gamma.tobytes() and lam.tobytes() == w.lam.tobytes()
    L, h = _svils.load(), w.dev._h
    one, node, y, off = np.ones(1) * 0.5, np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint8), np.array([0, 0], dtype=np.uint64)
    assert L.svils_batch_step_strat(h, 1, None, off.ctypes.data, None, None, one.ctypes.data, one.ctypes.data, one.ctypes.data) == -1
    assert L.svils_batch_step_strat(h, 1, node.ctypes.data, None, None, None, one.ctypes.data, one.ctypes.data, one.ctypes.data) == -1
    off[1] = 1
    assert L.svils_batch_step_strat(h, 1, node.ctypes.data, off.ctypes.data, None, y.ctypes.data, one.ctypes.data, one.ctypes.data,
                                    one.ctypes.data) == -1
    assert L.svils_batch_get_lag(h, None) == -1
    assert w.dev.state()[0].tobytes() == w.gamma.tobytes()
    w.dev.step_strat([good])                                                    # and the handle still works
    assert w.dev.stats()[0] == 12 and w.dev.lag() == w.n - 13
    with pytest.raises(_svils.SvilsError):                                      # with rows behind: still nothing changes
        w.dev.step_strat([good, cases[3]])
    assert w.dev.lag() == w.n - 13
    d = w.handle()
    d.step_strat([good])
    assert d.state()[0].tobytes() == w.dev.state()[0].tobytes()
    d.close()


def _files_agree(fa, fb, ub):
    """as tests/test_gpu_infset.py: two printed arrays (five decimals) of states within rtol 1e-7 of each other agree at rtol
    1e-7, except where the rounding to five decimals falls between the two unrounded values -- such a cell is one unit of the
    last decimal apart and the unrounded value `ub` lies within its rtol 1e-7 of a rounding boundary.  Returns their number"""
    out = ~np.isclose(fa, fb, rtol=RTOL, atol=0)
    assert np.all(np.abs(fa[out] - fb[out]) <= 1e-5 * (1 + 1e-9))
    x = ub[out] * 1e5
    assert np.all(np.abs(x - np.floor(x) - 0.5) <= RTOL * x + 1e-9 * x)
    return int(out.sum())


# What tests/test_gpu_infset.py's CLI comparison runs.  Seed 4: the exit margins of all 300 restated steps are clear (checked on
# the host with sampled_cases.assert_exits_are_clear; with seeds 1, 2, 3, 5 and 8 a pair sits within 1e-4 of the threshold
# at iteration 184, 265, 165, 295 and 222), and every block of non-links finds its 100 nodes within a lap
CLI_ITERATIONS = 300


def test_cli_and_both_engine_backends_on_lfr(graph_files, tmp_path):
    """-snode on the device against -host-loops of the same seed: 300 iterations with -no-stop, three report intervals of
    100 steps, each one svils_batch_step_strat call.  gamma.txt / lambda.txt agree at rtol 1e-7 (_files_agree says what a
    five-decimal file may do at a rounding boundary); the unrounded states of the same iterations, through both
    StratNodeEngine backends, agree at rtol 1e-7 alone and are what the files print"""
    common = ["-file", graph_files["lfr"], "-n", "1000", "-k", "28", "-seed", "4"]
    out = {}
    for name, extra in (("gpu", []), ("host", ["-host-loops"])):
        (tmp_path / name).mkdir()
        r = subprocess.run([SVINET] + common + ["-snode", "-no-stop", "-max-iterations", str(CLI_ITERATIONS - 1), "-outdir", str(tmp_path / name)]
                           + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        d = tmp_path / name / "n1000-k28-mmsb-seed4-SUrnode"
        assert list(np.loadtxt(d / "heldout.txt")[:, 0]) == [0, 100, 200, 300]
        out[name] = (np.loadtxt(d / "gamma.txt")[:, 2:], np.loadtxt(d / "lambda.txt")[:, 1:], (d / "heldout-pairs.txt").read_bytes())
    assert out["gpu"][2] == out["host"][2]
    assert out["gpu"][0].shape == (1000, 28) and np.all(out["gpu"][0] > 0)
    eng = {}
    for name, on_device in (("gpu", True), ("host", False)):
        e = StratNodeEngine(graph_files["lfr"], 1000, 28, on_device=on_device, seed=4)
        for _ in range(CLI_ITERATIONS // 100):
            e.sweep()
            assert not e.report()
        eng[name] = (e.gamma, e.lam, e.schedule(), e.rows)
        for x, printed in zip(eng[name][:2], out[name][:2]):                    # the files print these states
            assert np.all(np.abs(printed - x) <= 0.5e-5 * (1 + 1e-6))
        e.close()
    np.testing.assert_allclose(eng["gpu"][0], eng["host"][0], rtol=RTOL)
    np.testing.assert_allclose(eng["gpu"][1], eng["host"][1], rtol=RTOL)
    np.testing.assert_allclose(eng["gpu"][3], eng["host"][3], rtol=RTOL)
    flipped = _files_agree(out["gpu"][0], out["host"][0], eng["host"][0]) + _files_agree(out["gpu"][1], out["host"][1], eng["host"][1])
    print("cells printed one unit apart at a rounding boundary: %d of %d" % (flipped, out["gpu"][0].size + out["gpu"][1].size))
    assert {d["kind"] for d in eng["gpu"][2]} == {0, 1}                         # both kinds of step on both backends
    for x, y in zip(eng["gpu"][2], eng["host"][2]):
        assert np.array_equal(x["partner"], y["partner"])
        assert (x["start"], x["kind"], x["scale"], x["rho_gamma"], x["rho_lambda"]) == (y["start"], y["kind"], y["scale"], y["rho_gamma"], y["rho_lambda"])
        assert x["kind"] == 0 or len(x["partner"]) == 100
