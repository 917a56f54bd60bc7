"""-m gpu: -batch-gpu, the all-pairs batch engine on the device (svils_batch_*, csrc/svils_batch.hip).

The reference is oracle/batch_oracle.py (the restatement tests/test_batch.py holds the host engine to), the tolerance that
file's: rtol 1e-7 on gamma, lambda and the heldout row -- the fixed point stops on a threshold, so a last-bit difference can
move one pair's exit by a round.  Starts are the host engine's own (its samplers, its gamma), heldout ratio 0.1."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import batch_cases as BC
from oracle import batch_oracle as B
from svinet_amd import _svils
from svinet_amd.host_api import BatchEngine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
RTOL = 1e-7


def _variant_ks():
    """for every distinct (W, V) svils_batch_variant reports over k = 2 .. 256 the smallest and the largest k that map to it"""
    by = {}
    for k in range(2, _svils.BATCH_MAX_K + 1):
        by.setdefault(_svils.batch_variant(k), []).append(k)
    ks = set()
    for v in by.values():
        ks.update((v[0], v[-1]))
    return sorted(ks | {2, 3, 4, 5, 33, 65, 200, 256})


class Start:
    """the host engine's start on a graph file, the numpy view of it, and a device handle holding the same"""

    def __init__(self, path, n, k, host_sweeps=0, skip_extra=(), eta_type="uniform"):
        e = BatchEngine(path, n, k, heldout_ratio=0.1, eta_type=eta_type)
        for _ in range(host_sweeps):
            e.sweep()
        self.n, self.k, self.eta, self.ones_prob = e.n, k, e.eta, e.ones_prob
        self.alpha = 1.0 / k
        self.gamma, self.lam = e.gamma, e.lam
        self.edges = e.edges
        self.adj = BC.adjacency(e.n, e.edges)
        self.skip = {tuple(int(x) for x in r) for r in e.heldout} | {tuple(int(x) for x in r) for r in e.validation}
        self.skip |= {tuple(r) for r in skip_extra}
        self.hsorted = sorted({tuple(int(x) for x in r) for r in e.heldout})
        self.vsorted = sorted({tuple(int(x) for x in r) for r in e.validation})
        e.close()
        self.dev = _svils.Batch(self.n, k, self.alpha, self.eta)
        self.dev.set_graph(self.edges, sorted(self.skip))
        self.dev.set_state(self.gamma, self.lam)
        self.trained = self.n * (self.n - 1) // 2 - len(self.skip)

    def heldout_y(self):
        return np.array([self.adj[a, b] for a, b in self.hsorted], dtype=np.uint8)


def _compare_sweeps(s, nsweeps):
    g, lam = s.gamma, s.lam
    for _ in range(nsweeps):
        g, lam = B.sweep(g, lam, s.adj, s.skip, s.alpha, s.eta)
        s.dev.sweep()
        dg, dl = s.dev.state()
        np.testing.assert_allclose(dg, g, rtol=RTOL)
        np.testing.assert_allclose(dl, lam, rtol=RTOL)
        pairs_done, _, rounds_max, underflow = s.dev.stats()
        assert pairs_done == s.trained and underflow == 0 and 2 <= rounds_max <= 50
        if s.hsorted:
            y = s.heldout_y()
            u = s.dev.pair_loglik(s.hsorted, y)
            np.testing.assert_allclose(BC.heldout_row(u, y, s.ones_prob), B.heldout_row(g, lam, s.hsorted, s.adj, s.ones_prob), rtol=RTOL)
    # every trained pair adds one unit of mass to each endpoint
    assert abs((dg - s.alpha).sum() - 2 * s.trained) < 1e-8
    return g, lam


@pytest.mark.parametrize("k", _variant_ks())
def test_sweeps_match_the_oracle_for_every_variant(graph_files, k):
    _compare_sweeps(Start(graph_files["assort"], 75, k), 2)


@pytest.mark.parametrize("k", [4, 5])
@pytest.mark.parametrize("n", [10, 64, 65, 129])
def test_sweeps_match_the_oracle_at_tile_edges(tmp_path, n, k):
    """fewer nodes than a tile (a ring of 10 links), one tile exactly, one node and one row past it, two tiles and a node"""
    links = BC.planted_links(n, 2, 0.0 if n == 10 else 0.3, 0.0 if n == 10 else 0.03, seed=100 + n)
    if n == 10:
        assert len(links) == 10
    s = Start(BC.write_graph(tmp_path / "g.txt", links), n, k)
    assert s.n == n
    _compare_sweeps(s, 3)


def test_sweeps_match_the_oracle_on_six_blocks(tmp_path):
    """the LFR shape in small: n = 300 in 6 blocks at k = 28"""
    links = BC.planted_links(300, 6, 0.25, 0.01, seed=28)
    _compare_sweeps(Start(BC.write_graph(tmp_path / "g.txt", links), 300, 28), 2)


def test_round_counts_that_differ_inside_a_wavefront(graph_files):
    """k = 33 on assort after 10 host sweeps: pairs of 4 to 42 rounds share wavefronts; the kernel's round counter equals
    the restated one exactly"""
    s = Start(graph_files["assort"], 75, 33, host_sweeps=10)
    rounds = BC.sweep_rounds(s.gamma, s.lam, s.adj, s.skip)
    assert rounds.min() <= 6 and rounds.max() >= 40
    _compare_sweeps(s, 1)
    pairs_done, rounds_total, rounds_max, _ = s.dev.stats()
    assert pairs_done == len(rounds)
    assert rounds_max == rounds.max() >= 40
    assert rounds_total == int(rounds.sum())


def test_pairs_that_reach_the_cap_of_50_rounds(graph_files):
    """k = 4 on assort with -eta-type fromdata, from the start: on the CPU this state needs 6 to 50 rounds, the pairs at 50
    leave by the cap and not by the test"""
    s = Start(graph_files["assort"], 75, 4, eta_type="fromdata")
    rounds = BC.sweep_rounds(s.gamma, s.lam, s.adj, s.skip)
    assert rounds.max() == 50 and rounds.min() < 10
    _compare_sweeps(s, 1)
    pairs_done, rounds_total, rounds_max, _ = s.dev.stats()
    assert (pairs_done, rounds_total, rounds_max) == (len(rounds), int(rounds.sum()), 50)


def test_skipped_pairs_in_every_kind_of_tile(tmp_path):
    """n = 150, k = 4 (tiles of 64 x 64): skipped pairs in a diagonal tile, an off-diagonal tile and the ragged last tiles"""
    n, k = 150, 4
    links = BC.planted_links(n, 3, 0.3, 0.02, seed=150)
    extra = [(3, 40), (5, 100), (64, 65), (70, 149), (130, 140), (148, 149)]
    s = Start(BC.write_graph(tmp_path / "g.txt", links), n, k, skip_extra=extra)
    assert s.n == n and all(e in s.skip for e in extra)
    _compare_sweeps(s, 2)
    dg, _ = s.dev.state()
    assert abs((dg - s.alpha).sum() - 2 * (n * (n - 1) // 2 - len(s.skip))) < 1e-8
    assert s.dev.stats()[0] == n * (n - 1) // 2 - len(s.skip)


@pytest.mark.parametrize("n,k", [(2000, 8), (4160, 4)])
def test_two_handles_agree_bitwise(n, k):
    """no oracle at this size: two handles, three sweeps each, gamma and lambda equal bit for bit, mass conserved.
    n = 4160 has 2145 tiles, more than one launch of the pair kernel holds (the partials of the launches are added in order).
    Mass bound: 2 P units summed in n k cells of at most n terms each: at most 2 P n eps of rounding."""
    links = BC.planted_links(n, 8, 0.05, 0.002, seed=n)
    rs = np.random.RandomState(n + 1)
    gamma = rs.gamma(100.0, 0.01, (n, k))
    lam = np.tile([1.0, 1.0], (k, 1))
    skip = links[::97][:50]
    out = []
    for _ in range(2):
        d = _svils.Batch(n, k, 1.0 / k, (1.0, 1.0))
        d.set_graph(links, skip)
        d.set_state(gamma, lam)
        d.sweep(3)
        out.append(d.state() + (d.stats(),))
        d.close()
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    assert out[0][2] == out[1][2]
    trained = n * (n - 1) // 2 - len(skip)
    assert out[0][2][0] == trained and out[0][2][3] == 0
    assert abs((out[0][0] - 1.0 / k).sum() - 2 * trained) < 2 * trained * n * np.finfo(float).eps
    # lambda: the products phi1 phi2 of a pair sum to at most 1
    assert 0 < (out[0][1] - 1.0).sum() <= trained


@pytest.mark.parametrize("k", [4, 200])
def test_pair_likelihoods_match_the_oracle(graph_files, k):
    s = Start(graph_files["assort"], 75, k)
    s.dev.sweep(2)
    g, lam = s.dev.state()
    pairs = s.hsorted + s.vsorted
    y = np.array([s.adj[a, b] for a, b in pairs], dtype=np.uint8)
    assert len(pairs) > 100 and 0 < y.sum() < len(y)
    ref = np.array([B.edge_likelihood(g, lam, a, b, yy) for (a, b), yy in zip(pairs, y)])
    np.testing.assert_allclose(s.dev.pair_loglik(pairs, y), ref, rtol=0, atol=1e-9)
    # a pair whose sum falls below the floor of 1e-30: two nodes with all their mass in different communities
    g2 = g.copy()
    g2[0], g2[1] = 1e-40, 1e-40
    g2[0, 0], g2[1, 1] = 1.0, 1.0
    s.dev.set_state(g2, lam)
    both = s.dev.pair_loglik([(0, 1), (0, 1)], [1, 0])
    assert B.edge_likelihood(g2, lam, 0, 1, 1) == np.log(1e-30) and abs(both[0] - np.log(1e-30)) < 1e-9
    assert abs(both[1] - B.edge_likelihood(g2, lam, 0, 1, 0)) < 1e-9


def test_pair_likelihood_lists_regrow_and_go_with_the_graph(graph_files):
    """the call's lists are grown on demand inside the graph's scope: 3 pairs, 50 (regrown), 3 (kept), a new graph (released
    with the old one), 50 (allocated anew) -- every result is, byte for byte, that of a fresh handle's first call"""
    s = Start(graph_files["assort"], 75, 5)
    rs = np.random.RandomState(19)
    pairs = np.array([(a, b) for a, b in np.sort(rs.randint(0, 75, size=(80, 2)), axis=1) if a != b][:50])
    y = np.array([s.adj[a, b] for a, b in pairs], dtype=np.uint8)
    assert len(pairs) == 50 and 0 < y.sum() < 50

    def fresh(m):
        d = _svils.Batch(s.n, s.k, s.alpha, s.eta)
        d.set_state(s.gamma, s.lam)
        out = d.pair_loglik(pairs[:m], y[:m])
        d.close()
        return out

    ref = {m: fresh(m) for m in (3, 50)}
    assert ref[50][:3].tobytes() == ref[3].tobytes()
    for m in (3, 50, 3):
        assert s.dev.pair_loglik(pairs[:m], y[:m]).tobytes() == ref[m].tobytes()
    s.dev.set_graph(s.edges, sorted(s.skip))
    assert s.dev.pair_loglik(pairs, y).tobytes() == ref[50].tobytes()
    s.dev.sweep()                                                             # the handle still sweeps: the second graph is whole
    assert s.dev.stats()[0] == s.trained


def test_host_engine_with_both_backends(graph_files):
    a = BatchEngine(graph_files["assort"], 75, 4, heldout_ratio=0.1, eta_type="fromdata")
    b = BatchEngine(graph_files["assort"], 75, 4, heldout_ratio=0.1, eta_type="fromdata", on_device=True)
    assert np.array_equal(a.heldout, b.heldout) and np.array_equal(a.validation, b.validation)
    for _ in range(3):
        a.sweep()
        b.sweep()
        assert not a.report() and not b.report()
    assert a.iter == b.iter == 3 and a.rows.shape == b.rows.shape == (4, 10)
    np.testing.assert_allclose(b.rows, a.rows, rtol=RTOL)
    np.testing.assert_allclose(b.gamma, a.gamma, rtol=RTOL)
    np.testing.assert_allclose(b.lam, a.lam, rtol=RTOL)


def _cli(args, tmp, timeout=300):
    return subprocess.run([SVINET] + args + ["-outdir", str(tmp)], capture_output=True, text=True, timeout=timeout)


def test_cli_batch_gpu_runs_to_stop_and_finds_blocks(graph_files, tmp_path):
    """what tests/test_batch.py asserts of -batch, of -batch-gpu; the samplers' files are those of a -batch run"""
    common = ["-file", graph_files["assort"], "-n", "75", "-k", "4", "-eta-type", "fromdata", "-heldout-ratio", "0.1"]
    (tmp_path / "gpu").mkdir()
    (tmp_path / "host").mkdir()
    r = _cli(common + ["-batch-gpu"], tmp_path / "gpu")
    assert r.returncode == 0, r.stderr
    d = tmp_path / "gpu" / "n75-k4-mmsb-batch"
    for f in ("param.txt", "heldout-edges.txt", "validation-edges.txt", "heldout.txt", "validation.txt", "max.txt",
              "gamma.txt", "lambda.txt", "groups.txt", "communities.txt", "summary.txt"):
        assert (d / f).exists(), f
    it, _, a, _, max_h, _, why = (d / "max.txt").read_text().split()
    assert int(it) > 75 and int(why) in (0, 1)                          # stop rule is armed after n sweeps
    rows = np.loadtxt(d / "heldout.txt")
    assert rows.shape == (int(it) + 1, 11) and rows[-1, 10] > rows[0, 10]
    gam = np.loadtxt(d / "gamma.txt")
    assert gam.shape == (75, 6) and np.all(gam[:, 2:] > 0)
    assert np.loadtxt(d / "lambda.txt").shape == (4, 3)
    groups = np.loadtxt(d / "groups.txt")
    assert groups.shape == (75, 7) and np.allclose(groups[:, 2:6].sum(1), 1, atol=2e-3)
    label = dict(zip(groups[:, 1].astype(int), groups[:, 6].astype(int)))
    found = []
    for lo, hi in ((2, 21), (24, 44), (48, 66), (67, 75)):              # the generator's four blocks
        ls = [label[i] for i in range(lo, hi + 1)]
        top = max(set(ls), key=ls.count)
        assert ls.count(top) >= 0.85 * len(ls)
        found.append(top)
    assert len(set(found)) == 4
    comm = [l.split() for l in (d / "communities.txt").read_text().splitlines() if l.strip()]
    assert 3 <= len(comm) <= 4 and all(len(set(c)) == len(c) for c in comm)
    h = _cli(common + ["-batch", "-max-iterations", "1"], tmp_path / "host")
    assert h.returncode == 0, h.stderr
    for f in ("heldout-edges.txt", "validation-edges.txt"):
        assert (d / f).read_bytes() == (tmp_path / "host" / "n75-k4-mmsb-batch" / f).read_bytes(), f


def test_cli_batch_gpu_refuses_k_above_the_limit(graph_files, tmp_path):
    r = _cli(["-file", graph_files["assort"], "-n", "75", "-k", "300", "-batch-gpu"], tmp_path, timeout=60)
    assert r.returncode != 0 and "256" in r.stderr
    assert not list(tmp_path.iterdir())


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def test_scopes_set_graph_twice_and_destroy_in_flight():
    """the style of tests/test_gpu_tool_scopes.py: after a warm-up cycle, cycles of create -> set_graph (a refused one on the
    way, then a second graph) -> state -> sweeps -> destroy with the sweeps still in flight leave the free memory where it was;
    the second graph is the one the sweeps see"""
    L = _svils.load()
    n, k = 1500, 16
    g1, g2 = BC.planted_links(n, 4, 0.05, 0.002, seed=1), BC.planted_links(n, 4, 0.03, 0.004, seed=2)
    gamma = np.random.RandomState(3).gamma(100.0, 0.01, (n, k))
    lam = np.tile([1.0, 1.0], (k, 1))

    def cycle(check):
        d = _svils.Batch(n, k, 1.0 / k, (1.0, 1.0))
        d.set_graph(g1, g1[:40])
        bad = g1.copy()
        bad[-1] = bad[0]                     # a repeated link: refused, the handle keeps its graph
        assert L.svils_batch_set_graph(d._h, bad.ctypes.data, len(bad), None, 0) == -1
        bad[-1] = (5, 5)                     # a self pair
        assert L.svils_batch_set_graph(d._h, bad.ctypes.data, len(bad), None, 0) == -1
        d.set_state(gamma, lam)
        d.sweep(1)
        first = d.state()[0]
        d.set_graph(g2, g2[:10])
        d.set_state(gamma, lam)
        d.sweep(1)
        if check:
            second = d.state()[0]
            assert d.stats()[0] == n * (n - 1) // 2 - 10
            assert not np.array_equal(first, second)
            e = _svils.Batch(n, k, 1.0 / k, (1.0, 1.0))   # a fresh handle given the second graph alone agrees bit for bit
            e.set_graph(g2, g2[:10])
            e.set_state(gamma, lam)
            e.sweep(1)
            assert e.state()[0].tobytes() == second.tobytes()
            e.close()
        d.sweep(3)                           # enqueued, not waited for
        d.close()

    cycle(True)
    warm = _free_bytes()
    for _ in range(2):
        cycle(False)
        assert _free_bytes() >= warm - (2 << 20)
