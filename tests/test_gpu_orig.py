"""-m gpu: -orig, the full K x K blockmodel on the device (svils_orig_*, csrc/svils_orig.hip).

The reference is tests/orig_cases.py, a numpy restatement of one sweep of MMSBInferOrig::batch_infer.  Tolerance: rtol 1e-7
on gamma and beta, the bound the sibling engines are held to; the counters (pairs visited, rounds over all pairs, most
rounds of a pair) are exact.  On the CPU the restatement's round counts do not move under a permutation of the K columns
(another summation order) on states of this kind, and gamma / beta agree to 2e-15, so exact counters do not rest on luck."""
import functools
import os
import subprocess

import numpy as np
import pytest

import orig_cases as OC
from conftest import GOLDEN
from svinet_amd import _svils
from svinet_amd.host_api import OrigEngine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
ASSORT = os.path.join(GOLDEN, "graphs", "assort-75-4.txt")
RTOL = 1e-7
ERR_ARG, ERR_UNSUPPORTED = -1, -4
KS = (2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64)
# (k, n, seed) of the peaked states: n = 75 .. 96, every seed checked against OC.check_conditions below
PEAKED = ((2, 75, 103), (3, 82, 21), (4, 89, 22), (5, 96, 23), (15, 81, 24), (16, 88, 25), (17, 95, 26), (31, 80, 27),
          (32, 87, 28), (33, 94, 29), (48, 79, 30), (49, 84, 33), (63, 86, 31), (64, 93, 32))


def _device(n, k, links, skip, gamma, beta, launch_rows=0):
    d = _svils.Orig(n, k, 1.0 / k)
    if launch_rows:
        d.set_launch_rows(launch_rows)
    d.set_graph(links, skip)
    d.set_state(gamma, beta)
    return d


@functools.lru_cache(maxsize=None)
def _peaked_reference(k, n, seed):
    """the state and five restated sweeps from it: computed once, shared, never written to"""
    links, gamma, beta = OC.peaked_state(seed, n, k)
    adj = OC.adjacency(n, links)
    out, g, b = [], gamma, beta
    for _ in range(5):
        g, b, rounds, bad = OC.sweep(g, b, adj, (), 1.0 / k)
        out.append((g, b, rounds, bad))
    for a in (links, gamma, beta) + tuple(x for o in out for x in o):
        a.setflags(write=False)
    return links, gamma, beta, out


def _compare(dev, g, b, rounds_list):
    """the device state against (g, b) and its counters against the rounds of the sweeps of the last call"""
    dg, db = dev.state()
    np.testing.assert_allclose(dg, g, rtol=RTOL)
    np.testing.assert_allclose(db, b, rtol=RTOL)
    pairs, total, most, bad_norm, bad_beta = dev.stats()
    print("pairs %d rounds %d max %d | reference %d %d %d | max rel gamma %.3g beta %.3g" % (
        pairs, total, most, sum(len(r) for r in rounds_list), sum(int(r.sum()) for r in rounds_list),
        max(int(r.max()) for r in rounds_list), np.abs(dg / g - 1).max(), np.abs(db / b - 1).max()))
    assert pairs == sum(len(r) for r in rounds_list)
    assert total == sum(int(r.sum()) for r in rounds_list)
    assert most == max(int(r.max()) for r in rounds_list)
    assert bad_norm == 0 and bad_beta == 0


def test_the_matrix_covers_both_edges_of_every_instantiation():
    by = {}
    for k in range(2, _svils.ORIG_MAX_K + 1):
        by.setdefault(_svils.orig_variant(k), []).append(k)
    assert len(by) == 4
    for ks in by.values():
        assert ks[0] in KS and ks[-1] in KS, ks
    assert tuple(c[0] for c in PEAKED) == KS


@pytest.mark.parametrize("k,n,seed", PEAKED)
def test_peaked_states_one_sweep_and_five(k, n, seed):
    """pairs leave at many different rounds inside one tile, some only at the cap; one sweep, then five in one call"""
    links, gamma, beta, ref = _peaked_reference(k, n, seed)
    OC.check_conditions(ref[0][2], ref[0][3], ref[0][1])
    for g, b, rounds, bad in ref:
        assert not bad.any() and np.all((b > 0) & (b < 1))
    one = _device(n, k, links, (), gamma, beta)
    one.sweep(1)
    _compare(one, ref[0][0], ref[0][1], [ref[0][2]])
    five = _device(n, k, links, (), gamma, beta)
    five.sweep(5)
    _compare(five, ref[4][0], ref[4][1], [r[2] for r in ref])
    # every visited pair adds one unit of mass to each of its two sides
    assert abs((five.state()[0] - 1.0 / k).sum() - 2 * n * (n - 1)) < 1e-7


@pytest.mark.parametrize("k", KS)
def test_three_nodes(k):
    """fewer pairs than one tile: 6 ordered pairs, one link.  Five sweeps, or as many as the restatement keeps beta away from
    1 (6 pairs feed k * k blocks: at k >= 31 some block rate reaches 1 to the last bit within five sweeps, at k = 15 it
    comes within 1e-9 of it in the fifth)"""
    rs = np.random.RandomState(300 + k)
    links = np.array([[0, 1]], dtype=np.uint32)
    gamma, beta = rs.gamma(100.0, 0.01, size=(3, k)), OC.init_beta1(rs, k)
    adj = OC.adjacency(3, links)
    dev = _device(3, k, links, (), gamma, beta)
    g, b, rl = gamma, beta, []
    for _ in range(5):
        g2, b2, rounds, bad = OC.sweep(g, b, adj, (), 1.0 / k)
        if bad.any() or not np.all((b2 > 0) & (b2 < 1 - 1e-9)):
            break
        g, b = g2, b2
        rl.append(rounds)
    assert len(rl) >= (4 if k < 31 else 1)
    dev.sweep(len(rl))
    _compare(dev, g, b, rl)


def _edge_case(k, n=37):
    """n = 37: a partial last tile in every row (37 = 2 * 16 + 5).  Node 7 has no links, rows 20 .. 23 have none in their
    first tile (tiles without links beside tiles with them), and the skip list takes pairs at tile edges in ONE orientation"""
    links, gamma, beta = OC.peaked_state(400 + k, n, k)
    keep = (links != 7).all(1) & ~((links[:, 0] >= 20) & (links[:, 0] <= 23) & (links[:, 1] < 16)) \
        & ~((links[:, 1] >= 20) & (links[:, 1] <= 23) & (links[:, 0] < 16))
    links = np.ascontiguousarray(links[keep])
    skip = [(0, 15), (0, 16), (5, 31), (5, 32), (17, 0), (36, 35), (20, 36), (36, 0), (15, 16), (31, 32), (1, 0)]
    return n, links, skip, gamma, beta


@pytest.mark.parametrize("launch_rows", [0, 5])
@pytest.mark.parametrize("k", KS)
def test_tile_content_and_skips_at_tile_edges(k, launch_rows):
    """one launch for all rows, and launches of 5 rows (8 launches, the last of 2 rows)"""
    n, links, skip, gamma, beta = _edge_case(k)
    adj = OC.adjacency(n, links)
    assert adj[7].sum() == 0 and adj[20:24, :16].sum() == 0 and adj[20:24].sum() > 0
    assert all((b, a) not in skip for a, b in skip)
    dev = _device(n, k, links, skip, gamma, beta, launch_rows)
    g, b, rl = gamma, beta, []
    for _ in range(2):
        g, b, rounds, bad = OC.sweep(g, b, adj, skip, 1.0 / k)
        assert not bad.any() and np.all((b > 0) & (b < 1)) and len(rounds) == n * (n - 1) - len(skip)
        rl.append(rounds)
    dev.sweep(2)
    _compare(dev, g, b, rl)


def test_skipping_one_orientation_is_not_skipping_both():
    n, links, skip, gamma, beta = _edge_case(4)
    both = skip + [(b, a) for a, b in skip]
    one, two = _device(n, 4, links, skip, gamma, beta), _device(n, 4, links, both, gamma, beta)
    one.sweep(1)
    two.sweep(1)
    assert one.stats()[0] == two.stats()[0] + len(skip)
    assert not np.array_equal(one.state()[1], two.state()[1])


@pytest.mark.parametrize("case", [PEAKED[6], PEAKED[13]])
def test_runs_are_bitwise_reproducible(case):
    k, n, seed = case
    links, gamma, beta, _ = _peaked_reference(k, n, seed)
    a, b, c = (_device(n, k, links, (), gamma, beta) for _ in range(3))
    a.sweep(3)
    b.sweep(3)
    for _ in range(3):
        c.sweep(1)
    ga, ba = a.state()
    for other in (b, c):
        go, bo = other.state()
        assert np.array_equal(ga, go) and np.array_equal(ba, bo)


@pytest.mark.parametrize("case", [PEAKED[2], PEAKED[9]])
def test_pair_loglik(case):
    """the tolerance tests/test_gpu_batch.py holds svils_batch_pair_loglik to"""
    k, n, seed = case
    links, gamma, beta, ref = _peaked_reference(k, n, seed)
    dev = _device(n, k, links, (), gamma, beta)
    adj = OC.adjacency(n, links)
    rs = np.random.RandomState(seed)
    pairs = np.array([(a, b) for a, b in rs.randint(0, n, size=(200, 2)) if a != b] + [(1, 0), (0, 1), (n - 1, 0)])
    y = adj[pairs[:, 0], pairs[:, 1]].astype(np.uint8)
    np.testing.assert_allclose(dev.pair_loglik(pairs, y), OC.pair_loglik(gamma, beta, pairs, y), rtol=0, atol=1e-9)
    dev.sweep(1)
    np.testing.assert_allclose(dev.pair_loglik(pairs, 1 - y), OC.pair_loglik(ref[0][0], ref[0][1], pairs, 1 - y), rtol=0, atol=1e-9)
    assert dev.pair_loglik(np.zeros((0, 2)), np.zeros(0)).shape == (0,)


def test_pair_loglik_lists_regrow_and_go_with_the_graph():
    """tests/test_gpu_batch.py::test_pair_likelihood_lists_regrow_and_go_with_the_graph on this handle: 3 pairs, 50, 3, a new
    graph, 50 -- every result is, byte for byte, that of a fresh handle's first call"""
    k, n, seed = PEAKED[2]
    links, gamma, beta, _ = _peaked_reference(k, n, seed)
    adj = OC.adjacency(n, links)
    rs = np.random.RandomState(seed + 1)
    pairs = np.array([(a, b) for a, b in rs.randint(0, n, size=(80, 2)) if a != b][:50])
    y = adj[pairs[:, 0], pairs[:, 1]].astype(np.uint8)
    assert len(pairs) == 50 and 0 < y.sum() < 50
    ref = {m: _device(n, k, links, (), gamma, beta).pair_loglik(pairs[:m], y[:m]) for m in (3, 50)}
    assert ref[50][:3].tobytes() == ref[3].tobytes()
    dev = _device(n, k, links, (), gamma, beta)
    for m in (3, 50, 3):
        assert dev.pair_loglik(pairs[:m], y[:m]).tobytes() == ref[m].tobytes()
    dev.set_graph(links, ())
    assert dev.pair_loglik(pairs, y).tobytes() == ref[50].tobytes()
    dev.sweep(1)                                                              # the handle still sweeps: the second graph is whole
    assert dev.stats()[0] == n * (n - 1)


def test_a_block_that_saw_only_links_raises_the_flag():
    """a complete graph on 6 nodes, k = 3: num == tot bitwise, so every beta is exactly 1 after one sweep; the sweep behind
    it in the queue leaves the state alone, and the next call that waits names the cause"""
    n, k = 6, 3
    links = np.array([(a, b) for a in range(n) for b in range(a + 1, n)], dtype=np.uint32)
    rs = np.random.RandomState(63)
    gamma, beta = rs.gamma(100.0, 0.01, size=(n, k)), OC.init_beta1(rs, k)
    one, two = _device(n, k, links, (), gamma, beta), _device(n, k, links, (), gamma, beta)
    one.sweep(1)
    two.sweep(2)
    g1, b1 = one.state(check=False)
    g2, b2 = two.state(check=False)
    assert np.all(b1 == 1.0)
    g_ref = OC.sweep(gamma, beta, OC.adjacency(n, links), (), 1.0 / k)[0]
    np.testing.assert_allclose(g1, g_ref, rtol=RTOL)
    assert np.array_equal(g1, g2) and np.array_equal(b1, b2)
    assert one.stats()[4] == k * k and two.stats() == (n * (n - 1), one.stats()[1], one.stats()[2], 0, k * k)
    with pytest.raises(_svils.SvilsError) as ei:
        two.state()
    assert ei.value.code == ERR_UNSUPPORTED and "left (0, 1)" in str(ei.value)
    with pytest.raises(_svils.SvilsError) as ei:
        two.pair_loglik([(0, 1)], [1])
    assert ei.value.code == ERR_UNSUPPORTED
    two.set_state(gamma, beta)   # a new state lowers the flag
    assert np.array_equal(two.state()[0], gamma)


def test_argument_errors_leave_the_state_untouched():
    k, n, seed = PEAKED[2]
    links, gamma, beta, ref = _peaked_reference(k, n, seed)
    dev = _device(n, k, links, (), gamma, beta)
    L, h = _svils.load(), dev._h
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)

    def set_graph(lk, sk=()):
        lk, sk = u32(lk).reshape(-1, 2), u32(sk).reshape(-1, 2)
        return L.svils_orig_set_graph(h, lk.ctypes.data, len(lk), sk.ctypes.data, len(sk))

    assert set_graph([(3, 3)]) == ERR_ARG and set_graph([(4, 2)]) == ERR_ARG and set_graph([(0, n)]) == ERR_ARG
    assert set_graph([(0, 1), (0, 1)]) == ERR_ARG and b"repeated" in L.svils_last_error()
    assert set_graph([(0, 1)], [(2, 2)]) == ERR_ARG and set_graph([(0, 1)], [(n, 0)]) == ERR_ARG
    assert set_graph([(0, 1)], [(2, 1), (2, 1)]) == ERR_ARG and set_graph([(0, 1)], [(2, 1), (1, 2)]) == 0
    dev.set_graph(links)
    bad_g, bad_b = gamma.copy(), beta.copy()
    bad_g[5, 1] = -1.0
    bad_b[0, 0] = 1.0
    for g, b in ((bad_g, beta), (gamma, bad_b), (np.where(bad_g < 0, np.inf, gamma), beta), (gamma, np.where(bad_b == 1, 0.0, beta))):
        g, b = np.ascontiguousarray(g), np.ascontiguousarray(b)
        assert L.svils_orig_set_state(h, g.ctypes.data, b.ctypes.data) == ERR_ARG
    assert L.svils_orig_set_state(h, None, None) == ERR_ARG
    pr, yy, out = u32([(2, 2)]), np.zeros(1, dtype=np.uint8), np.zeros(1)
    assert L.svils_orig_pair_loglik(h, pr.ctypes.data, yy.ctypes.data, 1, out.ctypes.data) == ERR_ARG
    g0, b0 = dev.state()
    assert np.array_equal(g0, gamma) and np.array_equal(b0, beta)
    dev.sweep(1)
    _compare(dev, ref[0][0], ref[0][1], [ref[0][2]])
    ms = dev.timing()
    assert np.all(ms >= 0)
    fresh = _svils.Orig(n, k, 1.0 / k)
    assert L.svils_orig_sweep(fresh._h, 1) == ERR_ARG   # no graph, no state
    assert L.svils_orig_get_state(fresh._h, None, None) == ERR_ARG
    assert L.svils_orig_sweep(None, 1) == ERR_ARG and L.svils_orig_get_timing(None, None) == ERR_ARG


def test_engine_on_the_device_against_host_loops():
    """the same draws, the same skip list (held-out pairs in the drawn orientation alone), the same rows"""
    dev = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=True)
    host = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    assert np.array_equal(dev.heldout, host.heldout) and np.array_equal(dev.validation, host.validation)
    assert np.array_equal(dev.gamma, host.gamma) and np.array_equal(dev.beta, host.beta)
    for _ in range(3):
        dev.sweep()
        host.sweep()
        dev.report()
        host.report()
    np.testing.assert_allclose(dev.gamma, host.gamma, rtol=RTOL)
    np.testing.assert_allclose(dev.beta, host.beta, rtol=RTOL)
    assert dev.rows.shape == host.rows.shape == (8, 8)
    np.testing.assert_allclose(dev.rows, host.rows, rtol=RTOL)


def test_cli_on_the_device_against_host_loops(tmp_path):
    out = {}
    for which, extra in (("device", []), ("host", ["-host-loops"])):
        d = tmp_path / which
        d.mkdir()
        r = subprocess.run([SVINET, "-file", ASSORT, "-n", "75", "-k", "4", "-orig", "-max-iterations", "3", "-heldout-ratio", "0.1"] + extra,
                           capture_output=True, text=True, timeout=120, cwd=str(d))
        assert r.returncode == 0, r.stderr
        out[which] = d / "n75-k4-mmsb-U"
    for f in ("heldout-edges.txt", "validation-edges.txt", "groups.txt", "communities.txt", "summary.txt"):
        assert (out["device"] / f).read_text() == (out["host"] / f).read_text(), f
    for f in ("heldout.txt", "validation.txt"):   # equal as text apart from the duration column
        rows = [[l.split("\t") for l in (out[w] / f).read_text().splitlines()] for w in ("device", "host")]
        assert len(rows[0]) == 4 and [r[:1] + r[2:] for r in rows[0]] == [r[:1] + r[2:] for r in rows[1]], f
    for f in ("gamma.txt", "beta.txt"):
        np.testing.assert_allclose(np.loadtxt(out["device"] / f), np.loadtxt(out["host"] / f), rtol=RTOL)
