"""-m gpu: the lower bound of -orig on the device (svils_orig_elbo, csrc/svils_orig_elbo.hip).

The reference is tests/orig_elbo_cases.py, a numpy restatement on scipy's gammaln and digamma.  Every state is first held to
its check_conditions -- every pair term and every node term negative, the magnitudes of the parts below 50 |P| -- so that no
sum cancels and rtol 1e-9 (the project's figure for -logl, section 4k) on total, P and N means something: the device sums
at most n (n - 1) K^2 < 4e7 products in fp64, a relative rounding error below 1e-12 of the magnitudes, 5e-11 of |P| at the
ratio of 50.  Pairs and the round total are exact (see tests/test_gpu_orig.py on why that does not rest on luck)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import orig_cases as OC
import orig_elbo_cases as EC
from conftest import GOLDEN
from svinet_amd import _svils
from svinet_amd.host_api import OrigEngine
from test_gpu_orig import KS, PEAKED, _device, _edge_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
ASSORT = os.path.join(GOLDEN, "graphs", "assort-75-4.txt")
RTOL = 1e-9
ERR_ARG, ERR_UNSUPPORTED = -1, -4


def three_nodes(k):
    """the state of tests/test_gpu_orig.py::test_three_nodes: 6 ordered pairs, one link"""
    rs = np.random.RandomState(300 + k)
    return 3, np.array([[0, 1]], dtype=np.uint32), [], rs.gamma(100.0, 0.01, size=(3, k)), OC.init_beta1(rs, k)


def underflow_state():
    """n = 20, K = 4: gamma = 1e-3 in column 0 of the even nodes and column 3 of nodes 1, 5, 9, so Elogpi is about -1000
    there and exp() of it is exactly 0 -- entries of phi1 and phi2 that are exact zeros"""
    links, gamma, beta = OC.plain_state(77, 20, 4)
    gamma = gamma.copy()
    gamma[0::2, 0] = 1e-3
    gamma[1:10:4, 3] = 1e-3
    return 20, links, [], gamma, beta


@functools.lru_cache(maxsize=None)
def _reference(kind, k):
    """(n, links, skip, gamma, beta, restated bound): computed once, shared, never written to"""
    if kind == "three":
        n, links, skip, gamma, beta = three_nodes(k)
    elif kind == "edge":
        n, links, skip, gamma, beta = _edge_case(k)
    elif kind == "underflow":
        n, links, skip, gamma, beta = underflow_state()
    else:
        _, n, seed = PEAKED[KS.index(k)]
        links, gamma, beta = OC.peaked_state(seed, n, k)
        skip = []
    r = EC.elbo(gamma, beta, OC.adjacency(n, links), skip, 1.0 / k)
    EC.check_conditions(r, beta, peaked=kind == "peaked")
    for a in (links, gamma, beta, r["pair"], r["node"], r["rounds"]):
        a.setflags(write=False)
    return n, links, tuple(skip), gamma, beta, r


def _against(dev, r):
    got = dev.elbo()
    pairs, rounds, most, bad = dev.elbo_stats()
    want = (r["total"], r["P"], r["N"])
    print("device %r | restatement %r | rel %s | pairs %d rounds %d" % (got, want, [abs(a / b - 1) for a, b in zip(got, want)], pairs, rounds))
    assert np.all(np.isfinite(got))
    np.testing.assert_allclose(got, want, rtol=RTOL)
    assert got[0] == got[1] + got[2]
    assert (pairs, rounds, most, bad) == (len(r["pair"]), int(r["rounds"].sum()), int(r["rounds"].max()), 0)
    return got


@pytest.mark.parametrize("kind", ["three", "edge", "peaked"])
@pytest.mark.parametrize("k", KS)
def test_against_the_restatement(k, kind):
    """every instantiation at both edges: n = 3 (fewer pairs than a tile), n = 37 (partial tiles, a node without links, skips
    in one orientation at the tile edges 15 / 16), and the peaked states n = 75 .. 96 (exits at many rounds inside a tile)"""
    n, links, skip, gamma, beta, r = _reference(kind, k)
    dev = _device(n, k, links, skip, gamma, beta)
    _against(dev, r)
    g, b = dev.state()
    assert np.array_equal(g, gamma) and np.array_equal(b, beta)   # the pass leaves the state alone
    assert dev.stats() == (0, 0, 0, 0, 0)                         # ... and the sweep's counters
    assert np.all(dev.elbo_timing() >= 0)


@pytest.mark.parametrize("k", [5, 32, 49, 64])
def test_bitwise_equal_across_launch_cuts_handles_and_calls(k):
    """n = 37: one launch, 8 launches of 5 rows (the last of 2), 37 launches of one row; a second handle; a second call"""
    n, links, skip, gamma, beta, r = _reference("edge", k)
    one = _device(n, k, links, skip, gamma, beta)
    first = one.elbo()
    assert one.elbo() == first
    for rows in (5, 1):
        cut = _device(n, k, links, skip, gamma, beta, rows)
        assert cut.elbo() == first and cut.elbo_stats() == one.elbo_stats()
    assert _device(n, k, links, skip, gamma, beta).elbo() == first


@pytest.mark.parametrize("k", [4, 16, 33, 64])
def test_a_pass_between_two_sweeps_changes_nothing(k):
    """sweep - elbo - sweep against sweep - sweep: gamma, beta, the counters and the link queries bit for bit"""
    n, links, skip, gamma, beta, _ = _reference("peaked", k)
    a, b = _device(n, k, links, skip, gamma, beta), _device(n, k, links, skip, gamma, beta)
    pairs = np.array([(0, 1), (5, 3), (n - 1, 0)])
    a.sweep(1)
    b.sweep(1)
    pa = a.link_prob(pairs)          # the cache of pi is built before the pass ...
    mid = a.elbo()
    assert a.stats() == b.stats()    # the pass has a counter block of its own
    assert np.array_equal(a.link_prob(pairs), pa) and np.array_equal(b.link_prob(pairs), pa)   # ... and still stands after it
    a.sweep(1)
    b.sweep(1)
    (ga, ba), (gb, bb) = a.state(), b.state()
    assert np.array_equal(ga, gb) and np.array_equal(ba, bb) and a.stats() == b.stats()
    assert np.array_equal(a.link_prob(pairs), b.link_prob(pairs))
    assert a.elbo() == b.elbo() and a.elbo()[0] > mid[0]   # the bound rises from sweep to sweep on these states


def test_exact_zeros_in_phi_add_nothing():
    n, links, skip, gamma, beta, r = _reference("underflow", 4)
    assert (r["phi1"] == 0).sum() > 50 and (r["phi2"] == 0).sum() > 50
    _against(_device(n, 4, links, skip, gamma, beta), r)


def test_the_degenerate_flag_is_an_error_and_the_state_stays():
    """tests/test_gpu_orig.py::test_a_block_that_saw_only_links_raises_the_flag: a complete graph, every beta exactly 1"""
    n, k = 6, 3
    links = np.array([(a, b) for a in range(n) for b in range(a + 1, n)], dtype=np.uint32)
    rs = np.random.RandomState(63)
    gamma, beta = rs.gamma(100.0, 0.01, size=(n, k)), OC.init_beta1(rs, k)
    dev = _device(n, k, links, (), gamma, beta)
    before = dev.elbo()
    assert np.all(np.isfinite(before))
    dev.sweep(1)
    out = np.full(3, 7.0)
    assert _svils.load().svils_orig_elbo(dev._h, out.ctypes.data) == ERR_UNSUPPORTED
    assert b"left (0, 1)" in _svils.load().svils_last_error() and out.tolist() == [7.0, 7.0, 7.0]
    g1, b1 = dev.state(check=False)
    with pytest.raises(_svils.SvilsError):
        dev.elbo()
    g2, b2 = dev.state(check=False)
    assert np.array_equal(g1, g2) and np.array_equal(b1, b2)
    dev.set_state(gamma, beta)   # a new state lowers the flag
    assert dev.elbo() == before


def test_argument_errors():
    k, n, seed = PEAKED[2]
    links, gamma, beta = OC.peaked_state(seed, n, k)
    L = _svils.load()
    out = np.zeros(3)
    fresh = _svils.Orig(n, k, 1.0 / k)
    assert L.svils_orig_elbo(fresh._h, out.ctypes.data) == ERR_ARG      # no graph, no state
    fresh.set_graph(links)
    assert L.svils_orig_elbo(fresh._h, out.ctypes.data) == ERR_ARG      # no state
    assert fresh.elbo_stats() == (0, 0, 0, 0) and np.all(fresh.elbo_timing() == -1)
    fresh.set_state(gamma, beta)
    assert L.svils_orig_elbo(fresh._h, None) == ERR_ARG
    assert L.svils_orig_elbo(None, out.ctypes.data) == ERR_ARG and L.svils_orig_get_elbo_timing(fresh._h, None) == ERR_ARG
    assert L.svils_orig_get_elbo_stats(None, None, None, None, None) == ERR_ARG
    assert L.svils_orig_elbo(fresh._h, out.ctypes.data) == 0 and out[0] == out[1] + out[2]
    assert L.svils_orig_get_elbo_stats(fresh._h, None, None, None, None) == 0


def test_engine_on_the_device_against_host_loops():
    dev = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=True, logl=True)
    host = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False, logl=True)
    for _ in range(3):
        dev.sweep()
        host.sweep()
        dev.report()
        host.report()
    assert dev.logl_rows.shape == host.logl_rows.shape == (4, 2)
    np.testing.assert_allclose(dev.logl_rows, host.logl_rows, rtol=RTOL)
    np.testing.assert_allclose(dev.elbo(), host.elbo(), rtol=RTOL)
    assert dev.elbo_stats == host.elbo_stats


def test_cli_on_the_device_against_host_loops(tmp_path):
    rows = {}
    for which, extra in (("device", []), ("host", ["-host-loops"])):
        d = tmp_path / which
        d.mkdir()
        r = subprocess.run([SVINET, "-file", ASSORT, "-n", "75", "-k", "4", "-orig", "-max-iterations", "3", "-heldout-ratio", "0.1",
                            "-logl", "-no-stop"] + extra, capture_output=True, text=True, timeout=120, cwd=str(d))
        assert r.returncode == 0, r.stderr
        rows[which] = [l.split("\t") for l in (d / "n75-k4-mmsb-U" / "logl.txt").read_text().splitlines()]
    assert [x[0] for x in rows["device"]] == ["0", "1", "2", "3"] == [x[0] for x in rows["host"]]
    # (five decimals of a value near -3e4: rtol 1e-9 is three units of the last printed digit)
    np.testing.assert_allclose([float(x[2]) for x in rows["device"]], [float(x[2]) for x in rows["host"]], rtol=RTOL)


def test_cli_on_the_device_ends_by_itself(tmp_path):
    r = subprocess.run([SVINET, "-file", ASSORT, "-n", "75", "-k", "4", "-orig", "-heldout-ratio", "0.1", "-logl", "-rfreq", "1"],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    d = tmp_path / "n75-k4-mmsb-U"
    assert (d / "max.txt").exists() or (d / "done.txt").exists()
    assert len((d / "logl.txt").read_text().splitlines()) > 10
    assert np.loadtxt(d / "beta.txt").shape == (4, 4) and np.loadtxt(d / "gamma.txt").shape == (75, 6)
