"""-m gpu: the K x K kind of svils_ppc_* (host_api.PPC.set_params_orig) and `svinet -ppc-orig` against the numpy restatement
tools/restate_ppc_orig.py and closed forms.  The draw is a definition, so link lists, degrees,
triangles, blocks and block sizes are asked to be EQUAL; blogpe, transitivity and the mean local clustering within rtol
1e-12 (one rounding of a sum against math.fsum, and the last bit of log: section 4l's tolerance, for its reason)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import ppc_cases as PC
import ppc_orig_cases as OC
from ppc_cases import R
from ppc_orig_cases import RO

sys.path.insert(0, os.path.join(ROOT, "tools"))
import restate_findk  # noqa: E402
import restate_hops as H  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
RTOL = 1e-12
COUNTS = ("ones", "max_deg", "argmax_deg", "triangles", "wedges")


def _ppc(n, k, **kw):
    from svinet_amd.host_api import PPC
    return PPC(n, k, **kw)


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.allclose(a, b, rtol=RTOL, atol=0.0, equal_nan=True)


def _check_stats(got, want):
    assert np.array_equal(got["links"].astype(np.int64), want["links"])
    for name in ("deg", "tri", "colour"):
        assert np.array_equal(np.asarray(got[name]).astype(np.int64), np.asarray(want[name]).astype(np.int64)), name
    assert np.array_equal(got["join"], want["join"])
    for name in COUNTS:
        assert got[name] == want[name], name
    assert np.array_equal(got["block_size"].astype(np.int64), want["bsize"])
    assert _close(got["block_logpe"], want["blogpe"]), (got["block_logpe"], want["blogpe"])
    for name in ("transitivity", "clustering", "offdiag_share"):
        assert _close(got[name], want[name]), (name, got[name], want[name])
    assert "size" not in got and "logpe" not in got


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def _same(a, b):
    for name in ("links", "deg", "tri", "colour", "join", "block_size"):
        assert np.array_equal(a[name], b[name]), name
    for name in COUNTS:
        assert a[name] == b[name], name
    for name in ("block_logpe", "transitivity", "clustering", "offdiag_share"):
        assert np.array_equal(_bits(a[name]), _bits(b[name])), name


@pytest.mark.parametrize("K", OC.EQUALITY_K)
@pytest.mark.parametrize("n", OC.EQUALITY_N)
def test_draw_and_statistics_equal_the_restatement(n, K):
    pi, B = OC.random_model(n, K, 1)
    ppc = _ppc(n, K)
    ppc.set_params_orig(pi, B)
    for seed, r in PC.EQUALITY_DRAWS:
        links = ppc.draw(seed=seed, r=r)
        want = RO.draw(pi, B, seed, r)
        assert np.array_equal(links.astype(np.int64), want), (seed, r)
        _check_stats(ppc.stats(), RO.stats(want, pi, B))
    ppc.close()


@pytest.mark.parametrize("n,K", [(65, 5), (130, 20), (63, 2)])
def test_exact_sums_decide_as_the_restatement(n, K):
    """one-hot / halves / quarters and rates in {0, 0.5, 1}: every sum is exact in any order, ratios of exactly 0.5 among them"""
    pi, B = OC.power_of_two_model(n, K, 3)
    ppc = _ppc(n, K)
    ppc.set_params_orig(pi, B)
    for seed, r in PC.EQUALITY_DRAWS:
        want = RO.draw(pi, B, seed, r)
        assert np.array_equal(ppc.draw(seed=seed, r=r).astype(np.int64), want)
        s = RO.stats(want, pi, B)
        assert np.any(s["ratio"] == 0.5)
        _check_stats(ppc.stats(), s)
    ppc.close()


@pytest.mark.parametrize("K", [5, 20])
def test_diagonal_rates_are_the_assortative_draw(K):
    n = 130
    pi, beta = PC.random_model(n, K, 1)
    ppc = _ppc(n, K)
    for seed, r in PC.EQUALITY_DRAWS:
        ppc.set_params(pi, beta)
        links = ppc.draw(seed=seed, r=r)
        a = ppc.stats()
        ppc.set_params_orig(pi, np.diag(beta))
        assert np.array_equal(ppc.draw(seed=seed, r=r), links) and len(links) > 100
        o = ppc.stats()
        assert np.array_equal(o["colour"], a["colour"] * (K + 1)) and np.array_equal(o["join"], a["join"])
        assert np.array_equal(np.diag(o["block_size"]), a["size"]) and o["block_size"].sum() == a["size"].sum()
        assert np.array_equal(_bits(np.diag(o["block_logpe"])), _bits(a["logpe"]))
        assert o["offdiag_share"] == 0.0
        for name in COUNTS:
            assert o[name] == a[name], name
    ppc.close()


def test_pairs_on_the_edge_are_rechecked():
    pi, B, want_pairs = OC.on_the_edge_model()
    ppc = _ppc(OC.EDGE_N, OC.EDGE_K)
    links = ppc.draw(pi, B=B, seed=OC.EDGE_SEED, r=OC.EDGE_R)
    want = RO.draw(pi, B, OC.EDGE_SEED, OC.EDGE_R)
    assert np.array_equal(links.astype(np.int64), want)
    have = set(map(tuple, links.tolist()))
    for pq, y in want_pairs.items():
        assert (pq in have) == y, pq
    rechecked = ppc.draw_counts()[1]
    print("rechecked pairs:", rechecked)
    assert 3 <= rechecked <= 0.01 * OC.EDGE_N * (OC.EDGE_N - 1) / 2
    _check_stats(ppc.stats(), RO.stats(want, pi, B))
    ppc.close()


def test_closed_forms():
    n = 130
    ppc = _ppc(n, 2)
    # the smaller id indexes the rows of B: even p < odd q alone
    pi, B = OC.parity_model(n, OC.ORIENTED)
    links = ppc.draw(pi, B=B, seed=4, r=1)
    assert np.array_equal(links.astype(np.int64), OC.oriented_pairs(n))
    s = ppc.stats()
    assert np.all(s["colour"] == 1) and np.all(s["join"]) and s["block_size"].tolist() == [[0, len(links)], [0, 0]]
    assert s["offdiag_share"] == 1.0 and not s["block_logpe"].any()
    # complete bipartite, 65 x 65
    pi, B = OC.parity_model(n, OC.BIPARTITE)
    links = ppc.draw(pi, B=B, seed=4, r=1)
    assert np.array_equal(links.astype(np.int64), OC.bipartite_pairs(n)) and len(links) == 4225
    s = ppc.stats()
    assert s["ones"] == 4225 and s["triangles"] == 0 and s["transitivity"] == 0.0 and s["clustering"] == 0.0 and not s["tri"].any()
    assert np.all(s["deg"] == 65) and s["wedges"] == 130 * (65 * 64 // 2)
    assert s["offdiag_share"] == 1.0 and s["block_size"].tolist() == [[0, 65 * 66 // 2], [65 * 64 // 2, 0]]
    assert np.array_equal(s["colour"], np.where(links[:, 0] % 2 == 0, 1, 2)) and not s["block_logpe"].any()
    h = ppc.hops()
    assert h["diameter"] == 2 and h["components"] == 1 and h["largest"] == n and h["isolated"] == 0
    assert h["D"].tolist() == [n, 2 * 4225, n * (n - 1) - 2 * 4225]
    ppc.close()


def test_replicates_average_to_the_model():
    b = OC.expectation_bounds()
    ppc = _ppc(OC.EXP_N, OC.EXP_K)
    ppc.set_params_orig(b[0], b[1])
    ones, degs = [], []
    for r in range(OC.EXP_R):
        links = ppc.draw(seed=OC.EXP_SEED, r=r)
        ones.append(len(links))
        degs.append(PC.degrees(links, OC.EXP_N))
    PC.check_expectation(ones, degs, b)
    ppc.close()


def test_a_replicate_does_not_depend_on_the_launches_or_the_order():
    n, K, seed, r = 130, 20, 77, 3
    pi, B = OC.random_model(n, K, 8)
    _, beta = PC.random_model(n, K, 8)
    a = _ppc(n, K)
    a.draw(pi, B=B, seed=seed, r=r)
    first = a.stats()
    assert len(first["links"]) > 100 and first["triangles"] > 0
    for batch in (1, 3, 0):
        a.set_tile_batch(batch)
        a.draw(seed=seed, r=r)
        _same(a.stats(), first)
    b = _ppc(n, K)   # a fresh handle, with another list and another replicate in between
    b.set_params_orig(pi, B)
    b.observe(np.array([[0, 1], [5, 129], [64, 65]]))
    assert np.array_equal(b.links(), [[0, 1], [5, 129], [64, 65]])
    b.draw(seed=seed, r=r + 1)
    b.observe(first["links"][::-1])
    _same(b.stats(), first)
    b.draw(seed=seed, r=r)
    _same(b.stats(), first)
    assert first["rechecked"] == b.draw_counts()[1]
    # the other kind and back: the list stays, the statistics are the current kind's
    b.set_params(pi, beta)
    assert np.array_equal(b.links(), first["links"])
    other = b.stats()
    want = R.stats(first["links"].astype(np.int64), pi, beta)
    assert np.array_equal(other["colour"], want["colour"]) and np.array_equal(other["size"], want["size"]) and "block_size" not in other
    b.set_params_orig(pi, B)
    assert np.array_equal(b.links(), first["links"])
    _same(b.stats(), first)
    b.draw(pi, beta, seed, r)
    assert np.array_equal(b.links().astype(np.int64), R.draw(pi, beta, seed, r))
    b.draw(pi, B=B, seed=seed, r=r)
    _same(b.stats(), first)
    a.close()
    b.close()


def test_a_list_too_small_keeps_the_state():
    from svinet_amd._svils import SvilsError
    n, K = 65, 5
    pi, B = OC.random_model(n, K, 1)
    counts = [len(RO.draw(pi, B, 9, r)) for r in range(6)]
    small, big = int(np.argmin(counts)), int(np.argmax(counts))
    assert counts[small] < counts[big]
    ppc = _ppc(n, K, max_links=counts[small])
    ppc.set_params_orig(pi, B)
    ppc.draw(seed=9, r=small)
    before = ppc.stats()
    with pytest.raises(SvilsError) as ei:
        ppc.draw(seed=9, r=big)
    assert ei.value.code == -3 and str(counts[big]) in str(ei.value)
    assert ppc.draw_counts()[0] == counts[big]
    assert np.array_equal(ppc.links(), before["links"])
    _same(ppc.stats(), before)
    ppc.close()


def test_argument_refusals():
    from svinet_amd import _svils
    L = _svils.load()
    n = 9
    big = _ppc(n, 65)
    pi65 = OC.one_hot(np.arange(n), 65)
    assert L.svils_ppc_set_params_orig(big._h, pi65.ctypes.data, np.zeros((65, 65)).ctypes.data) == -4
    assert b"SVILS_ORIG_MAX_K" in L.svils_last_error()
    big.set_params(pi65, np.full(65, 0.5))          # the assortative kind holds k = 65
    big.close()
    one = _ppc(n, 1)
    assert L.svils_ppc_set_params_orig(one._h, np.ones((n, 1)).ctypes.data, np.ones((1, 1)).ctypes.data) == -4
    one.close()
    K = 3
    pi = OC.one_hot(np.arange(n) % K, K)
    ppc = _ppc(n, K)
    for v in (1.0 + 2.0 ** -52, -0.1, np.nan, np.inf):
        B = np.full((K, K), 0.5)
        B[1, 2] = v
        assert L.svils_ppc_set_params_orig(ppc._h, pi.ctypes.data, B.ctypes.data) == -1 and b"B[1][2]" in L.svils_last_error(), v
    bad = pi.copy()
    bad[4] *= 0.5
    assert L.svils_ppc_set_params_orig(ppc._h, bad.ctypes.data, np.full((K, K), 0.5).ctypes.data) == -1 and b"row 4" in L.svils_last_error()
    assert L.svils_ppc_set_params_orig(ppc._h, None, None) == -1
    assert L.svils_ppc_draw(ppc._h, 1, 2) == -1     # no refused call made the kind current
    size, val = np.zeros(K * K, np.uint64), np.zeros(K * K)
    ppc.draw(pi, B=np.ones((K, K)), seed=1, r=2)
    assert L.svils_ppc_get_blocks(ppc._h, size.ctypes.data, val.ctypes.data) == -1          # before svils_ppc_stats
    ppc.stats()
    assert L.svils_ppc_get_blocks(ppc._h, size.ctypes.data, val.ctypes.data) == 0 and size.sum() == n * (n - 1) // 2
    assert L.svils_ppc_get_communities(ppc._h, size.ctypes.data, val.ctypes.data) == -1 and b"svils_ppc_get_blocks" in L.svils_last_error()
    ppc.set_params(pi, np.ones(K))
    ppc.stats()
    assert L.svils_ppc_get_communities(ppc._h, size.ctypes.data, val.ctypes.data) == 0
    assert L.svils_ppc_get_blocks(ppc._h, size.ctypes.data, val.ctypes.data) == -1 and b"svils_ppc_get_communities" in L.svils_last_error()
    ppc.close()


# ---- the command line end to end ----

SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")


def _cli(args, cwd):
    r = subprocess.run([SVINET] + [str(a) for a in args], cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r


def _files_under(d):
    out = {}
    for base, _, files in os.walk(str(d)):
        for f in files:
            out[os.path.relpath(os.path.join(base, f), str(d))] = open(os.path.join(base, f)).read()
    return out


def _observed():
    links, seq2id = restate_findk.read_graph(OC.GRAPH, OC.CLI_N)
    return np.asarray(links, np.int64).reshape(-1, 2), len(seq2id)


def _hop_texts(links, n, gamma, B, draws, seed, mean):
    return H.hops_texts(H.all_of(links, n), [H.all_of(l, n) for _, l in RO.replicates(gamma, B, draws, seed, mean)])


@pytest.mark.parametrize("mean,hops", [(True, False), (False, False), (False, True)])
def test_cli_files_equal_the_restatement(tmp_path, mean, hops):
    shutil.copy(os.path.join(GOLDEN, "ref_assort_batch", "gamma.txt"), str(tmp_path))
    B = OC.cli_rates()
    (tmp_path / "beta.txt").write_text(OC.beta_text(B))
    links, n = _observed()
    gamma = OC.read_gamma(str(tmp_path / "gamma.txt"))
    _cli(["-file", OC.GRAPH, "-n", OC.CLI_N, "-k", OC.CLI_K, "-ppc-orig", "-ppc-draws", 5, "-seed", 17, "-ppc-save", 2] +
         (["-ppc-mean"] if mean else []) + (["-ppc-hops"] if hops else []), tmp_path)
    want = RO.ppc_orig_texts(links, gamma, B, 5, 17, mean, save=2)
    if hops:
        want.update(_hop_texts(links, n, gamma, B, 5, 17, mean))
    got = _files_under(tmp_path)
    assert set(got) == set(want) | {"gamma.txt", "beta.txt"}, sorted(got)
    for name, text in want.items():
        assert got[name] == text, name
    assert len(got["ppc/rep.txt"].splitlines()) == 5 and len(got["ppc/summary.txt"].splitlines()) == 8
    assert len(got["ppc/block_size.txt"].splitlines()) == OC.CLI_K ** 2 and got["ppc/summary.txt"].splitlines()[7].startswith("offdiag_share\t")
    assert len(got["ppc/0/network.dat"].splitlines()) > 100


def test_cli_checks_a_real_fit(tmp_path):
    """`svinet -orig` in one process, `svinet -ppc-orig` in its output directory in another: the files are the restatement's,
    computed from the gamma.txt and beta.txt the fit wrote"""
    _cli(["-file", OC.GRAPH, "-n", OC.CLI_N, "-k", OC.CLI_K, "-orig", "-max-iterations", 2, "-seed", 3], tmp_path)
    fit, = [d for d in tmp_path.iterdir() if d.is_dir()]        # n75-k4-mmsb-seed3-U
    before = set(_files_under(fit))
    assert {"gamma.txt", "beta.txt"} <= before
    _cli(["-file", OC.GRAPH, "-n", OC.CLI_N, "-k", OC.CLI_K, "-ppc-orig", "-ppc-draws", 3, "-seed", 3], fit)
    links, _ = _observed()
    want = RO.ppc_orig_texts(links, OC.read_gamma(str(fit / "gamma.txt")), OC.read_rates(str(fit / "beta.txt")), 3, 3, False)
    got = _files_under(fit)
    assert set(got) == before | set(want), sorted(set(got) - before)
    for name, text in want.items():
        assert got[name] == text, name
