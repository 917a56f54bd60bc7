"""-m gpu: svils_ppc_* (host_api.PPC) and `svinet -ppc` / `-gen` against the numpy restatement tools/restate_ppc.py and closed forms.  The draw is a
definition, so link lists, degrees, triangles, colours and community sizes are asked to be EQUAL;
logpe, transitivity and the mean local clustering within rtol 1e-12 (one rounding of a sum against math.fsum, and the
last bit of log)."""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import ppc_cases as PC
from ppc_cases import R

sys.path.insert(0, os.path.join(ROOT, "tools"))
import restate_findk  # noqa: E402
import restate_gml  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
RTOL = 1e-12


def _ppc(n, k, **kw):
    from svinet_amd.host_api import PPC
    return PPC(n, k, **kw)


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.allclose(a, b, rtol=RTOL, atol=0.0, equal_nan=True)


def _check_stats(got, want):
    assert np.array_equal(got["links"].astype(np.int64), want["links"])
    for name in ("deg", "tri", "colour", "size"):
        assert np.array_equal(np.asarray(got[name]).astype(np.int64), np.asarray(want[name]).astype(np.int64)), name
    assert np.array_equal(got["join"], want["join"])
    for name in ("ones", "max_deg", "argmax_deg", "triangles", "wedges"):
        assert got[name] == want[name], name
    for name in ("logpe", "transitivity", "clustering"):
        assert _close(got[name], want[name]), (name, got[name], want[name])


def _same(a, b):
    for name in ("links", "deg", "tri", "colour", "join", "size"):
        assert np.array_equal(a[name], b[name]), name
    for name in ("ones", "max_deg", "argmax_deg", "triangles", "wedges"):
        assert a[name] == b[name], name
    for name in ("logpe", "transitivity", "clustering"):
        assert np.array_equal(np.asarray(a[name], np.float64).view(np.int64), np.asarray(b[name], np.float64).view(np.int64)), name


@pytest.mark.parametrize("K", PC.EQUALITY_K)
@pytest.mark.parametrize("n", PC.EQUALITY_N)
def test_draw_and_statistics_equal_the_restatement(n, K):
    pi, beta = PC.random_model(n, K, 1)
    ppc = _ppc(n, K)
    ppc.set_params(pi, beta)
    for seed, r in PC.EQUALITY_DRAWS:
        links = ppc.draw(seed=seed, r=r)
        want = R.draw(pi, beta, seed, r)
        assert np.array_equal(links.astype(np.int64), want), (seed, r)
        _check_stats(ppc.stats(), R.stats(want, pi, beta))
    ppc.close()


@pytest.mark.parametrize("n,K", [(65, 5), (130, 20), (63, 2)])
def test_exact_sums_decide_as_the_restatement(n, K):
    """one-hot / halves / quarters and beta in {0, 0.5, 1}: tile sums equal to the ascending sum, or a rounding away"""
    pi, beta = PC.power_of_two_model(n, K, 3)
    ppc = _ppc(n, K)
    ppc.set_params(pi, beta)
    for seed, r in PC.EQUALITY_DRAWS:
        want = R.draw(pi, beta, seed, r)
        assert np.array_equal(ppc.draw(seed=seed, r=r).astype(np.int64), want)
        _check_stats(ppc.stats(), R.stats(want, pi, beta))
    ppc.close()


def test_pairs_on_the_edge_are_rechecked():
    pi, beta, want_pairs = PC.on_the_edge_model()
    ppc = _ppc(PC.EDGE_N, PC.EDGE_K)
    links = ppc.draw(pi, beta, PC.EDGE_SEED, PC.EDGE_R)
    want = R.draw(pi, beta, PC.EDGE_SEED, PC.EDGE_R)
    assert np.array_equal(links.astype(np.int64), want)
    have = set(map(tuple, links.tolist()))
    for pq, y in want_pairs.items():
        assert (pq in have) == y, pq
    rechecked = ppc.draw_counts()[1]
    print("rechecked pairs:", rechecked)
    assert 3 <= rechecked <= 0.01 * PC.EDGE_N * (PC.EDGE_N - 1) / 2
    ppc.close()


def test_cliques_in_closed_form():
    n = sum(PC.BLOCKS)
    ppc = _ppc(n, len(PC.BLOCKS))
    ppc.draw(*PC.block_model(1.0), seed=4, r=1)
    s = ppc.stats()
    m = np.repeat(PC.BLOCKS, PC.BLOCKS)
    assert s["ones"] == sum(b * (b - 1) // 2 for b in PC.BLOCKS) == len(s["links"])
    assert np.array_equal(s["deg"], m - 1)
    assert np.array_equal(s["tri"], (m - 1) * (m - 2) // 2)
    assert s["triangles"] == sum(math.comb(b, 3) for b in PC.BLOCKS)
    assert s["transitivity"] == 1.0 and s["clustering"] == 1.0
    assert s["max_deg"] == 37 and s["argmax_deg"] == 27
    assert np.array_equal(s["size"], [b * (b - 1) // 2 for b in PC.BLOCKS]) and np.all(s["join"])
    assert np.array_equal(s["logpe"], np.zeros(3))
    assert np.array_equal(s["colour"], np.repeat(np.arange(3), [b * (b - 1) // 2 for b in PC.BLOCKS]))
    # beta = 0: nothing is drawn
    ppc.draw(*PC.block_model(0.0), seed=4, r=1)
    s = ppc.stats()
    assert s["ones"] == 0 and s["links"].shape == (0, 2) and s["triangles"] == 0 and s["wedges"] == 0 and s["max_deg"] == 0
    assert not s["deg"].any() and not s["tri"].any() and not s["size"].any() and not s["logpe"].any()
    assert math.isnan(s["transitivity"]) and s["clustering"] == 0.0
    ppc.close()


def test_replicates_average_to_the_model():
    b = PC.expectation_bounds()
    pi, beta = b[0], b[1]
    ppc = _ppc(PC.EXP_N, PC.EXP_K)
    ppc.set_params(pi, beta)
    ones, degs = [], []
    for r in range(PC.EXP_R):
        links = ppc.draw(seed=PC.EXP_SEED, r=r)
        ones.append(len(links))
        degs.append(PC.degrees(links, PC.EXP_N))
    PC.check_expectation(ones, degs, b)
    ppc.close()


def test_a_replicate_does_not_depend_on_the_launches():
    n, K, seed, r = 130, 20, 77, 3
    pi, beta = PC.random_model(n, K, 8)
    a = _ppc(n, K)
    a.draw(pi, beta, seed, r)
    first = a.stats()
    for batch in (1, 4, 0):
        a.set_tile_batch(batch)
        a.draw(seed=seed, r=r)
        _same(a.stats(), first)
    b = _ppc(n, K)   # a fresh handle, with another list and another replicate in between
    b.set_params(pi, beta)
    b.observe(np.array([[0, 1], [5, 129], [64, 65]]))
    assert np.array_equal(b.links(), [[0, 1], [5, 129], [64, 65]])
    b.draw(seed=seed, r=r + 1)
    b.observe(first["links"][::-1])
    _same(b.stats(), first)
    b.draw(seed=seed, r=r)
    _same(b.stats(), first)
    assert first["rechecked"] == b.draw_counts()[1]
    a.close()
    b.close()


def test_observed_network_against_the_graph_and_the_link_communities():
    from svinet_amd.host_api import LinkCommunities
    links, seq2id = restate_findk.read_graph(os.path.join(GOLDEN, "graphs", "assort-75-4.txt"), 75)
    links = np.asarray(links, np.int64).reshape(-1, 2)
    links = links[np.lexsort((links[:, 1], links[:, 0]))]
    n = len(seq2id)
    gamma, _, lam = restate_gml.load_model(os.path.join(GOLDEN, "ref_assort_batch"), n, 4)
    pi, beta = R.mean_params(gamma, lam)
    ppc = _ppc(n, 4)
    ppc.set_params(pi, beta)
    ppc.observe(links[::-1])
    s = ppc.stats()
    assert np.array_equal(s["links"].astype(np.int64), links)
    A = np.zeros((n, n), np.int64)
    A[links[:, 0], links[:, 1]] = A[links[:, 1], links[:, 0]] = 1
    assert np.array_equal(s["deg"], A.sum(1))
    assert np.array_equal(s["tri"], ((A @ A) * A).sum(1) // 2) and s["tri"].any()
    lc = LinkCommunities(links, gamma, lam)
    assert np.array_equal(s["colour"], lc["colour"]) and np.array_equal(s["join"], lc["join"])
    assert np.array_equal(s["size"], np.bincount(lc["colour"][lc["join"]], minlength=4))
    _check_stats(s, R.stats(links, pi, beta))
    ppc.close()


def test_a_list_too_small_keeps_the_state():
    from svinet_amd._svils import SvilsError
    n, K = 65, 5
    pi, beta = PC.random_model(n, K, 1)
    counts = [len(R.draw(pi, beta, 9, r)) for r in range(6)]
    small, big = int(np.argmin(counts)), int(np.argmax(counts))
    assert counts[small] < counts[big]
    ppc = _ppc(n, K, max_links=counts[small])
    ppc.set_params(pi, beta)
    ppc.draw(seed=9, r=small)
    before = ppc.stats()
    with pytest.raises(SvilsError) as ei:
        ppc.draw(seed=9, r=big)
    assert ei.value.code == -3 and str(counts[big]) in str(ei.value)
    assert ppc.draw_counts()[0] == counts[big]
    assert np.array_equal(ppc.links(), before["links"])
    _same(ppc.stats(), before)
    with pytest.raises(SvilsError) as ei:
        ppc.observe(R.draw(pi, beta, 9, big))
    assert ei.value.code == -3
    assert np.array_equal(ppc.draw(seed=9, r=small), before["links"])
    _same(ppc.stats(), before)
    ppc.close()


# ---- the command line end to end ----

SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")


def _cli(args, cwd):
    r = subprocess.run([SVINET] + [str(a) for a in args], cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r


def _files_under(d):
    out = {}
    for base, _, files in os.walk(str(d)):
        for f in files:
            out[os.path.relpath(os.path.join(base, f), str(d))] = open(os.path.join(base, f)).read()
    return out


def _assort(tmp_path):
    for m in ("gamma.txt", "lambda.txt"):
        shutil.copy(os.path.join(GOLDEN, "ref_assort_batch", m), str(tmp_path))
    path = os.path.join(GOLDEN, "graphs", "assort-75-4.txt")
    links, seq2id = restate_findk.read_graph(path, 75)
    gamma, _, lam = restate_gml.load_model(os.path.join(GOLDEN, "ref_assort_batch"), len(seq2id), 4)
    return path, np.asarray(links, np.int64).reshape(-1, 2), gamma, lam


@pytest.mark.parametrize("mean", [True, False])
def test_cli_ppc_files_equal_the_restatement(tmp_path, mean):
    path, links, gamma, lam = _assort(tmp_path)
    _cli(["-file", path, "-n", 75, "-k", 4, "-ppc", "-ppc-draws", 5, "-seed", 17, "-ppc-save", 2] + (["-ppc-mean"] if mean else []), tmp_path)
    want = R.ppc_texts(links, gamma, lam, 5, 17, mean, save=2)
    got = _files_under(tmp_path)
    assert set(got) == set(want) | {"gamma.txt", "lambda.txt"}, sorted(got)
    for name, text in want.items():
        assert got[name] == text, name
    assert len(got["ppc/rep.txt"].splitlines()) == 5 and len(got["ppc/summary.txt"].splitlines()) == 7


def test_cli_gen_files_equal_the_restatement(tmp_path):
    _cli(["-n", 65, "-k", 4, "-gen", "-seed", 3], tmp_path)
    want = R.gen_texts(65, 4, 3)
    got = _files_under(tmp_path)
    assert set(got) == set(want), sorted(got)
    for name, text in want.items():
        assert got[name] == text, name
    assert len(got["gen/network_gen.dat"].splitlines()) > 100
