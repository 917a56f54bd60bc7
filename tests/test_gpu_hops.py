"""-m gpu: svils_ppc_hops (host_api.PPC.hops) and `svinet -ppc -ppc-hops` against the plain-BFS restatement
tools/restate_hops.py, closed forms and boolean matrix powers.  The computation is integer, so D,
ecc, comp and every count are asked to be EQUAL, for any hop batch; effdiam and meandist (a few host doubles in a fixed
order) at rtol 1e-15; the files of the command line as text."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import hops_cases as HC
from hops_cases import H, PC, R

sys.path.insert(0, os.path.join(ROOT, "tools"))
import restate_findk  # noqa: E402
import restate_gml  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
INTS = ("D", "ecc", "comp", "reachable", "diameter", "components", "largest", "isolated")


def _ppc(n, k=2, **kw):
    from svinet_amd.host_api import PPC
    return PPC(n, k, **kw)


def _identical(a, b):
    for name in INTS:
        assert np.array_equal(np.asarray(a[name]), np.asarray(b[name])), name
    for name in ("effdiam", "meandist"):
        assert np.array_equal(np.float64(a[name]), np.float64(b[name]), equal_nan=True), name


@pytest.mark.parametrize("words", [1, 0])
@pytest.mark.parametrize("name", sorted(HC.closed_forms()))
def test_closed_forms(name, words):
    n, links, D, ecc, comp = form = HC.closed_forms()[name]
    ppc = _ppc(n)
    ppc.observe(np.array(links, np.uint32).reshape(-1, 2))
    ppc.set_hop_batch(words, 8 if name == "path-130" else 0)
    got = ppc.hops()
    HC.check_closed_form(got, form)
    HC.same_hops(got, H.all_of(links, n))
    # per pass: a seed, a close, and the levels up to the first empty one (the largest ecc of its sources + 1), in whole chunks
    ms, launches = ppc.hop_timing()
    per, chunk = 64 * (words or 8), 8
    far = [max(ecc[s0:s0 + per]) + 1 for s0 in range(0, n, per)]
    assert ms > 0 and sum(2 + f for f in far) <= launches <= sum(2 + -(-f // chunk) * chunk for f in far), (launches, far)
    if name == "path-130" and words == 1:
        assert far == [130, 128, 130] and launches > 3 * (2 + 15 * chunk)      # three passes, the last of 2 sources; many chunks
    ppc.close()


@pytest.mark.parametrize("n,deg,seed,r", HC.replicate_cases())
def test_replicates_equal_the_restatement(n, deg, seed, r):
    links, want = HC.replicate(n, deg, seed, r)
    pi, beta = HC.model(n, deg)
    ppc = _ppc(n, HC.K)
    assert np.array_equal(ppc.draw(pi, beta, seed, r).astype(np.int64), links)
    HC.same_hops(ppc.hops(), want)
    ppc.close()


@pytest.mark.parametrize("n", [130, 1100])
def test_no_result_depends_on_the_batch(n):
    seed, r = HC.SPARSE_DRAWS[n][0]
    links, want = HC.replicate(n, HC.SPARSE_DEG, seed, r)
    pi, beta = HC.model(n, HC.SPARSE_DEG)
    ppc = _ppc(n, HC.K)
    ppc.draw(pi, beta, seed, r)
    first = ppc.hops()
    HC.same_hops(first, want)
    _identical(ppc.hops(), first)                               # twice the same call
    for words in (1, 2, 3, 8):
        for chunk in (1, 3, 0):
            ppc.set_hop_batch(words, chunk)
            _identical(ppc.hops(), first)
    fresh = _ppc(n, HC.K)
    fresh.observe(links)
    _identical(fresh.hops(), first)
    from svinet_amd._svils import SvilsError
    with pytest.raises(SvilsError) as ei:
        fresh.set_hop_batch(9, 1)
    assert ei.value.code == -1
    fresh.close()
    ppc.close()


def _getters_refuse(ppc):
    import ctypes as C
    from svinet_amd import _svils
    L = _svils.load()
    buf, val, lev = (C.c_uint64 * 8)(), (C.c_double * 2)(), C.c_uint32()
    assert L.svils_ppc_get_hops(ppc._h, C.byref(lev), buf, 8) == -1 and b"svils_ppc_hops has not run" in L.svils_last_error()
    assert L.svils_ppc_get_hop_nodes(ppc._h, None, None) == -1
    assert L.svils_ppc_get_hop_summary(ppc._h, buf, val) == -1


def _assort():
    path = os.path.join(GOLDEN, "graphs", "assort-75-4.txt")
    links, seq2id = restate_findk.read_graph(path, 75)
    links = np.asarray(links, np.int64).reshape(-1, 2)
    gamma, _, lam = restate_gml.load_model(os.path.join(GOLDEN, "ref_assort_batch"), len(seq2id), 4)
    return path, links, gamma, lam


def test_results_belong_to_their_list():
    _, links, gamma, lam = _assort()
    n = gamma.shape[0]
    pi, beta = R.mean_params(gamma, lam)
    ppc = _ppc(n, 4)
    assert ppc.hop_timing() == (-1.0, -1)
    _getters_refuse(ppc)                                        # before any svils_ppc_hops
    ppc.set_params(pi, beta)
    drawn = ppc.draw(seed=3, r=0)
    HC.same_hops(ppc.hops(), H.all_of(drawn, n))
    ppc.observe(links)
    _getters_refuse(ppc)                                        # another list: the results are gone
    got = ppc.hops()
    HC.same_hops(got, H.all_of(links, n))
    D, ecc, comp = HC.matrix_power_route(links, n)
    assert got["D"].tolist() == D and got["ecc"].tolist() == ecc and got["comp"].tolist() == comp
    ppc.draw(seed=3, r=1)
    _getters_refuse(ppc)
    ppc.close()


def test_a_list_too_small_keeps_the_hop_results():
    import ctypes as C
    from svinet_amd import _svils
    n, K = 65, 5
    pi, beta = PC.random_model(n, K, 1)
    counts = [len(R.draw(pi, beta, 9, r)) for r in range(6)]
    small, big = int(np.argmin(counts)), int(np.argmax(counts))
    ppc = _ppc(n, K, max_links=counts[small])
    ppc.set_params(pi, beta)
    ppc.draw(seed=9, r=small)
    before = ppc.hops()
    with pytest.raises(_svils.SvilsError) as ei:
        ppc.draw(seed=9, r=big)
    assert ei.value.code == -3
    L = _svils.load()
    counts6, values, ecc, comp = np.zeros(6, np.uint64), np.zeros(2), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    assert L.svils_ppc_get_hop_summary(ppc._h, counts6.ctypes.data, values.ctypes.data) == 0
    assert L.svils_ppc_get_hop_nodes(ppc._h, ecc.ctypes.data, comp.ctypes.data) == 0
    D, lev = np.zeros(int(counts6[5]), np.uint64), C.c_uint32()
    assert L.svils_ppc_get_hops(ppc._h, C.byref(lev), D.ctypes.data, len(D)) == 0 and lev.value == len(D)
    assert np.array_equal(D, before["D"]) and np.array_equal(ecc, before["ecc"]) and np.array_equal(comp, before["comp"])
    assert [int(c) for c in counts6[:5]] == [before[k] for k in ("reachable", "diameter", "components", "largest", "isolated")]
    assert values[0] == before["effdiam"] and values[1] == before["meandist"]
    HC.same_hops(before, H.all_of(R.draw(pi, beta, 9, small), n))
    ppc.close()


def test_hops_and_stats_do_not_touch_each_other():
    n, K, seed, r = 130, HC.K, 77, 3
    pi, beta = HC.model(n, HC.DENSE_DEG)
    keys = ("links", "deg", "tri", "colour", "join", "size", "logpe", "ones", "max_deg", "argmax_deg", "triangles", "wedges",
            "transitivity", "clustering")

    def same_stats(a, b):
        for k in keys:
            if k in ("logpe", "transitivity", "clustering"):
                assert np.array_equal(np.asarray(a[k], np.float64), np.asarray(b[k], np.float64), equal_nan=True), k
            else:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k

    alone = _ppc(n, K)
    alone.draw(pi, beta, seed, r)
    stats = alone.stats()
    a = _ppc(n, K)
    a.draw(pi, beta, seed, r)
    sa = a.stats()
    ha = a.hops()
    import ctypes as C
    from svinet_amd import _svils
    L = _svils.load()
    counts, values = np.zeros(5, np.uint64), np.zeros(2)
    assert L.svils_ppc_get_summary(a._h, counts.ctypes.data, values.ctypes.data) == 0      # still answered after hops
    assert [int(c) for c in counts] == [stats[k] for k in ("ones", "max_deg", "argmax_deg", "triangles", "wedges")]
    deg, tri = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    assert L.svils_ppc_get_nodes(a._h, deg.ctypes.data, tri.ctypes.data) == 0
    assert np.array_equal(deg, stats["deg"]) and np.array_equal(tri, stats["tri"])
    size, logpe = np.zeros(K, np.uint64), np.zeros(K)
    assert L.svils_ppc_get_communities(a._h, size.ctypes.data, logpe.ctypes.data) == 0
    assert np.array_equal(size, stats["size"]) and np.array_equal(logpe, stats["logpe"])
    same_stats(sa, stats)
    b = _ppc(n, K)
    b.draw(pi, beta, seed, r)
    hb = b.hops()
    same_stats(b.stats(), stats)
    _identical(ha, hb)
    _identical(b.hops(), hb)
    HC.same_hops(ha, H.all_of(stats["links"], n))
    for p in (alone, a, b):
        p.close()


# ---- the command line end to end ----

SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
HOP_FILES = {"obs-hop.txt", "ppc/ppc-hop.txt", "ppc/obs-hops.txt", "ppc/rep-hops.txt", "ppc/hops-summary.txt"}


def _run(args, cwd):
    os.makedirs(str(cwd))
    for m in ("gamma.txt", "lambda.txt"):
        shutil.copy(os.path.join(GOLDEN, "ref_assort_batch", m), str(cwd))
    r = subprocess.run([SVINET] + [str(a) for a in args], cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = {}
    for base, _, files in os.walk(str(cwd)):
        for f in files:
            out[os.path.relpath(os.path.join(base, f), str(cwd))] = open(os.path.join(base, f)).read()
    return out


@pytest.mark.parametrize("mean", [True, False])
def test_cli_hop_files_equal_the_restatement(tmp_path, mean):
    path, links, gamma, lam = _assort()
    args = ["-file", path, "-n", 75, "-k", 4, "-ppc", "-ppc-draws", 3, "-seed", 17] + (["-ppc-mean"] if mean else [])
    without = _run(args, tmp_path / "without")
    with_ = _run(args + ["-ppc-hops"], tmp_path / "with")
    assert not HOP_FILES & set(without) and set(with_) == set(without) | HOP_FILES, sorted(with_)
    for name, text in without.items():
        assert with_[name] == text, name                          # byte for byte what the run without the flag writes
    want = H.ppc_hops_texts(links, gamma, lam, 3, 17, mean)
    assert set(want) == HOP_FILES
    for name, text in want.items():
        assert with_[name] == text, name
    assert len(with_["ppc/rep-hops.txt"].splitlines()) == 3 and len(with_["ppc/hops-summary.txt"].splitlines()) == 6
