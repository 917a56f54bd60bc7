"""-rnode / -rpair / -rpair -stratified without a device: the host loops of svinet_amd/host/mmsbbatch.cc against
tests/sampled_cases.py (a restatement of one step of MMSBInfer::infer, src/mmsbinfer.cc:459-740), the drawn schedule, the
step sizes, the command line with -host-loops and every refusal.

Tolerance: rtol 1e-7 on gamma, lambda and the heldout row, the one tests/test_batch.py holds this fixed point to;
sampled_cases.assert_exits_are_clear is asserted for every compared step."""
import os
import subprocess

import numpy as np
import pytest

import batch_cases as BC
import sampled_cases as SC
from oracle import batch_oracle as B
from svinet_amd import _svils
from svinet_amd.host_api import SampledEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
RTOL = 1e-7
MODES = ("rnode", "rpair", "rpair-stratified")
N, K = 75, 4


def _engine(graph_files, mode, **kw):
    return SampledEngine(graph_files["assort"], N, K, mode, heldout_ratio=0.1, **kw)


def _skip(e):
    return {tuple(int(x) for x in r) for r in e.heldout} | {tuple(int(x) for x in r) for r in e.validation}


def _have_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.parametrize("mode", MODES)
def test_host_loops_match_the_restatement(graph_files, mode):
    e = _engine(graph_files, mode, nodelay=(mode == "rpair"))
    adj = BC.adjacency(e.n, e.edges)
    g, lam = e.gamma, e.lam
    hsorted = sorted({tuple(int(x) for x in r) for r in e.heldout})
    for s in range(6):
        e.step(1)
        d = e.schedule[s]
        p, q = d["pairs"][:, 0].astype(np.int64), d["pairs"][:, 1].astype(np.int64)
        SC.assert_exits_are_clear(g, lam, adj, p, q)
        g, lam, _ = SC.step(g, lam, adj, p, q, 1.0 / K, e.eta, d["scale"], d["rho_gamma"], d["rho_lambda"])
        np.testing.assert_allclose(e.gamma, g, rtol=RTOL)
        np.testing.assert_allclose(e.lam, lam, rtol=RTOL)
    assert e.iter == 6 and not e.report()
    np.testing.assert_allclose(e.rows[-1, 1:], B.heldout_row(g, lam, hsorted, adj, e.ones_prob), rtol=RTOL)
    assert e.rows.shape == (2, 10) and e.rows[-1, 0] == 6


@pytest.mark.parametrize("mode", MODES)
def test_the_drawn_schedule(graph_files, mode):
    e = _engine(graph_files, mode)
    skip = _skip(e)
    adj = BC.adjacency(e.n, e.edges)
    e.step(8)
    sched = e.schedule
    assert len(sched) == 8 and e.total_pairs == N * (N - 1) // 2
    for s, d in enumerate(sched):
        pairs = [tuple(int(x) for x in r) for r in d["pairs"]]
        assert all(p < q < e.n for p, q in pairs) and not skip & set(pairs)          # no held-out or validation pair
        assert d["rho_gamma"] == SC.rho_gamma(s) and d["rho_lambda"] < 0              # delayed: 8 * 37 < 2775
        if mode == "rnode":
            a = d["node"]
            assert all(a in pq for pq in pairs) and len(set(pairs)) == len(pairs)
            assert len(pairs) == e.n - 1 - sum(1 for pq in skip if a in pq)
            assert d["scale"] == e.n / 2.0
            continue
        assert len(pairs) == e.n // 2
        y = np.array([adj[pq] for pq in pairs])
        if mode == "rpair":
            assert d["family"] == 0 and d["scale"] == e.total_pairs / (e.n // 2)
        else:
            assert d["family"] == s % 2 and np.all(y == d["family"])                  # 0, 1, 0, ..: non-links, links
            prob = e.ones_prob if d["family"] else 1 - e.ones_prob
            assert d["scale"] == pytest.approx(e.total_pairs * prob / (e.n // 2), rel=1e-12)


def test_step_sizes_follow_the_closed_forms():
    assert SC.rho_gamma(0) == 1025.0 ** -0.5 and SC.rho_gamma(250) == 1027.5 ** -0.5
    assert SC.rho_lambda(76, 76) == 1026.0 ** -0.9 and SC.rho_lambda(100, 76) == 1050.0 ** -0.9
    assert SC.rho_gamma(7, nodetau0=10.0, nodekappa=0.75) == 11.07 ** -0.75
    assert SC.rho_lambda(5, 0, tau0=10.0, kappa=0.6) == 17.0 ** -0.6


def test_lambda_waits_until_the_sampled_pairs_exceed_all_pairs(graph_files):
    """lambda learning begins once iter * s > total_pairs (:613): 37 iter > 2775, iteration 76 on; -nodelay: the first"""
    e = _engine(graph_files, "rpair", tau0=10.0, kappa=0.6, nodetau0=10.0, nodekappa=0.75)
    lam0, g0 = e.lam, e.gamma
    e.step(76)
    assert e.lam.tobytes() == lam0.tobytes() and not np.array_equal(e.gamma, g0)
    e.step(2)
    assert not np.array_equal(e.lam, lam0)
    sched = e.schedule
    assert [d["rho_lambda"] < 0 for d in sched] == [True] * 76 + [False] * 2
    assert sched[76]["rho_lambda"] == SC.rho_lambda(76, 76, tau0=10.0, kappa=0.6)
    assert sched[77]["rho_lambda"] == SC.rho_lambda(77, 76, tau0=10.0, kappa=0.6)
    assert sched[77]["rho_gamma"] == SC.rho_gamma(77, nodetau0=10.0, nodekappa=0.75)
    d = _engine(graph_files, "rnode", nodelay=True)
    lam0 = d.lam
    d.step(1)
    assert not np.array_equal(d.lam, lam0) and d.schedule[0]["rho_lambda"] == SC.rho_lambda(0, 0)


def _cli(args, tmp, timeout=300):
    return subprocess.run([SVINET] + args + ["-outdir", str(tmp)], capture_output=True, text=True, timeout=timeout)


def test_cli_rnode_host_loops_writes_the_batch_file_set(graph_files, tmp_path):
    common = ["-file", graph_files["assort"], "-n", "75", "-k", "4", "-heldout-ratio", "0.1"]
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    r = _cli(common + ["-rnode", "-host-loops", "-max-iterations", "250"], tmp_path / "a")
    assert r.returncode == 0, r.stderr
    d = tmp_path / "a" / "n75-k4-mmsb-Urnode"
    for f in ("param.txt", "heldout-edges.txt", "validation-edges.txt", "heldout.txt", "validation.txt", "max.txt",
              "gamma.txt", "lambda.txt", "groups.txt", "communities.txt", "summary.txt"):
        assert (d / f).exists(), f
    rows = np.loadtxt(d / "heldout.txt")
    assert rows.shape == (3, 11) and list(rows[:, 0]) == [0, 100, 200]
    assert sorted(set(np.loadtxt(d / "validation.txt")[:, 0])) == [0, 100, 200]   # (a new best held-out value adds a row)
    gam = np.loadtxt(d / "gamma.txt")
    assert gam.shape == (75, 6) and np.all(gam[:, 2:] > 0)
    param = (d / "param.txt").read_text()
    assert "randomnode: True" in param and "delaylearn: True" in param and "reportfreq: 100" in param
    assert "learning lambda since (iter): 76" in param
    h = _cli(common + ["-batch", "-max-iterations", "1"], tmp_path / "b")
    assert h.returncode == 0, h.stderr
    for f in ("heldout-edges.txt", "validation-edges.txt"):
        assert (d / f).read_bytes() == (tmp_path / "b" / "n75-k4-mmsb-batch" / f).read_bytes(), f


@pytest.mark.parametrize("flags,name", [(["-rnode"], "Urnode"), (["-rnode", "-nodelay"], "rnode"), (["-rpair"], "Urpair"),
                                        (["-rpair", "-nodelay"], "rpair"), (["-rpair", "-stratified"], "SUrpair"),
                                        (["-stratified", "-nodelay", "-rpair"], "Srpair")])
def test_cli_directory_names(graph_files, tmp_path, flags, name):
    """src/env.hh:529-546; -rfreq given before the flag stays"""
    r = _cli(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-heldout-ratio", "0.1", "-rfreq", "2"] + flags +
             ["-host-loops", "-max-iterations", "3"], tmp_path)
    assert r.returncode == 0, r.stderr
    d = tmp_path / ("n75-k4-mmsb-" + name)
    assert d.is_dir() and [p.name for p in tmp_path.iterdir()] == [d.name]
    assert list(np.loadtxt(d / "heldout.txt")[:, 0]) == [0, 2, 4]


REFUSALS = [
    (["-stratified", "-rnode"], "-stratified -rnode"),
    (["-stratified"], "-stratified"),
    (["-rnode", "-scale", "2"], "-scale"),
    (["-rpair", "-scale", "0.5"], "-scale"),
    (["-rnode", "-rpair"], "-rpair"),
] + [([mode, other] + extra, other) for mode in ("-rnode", "-rpair")
     for other, extra in (("-link-sampling", []), ("-findk", []), ("-batch", []), ("-gml", []), ("-lcstats", []), ("-kshard", []),
                          ("-sharded", []), ("-minibatch", ["8"]), ("-predict-pairs", ["x"]), ("-recommend", ["3"]),
                          ("-rank-pairs", ["x"]), ("-rank-heldout", []), ("-adamic-adar", []))] + [
    (["-rnode", "-gpus", "2"], "-gpus"), (["-rpair", "-gpus", "2"], "-gpus"),
    (["-link-sampling", "-rpair"], "-rpair"), (["-batch", "-rnode"], "-rnode"),
]


@pytest.mark.parametrize("flags,named", REFUSALS)
def test_cli_refusals(tmp_path, flags, named):
    for order in (flags, flags[::-1] if len(flags) == 2 and not flags[1][0].isdigit() and flags[1] != "x" else flags):
        r = _cli(["-file", "x", "-n", "75", "-k", "4"] + order, tmp_path, timeout=60)
        assert r.returncode == 2 and named in r.stderr, (order, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


def test_cli_limits_are_checked_before_anything_is_read(tmp_path):
    for mode in ("-rnode", "-rpair"):
        for size, limit in ((["-n", "75", "-k", "300"], "256"), (["-n", "40000", "-k", "4"], "32768")):
            r = _cli(["-file", "x"] + size + [mode], tmp_path, timeout=60)
            assert r.returncode == 2 and limit in r.stderr and mode in r.stderr, r.stderr
    assert not list(tmp_path.iterdir())
    r = _cli(["-help"], tmp_path)
    for flag in ("-rnode", "-rpair", "-stratified", "-nodelay", "-host-loops"):
        assert "\t%s\t" % flag in r.stdout


def test_cli_without_a_gpu_fails_loudly_after_the_host_setup(graph_files, tmp_path):
    if _have_gpu():
        pytest.skip("GPU present")
    r = _cli(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-rpair", "-stratified", "-heldout-ratio", "0.1"], tmp_path, timeout=120)
    assert r.returncode != 0 and "no CPU path" in r.stderr
    assert (tmp_path / "n75-k4-mmsb-SUrpair" / "heldout-edges.txt").exists()
    assert not list(tmp_path.rglob("gamma.txt")) and not list(tmp_path.rglob("heldout.txt"))
    with pytest.raises(_svils.SvilsError) as ei:
        _engine(graph_files, "rnode", on_device=True)
    assert ei.value.code == -2 and "no CPU path" in str(ei.value)


def test_step_entry_points_refuse_a_null_handle():
    """as the other entry points of the handle: "no HIP device" where there is none, else a bad argument"""
    L = _svils.load()
    assert "svils_batch_step_node" in _svils.EXPORTS and "svils_batch_step_pairs" in _svils.EXPORTS
    null = -1 if _have_gpu() else -2
    one = np.ones(1)
    node = np.zeros(1, dtype=np.uint32)
    off = np.array([0, 1], dtype=np.uint64)
    pair = np.array([[0, 1]], dtype=np.uint32)
    assert L.svils_batch_step_node(None, 1, node.ctypes.data, 1.0, one.ctypes.data, one.ctypes.data) == null
    assert L.svils_batch_step_node(None, 1, None, 1.0, None, None) == null
    assert L.svils_batch_step_pairs(None, 1, off.ctypes.data, pair.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data) == null
    assert L.svils_batch_step_pairs(None, 1, None, None, None, None, None) == null
    if not _have_gpu():
        assert b"no CPU path" in L.svils_last_error()
    assert L.svils_abi_version() == 8
