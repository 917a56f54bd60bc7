"""-snode without a device: the host loops of svinet_amd/host/mmsbbatch.cc against snode_cases.step (one eager step of
FastAMM2::infer, src/fastamm2.cc:535-702: all n rows move), the drawn lists with their scales and step sizes, the setup
shared with -infset, the command line with -host-loops and every refusal.

Tolerance: rtol 1e-7 on gamma and lambda, the one tests/test_sampled.py and tests/test_infset.py hold this fixed point to;
sampled_cases.assert_exits_are_clear is asserted for every compared step."""
import os
import subprocess

import numpy as np
import pytest

import batch_cases as BC
import sampled_cases as SC
import snode_cases as NC
from svinet_amd import _svils, host_api
from svinet_amd.host_api import InfsetEngine, StratNodeEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
RTOL = 1e-7
N, K = 75, 4


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _cli(args, tmp, timeout=300, cwd=None):
    return subprocess.run([SVINET] + args + ["-outdir", str(tmp)], capture_output=True, text=True, timeout=timeout, cwd=cwd)


def _engine(graph_files, **kw):
    kw.setdefault("heldout_ratio", 0.1)
    return StratNodeEngine(graph_files["assort"], N, K, **kw)


def _skip(e):
    return {tuple(int(x) for x in r) for r in e.heldout} | {tuple(int(x) for x in r) for r in e.validation}


def _follow(e, nsteps):
    """e stepped one iteration at a time against the restatement; returns the kinds drawn"""
    adj = BC.adjacency(e.n, e.edges)
    g, lam = e.gamma, e.lam
    kinds = []
    for s in range(nsteps):
        e.step(1)
        d = e.schedule()[s]
        kinds.append(d["kind"])
        SC.assert_exits_are_clear(g, lam, adj, *NC.pairs_of(d))
        g0 = g
        g, lam, _ = NC.step(g, lam, adj, d, 1.0 / K, e.eta)
        np.testing.assert_allclose(e.gamma, g, rtol=RTOL)
        np.testing.assert_allclose(e.lam, lam, rtol=RTOL)
        rest = np.setdiff1d(np.arange(e.n), np.append(d["partner"], d["start"]))
        rho = d["rho_gamma"]
        assert len(rest) and np.array_equal(g[rest], (1 - rho) * g0[rest] + rho * (1.0 / K))   # every other row moves towards alpha
        assert not np.any(e.gamma[rest] == g0[rest])
    assert e.iter == nsteps
    return kinds


def test_host_loops_match_the_restatement_with_both_kinds_of_step(graph_files):
    e = _engine(graph_files, seed=3)
    assert set(_follow(e, 20)) == {0, 1}                                           # the chance of a non-link step is 1/2
    assert not e.report() and e.rows.shape == (2, 10) and e.rows[-1, 0] == 20
    assert set(_follow(_engine(graph_files, seed=4, inf_epsilon=0.0), 4)) == {0}  # and each kind forced through that chance
    assert set(_follow(_engine(graph_files, seed=4, inf_epsilon=1.0), 4)) == {1}


def test_the_drawn_lists_scales_and_step_sizes(graph_files):
    import infset_cases as IC
    e = _engine(graph_files, seed=5)
    skip = _skip(e)
    nbrs = IC.adjacency_lists(e.n, e.edges)
    shuffled = e.shuffled()
    assert sorted(shuffled) == list(range(e.n)) and list(shuffled) != list(range(e.n))
    e.sweep()                                                                      # one report interval: 100 iterations
    sched = e.schedule()
    assert len(sched) == 100 == e.iter and {d["kind"] for d in sched} == {0, 1}
    adj = BC.adjacency(e.n, e.edges)
    assert NC.setsize(e.n) == 7 and NC.block_starts(e.n) == list(range(0, 75, 7))
    for it, d in enumerate(sched):
        partner = [int(x) for x in d["partner"]]
        lists = [NC.expected_partners(d["kind"], d["start"], q0, shuffled, nbrs, skip) for q0 in (NC.block_starts(e.n) if d["kind"] else [0])]
        assert partner in lists
        assert np.array_equal(d["y"], adj[d["start"], d["partner"]])
        assert len(set(partner)) == len(partner) and d["start"] not in partner
        if d["kind"] == 1:
            assert not d["y"].any() and len(partner) == NC.setsize(e.n)            # every walk finds its set within a lap
        else:
            assert d["y"].all()
        assert d["scale"] == NC.scale_of(d["kind"], e.n)
        assert d["rho_gamma"] == NC.rho_gamma(it) and d["rho_lambda"] == NC.rho_lambda(it)
    assert NC.scale_of(0, 75) == 75.0 and NC.scale_of(1, 75) == 750.0              # n / (2 (1 - 1/2)), 10 n / (2 / 2)
    assert NC.rho_gamma(0) == 1025.0 ** -0.5 and NC.rho_gamma(7) == 1032.0 ** -0.5
    assert NC.rho_lambda(0) == 1026.0 ** -0.9 and NC.rho_lambda(5, tau0=10.0, kappa=0.6) == 17.0 ** -0.6
    e = _engine(graph_files, seed=5, nodetau0=3.0, nodekappa=0.75, tau0=10.0, kappa=0.6)   # the step-size flags reach the draw
    e.step(3)
    assert [d["rho_gamma"] for d in e.schedule()] == [NC.rho_gamma(i, 3.0, 0.75) for i in range(3)]
    assert [d["rho_lambda"] for d in e.schedule()] == [NC.rho_lambda(i, 10.0, 0.6) for i in range(3)]


def test_the_setup_is_that_of_infset(graph_files, tmp_path):
    """FastAMM2's constructor is FastAMM's: the shuffle, the held-out sets and the initial state of the same seed"""
    nb = str(tmp_path / "neighbors.bin")
    host_api.preprocess(graph_files["assort"], N, nb)
    for seed in (0, 7):
        a = _engine(graph_files, seed=seed)
        b = InfsetEngine(graph_files["assort"], N, K, nb, heldout_ratio=0.1, seed=seed)
        assert a.heldout.tobytes() == b.heldout.tobytes() and a.validation.tobytes() == b.validation.tobytes()
        assert a.gamma.tobytes() == b.gamma.tobytes() and a.lam.tobytes() == b.lam.tobytes()
        assert np.array_equal(a.shuffled(), b.shuffled)
        assert a.rows.tobytes() == b.rows.tobytes()                                # the row of iteration 0


@pytest.mark.parametrize("flags,name", [([], "SUrnode"), (["-nodelay"], "Srnode")])
def test_cli_host_loops(graph_files, tmp_path, flags, name):
    common = ["-file", graph_files["assort"], "-n", "75", "-k", "4", "-heldout-ratio", "0.1"]
    r = _cli(common + ["-rfreq", "40", "-snode", "-host-loops", "-max-iterations", "100"] + flags, tmp_path)
    assert r.returncode == 0, r.stderr
    d = tmp_path / ("n75-k4-mmsb-" + name)
    assert d.is_dir() and [p.name for p in tmp_path.iterdir()] == [d.name]
    for f in ("param.txt", "heldout-pairs.txt", "validation-pairs.txt", "precision-pairs.txt", "heldout.txt", "validation.txt",
              "max.txt", "gamma.txt", "lambda.txt", "groups.txt", "communities.txt", "summary.txt"):
        assert (d / f).exists(), f
    assert not (d / "heldout-edges.txt").exists()
    rows = np.loadtxt(d / "heldout.txt")
    assert rows.shape == (3, 11) and list(rows[:, 0]) == [0, 40, 80]               # -rfreq given before the flag stays
    gam = np.loadtxt(d / "gamma.txt")
    assert gam.shape == (75, 6) and np.all(gam[:, 2:] > 0)
    assert np.loadtxt(d / "lambda.txt").shape == (4, 3)
    param = (d / "param.txt").read_text()
    assert "inf_epsilon: 0.5" in param and "noninf_setsize: 7" in param and "reportfreq: 40" in param
    if flags:
        return
    # the default report interval is -rnode's; the held-out files are those of an -infset run of the same seed
    work = tmp_path / "work"
    for sub in (work, tmp_path / "b", tmp_path / "c"):
        sub.mkdir()
    r = _cli(common + ["-snode", "-host-loops", "-max-iterations", "250", "-logl"], tmp_path / "b")
    assert r.returncode == 0, r.stderr
    b = tmp_path / "b" / "n75-k4-mmsb-SUrnode"
    assert list(np.loadtxt(b / "heldout.txt")[:, 0]) == [0, 100, 200] and "reportfreq: 100" in (b / "param.txt").read_text()
    assert list(np.loadtxt(b / "logl.txt")[:, 0]) == [0, 100, 200]
    host_api.preprocess(graph_files["assort"], N, str(work / "neighbors.bin"))
    r = _cli(common + ["-infset", "-host-loops", "-max-iterations", "1"], tmp_path / "c", cwd=str(work))
    assert r.returncode == 0, r.stderr
    for f in ("heldout-pairs.txt", "validation-pairs.txt"):
        assert (d / f).read_bytes() == (tmp_path / "c" / "n75-k4-mmsb-infset" / f).read_bytes(), f


REFUSALS = [(["-snode", other] + extra, other)
            for other, extra in (("-link-sampling", []), ("-findk", []), ("-batch", []), ("-batch-gpu", []), ("-gml", []),
                                 ("-lcstats", []), ("-rnode", []), ("-rpair", []), ("-stratified", []), ("-kshard", []),
                                 ("-sharded", []), ("-minibatch", ["8"]), ("-predict-pairs", ["x"]), ("-recommend", ["3"]),
                                 ("-rank-pairs", ["x"]), ("-rank-heldout", []), ("-adamic-adar", []), ("-gpus", ["2"]),
                                 ("-scale", ["2"]), ("-infset", []), ("-preprocess", []), ("-orig", []), ("-ppc", []), ("-gen", []))]


@pytest.mark.parametrize("flags,named", REFUSALS)
def test_cli_refusals(tmp_path, flags, named):
    named = "-batch" if named == "-batch-gpu" else named
    for order in (flags, flags[::-1] if len(flags) == 2 else flags):
        r = _cli(["-file", "x", "-n", "75", "-k", "4"] + order, tmp_path, timeout=60)
        assert r.returncode == 2 and named in r.stderr and "-snode" in r.stderr, (order, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


def test_stratified_rnode_stays_refused_and_names_the_flag(tmp_path):
    for order in (["-stratified", "-rnode"], ["-rnode", "-stratified"]):
        r = _cli(["-file", "x", "-n", "75", "-k", "4"] + order, tmp_path, timeout=60)
        assert r.returncode == 2 and "-stratified -rnode" in r.stderr and "use -snode" in r.stderr
    assert not list(tmp_path.iterdir())


def test_cli_limits_are_checked_before_anything_is_read(tmp_path):
    for size, limit in ((["-n", "75", "-k", "300"], "256"), (["-n", "40000", "-k", "4"], "32768")):
        r = _cli(["-file", "x"] + size + ["-snode"], tmp_path, timeout=60)
        assert r.returncode == 2 and limit in r.stderr and "-snode" in r.stderr, r.stderr
    assert not list(tmp_path.iterdir())
    r = _cli(["-help"], tmp_path)
    assert r.returncode == 0 and "\t-snode\t" in r.stdout


def test_cli_without_a_gpu_fails_loudly_after_the_host_setup(graph_files, tmp_path):
    if _have_gpu():
        pytest.skip("GPU present")
    r = _cli(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-snode", "-heldout-ratio", "0.1"], tmp_path, timeout=120)
    assert r.returncode != 0 and "no CPU path" in r.stderr
    assert (tmp_path / "n75-k4-mmsb-SUrnode" / "heldout-pairs.txt").exists()
    assert not list(tmp_path.rglob("gamma.txt")) and not list(tmp_path.rglob("heldout.txt"))
    with pytest.raises(_svils.SvilsError) as ei:
        _engine(graph_files, on_device=True)
    assert ei.value.code == -2 and "no CPU path" in str(ei.value)


def test_strat_entry_points_are_exported_and_refuse_a_null_handle():
    L = _svils.load()
    assert "svils_batch_step_strat" in _svils.EXPORTS and "svils_batch_get_lag" in _svils.EXPORTS
    assert L.svils_abi_version() == 8
    null = -1 if _have_gpu() else -2
    one, node, y = np.ones(1) * 0.5, np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint8)
    off = np.array([0, 1], dtype=np.uint64)
    assert L.svils_batch_step_strat(None, 1, node.ctypes.data, off.ctypes.data, node.ctypes.data, y.ctypes.data, one.ctypes.data,
                                    one.ctypes.data, one.ctypes.data) == null
    assert L.svils_batch_step_strat(None, 1, None, None, None, None, None, None, None) == null
    assert L.svils_batch_get_lag(None, None) == null
    if not _have_gpu():
        assert b"no CPU path" in L.svils_last_error()
