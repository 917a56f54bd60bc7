"""-infset / -preprocess without a device: neighbors.bin against tests/infset_cases.py::preprocess_walk (a restatement of
Network::set_neighborhood_sets, src/network.cc:558-686), the host loops of svinet_amd/host/mmsbbatch.cc against
infset_cases.step (one step of FastAMM::infer, src/fastamm.cc:549-672), the drawn schedule with its counters and step
sizes, the command line with -host-loops and every refusal.

Tolerance: rtol 1e-7 on gamma and lambda, the one tests/test_sampled.py holds this fixed point to;
sampled_cases.assert_exits_are_clear is asserted for every compared step."""
import os
import subprocess

import numpy as np
import pytest

import batch_cases as BC
import infset_cases as IC
import sampled_cases as SC
from svinet_amd import _svils, host_api
from svinet_amd.host_api import BatchEngine, InfsetEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
RTOL = 1e-7
N, K = 75, 4


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _cli(args, tmp, timeout=300, cwd=None):
    return subprocess.run([SVINET] + args + ["-outdir", str(tmp)], capture_output=True, text=True, timeout=timeout, cwd=cwd)


def _edges(path, n, k=4):
    e = BatchEngine(path, n, k, heldout_ratio=0.1)
    edges, nn = e.edges, e.n
    e.close()
    return nn, edges


@pytest.fixture(scope="module")
def assort_sets(graph_files, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("nb") / "neighbors.bin")
    host_api.preprocess(graph_files["assort"], N, out)
    return out


@pytest.mark.parametrize("name,n", [("assort", 75), ("lfr", 1000)])
def test_preprocess_writes_the_restated_sets_byte_for_byte(graph_files, tmp_path, name, n):
    r = _cli(["-file", graph_files[name], "-n", str(n), "-k", "4", "-preprocess"], tmp_path)
    assert r.returncode == 0, r.stderr
    d = tmp_path / ("n%d-k4-mmsb-infset" % n)
    nn, edges = _edges(graph_files[name], n)
    assert nn == n
    nbrs = IC.adjacency_lists(n, edges)
    sets = IC.preprocess_walk(nbrs)
    assert (d / "neighbors.bin").read_bytes() == IC.neighbors_bytes(sets)
    assert not (d / "gamma.txt").exists() and not (d / "heldout.txt").exists()     # it exits after the pass
    read = host_api.read_neighbors(str(d / "neighbors.bin"), n)
    assert max(len(z) for z in read) <= IC.LIMIT and any(len(z) == IC.LIMIT for z in read) == (name == "lfr")
    for i, z in enumerate(read):
        z = [int(x) for x in z]
        assert i not in z and not set(z) & set(nbrs[i]) and len(set(z)) == len(z)
        assert all(set(nbrs[i]) & set(nbrs[p]) for p in z)                         # two hops away


def test_preprocess_gives_an_isolated_node_an_empty_set(tmp_path):
    """-n 12 with ten nodes in the file: nodes 10 and 11 have no link; a path end has one two-hop non-neighbour"""
    links = np.array([(i, i + 1) for i in range(9)], dtype=np.uint32)
    path = BC.write_graph(tmp_path / "g.txt", links)
    out = str(tmp_path / "neighbors.bin")
    host_api.preprocess(path, 12, out)
    sets = host_api.read_neighbors(out, 12)
    assert [len(z) for z in sets] == [1, 1, 2, 2, 2, 2, 2, 2, 1, 1, 0, 0]
    assert open(out, "rb").read() == IC.neighbors_bytes(IC.preprocess_walk(IC.adjacency_lists(12, links)))


def _engine(graph_files, assort_sets, **kw):
    kw.setdefault("heldout_ratio", 0.1)
    return InfsetEngine(graph_files["assort"], N, K, assort_sets, **kw)


def _skip(e):
    return {tuple(int(x) for x in r) for r in e.heldout} | {tuple(int(x) for x in r) for r in e.validation}


def test_host_loops_match_the_restatement_with_both_kinds_of_step(graph_files, assort_sets):
    e = _engine(graph_files, assort_sets, inf_epsilon=0.3, seed=3)
    adj = BC.adjacency(e.n, e.edges)
    g, lam = e.gamma, e.lam
    counts = np.zeros(e.n, dtype=np.int64)
    kinds = []
    for s in range(20):
        before = e.gamma
        e.step(1)
        d = e.schedule[s]
        kinds.append(d["kind"])
        p, q = IC.pairs_of(d)
        SC.assert_exits_are_clear(g, lam, adj, p, q)
        # the step sizes are those of the counters before the step; every row of the star is counted once
        assert d["rho_start"] == IC.rho_node(counts[d["start"]])
        assert np.array_equal(d["rho_partner"], [IC.rho_node(c) for c in counts[d["partner"]]])
        assert d["rho_lambda"] == IC.rho_lambda(s) and d["scale"] == IC.scale_of(d["kind"], e.n, 0.3)
        counts[d["start"]] += 1
        counts[d["partner"]] += 1
        g0 = g
        g, lam, _ = IC.step(g, lam, adj, d, 1.0 / K, e.eta)
        np.testing.assert_allclose(e.gamma, g, rtol=RTOL)
        np.testing.assert_allclose(e.lam, lam, rtol=RTOL)
        rest = np.setdiff1d(np.arange(e.n), np.append(d["partner"], d["start"]))
        assert g[rest].tobytes() == g0[rest].tobytes() and e.gamma[rest].tobytes() == before[rest].tobytes()   # no other row moves
    assert set(kinds) == {0, 1}
    assert np.array_equal(e.node_counts, counts) and e.iter == 20
    assert not e.report() and e.rows.shape == (2, 10) and e.rows[-1, 0] == 20


def test_the_drawn_schedule(graph_files, assort_sets):
    e = _engine(graph_files, assort_sets, inf_epsilon=0.25, seed=5)
    skip = _skip(e)
    nbrs = IC.adjacency_lists(e.n, e.edges)
    zeros = [[int(x) for x in z] for z in host_api.read_neighbors(assort_sets, N)]
    shuffled = e.shuffled
    assert sorted(shuffled) == list(range(e.n)) and list(shuffled) != list(range(e.n))
    e.step(40)
    sched = e.schedule
    assert len(sched) == 40 and {d["kind"] for d in sched} == {0, 1}
    adj = BC.adjacency(e.n, e.edges)
    for d in sched:
        partner = [int(x) for x in d["partner"]]
        assert partner in IC.expected_partners(d, e.n, nbrs, zeros, skip, shuffled)
        assert np.array_equal(d["y"], adj[d["start"], d["partner"]])
        assert len(set(partner)) == len(partner) and d["start"] not in partner
        if d["kind"] == 1:
            assert not d["y"].any() and len(partner) <= IC.NONINF_SETSIZE
    # the default chance of a non-informative step, 1e-4, shows none in 40 iterations
    e = _engine(graph_files, assort_sets, seed=5)
    e.step(40)
    assert {d["kind"] for d in e.schedule} == {0} and e.schedule[0]["scale"] == e.n / 2.0


def test_step_sizes_follow_the_closed_forms():
    assert IC.rho_node(0) == 1025.0 ** -0.5 and IC.rho_node(7) == 1032.0 ** -0.5
    assert IC.rho_node(3, nodetau0=0.0, nodekappa=0.75) == 4.0 ** -0.75 and IC.rho_node(0, nodetau0=0.0) == 1.0
    assert IC.rho_lambda(0) == 1026.0 ** -0.9 and IC.rho_lambda(5, tau0=10.0, kappa=0.6) == 17.0 ** -0.6
    assert IC.scale_of(0, 75) == 37.5 and IC.scale_of(1, 75) == 75.0 * 75.0 / (2 * 1e-4 * 200)


def test_the_shuffle_comes_before_the_heldout_sampler(graph_files, assort_sets):
    """FastAMM's constructor shuffles the nodes first (src/fastamm.cc:85): the held-out sets differ from a -batch run's"""
    e = _engine(graph_files, assort_sets)
    b = BatchEngine(graph_files["assort"], N, K, heldout_ratio=0.1)
    assert e.heldout.shape == b.heldout.shape and not np.array_equal(e.heldout, b.heldout)
    held = [tuple(int(x) for x in r) for r in e.heldout]
    assert len(set(held)) == len(held) and not set(held) & {tuple(int(x) for x in r) for r in e.validation}


def test_cli_infset_host_loops(graph_files, tmp_path):
    common = ["-file", graph_files["assort"], "-n", "75", "-k", "4", "-heldout-ratio", "0.1"]
    work = tmp_path / "work"
    work.mkdir()
    r = _cli(common + ["-infset", "-host-loops", "-rfreq", "50", "-max-iterations", "120"], tmp_path, cwd=str(work))
    assert r.returncode != 0 and "error: cannot find neighbors.bin from preprocessing the network" in r.stderr
    assert not list(tmp_path.rglob("heldout.txt"))
    r = _cli(common + ["-preprocess"], tmp_path)
    assert r.returncode == 0, r.stderr
    d = tmp_path / "n75-k4-mmsb-infset"
    os.replace(d / "neighbors.bin", work / "neighbors.bin")
    r = _cli(common + ["-infset", "-host-loops", "-rfreq", "50", "-max-iterations", "120"], tmp_path, cwd=str(work))
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["n75-k4-mmsb-infset", "work"]
    for f in ("param.txt", "heldout-pairs.txt", "validation-pairs.txt", "precision-pairs.txt", "heldout.txt", "validation.txt",
              "max.txt", "gamma.txt", "lambda.txt", "groups.txt", "communities.txt", "summary.txt"):
        assert (d / f).exists(), f
    assert not (d / "heldout-edges.txt").exists()
    rows = np.loadtxt(d / "heldout.txt")
    assert rows.shape == (3, 11) and list(rows[:, 0]) == [0, 50, 100]
    gam = np.loadtxt(d / "gamma.txt")
    assert gam.shape == (75, 6) and np.all(gam[:, 2:] > 0)
    assert np.loadtxt(d / "lambda.txt").shape == (4, 3)
    param = (d / "param.txt").read_text()
    assert "inf_epsilon: 0.0001" in param and "noninf_setsize: 200" in param and "reportfreq: 50" in param
    (work / "neighbors.bin").write_bytes((work / "neighbors.bin").read_bytes()[:-4])         # a file of another graph
    r = _cli(common + ["-infset", "-host-loops"], tmp_path, cwd=str(work))
    assert r.returncode != 0 and "neighbors.bin does not belong to this network" in r.stderr


REFUSALS = [([mode, other] + extra, other) for mode in ("-infset", "-preprocess")
            for other, extra in (("-link-sampling", []), ("-findk", []), ("-batch", []), ("-batch-gpu", []), ("-gml", []),
                                 ("-lcstats", []), ("-rnode", []), ("-rpair", []), ("-stratified", []), ("-kshard", []),
                                 ("-sharded", []), ("-minibatch", ["8"]), ("-predict-pairs", ["x"]), ("-recommend", ["3"]),
                                 ("-rank-pairs", ["x"]), ("-rank-heldout", []), ("-adamic-adar", []), ("-gpus", ["2"]),
                                 ("-scale", ["2"]))]


@pytest.mark.parametrize("flags,named", REFUSALS)
def test_cli_refusals(tmp_path, flags, named):
    named = "-batch" if named == "-batch-gpu" else named
    for order in (flags, flags[::-1] if len(flags) == 2 else flags):
        r = _cli(["-file", "x", "-n", "75", "-k", "4"] + order, tmp_path, timeout=60)
        assert r.returncode == 2 and named in r.stderr and flags[0] in r.stderr, (order, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


def test_cli_limits_are_checked_before_anything_is_read(tmp_path):
    for size, limit in ((["-n", "75", "-k", "300"], "256"), (["-n", "40000", "-k", "4"], "32768")):
        r = _cli(["-file", "x"] + size + ["-infset"], tmp_path, timeout=60)
        assert r.returncode == 2 and limit in r.stderr and "-infset" in r.stderr, r.stderr
    assert not list(tmp_path.iterdir())
    r = _cli(["-help"], tmp_path)
    for flag in ("-infset", "-preprocess", "-host-loops"):
        assert "\t%s\t" % flag in r.stdout


def test_cli_without_a_gpu_fails_loudly_after_the_host_setup(graph_files, assort_sets, tmp_path):
    if _have_gpu():
        pytest.skip("GPU present")
    r = _cli(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-infset", "-heldout-ratio", "0.1"], tmp_path, timeout=120,
             cwd=os.path.dirname(assort_sets))
    assert r.returncode != 0 and "no CPU path" in r.stderr
    assert (tmp_path / "n75-k4-mmsb-infset" / "heldout-pairs.txt").exists()
    assert not list(tmp_path.rglob("gamma.txt")) and not list(tmp_path.rglob("heldout.txt"))
    with pytest.raises(_svils.SvilsError) as ei:
        _engine(graph_files, assort_sets, on_device=True)
    assert ei.value.code == -2 and "no CPU path" in str(ei.value)


def test_star_entry_point_refuses_a_null_handle():
    L = _svils.load()
    assert "svils_batch_step_star" in _svils.EXPORTS and "svils_batch_set_star_chain" in _svils.EXPORTS
    null = -1 if _have_gpu() else -2
    one, node, y = np.ones(1), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint8)
    off = np.array([0, 1], dtype=np.uint64)
    assert L.svils_batch_step_star(None, 1, node.ctypes.data, off.ctypes.data, node.ctypes.data, y.ctypes.data, one.ctypes.data,
                                   one.ctypes.data, one.ctypes.data, one.ctypes.data) == null
    assert L.svils_batch_step_star(None, 1, None, None, None, None, None, None, None, None) == null
    assert L.svils_batch_set_star_chain(None, 4) == null
    if not _have_gpu():
        assert b"no CPU path" in L.svils_last_error()
    assert L.svils_abi_version() == 8
