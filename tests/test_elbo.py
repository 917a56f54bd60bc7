"""-logl without a device: the restatement of tests/elbo_cases.py against its literal scalar loops, the host loops of
svinet_amd/host/mmsbbatch.cc (MMSBBatch::elbo) against the restatement at rtol 1e-9, the rows of logl.txt the CLI writes
for -batch / -rnode / -rpair / -infset with -host-loops, the -accuracy rule that writes done.txt, and the answers of the
two new entry points of include/svils.h where there is no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import batch_cases as BC
import elbo_cases as EC
from svinet_amd import _svils, host_api
from svinet_amd.host_api import BatchEngine, InfsetEngine, SampledEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
ERR_ARG, ERR_DEVICE = -1, -2


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _cli(args, tmp, timeout=300, cwd=None):
    return subprocess.run([SVINET] + args + ["-outdir", str(tmp)], capture_output=True, text=True, timeout=timeout, cwd=cwd)


def _skip(e):
    return {tuple(int(x) for x in r) for r in e.heldout} | {tuple(int(x) for x in r) for r in e.validation}


def _planted_state(n, k, blocks, seed, sweeps):
    """a planted graph, a Gamma(100, 0.01) start, `sweeps` batch sweeps of the oracle, a few skipped pairs"""
    from oracle import batch_oracle as B
    rs = np.random.RandomState(seed)
    links = BC.planted_links(n, blocks, 0.5, 0.05, seed)
    adj = BC.adjacency(n, links)
    skip = {(0, 1), (0, n - 1), (1, 3), (n - 2, n - 1)}
    gamma, lam = rs.gamma(100.0, 0.01, size=(n, k)), np.tile([1.0, 1.0], (k, 1))
    for _ in range(sweeps):
        gamma, lam = B.sweep(gamma, lam, adj, skip, 1.0 / k, (1.0, 1.0))
    return gamma, lam, adj, skip


@pytest.mark.parametrize("n,k,sweeps", [(5, 3, 1), (12, 4, 2)])
def test_restatement_equals_the_literal_loops(n, k, sweeps):
    """the vector form (S1 S2 - sum phi1 phi2 for the g != h loop, gammaln) against one scalar at a time"""
    gamma, lam, adj, skip = _planted_state(n, k, 2, 7 + n, sweeps)
    e = EC.Elbo(gamma, lam, adj, skip, 1.0 / k, (1.0, 1.0))
    assert len(e.rounds) == n * (n - 1) // 2 - len(skip)
    G, P, N = EC.literal(gamma, lam, adj, skip, 1.0 / k, (1.0, 1.0))
    np.testing.assert_allclose([e.G, e.P, e.N], [G, P, N], rtol=1e-12)
    assert e.total == e.G + e.P + e.N and e.P < 0 and e.N < 0


def test_exact_zero_phi_adds_zero():
    """gamma entries of 1e-3 beside entries of 50: some phi are exactly 0, every normaliser stays > 0, the bound is finite
    and the vector and the literal form agree on it"""
    n, k = 12, 4
    rs = np.random.RandomState(3)
    gamma = np.where(rs.random_sample((n, k)) < 0.5, 1e-3, 50.0)
    gamma[:, 0] = 50.0
    _, lam, adj, skip = _planted_state(n, k, 2, 19, 1)
    e = EC.Elbo(gamma, lam, adj, skip, 1.0 / k, (1.0, 1.0))
    assert e.phi_min == 0.0 and np.isfinite(e.total)
    np.testing.assert_allclose([e.G, e.P, e.N], EC.literal(gamma, lam, adj, skip, 1.0 / k, (1.0, 1.0)), rtol=1e-12)


def test_host_loops_match_the_restatement_on_assort(graph_files):
    e = BatchEngine(graph_files["assort"], 75, 4, heldout_ratio=0.1)
    for sweeps in range(3):
        r = EC.Elbo(e.gamma, e.lam, BC.adjacency(e.n, e.edges), _skip(e), 0.25, e.eta)
        if sweeps == 2:
            EC.check_conditions(r)
        for x in r.pair_terms, r.node_terms:
            assert np.all(x < 0)
        EC.assert_parts(e.elbo(), r)
        e.sweep()
    e.close()


def test_host_loops_match_the_restatement_on_a_planted_graph_with_skipped_pairs(tmp_path):
    n, k = 96, 9
    links = BC.planted_links(n, 3, 0.4, 0.03, seed=96)
    e = BatchEngine(BC.write_graph(tmp_path / "g.txt", links), n, k, heldout_ratio=0.1)
    assert e.n == n and len(_skip(e)) > 20
    for _ in range(3):
        e.sweep()
    r = EC.Elbo(e.gamma, e.lam, BC.adjacency(n, e.edges), _skip(e), 1.0 / k, e.eta)
    EC.check_conditions(r)
    before = e.gamma, e.lam
    EC.assert_parts(e.elbo(), r)
    assert np.array_equal(before[0], e.gamma) and np.array_equal(before[1], e.lam)   # the state is only read
    assert e.elbo() == e.elbo()
    e.close()


def _rows(path):
    return [line.split("\t") for line in open(path).read().splitlines()]


def _assert_rows(path, engine_rows):
    """1 + reports rows, each the engine's value at %.5f"""
    rows = _rows(path)
    assert len(rows) == len(engine_rows) >= 2, (rows, engine_rows)
    for row, (it, s) in zip(rows, engine_rows):
        assert len(row) == 3 and int(row[0]) == int(it) and int(row[1]) >= 0 and row[2] == "%.5f" % s, (row, it, s)


COMMON = ["-n", "75", "-k", "4", "-heldout-ratio", "0.1"]


def test_cli_batch_logl_rows(graph_files, tmp_path):
    """-batch -logl -max-iterations 3: the row of the constructor and one per report (four sweeps: the run ends once the
    count exceeds the bound)"""
    r = _cli(["-file", graph_files["assort"]] + COMMON + ["-batch", "-logl", "-no-stop", "-max-iterations", "3"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("approx. log likelihood = ") == 5
    e = BatchEngine(graph_files["assort"], 75, 4, heldout_ratio=0.1, logl=True)
    for _ in range(4):
        e.sweep()
        assert e.report() is False
    assert [int(x) for x in e.logl_rows[:, 0]] == [0, 1, 2, 3, 4]
    assert e.logl_rows[-1, 1] == e.elbo()[0]
    _assert_rows(tmp_path / "n75-k4-mmsb-batch" / "logl.txt", e.logl_rows)
    assert not (tmp_path / "n75-k4-mmsb-batch" / "done.txt").exists()   # the rule of done.txt is -accuracy's
    e.close()


@pytest.mark.parametrize("flags,mode,name", [(["-rnode"], "rnode", "Urnode"), (["-rpair"], "rpair", "Urpair")])
def test_cli_sampled_host_loops_logl_rows(graph_files, tmp_path, flags, mode, name):
    r = _cli(["-file", graph_files["assort"]] + COMMON + ["-rfreq", "2"] + flags +
             ["-host-loops", "-logl", "-no-stop", "-max-iterations", "3"], tmp_path)
    assert r.returncode == 0, r.stderr
    e = SampledEngine(graph_files["assort"], 75, 4, mode, heldout_ratio=0.1, logl=True)
    for _ in range(2):
        e.step(2)
        e.report()
    assert [int(x) for x in e.logl_rows[:, 0]] == [0, 2, 4]
    _assert_rows(tmp_path / ("n75-k4-mmsb-" + name) / "logl.txt", e.logl_rows)
    r = EC.Elbo(e.gamma, e.lam, BC.adjacency(e.n, e.edges), _skip(e), 0.25, e.eta)
    EC.assert_parts(e.elbo(), r)
    assert e.logl_rows[-1, 1] == e.elbo()[0]
    e.close()


def test_cli_infset_host_loops_logl_rows(graph_files, tmp_path):
    work = tmp_path / "work"
    work.mkdir()
    host_api.preprocess(graph_files["assort"], 75, str(work / "neighbors.bin"))
    r = _cli(["-file", graph_files["assort"]] + COMMON + ["-infset", "-host-loops", "-logl", "-no-stop", "-rfreq", "2",
                                                         "-max-iterations", "3"], tmp_path, cwd=str(work))
    assert r.returncode == 0, r.stderr
    e = InfsetEngine(graph_files["assort"], 75, 4, str(work / "neighbors.bin"), heldout_ratio=0.1, logl=True)
    for _ in range(2):
        e.step(2)
        e.report()
    _assert_rows(tmp_path / "n75-k4-mmsb-infset" / "logl.txt", e.logl_rows)
    r = EC.Elbo(e.gamma, e.lam, BC.adjacency(e.n, e.edges), _skip(e), 0.25, e.eta)
    EC.assert_parts(e.elbo(), r)
    e.close()


def test_without_logl_no_row_is_written(graph_files, tmp_path):
    """without -logl a run leaves the files it always left: logl.txt is the empty file the constructor has always
    created (as the reference's does, src/mmsbinfer.cc:153), no row, no line on stdout; an engine without logl keeps none"""
    r = _cli(["-file", graph_files["assort"]] + COMMON + ["-batch", "-no-stop", "-max-iterations", "2"], tmp_path)
    assert r.returncode == 0, r.stderr
    d = tmp_path / "n75-k4-mmsb-batch"
    assert (d / "logl.txt").read_bytes() == b"" and "approx. log likelihood" not in r.stdout
    assert not (d / "done.txt").exists()
    e = BatchEngine(graph_files["assort"], 75, 4, heldout_ratio=0.1)
    e.sweep()
    e.report()
    assert e.logl_rows.shape == (0, 2)
    e.close()


def _rule(rows, n):
    """the rule of src/mmsbinfer.cc:2062-2081 over the rows of logl.txt -> the rows at which it fires"""
    prev, fired = -2147483647.0, []
    for row in rows:
        it, w = int(row[0]), float(row[2])
        if (it > n or it > 5000) and w > prev and prev != 0 and abs((w - prev) / prev) < 1e-5:
            fired.append(row)
        prev = w
    return fired


def test_accuracy_rule_writes_done_txt(graph_files, tmp_path):
    """-batch -accuracy -logl -no-stop -max-iterations 200 on assort-75-4 (no held-out pairs under -accuracy): the rule,
    applied here to the rows of logl.txt (at the file's five decimals: the bound is of the order 1e3, so the rule's 1e-5
    relative step is three orders above the rounding), names the rows that fire; done.txt holds the last of them"""
    r = _cli(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-batch", "-accuracy", "-logl", "-no-stop",
              "-max-iterations", "200"], tmp_path)
    assert r.returncode == 0, r.stderr
    d = tmp_path / "n75-k4-mmsb-batch"
    rows = _rows(d / "logl.txt")
    assert [int(x[0]) for x in rows] == list(range(202))
    fired = _rule(rows, 75)
    assert fired, "the rule did not fire within 200 sweeps from the engine's start"
    assert int(fired[0][0]) > 75
    assert _rows(d / "done.txt") == [fired[-1]]
    w = np.array([float(x[2]) for x in rows])
    assert np.all(np.diff(w[1:]) > -1e-6 * np.abs(w[1:-1]))   # coordinate ascent: the bound does not fall


def test_logl_is_accepted_and_without_effect_elsewhere(tmp_path):
    """-logl with -link-sampling parses (the reference's LinkSampling never reads it); -help names it"""
    r = _cli(["-file", "x", "-n", "75", "-k", "4", "-link-sampling", "-logl", "-help"], tmp_path, timeout=60)
    assert r.returncode == 0 and "\t-logl\t" in r.stdout
    assert not list(tmp_path.iterdir())


def test_entry_points_without_a_handle():
    L = _svils.load()
    null = ERR_ARG if _have_gpu() else ERR_DEVICE
    parts = (C.c_double * 4)()
    assert L.svils_batch_elbo(None, parts, None, None) == null
    assert L.svils_batch_elbo(None, None, None, None) == null
    assert L.svils_batch_set_elbo_tiles(None, 1) == null
    assert L.svils_batch_set_elbo_tiles(None, 1 << 20) == null
    if not _have_gpu():
        assert b"no CPU path" in L.svils_last_error()
        with pytest.raises(_svils.SvilsError) as ei:
            _svils.Batch(10, 4, 0.25, (1.0, 1.0))
        assert ei.value.code == ERR_DEVICE
