"""-m "not gpu": the -single engine (the single-membership stochastic blockmodel, svinet_amd/host/sbm.cc) on the host loops
against the numpy restatement of tests/sbm_cases.py; the conditions every SBM case has to meet, asserted on the restatement
alone; the sample draws, the files, the command line's refusals, and the device library's answers without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sbm_cases as S
from conftest import GOLDEN, ROOT
from svinet_amd import _svils
from svinet_amd.host_api import SbmEngine

ASSORT = os.path.join(GOLDEN, "graphs", "assort-75-4.txt")
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
ERR_ARG, ERR_DEVICE, ERR_UNSUPPORTED = -1, -2, -4
B = _svils.sbm_variant(4)[1]


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _engine_case(eng):
    """the engine's graph, samples and start as a case of the restatement"""
    return S.Case("engine", eng.n, eng.k, np.sort(eng.edges, axis=1), eng.skip, (eng.phi, eng.gamma, eng.lam))


@pytest.fixture(scope="module")
def planted_files(tmp_path_factory):
    """the prototype's three graphs as edge lists: (path, n, K, seed)"""
    d = tmp_path_factory.mktemp("sbm")
    out = []
    for n, K, seed in ((61, 4, 1), (97, 7, 2), (130, 3, 3)):
        links, _ = S.planted(n, K, seed)
        path = os.path.join(str(d), "planted-%d.txt" % n)
        np.savetxt(path, links, fmt="%d", delimiter="\t")
        out.append((path, n, K, seed))
    return out


# ---- the case conditions, on the restatement alone -------------------------------------------------------------------------
def _msums_of(case):
    """the msums of the E-step and of every whole iteration a device test compares the case over"""
    ms = list(case.estep()[2])
    if S.iters_compared(case):
        for m in case.iterate(S.iters_compared(case))[4]:
            ms += list(m)
    return np.array(ms)


@pytest.mark.parametrize("case", S.all_cases(B), ids=lambda c: c.name)
def test_no_pass_count_hinges_on_rounding(case):
    """every pass's msum of every case lies outside [0.009, 0.011]: 10 % from the threshold of the exit rule"""
    ms = _msums_of(case)
    assert not np.any((ms >= 0.009) & (ms <= 0.011)), ms


@pytest.mark.parametrize("case", S.all_cases(B), ids=lambda c: c.name)
def test_estep_does_not_amplify_a_perturbation(case):
    """a start moved by 1e-13 relative ends the E-step within 1e-9 of the unmoved one: a trajectory comparison at 1e-7 is sound"""
    rng = np.random.RandomState(5)
    phi = case.phi * (1.0 + 1e-13 * rng.uniform(-1, 1, case.phi.shape))
    phi /= phi.sum(axis=1, keepdims=True)
    T, Y = case.masks()
    got, npass, _ = S.estep(phi, case.gamma, case.lam, T, Y)
    ref, rpass, _ = case.estep()
    assert npass == rpass
    np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-200)


@pytest.mark.parametrize("case", [c for c in S.all_cases(B) if S.iters_compared(c)], ids=lambda c: c.name)
def test_iterations_do_not_amplify_a_perturbation(case):
    """the same over the whole iterations the device tests compare: the same pass counts, phi, gamma and lambda within 1e-9"""
    niter = S.iters_compared(case)
    rng = np.random.RandomState(5)
    phi = case.phi * (1.0 + 1e-13 * rng.uniform(-1, 1, case.phi.shape))
    phi /= phi.sum(axis=1, keepdims=True)
    T, Y = case.masks()
    got = S.iterate(phi, case.gamma, case.lam, case.eta, T, Y, niter)
    ref = case.iterate(niter)
    assert got[3] == ref[3]
    for g, r in zip(got[:3], ref[:3]):
        np.testing.assert_allclose(g, r, rtol=1e-9, atol=1e-200)


def test_the_matrix_has_both_edges_of_every_class():
    """the (V, W) classes of K = 2 .. SBM_MAX_K by the documented rules (no device library asked): nine classes, both edges of
    each in S.MATRIX"""
    by = {}
    for k in range(2, _svils.SBM_MAX_K + 1):
        by.setdefault(((k + 63) // 64, S.row_lanes(k)), []).append(k)
    assert sorted(by) == [(1, 2), (1, 4), (1, 8), (1, 16), (1, 32), (1, 64), (2, 64), (3, 64), (4, 64)]
    ks = [k for k, _ in S.MATRIX]
    assert sorted({k for v in by.values() for k in (v[0], v[-1])}) == ks
    assert [c.n for c in S.matrix_cases()] == [S.MATRIX_N] * len(ks) and S.MATRIX_N > 7 * B


@pytest.mark.parametrize("n,K", S.HUBS)
def test_hub_cases_are_what_they_claim(n, K):
    case = S.hub_case(n, K, B)
    T, Y = case.masks()
    hubs = S.hub_nodes(n, B)
    assert hubs[0] == 0 and hubs[2] == n - 1 and 0 < hubs[1] % B < B - 1 and B <= hubs[1] < n - B   # mid-block, blocks on both sides
    for h in hubs:
        assert Y[h].sum() == n - 1 > 2 * 64                           # split_row: three trips of 64 entries
    assert Y.sum(axis=1).max() == n - 1 and np.array_equal(Y, Y.T)
    srow = np.flatnonzero(~T[1] & (np.arange(n) != 1))                # node 1's skip row: in hub 0's block
    assert 1 < B and srow.shape[0] == S.HUB_SKIPS > 64
    assert 0 < Y[1, srow].sum() < srow.shape[0]                       # both y values
    assert (srow >= B).sum() > 64 and ((srow > 1) & (srow < B)).any()   # beyond the block (a second trip of the gather), and in it
    assert (~T).sum() == 2 * S.HUB_SKIPS + n                          # nothing else is skipped
    assert case.iterate(S.LOOP_ITERS)[3] == {4: [4, 10], 65: [5, 4]}[K]


@pytest.mark.parametrize("d", S.DENSE, ids=lambda d: "n%d-k%d" % d[:2])
def test_dense_cases_are_what_they_claim(d):
    case = S.dense_case(*d)
    T, Y = case.masks()
    assert case.skip.shape[0] == d[4] == len({tuple(p) for p in case.skip.tolist()}) and np.all(case.skip[:, 0] < case.skip[:, 1])
    y = case.y_of(case.skip)
    assert min(y.sum(), (1 - y).sum()) > 500                          # both y values, many of each
    assert abs(case.links.shape[0] - {260: 18900, 200: 10500}[case.n]) < 500
    rpasses = case.iterate(S.LOOP_ITERS)[3]
    assert rpasses == {260: [4, 3], 200: [10, 3]}[case.n]
    assert case.iterate(S.LOOP_ITERS)[2].min() > 0.9                  # lambda stays away from 0: rtol on it means something


@pytest.mark.parametrize("n,K,seed", S.RINGS)
def test_ring_cases_are_what_they_claim(n, K, seed):
    case = S.ring_case(n, K, seed)
    assert case.links.shape == (n, 2) and np.all(case.links[:, 0] < case.links[:, 1])
    deg = np.bincount(case.links.ravel(), minlength=n)
    assert np.all(deg == 2)
    sk = [tuple(p) for p in case.skip.tolist()]
    links = {tuple(p) for p in case.links.tolist()}
    y = np.array([p in links for p in sk])
    assert len(set(sk)) == len(sk) and np.all(case.skip[:, 0] < case.skip[:, 1])
    assert y.sum() == S.RING_SKIPS // 2 and 0.9 * S.RING_SKIPS // 2 <= (~y).sum() <= S.RING_SKIPS // 2
    np.testing.assert_allclose(case.phi.sum(axis=1), 1.0, rtol=1e-12)


@pytest.mark.parametrize("n,K,seed", [(61, 7, 1), (130, 4, 2), (61, 256, 1)])
def test_prefix_sum_restatement_against_the_masks(n, K, seed):
    """pair_sums_prefix, mstep_prefix and elbo_prefix (the references at sizes the masks cannot reach) against the mask-based
    M-step and bound, at the start and after one iteration"""
    import sbm_elbo_cases as E
    case = S.planted_case(n, K, seed)
    T, Y = case.masks()
    for phi, gamma, lam in ((case.phi, case.gamma, case.lam), case.iterate(1)[:3]):
        rgamma, rlam = S.mstep(phi, case.eta, T, Y)
        ggamma, glam = S.mstep_prefix(phi, case.eta, case.links, case.skip)
        np.testing.assert_allclose(ggamma, rgamma, rtol=1e-12)
        np.testing.assert_allclose(glam, rlam, rtol=1e-12)
        a, b, n1, n0 = S.pair_sums_prefix(phi, case.links, case.skip)
        tri = np.triu(T, 1)
        assert n1 == (tri & Y).sum() and n0 == (tri & ~Y).sum()
        ref = E.elbo(phi, gamma, lam, case.eta, T, Y)
        got = E.elbo_prefix(phi, gamma, lam, case.eta, case.links, case.skip)
        np.testing.assert_allclose(got[1], ref[1], rtol=1e-12)        # P: addends of one sign
        np.testing.assert_allclose(got[4], ref[4], rtol=1e-12)        # A
        for g, r in zip(got[:4], ref[:4]):
            assert abs(g - r) <= 1e-12 * ref[4]


def test_restatement_split_algebra_is_not_what_it_uses():
    """the reference sums of the restatement are direct: one E-step node update and the M-step against literal double loops"""
    c = S.planted_case(61, 4, 1)
    T, Y = c.masks()
    elogpi, elogbeta = S.elog(c.gamma, c.lam)
    K, p = c.K, 7
    a = elogpi.copy()
    for q in range(c.n):
        if T[p, q]:
            t = 0 if Y[p, q] else 1
            a += (1 - c.phi[q]) * elogbeta[K, t] + c.phi[q] * elogbeta[:K, t]
    first = S.estep(np.roll(c.phi, -p, axis=0), c.gamma, c.lam, np.roll(np.roll(T, -p, 0), -p, 1), np.roll(np.roll(Y, -p, 0), -p, 1), 1)[0][0]
    np.testing.assert_allclose(first, np.exp(a - a.max()) / np.exp(a - a.max()).sum(), rtol=1e-12)
    gamma, lam = S.mstep(c.phi, c.eta, T, Y)
    ref = c.eta.copy()
    for i in range(c.n):
        for j in range(i + 1, c.n):
            if T[i, j]:
                v = c.phi[i] * c.phi[j]
                ref[:K, 0 if Y[i, j] else 1] += v
                ref[K, 0 if Y[i, j] else 1] += (1 - v).sum()
    np.testing.assert_allclose(lam, ref, rtol=1e-12)
    np.testing.assert_allclose(gamma, S.ALPHA + c.phi.sum(0), rtol=1e-14)


# ---- the host loops against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
def test_host_loops_against_the_restatement(planted_files, which):
    path, n, K, seed = planted_files[which]
    eng = SbmEngine(path, n, K, seed=seed, heldout_ratio=0.05, on_device=False)
    assert eng.n == n and eng.iter == 0
    case = _engine_case(eng)
    case.eta = eng.eta
    assert np.array_equal(eng.eta[:K], np.ones((K, 2))) and np.array_equal(eng.eta[K], [0.0001, 1.0])
    T, Y = case.masks()
    ms_all = []
    phi, gamma, lam = case.phi, case.gamma, case.lam
    hv = np.concatenate([eng.heldout, eng.validation])
    for it in range(2):
        rphi, rpass, rms = S.estep(phi, gamma, lam, T, Y)
        assert not np.any((rms >= 0.009) & (rms <= 0.011)), rms       # the case conditions hold for the engine's own draws
        ms_all.append(rms)
        gamma, lam = S.mstep(rphi, case.eta, T, Y)
        phi = rphi
        eng.sweep()
        assert eng.iter == it + 1 and eng.passes == rpass
        np.testing.assert_allclose(eng.msums, rms, rtol=1e-9)
        np.testing.assert_allclose(eng.phi, phi, rtol=1e-9, atol=1e-200)
        np.testing.assert_allclose(eng.gamma, gamma, rtol=1e-9)
        np.testing.assert_allclose(eng.lam, lam, rtol=1e-9)
    rows = eng.rows
    assert rows.shape == (6, 8) and list(rows[:, 0]) == [0, 1] * 3 and list(rows[:, 1]) == [0, 0, 0, 0, 1, 1]
    for w, pairs in ((0, eng.heldout), (1, eng.validation)):          # the rows after the last sweep: the means over the sample
        order = np.lexsort((pairs[:, 1], pairs[:, 0]))                # (summed in the order of a std::map of pairs)
        y = case.y_of(pairs[order])
        ll = S.pair_loglik(phi, lam, pairs[order], y)
        np.testing.assert_allclose(rows[4 + w, [2, 4, 6]], [ll.mean(), ll[y == 0].mean(), ll[y == 1].mean()], rtol=1e-9)
        assert list(rows[4 + w, [3, 5, 7]]) == [len(y), (y == 0).sum(), (y == 1).sum()]
    assert hv.shape[0] == rows[0, 3] + rows[1, 3]


def test_lfr_engine_case(graph_files):
    """the engine case of tests/test_gpu_sbm.py (the LFR golden graph, two iterations): its conditions on the restatement, and
    the host loops -- what the device runs are held to there -- against the restatement.  Both are nine and four Gauss-Seidel passes
    of sums over 1000 partners taken in different orders (numpy's pairwise sums, the loops' running ones): they are held to the
    1e-7 of a trajectory comparison, not to the 1e-9 of the small cases above"""
    eng = SbmEngine(graph_files["lfr"], 1000, 28, seed=S.LFR_SEED, on_device=False)
    case = _engine_case(eng)
    case.eta = eng.eta
    rphi, rgamma, rlam, rpasses, rms = case.iterate(2)
    ms = np.concatenate(rms)
    assert not np.any((ms >= 0.009) & (ms <= 0.011)), ms
    assert rpasses == [9, 4]
    for it in range(2):
        eng.sweep()
        assert eng.passes == rpasses[it]
        np.testing.assert_allclose(eng.msums, rms[it], rtol=1e-7)
    np.testing.assert_allclose(eng.phi, rphi, rtol=1e-7, atol=1e-200)
    np.testing.assert_allclose(eng.gamma, rgamma, rtol=1e-7)
    np.testing.assert_allclose(eng.lam, rlam, rtol=1e-7)


def test_set_state_on_the_host_loops():
    eng = SbmEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    phi, gamma, lam = S.peaked_state(eng.n, 4)
    eng.set_state(phi, gamma, lam)
    case = S.Case("assort", eng.n, 4, np.sort(eng.edges, axis=1), eng.skip, (phi, gamma, lam))
    rphi, rpass, rms = case.estep()
    assert not np.any((rms >= 0.009) & (rms <= 0.011))
    eng.sweep()
    assert eng.passes == rpass
    np.testing.assert_allclose(eng.phi, rphi, rtol=1e-9, atol=1e-200)


# ---- the samples ---------------------------------------------------------------------------------------------------------
def test_sample_draws():
    eng = SbmEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    links = {tuple(sorted(e)) for e in eng.edges.tolist()}
    p = int(0.1 * len(links)) // 2
    for name, pairs, n0, n1 in (("heldout", eng.heldout, p, p), ("validation", eng.validation, p, p), ("precision", eng.precision, 100, 10)):
        y = np.array([tuple(e) in links for e in pairs.tolist()])
        assert pairs.shape == (n0 + n1, 2) and (y == 0).sum() == n0 and (y == 1).sum() == n1, name
        assert np.all(pairs[:, 0] < pairs[:, 1]) and pairs.max() < eng.n
    everything = [tuple(e) for e in eng.skip.tolist()]
    assert len(set(everything)) == len(everything) == 4 * p + 110                  # no pair in two samples
    assert {tuple(e) for e in eng.precision.tolist()} <= set(everything)          # the precision pairs are skipped too
    again = SbmEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    assert np.array_equal(again.skip, eng.skip) and np.array_equal(again.phi, eng.phi)
    other = SbmEngine(ASSORT, 75, 4, seed=7, heldout_ratio=0.1, on_device=False)
    assert not np.array_equal(other.skip, eng.skip)
    np.testing.assert_allclose(eng.phi.sum(axis=1), 1.0, rtol=1e-12)
    assert eng.gamma.shape == (4,) and eng.lam.shape == (5, 2) and np.all(eng.lam > 0) and abs(eng.gamma.mean() - 25) < 5


# ---- the command line ------------------------------------------------------------------------------------------------------
def _run(args, cwd, timeout=120):
    return subprocess.run([SVINET] + args, capture_output=True, text=True, timeout=timeout, cwd=str(cwd))


def test_cli_host_loops_files(tmp_path):
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-single", "-host-loops", "-max-iterations", "2", "-heldout-ratio", "0.1"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert [p.name for p in tmp_path.iterdir()] == ["n75-k4-mmsb-sbm"]
    d = tmp_path / "n75-k4-mmsb-sbm"
    assert {p.name for p in d.iterdir()} == {"convergence.txt", "gamma.txt", "heldout-pairs.txt", "heldout.txt", "infer.log", "lambda.txt",
                                            "logl.txt", "modularity.txt", "network.dat", "param.txt", "phi.txt", "precision.txt",
                                            "time.txt", "validation-pairs.txt", "validation.txt"}
    e = SbmEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)   # the library engine is the command line's engine
    e.sweep()
    e.sweep()
    for f in ("heldout.txt", "validation.txt"):
        rows = [l.split("\t") for l in (d / f).read_text().splitlines()]
        assert [r[0] for r in rows] == ["0", "0", "1"] and all(len(r) == 11 for r in rows)
        for r in rows:   # iter, secs, mean, count, mean of the non-links, count, mean of the links, count, three weighted columns (0)
            assert int(r[3]) == int(r[5]) + int(r[7]) and all(len(r[c].split(".")[1]) == 9 for c in (2, 4, 6, 8, 9, 10))
            assert float(r[2]) < 0 and [float(r[c]) for c in (8, 9, 10)] == [0, 0, 0]
    want = e.rows[e.rows[:, 0] == 0]
    got = np.array([[float(c) for c in l.split("\t")] for l in (d / "heldout.txt").read_text().splitlines()])
    np.testing.assert_allclose(got[:, [2, 4, 6]], want[:, [2, 4, 6]], atol=6e-10)
    phi = np.loadtxt(d / "phi.txt")
    assert phi.shape == (75, 6) and list(phi[:, 0]) == list(range(75))
    np.testing.assert_allclose(phi[:, 2:], e.phi, atol=5.1e-6)
    lam = np.loadtxt(d / "lambda.txt")
    assert lam.shape == (5, 3) and list(lam[:, 0]) == [0, 1, 2, 3, 4]
    np.testing.assert_allclose(lam[:, 1:], e.lam, atol=5.1e-6)
    gamma = np.loadtxt(d / "gamma.txt")
    assert gamma.shape == (4, 2)
    np.testing.assert_allclose(gamma[:, 1], e.gamma, atol=5.1e-6)
    assert all(len(l.split("\t")[2].split(".")[1]) == 5 for l in (d / "phi.txt").read_text().splitlines())
    for f, want in (("heldout-pairs.txt", e.heldout), ("validation-pairs.txt", e.validation)):
        text = (d / f).read_text()
        assert text.endswith("\n\n") and np.array_equal(np.loadtxt(d / f, dtype=int), want.astype(int))


@pytest.mark.parametrize("args,word", [
    ([], "-max-iterations"),
    (["-max-iterations", "3", "-batch"], "-batch"),
    (["-max-iterations", "3", "-batch-gpu"], "-batch"),
    (["-max-iterations", "3", "-link-sampling"], "-link-sampling"),
    (["-max-iterations", "3", "-rnode"], "-rnode"),
    (["-max-iterations", "3", "-rpair"], "-rpair"),
    (["-max-iterations", "3", "-stratified"], "-stratified"),
    (["-max-iterations", "3", "-snode"], "-snode"),
    (["-max-iterations", "3", "-infset"], "-infset"),
    (["-max-iterations", "3", "-preprocess"], "-preprocess"),
    (["-max-iterations", "3", "-orig"], "-orig"),
    (["-max-iterations", "3", "-findk"], "-findk"),
    (["-max-iterations", "3", "-gml"], "-gml"),
    (["-max-iterations", "3", "-lcstats"], "-lcstats"),
    (["-max-iterations", "3", "-ppc"], "-ppc"),
    (["-max-iterations", "3", "-ppc-orig"], "-ppc-orig"),
    (["-max-iterations", "3", "-gen"], "-gen"),
    (["-max-iterations", "3", "-sparse-graph"], "-sparse-graph"),
    (["-max-iterations", "3", "-logl"], "-logl"),
    (["-max-iterations", "3", "-gpus", "2"], "-gpus"),
    (["-max-iterations", "3", "-kshard"], "-kshard"),
    (["-max-iterations", "3", "-minibatch", "10"], "-minibatch"),
    (["-max-iterations", "3", "-scale", "2"], "-scale"),
    (["-max-iterations", "3", "-load", "x/"], "-load"),
    (["-max-iterations", "3", "-predict-pairs", "x"], "-predict-pairs"),
    (["-max-iterations", "3", "-recommend", "3"], "-recommend"),
    (["-max-iterations", "3", "-rank-pairs", "x"], "-rank-pairs"),
    (["-max-iterations", "3", "-rank-heldout"], "-rank-heldout"),
    (["-max-iterations", "3", "-adamic-adar"], "-adamic-adar"),
    (["-max-iterations", "3", "-k", "257"], "SVILS_SBM_MAX_K"),
])
def test_cli_refusals_create_nothing(tmp_path, args, word):
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-single"] + args, tmp_path)
    assert r.returncode == 2 and word in r.stderr and "-single" in r.stderr, (r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


def test_cli_k_above_the_device_limit_runs_on_the_host_loops(tmp_path):
    r = _run(["-file", ASSORT, "-n", "75", "-k", "257", "-single", "-host-loops", "-max-iterations", "1", "-heldout-ratio", "0.1"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert np.loadtxt(tmp_path / "n75-k257-mmsb-sbm" / "lambda.txt").shape == (258, 3)


def test_cli_refuses_a_graph_too_small_for_the_samples(tmp_path):
    g = tmp_path / "tiny.txt"
    g.write_text("".join("%d\t%d\n" % (i, i + 1) for i in range(8)))   # 8 links: the precision sample alone wants 10
    r = _run(["-file", str(g), "-n", "9", "-k", "2", "-single", "-host-loops", "-max-iterations", "1"], tmp_path)
    assert r.returncode != 0 and "needs 10 links and 100 non-links" in r.stderr


def test_cli_device_run_without_a_gpu_fails_and_writes_no_model(tmp_path):
    if _have_gpu():
        pytest.skip("GPU present")
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-single", "-max-iterations", "2", "-heldout-ratio", "0.1"], tmp_path)
    assert r.returncode != 0 and "no CPU path" in r.stderr
    assert not (tmp_path / "n75-k4-mmsb-sbm" / "phi.txt").exists()


# ---- the device library without a device ---------------------------------------------------------------------------------
def test_library_answers_without_a_device():
    L = _svils.load()
    names = [e for e in _svils.EXPORTS if e.startswith("svils_sbm_")]
    assert len(names) == 13 and all(hasattr(L, e) for e in names) and L.svils_abi_version() == 8
    assert _svils.sbm_variant(2) == (1, B) and _svils.sbm_variant(64) == (1, B) and _svils.sbm_variant(65) == (2, B)
    assert _svils.sbm_variant(256) == (4, B) and B >= 1
    v = ctypes.c_uint32()
    assert L.svils_sbm_variant(1, ctypes.byref(v), ctypes.byref(v)) == ERR_ARG
    assert L.svils_sbm_variant(257, ctypes.byref(v), ctypes.byref(v)) == ERR_UNSUPPORTED and b"SVILS_SBM_MAX_K" in L.svils_last_error()
    h = ctypes.c_void_p()
    eta = S.eta_of(300)
    for n, k, alpha, want in ((1, 4, 0.5, ERR_ARG), (10, 1, 0.5, ERR_ARG), (10, 4, 0.0, ERR_ARG), (10, 257, 0.5, ERR_UNSUPPORTED)):
        assert L.svils_sbm_create(0, n, k, alpha, eta.ctypes.data, ctypes.byref(h)) == want and not h.value   # before any device call
    bad = S.eta_of(4)
    bad[2, 1] = 0.0
    assert L.svils_sbm_create(0, 10, 4, 0.5, bad.ctypes.data, ctypes.byref(h)) == ERR_ARG and b"eta[5]" in L.svils_last_error()
    assert L.svils_sbm_create(0, 10, 4, 0.5, None, ctypes.byref(h)) == ERR_ARG
    if _have_gpu():
        return
    assert L.svils_sbm_create(0, 10, 4, 0.5, eta.ctypes.data, ctypes.byref(h)) == ERR_DEVICE and b"no CPU path" in L.svils_last_error()
    assert L.svils_sbm_sweep(None, 1) == ERR_DEVICE and L.svils_sbm_estep(None, 1, None, None) == ERR_DEVICE
    with pytest.raises(_svils.SvilsError) as ei:
        SbmEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=True)
    assert ei.value.code == ERR_DEVICE and "no CPU path" in str(ei.value)
