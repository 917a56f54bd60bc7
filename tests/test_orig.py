"""-orig without a device: the instantiation table of the pair kernel (svils_orig_variant), the limit and null-handle
answers of every svils_orig_* entry point, the restatement tests/test_gpu_orig.py compares the device with
(tests/orig_cases.py) against a plain-loop transcription of the same source lines, the host engine with -host-loops
(samplers, starts, sweeps against the restatement, the one-orientation skip) and the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orig_cases as OC
from conftest import GOLDEN
from svinet_amd import _svils
from svinet_amd.host_api import OrigEngine

ERR_ARG, ERR_DEVICE, ERR_UNSUPPORTED = -1, -2, -4


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def test_variant_table_covers_every_k():
    L = _svils.load()
    seen = {}
    for k in range(2, _svils.ORIG_MAX_K + 1):
        kp, ppw, lds = _svils.orig_variant(k)
        assert kp % 16 == 0 and k <= kp < k + 16 and ppw == 16, (k, kp, ppw)
        seen.setdefault((kp, ppw, lds), []).append(k)
    assert sorted(kp for kp, _, _ in seen) == [16, 32, 48, 64]
    assert [lds for (kp, _, lds) in sorted(seen)] == [False, False, True, True]
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert L.svils_orig_variant(65, C.byref(a), C.byref(b), C.byref(c)) == ERR_UNSUPPORTED
    assert b"SVILS_ORIG_MAX_K" in L.svils_last_error()
    for k in (0, 1):
        assert L.svils_orig_variant(k, C.byref(a), C.byref(b), C.byref(c)) == ERR_ARG
    assert L.svils_orig_variant(4, None, None, None) == ERR_ARG


def test_limits_and_null_handles_do_not_need_a_device():
    L = _svils.load()
    h = C.c_void_p()
    create = lambda n, k, alpha=0.25: L.svils_orig_create(0, n, k, alpha, C.byref(h))
    assert create(1, 4) == ERR_ARG and create(10, 1) == ERR_ARG and create(10, 4, alpha=0.0) == ERR_ARG
    assert L.svils_orig_create(0, 10, 4, 0.25, None) == ERR_ARG
    assert create(10, 65) == ERR_UNSUPPORTED and b"SVILS_ORIG_MAX_K" in L.svils_last_error()
    assert create(_svils.ORIG_MAX_N + 1, 4) == ERR_UNSUPPORTED and b"SVILS_ORIG_MAX_N" in L.svils_last_error()
    assert _svils.ORIG_MAX_N == _svils.BATCH_MAX_N and _svils.ORIG_MAX_K == 64
    assert h.value is None
    # a null handle answers as the other tool handles do: "no HIP device" where there is none, else a bad argument
    null = ERR_ARG if _have_gpu() else ERR_DEVICE
    assert L.svils_orig_set_graph(None, None, 0, None, 0) == null
    assert L.svils_orig_set_launch_rows(None, 1) == null
    assert L.svils_orig_set_state(None, None, None) == null
    assert L.svils_orig_get_state(None, None, None) == null
    assert L.svils_orig_sweep(None, 1) == null
    assert L.svils_orig_pair_loglik(None, None, None, 0, None) == null
    assert L.svils_orig_get_stats(None, None, None, None, None, None) == null
    assert L.svils_orig_get_timing(None, None) == null
    if not _have_gpu():
        assert b"no CPU path" in L.svils_last_error()
    assert L.svils_orig_destroy(None) == 0


def test_no_cpu_fallback():
    if _have_gpu():
        pytest.skip("GPU present")
    with pytest.raises(_svils.SvilsError) as ei:
        _svils.Orig(10, 4, 0.25)
    assert ei.value.code == ERR_DEVICE and "no CPU path" in str(ei.value)


def _loop_sweep(gamma, beta, adj, skip, alpha):
    """the sweep pair by pair, scalar loops in the order of the source (:217-269 and update_phis_until_conv)"""
    n, K = gamma.shape
    elogpi = OC.dir_exp(gamma)
    gnext = np.full((n, K), alpha)
    num, tot = np.zeros((K, K)), np.zeros((K, K))
    rounds = []
    for p in range(n):
        for q in range(n):
            if p == q or (p, q) in skip:
                continue
            y = adj[p, q]
            logf = np.log(beta) if y else np.log(1.0 - beta)
            phi1, phi2 = np.full(K, 1.0 / K), np.full(K, 1.0 / K)
            old1, old2 = np.zeros(K), np.zeros(K)
            r = 0
            for i in range(OC.ONLINE_ITERATIONS):
                if i % 2 == 0:
                    old1, old2 = phi1.copy(), phi2.copy()
                n1 = np.exp(elogpi[p] + logf @ phi2)
                n2 = np.exp(elogpi[q] + logf @ phi1)
                n1, n2 = n1 / n1.sum(), n2 / n2.sum()
                v1, v2 = np.abs(n1 - old1).mean(), np.abs(n2 - old2).mean()
                phi1, phi2 = n1, n2
                r = i + 1
                if i % 2 == 1 and v1 < OC.MEAN_CHANGE_THRESH and v2 < OC.MEAN_CHANGE_THRESH:
                    break
            rounds.append(r)
            gnext[p] += phi1
            gnext[q] += phi2
            num += y * np.outer(phi1, phi2)
            tot += np.outer(phi1, phi2)
    return gnext, num / tot, np.array(rounds)


@pytest.mark.parametrize("k,n,seed,peaked", [(4, 21, 5, True), (17, 19, 6, True), (3, 12, 7, False)])
def test_restatement_against_plain_loops(k, n, seed, peaked):
    links, gamma, beta = (OC.peaked_state if peaked else OC.plain_state)(seed, n, k)
    adj = OC.adjacency(n, links)
    skip = {(0, 1), (3, 2), (n - 1, 0)}
    g, b, rounds, bad = OC.sweep(gamma, beta, adj, skip, 1.0 / k)
    lg, lb, lrounds = _loop_sweep(gamma, beta, adj, skip, 1.0 / k)
    assert not bad.any() and len(rounds) == n * (n - 1) - 3
    assert np.array_equal(rounds, lrounds)
    if peaked:
        assert len(set(rounds.tolist())) >= 4
    np.testing.assert_allclose(g, lg, rtol=1e-12)
    np.testing.assert_allclose(b, lb, rtol=1e-12)
    assert abs((g - 1.0 / k).sum() - 2 * len(rounds)) < 1e-9


def test_restatement_keeps_the_untransposed_second_side():
    """with an asymmetric beta the second side's update with the transposed matrix gives another beta: the quirk is visible"""
    links, gamma, beta = OC.peaked_state(8, 15, 3)
    adj = OC.adjacency(15, links)
    assert not np.allclose(beta, beta.T)
    b = OC.sweep(gamma, beta, adj, (), 1.0 / 3)[1]
    p, q = OC.ordered_pairs(15)
    elogpi = OC.dir_exp(gamma)
    logf = np.where(adj[p, q][:, None, None] == 1, np.log(beta), np.log(1 - beta))
    phi1 = phi2 = np.full((len(p), 3), 1.0 / 3)
    for _ in range(OC.ONLINE_ITERATIONS):   # the textbook update: transposed for the second side, no early exit
        n1 = np.exp(elogpi[p] + np.einsum("mgh,mh->mg", logf, phi2))
        n2 = np.exp(elogpi[q] + np.einsum("mgh,mg->mh", logf, phi1))
        phi1, phi2 = n1 / n1.sum(1, keepdims=True), n2 / n2.sum(1, keepdims=True)
    other = ((phi1 * adj[p, q][:, None]).T @ phi2) / (phi1.T @ phi2)
    assert np.abs(other - b).max() > 1e-3


def test_pair_loglik_restatement():
    links, gamma, beta = OC.plain_state(9, 10, 4)
    pi = gamma / gamma.sum(1, keepdims=True)
    s = sum(pi[2, g] * pi[7, h] * (1 - beta[g, h]) for g in range(4) for h in range(4))
    np.testing.assert_allclose(OC.pair_loglik(gamma, beta, [(2, 7)], [0]), [np.log(s)], rtol=1e-13)
    assert OC.pair_loglik(gamma, beta, [(2, 7)], [1])[0] != OC.pair_loglik(gamma, beta, [(7, 2)], [1])[0]


# ---- the host engine (svinet_amd/host/mmsbinferorig.cc) with -host-loops, and the command line ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
ASSORT = os.path.join(GOLDEN, "graphs", "assort-75-4.txt")
RTOL = 1e-7


def _skip_of(e):
    return [tuple(int(x) for x in r) for r in e.heldout]


def test_sampler_draws_ordered_pairs():
    """s = heldout_ratio * ones, s / 2 non-links and s / 2 links in each list; pairs stay in the order drawn (both p < q and
    p > q occur); the validation list shares no pair with the held-out list in the same orientation"""
    e = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    adj = OC.adjacency(e.n, e.edges)
    half = int(0.1 * len(e.edges)) // 2
    for lst in (e.heldout, e.validation):
        y = adj[lst[:, 0], lst[:, 1]]
        assert (y == 1).sum() == half and (y == 0).sum() == half
        assert np.all(lst[:, 0] != lst[:, 1])
        assert (lst[:, 0] < lst[:, 1]).any() and (lst[:, 0] > lst[:, 1]).any()
    held = set(_skip_of(e))
    val = [tuple(int(x) for x in r) for r in e.validation]
    assert not held & set(val) and len(set(val)) == len(val)
    again = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    assert np.array_equal(again.heldout, e.heldout) and np.array_equal(again.gamma, e.gamma)
    other = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, seed=7, on_device=False)   # -seed is honoured
    assert not np.array_equal(other.heldout, e.heldout)


def test_beta_starts():
    e = OrigEngine(ASSORT, 75, 5, heldout_ratio=0.1, itype=0, on_device=False)
    b = e.beta
    assert np.all((b >= 0.01) & (b <= 0.99)) and np.allclose(b * 100, np.round(b * 100), atol=1e-12) and len(np.unique(b)) > 5
    g = e.gamma
    assert g.shape == (75, 5) and abs(g.mean() - 1.0) < 0.02 and 0.05 < g.std() < 0.2   # Gamma(100, 0.01)
    e = OrigEngine(ASSORT, 75, 5, heldout_ratio=0.1, itype=1, on_device=False)
    total = 75 * 74 / 2
    eta0 = total * (len(e.edges) / total) / 5
    eta1 = total / 25 - eta0
    if eta1 < 0:
        eta1 = 1.0
    want = np.full((5, 5), 1e-30)
    np.fill_diagonal(want, eta0 / (eta0 + eta1))
    np.testing.assert_allclose(e.beta, want, rtol=1e-14)


def test_host_loops_against_the_restatement_plain_state():
    e = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    adj, skip = OC.adjacency(e.n, e.edges), _skip_of(e)
    g, b = e.gamma, e.beta
    for _ in range(2):
        g, b, rounds, bad = OC.sweep(g, b, adj, skip, 0.25)
        assert not bad.any()
        e.sweep()
        np.testing.assert_allclose(e.gamma, g, rtol=RTOL)
        np.testing.assert_allclose(e.beta, b, rtol=RTOL)
        assert e.rounds_total == int(rounds.sum()) and len(rounds) == 75 * 74 - len(set(skip))
    assert e.iter == 2
    e.report()
    rows = e.rows
    assert rows.shape == (4, 8) and rows[:, 0].tolist() == [0, 1, 0, 1] and rows[:, 1].tolist() == [0, 0, 2, 2]
    for row, lst in ((rows[2], sorted(set(skip))), (rows[3], sorted({tuple(int(x) for x in r) for r in e.validation}))):
        y = np.array([adj[p, q] for p, q in lst])
        u = OC.pair_loglik(g, b, lst, y)
        np.testing.assert_allclose(row[2:], [u.mean(), len(u), u[y == 0].mean(), (y == 0).sum(), u[y == 1].mean(), (y == 1).sum()],
                                   rtol=RTOL)


@pytest.mark.parametrize("k,seed", [(4, 41), (17, 42)])
def test_host_loops_against_the_restatement_peaked_state(k, seed):
    e = OrigEngine(ASSORT, 75, k, heldout_ratio=0.1, on_device=False)
    adj, skip = OC.adjacency(e.n, e.edges), _skip_of(e)
    _, gamma, beta = OC.peaked_state(seed, 75, k)
    e.set_state(gamma, beta)
    g, b, rounds, bad = OC.sweep(gamma, beta, adj, skip, 1.0 / k)
    OC.check_conditions(rounds, bad, b)
    e.sweep()
    np.testing.assert_allclose(e.gamma, g, rtol=RTOL)
    np.testing.assert_allclose(e.beta, b, rtol=RTOL)
    assert e.rounds_total == int(rounds.sum())


def test_training_skips_one_orientation_only():
    """the reverse orientation of a held-out pair is trained on: skipping it as well gives another beta"""
    one = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    both = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    skip = _skip_of(one)
    rev = [(q, p) for p, q in skip if (q, p) not in skip]
    assert rev
    both.skip_also(rev)
    one.sweep()
    both.sweep()
    adj = OC.adjacency(one.n, one.edges)
    start = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    np.testing.assert_allclose(both.beta, OC.sweep(start.gamma, start.beta, adj, skip + rev, 0.25)[1], rtol=RTOL)
    np.testing.assert_allclose(one.beta, OC.sweep(start.gamma, start.beta, adj, skip, 0.25)[1], rtol=RTOL)
    assert np.abs(one.beta / both.beta - 1).max() > 1e-5


def test_device_backend_without_a_gpu_fails_loudly():
    if _have_gpu():
        pytest.skip("GPU present")
    with pytest.raises(_svils.SvilsError) as ei:
        OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=True)
    assert ei.value.code == ERR_DEVICE and "no CPU path" in str(ei.value)


def _run(args, cwd, timeout=120):
    return subprocess.run([SVINET] + args, capture_output=True, text=True, timeout=timeout, cwd=str(cwd))


@pytest.mark.parametrize("extra,name", [([], "n75-k4-mmsb-U"), (["-itype", "1"], "n75-k4-mmsb-U-i1"), (["-nodelay", "-seed", "3"], "n75-k4-mmsb-seed3-")])
def test_cli_host_loops(tmp_path, extra, name):
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-orig", "-host-loops", "-max-iterations", "3", "-heldout-ratio", "0.1"] + extra, tmp_path)
    assert r.returncode == 0, r.stderr
    assert [p.name for p in tmp_path.iterdir()] == [name]
    d = tmp_path / name
    files = {p.name for p in d.iterdir()}
    assert files == {"beta.txt", "communities.txt", "convergence.txt", "gamma.txt", "groups.txt", "heldout-edges.txt", "heldout.txt",
                     "infer.log", "logl.txt", "modularity.txt", "network.dat", "param.txt", "stats.txt", "summary.txt", "time.txt",
                     "validation-edges.txt", "validation.txt"}
    for f in ("heldout.txt", "validation.txt"):
        rows = [l.split("\t") for l in (d / f).read_text().splitlines()]
        assert [r[0] for r in rows] == ["0", "1", "2", "3"] and all(len(r) == 8 for r in rows)
        for r in rows:   # iter, secs, mean, count, mean of the non-links, count, mean of the links, count
            assert int(r[3]) == int(r[5]) + int(r[7]) and all(len(r[c].split(".")[1]) == 5 for c in (2, 4, 6))
            assert float(r[2]) < 0 and float(r[4]) < 0 and float(r[6]) < 0
    beta = np.loadtxt(d / "beta.txt")
    assert beta.shape == (4, 4) and np.all((beta > 0) & (beta < 1))
    gamma = np.loadtxt(d / "gamma.txt")
    assert gamma.shape == (75, 6) and abs((gamma[:, 2:] - 0.25).sum() - 2 * 75 * 74) < 200   # all but the held-out pairs
    assert len((d / "summary.txt").read_text().splitlines()) == 3
    assert len((d / "groups.txt").read_text().splitlines()) == 75
    held = np.loadtxt(d / "heldout-edges.txt", dtype=int)
    assert held.shape[1] == 2 and (held[:, 0] > held[:, 1]).any() and (held[:, 0] < held[:, 1]).any()
    if not extra:   # the library engine is the command line's engine
        e = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
        for _ in range(3):
            e.sweep()
        np.testing.assert_allclose(beta, e.beta, rtol=1e-10)
        assert np.array_equal(held, e.heldout.astype(int))


@pytest.mark.parametrize("args,word", [
    ([], "-max-iterations"),
    (["-max-iterations", "3", "-batch"], "-batch"),
    (["-max-iterations", "3", "-batch-gpu"], "-batch"),
    (["-max-iterations", "3", "-link-sampling"], "-link-sampling"),
    (["-max-iterations", "3", "-rnode"], "-rnode"),
    (["-max-iterations", "3", "-rpair"], "-rpair"),
    (["-max-iterations", "3", "-stratified"], "-stratified"),
    (["-max-iterations", "3", "-infset"], "-infset"),
    (["-max-iterations", "3", "-preprocess"], "-preprocess"),
    (["-max-iterations", "3", "-findk"], "-findk"),
    (["-max-iterations", "3", "-gml"], "-gml"),
    (["-max-iterations", "3", "-lcstats"], "-lcstats"),
    (["-max-iterations", "3", "-gpus", "2"], "-gpus"),
    (["-max-iterations", "3", "-kshard"], "-kshard"),
    (["-max-iterations", "3", "-minibatch", "10"], "-minibatch"),
    (["-max-iterations", "3", "-load", "x/"], "-load"),
    (["-max-iterations", "3", "-recommend", "3"], "-recommend"),
    (["-max-iterations", "3", "-rank-heldout"], "-rank-heldout"),
    (["-max-iterations", "3", "-k", "65"], "SVILS_ORIG_MAX_K"),
    (["-max-iterations", "3", "-n", "40000"], "SVILS_ORIG_MAX_N"),
])
def test_cli_refusals_create_nothing(tmp_path, args, word):
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-orig"] + args, tmp_path)
    assert r.returncode == 2 and word in r.stderr, (r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


def test_cli_device_run_without_a_gpu_fails_and_writes_no_model(tmp_path):
    if _have_gpu():
        pytest.skip("GPU present")
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-orig", "-max-iterations", "2", "-heldout-ratio", "0.1"], tmp_path)
    assert r.returncode != 0 and "no CPU path" in r.stderr
    assert not list(tmp_path.rglob("gamma.txt")) and not list(tmp_path.rglob("beta.txt"))
