"""CPU: the restatement tools/restate_ppc.py against the published Philox vectors, its own plain loops and the closed
forms the device is later held to (tests/test_gpu_ppc.py), and what svils_ppc_* answers without a device."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np

from conftest import ROOT
import ppc_cases as PC
from ppc_cases import R


def test_philox_known_answers():
    for ctr, key, out in PC.KAT:
        assert R.philox4x32_10(ctr, key) == out
    ctr = [np.array([c[0][i] for c in PC.KAT], np.uint64) for i in range(4)]   # the array form, one key at a time
    for j, (c, key, out) in enumerate(PC.KAT):
        w = R.philox4x32_10(ctr, key)
        assert tuple(int(x[j]) for x in w) == out


def test_uniform_is_53_bits_in_the_unit_interval():
    assert R.to_uniform(0, 0) == 0.0
    assert R.to_uniform(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53
    assert R.to_uniform(1 << 5, 0) == 2.0 ** -27 and R.to_uniform(0, 1 << 6) == 2.0 ** -53
    P, Q = R.all_pairs(40)
    u = R.pair_uniforms(5, 6, P, Q)
    assert u[17] == R.pair_uniform(5, 6, int(P[17]), int(Q[17])) and 0.4 < u.mean() < 0.6
    assert not np.array_equal(u, R.pair_uniforms(5, 7, P, Q)) and not np.array_equal(u, R.pair_uniforms(6, 6, P, Q))


def test_array_draw_is_the_loop_draw():
    for n, K in ((2, 2), (23, 5), (30, 67)):
        pi, beta = PC.random_model(n, K, 1)
        for seed, r in PC.EQUALITY_DRAWS[:2]:
            a = R.draw_loops(pi, beta, seed, r)
            assert np.array_equal(a, R.draw(pi, beta, seed, r))
            assert n == 2 or len(a) > 5


def test_edge_model_meets_its_conditions():
    pi, beta, want = PC.on_the_edge_model()
    assert np.allclose(pi.sum(1), 1.0, rtol=0, atol=1e-12) and np.all((beta >= 0) & (beta <= 1))
    for (p, q), c in zip(PC.EDGE_PAIRS, range(3)):
        assert R.pair_sum(pi[p], pi[q], beta) == beta[c]
    have = set(map(tuple, R.draw(pi, beta, PC.EDGE_SEED, PC.EDGE_R).tolist()))
    for pq, y in want.items():
        assert (pq in have) == y
    band, pairs = PC.band_pairs(pi, beta, PC.EDGE_SEED, PC.EDGE_R)
    assert 3 <= band <= 0.01 * pairs


def test_cliques_in_closed_form():
    pi, beta = PC.block_model(1.0)
    links = R.draw(pi, beta, 4, 1)
    s = R.stats(links, pi, beta)
    m = np.repeat(PC.BLOCKS, PC.BLOCKS)
    assert s["ones"] == sum(b * (b - 1) // 2 for b in PC.BLOCKS)
    assert np.array_equal(s["deg"], m - 1) and np.array_equal(s["tri"], (m - 1) * (m - 2) // 2)
    assert s["transitivity"] == 1.0 and s["clustering"] == 1.0 and not s["logpe"].any()
    assert len(R.draw(*PC.block_model(0.0), 4, 1)) == 0
    e = R.stats(np.zeros((0, 2), np.int64), pi, beta)
    assert e["ones"] == 0 and math.isnan(e["transitivity"]) and e["clustering"] == 0.0 and not e["size"].any()


def test_restatement_meets_the_expectations():
    b = PC.expectation_bounds()
    ones, degs = [], []
    for r in range(PC.EXP_R):
        links = R.draw(b[0], b[1], PC.EXP_SEED, r)
        ones.append(len(links))
        degs.append(PC.degrees(links, PC.EXP_N))
    PC.check_expectation(ones, degs, b)


def test_library_refusals_need_no_device():
    import torch
    from svinet_amd import _svils
    L = _svils.load()
    h = C.c_void_p()
    for n, k, word in ((_svils.PPC_MAX_N + 1, 4, b"SVILS_PPC_MAX_N"), (100, _svils.PPC_MAX_K + 1, b"SVILS_PPC_MAX_K")):
        assert L.svils_ppc_create(0, n, k, 10, C.byref(h)) == -4 and word in L.svils_last_error()
    assert L.svils_ppc_create(0, 100, 4, 10, None) == -1
    if not torch.cuda.is_available():
        assert L.svils_ppc_create(0, 100, 4, 10, C.byref(h)) == -2 and b"no CPU path" in L.svils_last_error()
        for f in (L.svils_ppc_stats, L.svils_ppc_destroy):
            assert f(None) in (0, -2)
        assert L.svils_ppc_draw(None, 1, 2) == -2 and b"no CPU path" in L.svils_last_error()
    else:
        assert L.svils_ppc_draw(None, 1, 2) == -1


# ---- the host side: its Philox, the parameter draws, the command line ----

def test_host_philox_is_the_restatements_word_for_word():
    from svinet_amd import host_api
    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 2 ** 32, (10000, 4), dtype=np.uint64)
    ctr[:3] = [c for c, _, _ in PC.KAT]
    key = (0xa4093822, 0x299f31d0)
    got = host_api.ppc_philox(ctr, key)
    want = R.philox4x32_10([ctr[:, i] for i in range(4)], key)
    for i in range(4):
        assert np.array_equal(got[:, i].astype(np.uint64), want[i])
    assert tuple(int(x) for x in got[2]) == PC.KAT[2][2]


def test_host_parameter_draws_repeat_and_differ():
    from svinet_amd import host_api
    rng = np.random.default_rng(12)
    gam, lam = rng.gamma(0.5, 2.0, (30, 6)) + 0.01, rng.gamma(2.0, 2.0, (6, 2))
    pi, beta = host_api.ppc_params(gam, lam, 7, 3)
    again = host_api.ppc_params(gam, lam, 7, 3)
    assert np.array_equal(pi, again[0]) and np.array_equal(beta, again[1])
    for seed, r in ((7, 4), (8, 3)):
        other = host_api.ppc_params(gam, lam, seed, r)
        assert not np.any(pi == other[0]) and not np.any(beta == other[1])
    assert np.all(pi >= 0) and np.all(np.abs(pi.sum(1) - 1.0) <= 1e-12) and np.all((beta > 0) & (beta < 1))
    # the restatement's stream is the same stream (same libm on one machine)
    assert np.array_equal(pi[:4], R.dirichlet_rows(gam[:4], 7, 3)) and np.array_equal(beta, R.beta_draws(lam, 7, 3))


def test_host_dirichlet_and_beta_moments():
    """R = 400 draws of one K = 5 row with shapes on both sides of 1, and of Beta pairs: every mean within five sigma of
    its closed form (one fixed seed)"""
    from svinet_amd import host_api
    R_, seed = 400, 2718
    g = np.array([0.05, 0.4, 1.0, 2.5, 9.0])
    lam = np.array([[0.3, 0.6], [1.0, 1.0], [4700.59, 0.77], [2.0, 7.0], [0.97, 6.33]])
    rows = np.tile(g, (R_, 1))                       # R rows of one replicate: variates (i, j), independent across i
    pi, _ = host_api.ppc_params(rows, lam, seed, 0)
    a0 = g.sum()
    mean, var = g / a0, g * (a0 - g) / (a0 * a0 * (a0 + 1))
    assert np.all(np.abs(pi.mean(0) - mean) <= 5 * np.sqrt(var / R_)), (pi.mean(0), mean)
    betas = np.array([host_api.ppc_params(rows[:1], lam, seed, r)[1] for r in range(R_)])
    a, b = lam[:, 0], lam[:, 1]
    bm, bv = a / (a + b), a * b / ((a + b) ** 2 * (a + b + 1))
    assert np.all(np.abs(betas.mean(0) - bm) <= 5 * np.sqrt(bv / R_)), (betas.mean(0), bm)


def _svinet(args, cwd):
    exe = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
    return subprocess.run([exe] + [str(a) for a in args], cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_cli_refusals(tmp_path):
    import torch
    golden = os.path.join(ROOT, "tests", "golden")
    for m in ("gamma.txt", "lambda.txt"):
        shutil.copy(os.path.join(golden, "ref_assort_batch", m), str(tmp_path))
    graph = ["-file", os.path.join(golden, "graphs", "assort-75-4.txt"), "-n", 75, "-k", 4]
    for args, word in ((graph + ["-ppc", "-gpus", 2], "-gpus"), (graph + ["-ppc", "-minibatch", 8], "-minibatch"),
                       (["-n", 65, "-k", 4, "-gen", "-orig"], "-orig"), (["-n", 65, "-k", 4, "-gen", "-disjoint"], "-disjoint"),
                       (["-n", 65, "-k", 4, "-gen", "-gp"], "-gp"), (["-n", 65, "-k", 4, "-gen", "-gpus", 2], "-gpus"),
                       (["-n", 32769, "-k", 4, "-gen"], "-n 32769"), (["-n", 65, "-k", 2049, "-gen"], "-k 2049"),
                       (graph[:2] + ["-n", 32769, "-k", 4, "-ppc"], "-n 32769"), (graph[:4] + ["-k", 2049, "-ppc"], "-k 2049")):
        r = _svinet(args, tmp_path)
        assert r.returncode == 2 and word in r.stderr, (args, r.returncode, r.stderr)
        assert ("unsupported option" in r.stderr) == (word in ("-disjoint", "-gp")), r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["gamma.txt", "lambda.txt"]      # refused before anything is created
    if not torch.cuda.is_available():
        for args in (graph + ["-ppc", "-ppc-draws", 2], ["-n", 65, "-k", 4, "-gen"]):
            r = _svinet(args, tmp_path)
            assert r.returncode not in (0, 2) and "no CPU path" in r.stderr and "unsupported option" not in r.stderr, (args, r.stderr)
