"""Models and expectations shared by tests/test_ppc.py (CPU: the restatement alone) and tests/test_gpu_ppc.py (the device
against the restatement).  Everything here is built from tools/restate_ppc.py and numpy; nothing reads the device."""
import math
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import restate_ppc as R  # noqa: E402

DBL_EPSILON = 2.220446049250313e-16

# the Random123 known-answer vectors of Philox4x32-10: (counter, key, output)
KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)

EQUALITY_N = (2, 63, 65, 130)          # below one 64-tile, one past it, two tiles and a ragged one
EQUALITY_K = (2, 5, 20, 67)            # not a multiple of 4, odd
EQUALITY_DRAWS = ((0, 0), (12345, 7), (0xfffffffe, 0xffffffff))   # (seed, r)


def random_model(n, K, seed):
    rng = np.random.default_rng([n, K, seed])
    pi = 0.4 * rng.dirichlet(np.full(K, 0.3), n)     # every community a little, and most of a node in one of three at most:
    pi[np.arange(n), rng.integers(0, min(K, 3), n)] += 0.6   # the graph stays dense enough at large K to have triangles
    return pi / pi.sum(1)[:, None], rng.uniform(0.3, 1.0, K)


def power_of_two_model(n, K, seed):
    """rows that are one-hot, two halves or four quarters; beta in {0, 0.5, 1}: every partial sum is exact in any order"""
    rng = np.random.default_rng([n, K, seed, 2])
    pi = np.zeros((n, K))
    for i in range(n):
        m = min(K, int(rng.choice([1, 1, 2, 4])))
        pi[i, rng.choice(K, m, replace=False)] = 1.0 / m
    beta = rng.choice([0.0, 0.5, 1.0], K)
    beta[0] = 0.5
    return pi, beta


EDGE_SEED, EDGE_R, EDGE_N, EDGE_K = 2024, 5, 65, 5
EDGE_PAIRS = ((0, 1), (2, 3), (4, 5))


def on_the_edge_model():
    """nodes (0, 1), (2, 3), (4, 5) are one-hot on communities 0, 1, 2, so s of those three pairs is beta_0, beta_1,
    beta_2 exactly, in any order of summation; the betas are the pairs' own uniforms of (EDGE_SEED, EDGE_R): u itself (no
    link: u < u is false), the next double above (a link) and the next below (none)"""
    pi, beta = random_model(EDGE_N, EDGE_K, 99)
    pi[:6] = 0.0
    pi[6:, :3] = 0.0           # nobody else is in communities 0 .. 2: those three pairs alone carry beta_0 .. beta_2
    pi[6:] /= pi[6:].sum(1)[:, None]
    for c, (p, q) in enumerate(EDGE_PAIRS):
        pi[p, c] = pi[q, c] = 1.0
    u = [R.pair_uniform(EDGE_SEED, EDGE_R, p, q) for p, q in EDGE_PAIRS]
    beta[0] = u[0]
    beta[1] = np.nextafter(u[1], 1.0)
    beta[2] = np.nextafter(u[2], 0.0)
    want = {EDGE_PAIRS[0]: False, EDGE_PAIRS[1]: True, EDGE_PAIRS[2]: False}
    return pi, beta, want


def band_pairs(pi, beta, seed, r):
    """pairs whose ascending sum lies within 2 K DBL_EPSILON s of u: the ones a recheck has to look at again"""
    P, Q = R.all_pairs(pi.shape[0])
    s = R.pair_sums(pi, beta, P, Q)
    u = R.pair_uniforms(seed, r, P, Q)
    return int(np.count_nonzero(np.abs(s - u) <= 2 * pi.shape[1] * DBL_EPSILON * s)), len(P)


BLOCKS = (7, 20, 38)


def block_model(b):
    n = sum(BLOCKS)
    pi = np.zeros((n, len(BLOCKS)))
    pi[np.arange(n), np.repeat(np.arange(len(BLOCKS)), BLOCKS)] = 1.0
    return pi, np.full(len(BLOCKS), float(b))


EXP_N, EXP_K, EXP_R, EXP_SEED = 65, 5, 200, 31


def expectation_bounds():
    """(pi, beta, sum of s, its 5 sigma bound for the mean of EXP_R replicates, the expected degrees, their 6 sigma bounds)"""
    pi, beta = random_model(EXP_N, EXP_K, 5)
    P, Q = R.all_pairs(EXP_N)
    s = R.pair_sums(pi, beta, P, Q)
    S = np.zeros((EXP_N, EXP_N))
    S[P, Q] = s
    S = S + S.T
    V = S * (1 - S)
    return (pi, beta, math.fsum(s), 5 * math.sqrt(math.fsum(s * (1 - s)) / EXP_R), S.sum(1), 6 * np.sqrt(V.sum(1) / EXP_R))


def check_expectation(ones, degs, bounds):
    """ones [R], degs [R][n] of the replicates against the closed-form expectations"""
    _, _, es, tol, edeg, tdeg = bounds
    assert abs(np.mean(ones) - es) <= tol, (np.mean(ones), es, tol)
    dev = np.abs(np.mean(degs, axis=0) - edeg)
    assert np.all(dev <= tdeg), (float(np.max(dev / tdeg)))


def degrees(links, n):
    return np.bincount(np.asarray(links, np.int64).reshape(-1), minlength=n)
