"""Models and expectations shared by tests/test_ppc_orig.py (CPU: the restatement alone) and tests/test_gpu_ppc_orig.py
(the device against the restatement): the K x K kind of svils_ppc.  Everything here is built from
tools/restate_ppc_orig.py, tests/ppc_cases.py and numpy; nothing reads the device."""
import math
import os
import sys

import numpy as np

from conftest import ROOT
import ppc_cases as PC
from ppc_cases import R

sys.path.insert(0, os.path.join(ROOT, "tools"))
import restate_ppc_orig as RO  # noqa: E402

EQUALITY_N = PC.EQUALITY_N             # below one 64-tile, one past it, two tiles and a ragged one
EQUALITY_K = (2, 5, 20, 64)            # K^2 terms over 64 lanes: fewer terms than lanes, a ragged last pass, exactly 64 passes
MEAN_DEGREE = 8.0


def band(K):
    """the relative band of the K x K kind: (K^2 + 2 K + 18) DBL_EPSILON"""
    return (K * K + 2 * K + 18) * PC.DBL_EPSILON


def random_rates(n, K, seed):
    """B [K][K]: dense, asymmetric, scaled so that the mean degree is about MEAN_DEGREE (rows of pi sum to 1, so a pair's
    s is about the mean rate); n = 2 keeps rates up to 1"""
    rng = np.random.default_rng([n, K, seed, 7])
    B = rng.uniform(0.2, 1.0, (K, K))
    return B * min(1.0, MEAN_DEGREE / (n - 1) / B.mean())


def random_model(n, K, seed):
    return PC.random_model(n, K, seed)[0], random_rates(n, K, seed)


def power_of_two_model(n, K, seed):
    """ppc_cases.power_of_two_model's rows (one-hot, two halves or four quarters) and rates in {0, 0.5, 1}: every partial
    sum is exact in any order, and a ratio x_max / s may be 0.5 exactly"""
    rng = np.random.default_rng([n, K, seed, 3])
    B = rng.choice([0.0, 0.5, 1.0], (K, K))
    B[0, 0] = 0.5
    return PC.power_of_two_model(n, K, seed)[0], B


def one_hot(classes, K):
    pi = np.zeros((len(classes), K))
    pi[np.arange(len(classes)), classes] = 1.0
    return pi


def parity_model(n, B):
    """one-hot pi, class p mod 2"""
    return one_hot(np.arange(n) % 2, 2), np.array(B, np.float64)


ORIENTED = [[0, 1], [0, 0]]            # exactly the pairs p < q with p even, q odd: the smaller id indexes the rows of B
BIPARTITE = [[0, 1], [1, 0]]           # complete bipartite between even and odd


def oriented_pairs(n):
    return np.array([(p, q) for p in range(n) for q in range(p + 1, n) if p % 2 == 0 and q % 2 == 1], np.int64).reshape(-1, 2)


def bipartite_pairs(n):
    return np.array([(p, q) for p in range(n) for q in range(p + 1, n) if (p + q) % 2 == 1], np.int64).reshape(-1, 2)


EDGE_SEED, EDGE_R, EDGE_N, EDGE_K = 2024, 5, 65, 8
EDGE_PAIRS = ((0, 1), (2, 3), (4, 5))


def band_pairs(pi, B, seed, r):
    """pairs whose definition sum lies within the band of u: the ones a recheck has to look at again"""
    P, Q = R.all_pairs(pi.shape[0])
    s = RO.pair_sums(pi, B, P, Q)
    u = R.pair_uniforms(seed, r, P, Q)
    return int(np.count_nonzero(np.abs(s - u) <= band(pi.shape[1]) * s)), len(P)


def on_the_edge_model():
    """every node one-hot, so s of a pair is one rate exactly, in the tile sum as in the definition.  Nodes 0 .. 5 are alone
    in classes 0 .. 5 and everybody else is in classes 6 and 7: the pairs (0, 1), (2, 3), (4, 5) alone carry B[0][1],
    B[2][3], B[4][5], which are the pairs' own uniforms of (EDGE_SEED, EDGE_R): u itself (no link: u < u is false), the
    next double above (a link) and the next below (none).  The restatement's band count stays inside the cap the device is
    held to"""
    rng = np.random.default_rng([EDGE_N, EDGE_K, 99])
    classes = np.concatenate([np.arange(6), rng.integers(6, 8, EDGE_N - 6)])
    pi = one_hot(classes, EDGE_K)
    B = random_rates(EDGE_N, EDGE_K, 99)
    u = [R.pair_uniform(EDGE_SEED, EDGE_R, p, q) for p, q in EDGE_PAIRS]
    B[0, 1] = u[0]
    B[2, 3] = np.nextafter(u[1], 1.0)
    B[4, 5] = np.nextafter(u[2], 0.0)
    want = {EDGE_PAIRS[0]: False, EDGE_PAIRS[1]: True, EDGE_PAIRS[2]: False}
    inside, pairs = band_pairs(pi, B, EDGE_SEED, EDGE_R)
    assert 3 <= inside <= 0.01 * pairs, (inside, pairs)
    return pi, B, want


EXP_N, EXP_K, EXP_R, EXP_SEED = 130, 5, 200, 31


def expectation_bounds():
    """ppc_cases.expectation_bounds for the K x K kind: (pi, B, sum of s, its 5 sigma bound for the mean of EXP_R
    replicates, the expected degrees, their 6 sigma bounds)"""
    pi, B = random_model(EXP_N, EXP_K, 5)
    P, Q = R.all_pairs(EXP_N)
    s = RO.pair_sums(pi, B, P, Q)
    S = np.zeros((EXP_N, EXP_N))
    S[P, Q] = s
    S = S + S.T
    V = S * (1 - S)
    return (pi, B, math.fsum(s), 5 * math.sqrt(math.fsum(s * (1 - s)) / EXP_R), S.sum(1), 6 * np.sqrt(V.sum(1) / EXP_R))


# ---- the command line: assort-75-4 with K = 4 ----

CLI_N, CLI_K = 75, 4
GRAPH = os.path.join(ROOT, "tests", "golden", "graphs", "assort-75-4.txt")


def cli_rates():
    """a disassortative B, as beta.txt holds it after "%.12g" """
    rng = np.random.default_rng(41)
    B = rng.uniform(0.01, 0.05, (CLI_K, CLI_K)) + 0.25 * (1.0 - np.eye(CLI_K)) * rng.uniform(0.5, 1.0, (CLI_K, CLI_K))
    return np.array([[float("%.12g" % v) for v in row] for row in B])


def beta_text(B):
    """MMSBInferOrig::save_model: K lines of K values, %.12g"""
    return "".join("\t".join("%.12g" % v for v in row) + "\n" for row in B)


def read_gamma(path):
    return np.loadtxt(path, ndmin=2)[:, 2:]


def read_rates(path):
    return np.loadtxt(path, ndmin=2)
