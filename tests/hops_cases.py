"""Graphs and expectations shared by tests/test_hops.py (CPU: the restatement tools/restate_hops.py alone) and
tests/test_gpu_hops.py (the device against it).  Nothing here reads the device; a restatement is computed once per graph."""
import functools
import math
import os
import sys

import numpy as np

from conftest import ROOT
import ppc_cases as PC
from ppc_cases import R

sys.path.insert(0, os.path.join(ROOT, "tools"))
import restate_hops as H  # noqa: E402

K = 5
MODEL_SEED = 1
# word and pass edges at every `words`: one word short of a bit, full, one bit over, three words at words = 1 (three passes,
# the last of 2 sources); 1100: three passes at words = 8, the last word of 12 bits
REPLICATE_N = (63, 64, 65, 130, 1100)
SPARSE_DEG, DENSE_DEG = 1.5, 6.0
# (seed, r) of the sparse replicates, picked with the restatement (tests/test_hops.py asserts what they were picked for):
# at least three components of two or more nodes, an isolated node, a diameter >= 5
SPARSE_DRAWS = {63: ((1, 0), (1, 1)), 64: ((1, 0), (1, 1)), 65: ((1, 0), (1, 1)), 130: ((1, 0), (1, 1)), 1100: ((1, 0), (1, 1))}
DENSE_DRAWS = ((1, 0), (2, 1))


@functools.lru_cache(maxsize=None)
def model(n, mean_deg):
    """ppc_cases.random_model with beta scaled so that a replicate's expected mean degree is mean_deg"""
    pi, beta = PC.random_model(n, K, MODEL_SEED)
    P, Q = R.all_pairs(n)
    have = 2.0 * math.fsum(R.pair_sums(pi, beta, P, Q)) / n
    return pi, beta * (mean_deg / have)


@functools.lru_cache(maxsize=None)
def replicate(n, mean_deg, seed, r):
    """(links [E][2], the restatement's all_of) of replicate (seed, r) of model(n, mean_deg)"""
    pi, beta = model(n, mean_deg)
    links = R.draw(pi, beta, seed, r)
    return links, H.all_of(links, n)


def replicate_cases():
    return [(n, SPARSE_DEG, s, r) for n in REPLICATE_N for s, r in SPARSE_DRAWS[n]] + \
           [(n, DENSE_DEG, s, r) for n in REPLICATE_N for s, r in DENSE_DRAWS]


def sparse_conditions(want):
    """(components of two or more nodes, isolated nodes, diameter) of a restatement"""
    sizes = np.bincount(want["comp"].astype(np.int64))
    return int(np.count_nonzero(sizes >= 2)), want["isolated"], want["diameter"]


def matrix_power_route(links, n):
    """independent of the restatement: boolean powers of the adjacency matrix, d(s, v) = the first power at which the
    entry turns true -> (D, ecc, comp) as lists"""
    A = np.zeros((n, n), bool)
    for p, q in np.asarray(links, np.int64).reshape(-1, 2):
        A[p, q] = A[q, p] = True
    dist = np.full((n, n), -1, np.int64)
    np.fill_diagonal(dist, 0)
    P = np.eye(n, dtype=bool)
    for h in range(1, n):
        P = (P.astype(np.int64) @ A.astype(np.int64)) > 0       # walks of length h
        new = P & (dist < 0)
        if not new.any():
            break
        dist[new] = h
    D = [int(np.count_nonzero(dist == h)) for h in range(int(dist.max()) + 1)]
    return D, dist.max(1).tolist(), [int(np.flatnonzero(dist[v] >= 0)[0]) for v in range(n)]


# ---- closed forms: name -> (n, links, D, ecc, comp) ----

def _clique(nodes):
    return [(nodes[i], nodes[j]) for i in range(len(nodes)) for j in range(i + 1, len(nodes))]


def path(n):
    return (n, [(i, i + 1) for i in range(n - 1)], [n] + [2 * (n - h) for h in range(1, n)], [max(s, n - 1 - s) for s in range(n)], [0] * n)


def cycle(n):   # odd n: two nodes at every distance 1 .. (n - 1) / 2
    assert n % 2 == 1
    return (n, [(i, i + 1) for i in range(n - 1)] + [(0, n - 1)], [n] + [2 * n] * ((n - 1) // 2), [(n - 1) // 2] * n, [0] * n)


def star(n):    # centre 0
    return (n, [(0, i) for i in range(1, n)], [n, 2 * (n - 1), (n - 1) * (n - 2)], [1] + [2] * (n - 1), [0] * n)


def complete(n):
    return (n, _clique(list(range(n))), [n, n * (n - 1)], [1] * n, [0] * n)


def empty(n):
    return (n, [], [n], [0] * n, list(range(n)))


def cliques(blocks):   # disjoint cliques over consecutive ids: ppc_cases.BLOCKS gives the labels 0, 7, 27
    n, links, comp, first = sum(blocks), [], [], 0
    for b in blocks:
        links += _clique(list(range(first, first + b)))
        comp += [first] * b
        first += b
    return (n, links, [n, sum(b * (b - 1) for b in blocks)], [1] * n, comp)


def bridged(a, b):     # cliques 0 .. a - 1 and a .. a + b - 1 joined by the link (a - 1, a)
    n = a + b
    links = _clique(list(range(a))) + _clique(list(range(a, n))) + [(a - 1, a)]
    D = [n, a * (a - 1) + b * (b - 1) + 2, 2 * ((a - 1) + (b - 1)), 2 * (a - 1) * (b - 1)]
    ecc = [3] * (a - 1) + [2, 2] + [3] * (b - 1)
    return (n, links, D, ecc, [0] * n)


def closed_forms():
    return {"path-130": path(130), "cycle-129": cycle(129), "star-65": star(65), "complete-65": complete(65), "empty-65": empty(65),
            "one-link": (2, [(0, 1)], [2, 2], [1, 1], [0, 0]), "three-cliques": cliques(PC.BLOCKS), "bridged-cliques": bridged(40, 31)}


def check_closed_form(got, form):
    n, links, D, ecc, comp = form
    assert [int(d) for d in got["D"]] == D, (got["D"], D)
    assert got["ecc"].tolist() == ecc and got["comp"].tolist() == comp
    assert got["diameter"] == len(D) - 1 and got["reachable"] == sum(D) - n
    sizes = np.bincount(comp, minlength=n)
    assert got["components"] == int(np.count_nonzero(sizes)) and got["largest"] == int(sizes.max())
    assert got["isolated"] == int(np.count_nonzero(PC.degrees(links, n) == 0)) if links else got["isolated"] == n
    far = sum(h * d for h, d in enumerate(D))
    assert (math.isnan(got["meandist"]) and far == 0) or got["meandist"] == far / (sum(D) - n)


def same_hops(a, b):
    """every integer equal; the two doubles at rtol 1e-15"""
    for name in ("D", "ecc", "comp"):
        assert np.array_equal(np.asarray(a[name]).astype(np.int64), np.asarray(b[name]).astype(np.int64)), name
    for name in ("reachable", "diameter", "components", "largest", "isolated"):
        assert a[name] == b[name], (name, a[name], b[name])
    for name in ("effdiam", "meandist"):
        x, y = float(a[name]), float(b[name])
        assert (math.isnan(x) and math.isnan(y)) or abs(x - y) <= 1e-15 * abs(y), (name, x, y)
