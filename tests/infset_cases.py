"""What tests/test_infset.py and tests/test_gpu_infset.py share: a numpy restatement of ONE informative-set step of the
reference's FastAMM::infer (src/fastamm.cc:565-616 with opt_process / opt_process_noninf, :915-1126) on top of
oracle/batch_oracle.py (dir_exp, phis -- imported, the oracle stays as it is) and batch_cases.phis_rounds; a plain-Python
restatement of the preprocessing walk (Network::set_neighborhood_sets, src/network.cc:558-686); and the drawn schedule."""
import struct

import numpy as np

import batch_cases as BC
from oracle import batch_oracle as B

TAU0, KAPPA, NODETAU0, NODEKAPPA = 1024.0, 0.9, 1024.0, 0.5   # src/env.hh:405-408
INF_EPSILON, NONINF_SETSIZE, LIMIT, PER_VISIT = 0.0001, 200, 100, 10   # src/fastamm.cc:18, src/network.cc:562, :630


def rho_node(c, nodetau0=NODETAU0, nodekappa=NODEKAPPA):
    """src/fastamm.cc:594 with :22 -- c the times the node's row was moved before"""
    return (nodetau0 + 1 + c) ** (-nodekappa)


def rho_lambda(it, tau0=TAU0, kappa=KAPPA):
    """:605 with :21; _lambda_start_iter = 0"""
    return (tau0 + 1 + it + 1) ** (-kappa)


def scale_of(kind, n, inf_epsilon=INF_EPSILON):
    """:587-588"""
    return n / 2.0 if kind == 0 else (float(n) * float(n)) / (2 * inf_epsilon * NONINF_SETSIZE)


def star(start, partner, adj, rho_partner, rho_start, scale, rho_lambda):
    partner = np.asarray(partner, dtype=np.int64).reshape(-1)
    return dict(start=int(start), partner=partner, y=adj[start, partner].astype(np.uint8) if len(partner) else np.zeros(0, np.uint8),
                rho_partner=np.asarray(rho_partner, dtype=np.float64).reshape(-1), rho_start=float(rho_start), scale=float(scale),
                rho_lambda=float(rho_lambda))


def pairs_of(s):
    a, j = s["start"], np.asarray(s["partner"], dtype=np.int64)
    return np.minimum(a, j), np.maximum(a, j)


def step(gamma, lam, adj, s, alpha, eta):
    """one star step from (gamma, lambda) -> new gamma, new lambda, the rounds of every pair.  Only the rows of the star
    move; rho_lambda < 0 returns lambda as it came"""
    a, j = s["start"], np.asarray(s["partner"], dtype=np.int64)
    p, q = pairs_of(s)
    K = gamma.shape[1]
    g, ta, lambdat = gamma.copy(), np.zeros(K), np.zeros((K, 2))
    rounds = np.zeros(0, dtype=np.int64)
    if len(j):
        assert len(set(j.tolist())) == len(j) and a not in set(j.tolist())
        y = adj[p, q]
        assert np.array_equal(y, np.asarray(s["y"], dtype=np.int64))
        elogpi, elogbeta = B.dir_exp(gamma), B.dir_exp(lam)
        phi1, phi2, rounds = BC.phis_rounds(elogpi, elogbeta, p, q, y)
        check1, check2 = B.phis(elogpi, elogbeta, p, q, y)
        assert np.array_equal(check1, phi1) and np.array_equal(check2, phi2)
        first = (p == a)[:, None]
        pa, pj = np.where(first, phi1, phi2), np.where(first, phi2, phi1)
        ta = pa.sum(0)
        pp = phi1 * phi2
        lambdat[:, 0] = (pp * (y[:, None] == 1)).sum(0)
        lambdat[:, 1] = (pp * (y[:, None] == 0)).sum(0)
        rj = np.asarray(s["rho_partner"], dtype=np.float64)[:, None]
        g[j] = (1 - rj) * gamma[j] + rj * (alpha + s["scale"] * pj)
    ra = s["rho_start"]
    g[a] = (1 - ra) * gamma[a] + ra * (alpha + s["scale"] * ta)
    rl = s["rho_lambda"]
    if rl < 0:
        return g, lam.copy(), rounds
    return g, (1 - rl) * lam + rl * (np.asarray(eta, dtype=np.float64)[None, :] + s["scale"] * lambdat), rounds


def adjacency_lists(n, edges):
    """every node's neighbours in link order (what the reader builds: both ends of a link get each other at once)"""
    out = [[] for _ in range(n)]
    for p, q in np.asarray(edges, dtype=np.int64):
        out[p].append(int(q))
        out[q].append(int(p))
    return out


def preprocess_walk(nbrs):
    """Network::set_neighborhood_sets: per node the neighbours round-robin, a visit scans the neighbour's list from the
    front and takes at most 10 not-yet-taken two-hop non-neighbours; a neighbour is exhausted once a scan runs off its end"""
    n = len(nbrs)
    sets = []
    for i in range(n):
        v, zeros = nbrs[i], []
        if not v:
            sets.append(zeros)
            continue
        mine, taken, exhausted = set(v), set(), set()
        j = 0
        while True:
            q = v[j]
            if q != i and q not in exhausted:
                u, k, c = nbrs[q], 0, 0
                while k < len(u) and len(zeros) < LIMIT:
                    p = u[k]
                    if p != i and p not in mine and p not in taken:
                        zeros.append(p)
                        taken.add(p)
                        c += 1
                        if c >= PER_VISIT:
                            break
                    k += 1
                if k == len(u):
                    exhausted.add(q)
            j = (j + 1) % len(v)
            if not (len(zeros) < LIMIT and len(exhausted) < len(v)):
                break
        sets.append(zeros)
    return sets


def neighbors_bytes(sets):
    """neighbors.bin: per node uint32 id, 8-byte count, uint32 ids"""
    out = bytearray()
    for i, z in enumerate(sets):
        out += struct.pack("<IQ", i, len(z)) + struct.pack("<%dI" % len(z), *z)
    return bytes(out)


def expected_partners(d, n, nbrs, zeros, skip, shuffled):
    """the partner lists the reference's loops would make for the drawn start node and kind: one list for kind 0, one per
    possible block start for kind 1 (the walk ends after one lap of the shuffled order)"""
    a = d["start"]
    ok = lambda j: (min(a, j), max(a, j)) not in skip
    if d["kind"] == 0:
        return [[j for j in nbrs[a] if ok(j)] + [j for j in zeros[a] if ok(j)]]
    mine, inf, out = set(nbrs[a]), set(zeros[a]), []
    for q0 in range(0, n, NONINF_SETSIZE):
        walk = [int(shuffled[(q0 + x) % n]) for x in range(n)]
        out.append([j for j in walk if j != a and j not in mine and ok(j) and j not in inf][:NONINF_SETSIZE])
    return out
