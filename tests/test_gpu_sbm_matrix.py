"""-m gpu: every instantiation and every loop shape of the stochastic blockmodel's device code (-single and -single-logl,
svinet_amd/csrc/svils_sbm.hip) against the numpy restatements of tests/sbm_cases.py and tests/sbm_elbo_cases.py, which sum
directly over the trained pairs -- the split into column sums and link / skip corrections is the device's alone.

Which case exists for which code:

  * the matrix (S.MATRIX, n = 61): both edges of every (V, W) class of K = 2 .. 256.  V = ceil(K / 64) columns per lane picks
    k_sbm_chain<B, V> (and <1, V>, the plain chain) -- V = 3 at K = 129 (one live column in the third register) and 192; W, the
    row lanes of k_sbm_links and k_sbm_elbo_rows, is 2, 4, 8, 16, 32, 64 at K = 2, 3-4, 5-8, 9-16, 17-32, 33 and above.  The whole
    iterations hold gamma and lambda (k_sbm_links, k_sbm_mstep, write_elog) at every W and V: at K = 256 row K of lambda is one
    thread's sum over all 256 sa / sb entries and write_elog's k <= K loop takes its second trip.  The guard test fails when the
    library gains a class the matrix does not hold;
  * the hub cases (n = 150, K = 4 and 65): CSR rows longer than a wavefront.  split_row counts a row 64 entries at a time: the
    three hubs of degree 149 take three trips, with all partners later, with partners on both sides and inside the block, with
    all earlier -- the gathers and the in-block turns then start after a long prefix; node 1's skip row (100 entries, both y
    values) does the same for add_rows_y;
  * the dense cases: link and skip lists longer than the first trip of the lane groups of k_sbm_links.  A wavefront's run has
    ceil(list / 1024) pairs and the G = 64 / W lane groups take every G-th: 19 links for 16 groups and 3 skipped pairs at
    K = 4, 11 links and 3 skipped pairs for 2 groups at K = 20.  Lane groups other than 0 go round more than once and take
    skipped pairs, so the Y1 / Y0 butterfly adds something other than zeros.  The test asserts these shapes from the list lengths;
  * pair likelihoods at K = 65 and 256: the k += 64 loop of k_sbm_pair_ll makes two and four trips;
  * the rings (n = 16 500 and 65 553, K = 3): k_sbm_colsum with 65 and 257 nodes per block, k_sbm_elbo_rows with 17 rows per
    piece.  The O(n^2) restatement cannot run there; the reference is the O(n K) prefix-sum restatement
    (S.pair_sums_prefix, E.elbo_prefix: direct pair sums in np.longdouble), which tests/test_sbm.py holds to the mask-based one.

phi, gamma, lambda and msum are held at rtol 1e-7 (atol 1e-200), pass counts exactly, the bound at E.RTOL_A times A, and
everything that is the same additions in the same order to equal bits.  tests/test_sbm.py asserts, on the restatement alone,
that no msum of any pass compared here lies within 10 % of the exit threshold, and that neither the E-step nor the whole
iterations amplify a 1e-13 perturbation beyond 1e-9.  The one tolerance of its own is the 1e-9 of the ring's M-step: n 2^-53,
the bound on a fixed-order fp64 sum of n like-signed terms, is 7e-12 at n = 65 553; 1e-9 is over 100 times that, the margin
tests/sbm_elbo_cases.py argues for."""
import numpy as np
import pytest

import sbm_cases as S
import sbm_elbo_cases as E
from svinet_amd import _svils

pytestmark = pytest.mark.gpu

B = _svils.sbm_variant(4)[1]
RTOL = 1e-7
LINK_WAVES = 1024                        # wavefronts (= contiguous runs) of k_sbm_links
COLSUM_BLOCKS, COLSUM_FLOOR = 256, 64    # k_sbm_colsum: at most so many blocks, of at least so many nodes


def _handle(case):
    h = _svils.Sbm(case.n, case.K, S.ALPHA, case.eta)
    h.set_graph(case.links, case.skip)
    h.set_state(case.phi, case.gamma, case.lam)
    return h


def _close(got, ref):
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=1e-200)


def _sweep(h, case, niter, nodes=0, plain=False):
    """niter iterations from the case's start -> everything they leave: phi, gamma, lambda, the last msums, the pass counts"""
    h.set_launch_nodes(nodes)
    h.set_plain_chain(plain)
    h.set_state(case.phi, case.gamma, case.lam)
    h.sweep(niter)
    last, total, ms = h.stats()
    return h.state() + (ms, np.array([last, total]))


def _same_bits(got, ref, what):
    for a, b in zip(got, ref):
        assert np.array_equal(a, b), what


def _against_iterate(got, case, niter):
    rphi, rgamma, rlam, rpasses, rms = case.iterate(niter)
    phi, gamma, lam, ms, counts = got
    assert list(counts) == [rpasses[-1], sum(rpasses)]
    _close(ms, rms[-1])
    _close(phi, rphi)
    _close(gamma, rgamma)
    _close(lam, rlam)


def _against_elbo(h, case):
    got = h.elbo()
    ref = E.case_elbo(case, h.state())
    print("%s: got %r ref %r A %.6e" % (case.name, got, ref[:4], ref[4]))
    assert got[0] == (got[1] + got[2]) + got[3]
    for name, g, r in zip(("total", "P", "N", "G"), got, ref):
        assert abs(g - r) <= E.RTOL_A * ref[4], (name, g, r, abs(g - r) / ref[4])


# ---- 1. every instantiation, both edges ------------------------------------------------------------------------------------------
def test_the_matrix_covers_both_edges_of_every_instantiation():
    by = {}
    for k in range(2, _svils.SBM_MAX_K + 1):
        by.setdefault((_svils.sbm_variant(k)[0], S.row_lanes(k)), []).append(k)
    assert len(by) == 9
    ks = [k for k, _ in S.MATRIX]
    for key, members in by.items():
        assert members[0] in ks and members[-1] in ks, (key, members)
    assert [(c.n, c.K) for c in S.matrix_cases()] == [(S.MATRIX_N, k) for k in ks]


@pytest.mark.parametrize("case", S.matrix_cases(), ids=lambda c: "k%d" % c.K)
def test_matrix_against_the_restatement(case):
    h = _handle(case)
    npass, ms = h.estep()                                # the whole E-step
    rphi, rpass, rms = case.estep()
    assert npass == rpass and h.stats()[:2] == (rpass, rpass)
    _close(ms, rms)
    phi = h.state()[0]
    _close(phi, rphi)
    one = _sweep(h, case, 1)                             # whole iterations from the same start
    _against_iterate(one, case, 1)
    three = _sweep(h, case, S.MATRIX_ITERS)
    _against_iterate(three, case, S.MATRIX_ITERS)
    _against_elbo(h, case)                               # the bound at the state the handle holds after them
    if _svils.sbm_variant(case.K)[0] >= 2:               # the plain chain k_sbm_chain<1, V>: the same additions in the same order
        _same_bits(_sweep(h, case, S.MATRIX_ITERS, plain=True), three, "plain chain")
        h.set_state(case.phi, case.gamma, case.lam)
        npass1, ms1 = h.estep()
        assert npass1 == npass and np.array_equal(ms1, ms) and np.array_equal(h.state()[0], phi)
    h.close()


# ---- 2. rows longer than a wavefront ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K", S.HUBS)
def test_rows_longer_than_a_wavefront(n, K):
    case = S.hub_case(n, K, B)
    deg = np.bincount(case.links.ravel(), minlength=n)
    sdeg = np.bincount(case.skip.ravel(), minlength=n)
    assert all(deg[p] == n - 1 > 2 * 64 for p in S.hub_nodes(n, B)) and sdeg[1] > 64     # split_row: three trips, two trips
    h = _handle(case)
    npass, ms = h.estep()
    rphi, rpass, rms = case.estep()
    assert npass == rpass
    _close(ms, rms)
    _close(h.state()[0], rphi)
    ref = _sweep(h, case, S.LOOP_ITERS)
    _against_iterate(ref, case, S.LOOP_ITERS)
    for nodes in (1, B, B + 3, n):                       # where a block starts moves additions between the gather and the turn
        _same_bits(_sweep(h, case, S.LOOP_ITERS, nodes=nodes), ref, nodes)
    _same_bits(_sweep(h, case, S.LOOP_ITERS, plain=True), ref, "plain chain")
    h.close()


# ---- 3. link and skip lists longer than the lane groups' first trip -----------------------------------------------------------------
@pytest.mark.parametrize("d", S.DENSE, ids=lambda d: "n%d-k%d" % d[:2])
def test_lists_longer_than_the_first_trip(d):
    case = S.dense_case(*d)
    G = 64 // S.row_lanes(case.K)
    perl, pers = -(-case.links.shape[0] // LINK_WAVES), -(-case.skip.shape[0] // LINK_WAVES)
    trips = lambda per, g: len(range(g, per, G))         # of lane group g over a run of per pairs
    y = case.y_of(case.skip)
    print("%s: %d links, run %d; %d skipped pairs, run %d; %d lane groups" % (case.name, case.links.shape[0], perl, case.skip.shape[0], pers, G))
    assert G >= 2 and case.links.shape[0] >= 2 * perl and case.skip.shape[0] >= 2 * pers   # whole runs exist
    assert trips(perl, 1) >= 2                           # a lane group other than 0 goes round the link loop twice
    assert trips(pers, 1) >= 1 and pers == 3             # ... and takes a skipped pair
    for g in range(1, min(G, pers)):                     # of both y values, somewhere in the list
        mine = y[[e for w in range(LINK_WAVES) for e in range(w * pers + g, min((w + 1) * pers, y.shape[0]), G)]]
        assert 0 < mine.sum() < mine.shape[0], g
    assert (perl, G) == {4: (19, 16), 20: (11, 2)}[case.K]
    h = _handle(case)
    _against_iterate(_sweep(h, case, S.LOOP_ITERS), case, S.LOOP_ITERS)
    _against_elbo(h, case)
    h.close()


# ---- 4. pair likelihoods at K > 64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [65, 256])
def test_pair_loglik_above_one_trip(K):
    case = S.planted_case(S.MATRIX_N, K, dict(S.MATRIX)[K])
    h = _handle(case)
    h.sweep(1)
    phi, gamma, lam = h.state()
    rng = np.random.RandomState(3)
    pairs = np.array([(p, q) for p, q in rng.randint(0, case.n, (300, 2)) if p != q], dtype=np.uint32)
    y = rng.randint(0, 2, pairs.shape[0]).astype(np.uint8)
    assert pairs.shape[0] > 280 and 0 < y.sum() < y.shape[0]
    np.testing.assert_allclose(h.pair_loglik(pairs, y), S.pair_loglik(phi, lam, pairs, y), rtol=1e-9)
    h.close()


# ---- 5. partition sizes above the floor -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,seed", S.RINGS)
def test_partitions_above_the_floor(n, K, seed):
    case = S.ring_case(n, K, seed)
    nb = min(COLSUM_BLOCKS, -(-n // COLSUM_FLOOR))
    per = -(-n // nb)                                    # nodes of a block of k_sbm_colsum
    eper = max(_svils.SBMELBO_PIECE_ROWS, -(-n // _svils.SBMELBO_MAX_PIECES))   # rows of a piece of k_sbm_elbo_rows
    assert (per, eper) == {16500: (65, 16), 65553: (257, 17)}[n]
    h = _handle(case)
    # (a) the bound of the set state
    got = h.elbo()
    ref = E.elbo_prefix(case.phi, case.gamma, case.lam, case.eta, case.links, case.skip)
    print("%s: got %r ref %r A %.6e" % (case.name, got, ref[:4], ref[4]))
    assert got[0] == (got[1] + got[2]) + got[3]
    for name, g, r in zip(("total", "P", "N", "G"), got, ref):
        assert abs(g - r) <= E.RTOL_A * ref[4], (name, g, r, abs(g - r) / ref[4])
    # N is a sum of its own (k_sbm_elbo_rows and the fold of its pieces), and A is 10^4 times the addends of N here: N is held
    # to the same RTOL_A times the absolute sum of ITS addends as well, which a single lost row exceeds
    elogpi, _ = S.elog(case.gamma, case.lam)
    AN = np.abs(case.phi * elogpi).sum() + np.abs(E.entropy(case.phi))
    assert abs(got[2] - ref[2]) <= E.RTOL_A * AN, (got[2], ref[2], AN)
    # (b) the M-step of one iteration against the prefix-sum M-step of the phi read back
    one = _sweep(h, case, 1)
    phi, gamma, lam = one[:3]
    rgamma, rlam = S.mstep_prefix(phi, case.eta, case.links, case.skip)
    print("passes %r msums %r; gamma %r; lambda %r" % (one[4], one[3], gamma, lam))
    np.testing.assert_allclose(gamma, S.ALPHA + phi.sum(axis=0), rtol=1e-9)
    np.testing.assert_allclose(gamma, rgamma, rtol=1e-9)
    np.testing.assert_allclose(lam, rlam, rtol=1e-9)
    # (c) the rows of phi
    assert np.all(phi >= 0) and np.max(np.abs(phi.sum(axis=1) - 1.0)) <= 1e-12
    # (d) launch cuts and the plain chain
    for nodes in (1000, n):
        _same_bits(_sweep(h, case, 1, nodes=nodes), one, nodes)
    if n == S.RINGS[0][0]:
        _same_bits(_sweep(h, case, 1, plain=True), one, "plain chain")
    h.close()
