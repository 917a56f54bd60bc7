"""-m "not gpu": the variational lower bound of the -single engine (-single-logl; svinet_amd/host/sbm.cc).
The restatement of tests/sbm_elbo_cases.py against the reference's literal loops; the -host-loops engine against the restatement;
what the bound does across an E-step pass and across the M-step, on the restatement alone; the stop rules, compute_precision's
ranking, the command line, and the device library's answers without a device.

Every comparison with the restatement is held to 1e-9 A, A the sum of the absolute values of all addends of the total
(tests/sbm_elbo_cases.py derives it)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sbm_cases as S
import sbm_elbo_cases as E
from conftest import GOLDEN, ROOT
from svinet_amd import _svils
from svinet_amd.host_api import SbmEngine, sbm_rank_precision

ASSORT = os.path.join(GOLDEN, "graphs", "assort-75-4.txt")
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
ERR_ARG = -1
B = _svils.sbm_variant(4)[1]
MODEL_FILES = {"phi.txt", "lambda.txt", "gamma.txt"}
ASSORT_ARGS = ["-file", ASSORT, "-n", "75", "-k", "4", "-heldout-ratio", "0.1", "-host-loops"]


def _engine_case(eng):
    c = S.Case("engine", eng.n, eng.k, np.sort(eng.edges, axis=1), eng.skip, (eng.phi, eng.gamma, eng.lam))
    c.eta = eng.eta
    return c


# ---- the restatement against the reference's loops ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", [S.planted_case(12, 3, 5), S.planted_case(9, 2, 6, "peaked")], ids=lambda c: c.name)
def test_restatement_against_the_literal_loops(case):
    T, Y = case.masks()
    total, P, N, G, A = E.case_elbo(case)
    s, A1 = E.literal_elbo(case.phi, case.gamma, case.lam, case.eta, T, Y)
    print("total %.12f literal %.12f A %.6f" % (total, s, A))
    assert abs(total - s) <= 1e-12 * A and abs(A - A1) <= 1e-12 * A
    assert total == P + N + G and A > abs(total)


# ---- the host loops against the restatement -----------------------------------------------------------------------------------
def test_host_loops_against_the_restatement():
    eng = SbmEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    for it in range(3):                                          # the start state, and the states after one and two iterations
        ref = E.case_elbo(_engine_case(eng))
        got = eng.elbo()
        print(it, got, ref)
        assert got[0] == (got[1] + got[2]) + got[3]
        np.testing.assert_allclose(got, ref[:4], rtol=0, atol=E.RTOL_A * ref[4])
        eng.sweep()
    assert eng.logl_rows.shape == (0, 2) and eng.stop_rule_verdict == 0   # logl=False: no row, no rule


# ---- what the bound does across the two steps, on the restatement alone ----------------------------------------------------------
@pytest.mark.parametrize("case", S.all_cases(B), ids=lambda c: c.name)
def test_an_estep_pass_does_not_lower_the_bound(case):
    """the E-step is the exact coordinate update of every row of phi for THIS bound (the constant the softmax cancels is the
    only difference): a pass from the case's state, and one from the state after one iteration, may lose rounding alone"""
    T, Y = case.masks()
    b0 = E.case_elbo(case)
    b1 = E.case_elbo(case, (case.estep(1)[0], case.gamma, case.lam))
    phi1 = case.estep()[0]
    gamma1, lam1 = S.mstep(phi1, case.eta, T, Y)
    c0 = E.case_elbo(case, (phi1, gamma1, lam1))
    c1 = E.case_elbo(case, (S.estep(phi1, gamma1, lam1, T, Y, 1)[0], gamma1, lam1))
    print("steps %.6e %.6e  A %.6e" % (b1[0] - b0[0], c1[0] - c0[0], b0[4]))
    assert b1[0] - b0[0] >= -E.RTOL_A * b0[4]
    assert c1[0] - c0[0] >= -E.RTOL_A * c0[4]


def test_the_mstep_lowers_the_bound():
    """row K of lambda sums 1 - phi_ik phi_jk over k (src/sbm.cc:512-515), the bound's pair term has 1 - sum_k: the M-step is not
    the coordinate update of this bound, and the first one of the peaked case lowers it by more than 30"""
    case = S.planted_case(61, 4, 1, "peaked")
    T, Y = case.masks()
    phi1 = case.estep()[0]
    before = E.case_elbo(case, (phi1, case.gamma, case.lam))[0]
    after = E.case_elbo(case, (phi1,) + S.mstep(phi1, case.eta, T, Y))[0]
    print("before %.2f after %.2f" % (before, after))
    assert before - after > 30


def test_exact_zeros_add_nothing():
    case = S.planted_case(61, 4, 1)
    phi, gamma, lam = E.one_hot_state(61, 4)
    total, P, N, G, A = E.case_elbo(case, (phi, gamma, lam))
    assert np.isfinite([total, P, N, G, A]).all() and E.entropy(phi) == 0.0
    elogpi, _ = S.elog(gamma, lam)
    assert abs(N - elogpi[S.groups_of(61, 4)].sum()) <= E.RTOL_A * A


# ---- the stop rules ------------------------------------------------------------------------------------------------------------
def test_stop_rules_on_made_up_sequences():
    def engine(stop=True):
        return SbmEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False, logl=True, stop=stop)

    # the gain rule: s > prev, prev != 0, |(s - prev) / prev| < 1e-5
    assert engine().feed_stop_rule([(0, -100.0), (1, -90.0), (2, -89.9995)]) == [0, 0, 2]
    assert engine().feed_stop_rule([(0, -100.0), (1, -90.0), (2, -89.99)]) == [0, 0, 0]          # a gain of 1.1e-4
    assert engine().feed_stop_rule([(0, 0.0), (1, 1e-9)]) == [0, 0]                              # prev == 0 never fires
    # the drop rule: below the maximum at more than 3 reports with iter > 10
    seq = [(0, -50.0)] + [(i, -60.0 - i) for i in range(1, 20)]
    assert engine().feed_stop_rule(seq) == [0] * 14 + [1]                                        # iters 11, 12, 13, 14: the fourth
    # a new maximum clears the count
    seq = [(0, -50.0), (11, -60.0), (12, -61.0), (13, -62.0), (14, -40.0), (15, -45.0), (16, -46.0), (17, -47.0), (18, -48.0)]
    assert engine().feed_stop_rule(seq) == [0] * 8 + [1]
    # -no-stop: neither rule answers
    assert engine(stop=False).feed_stop_rule([(0, -100.0), (1, -90.0), (2, -89.9995)] + seq[1:]) == [0] * 11


# ---- compute_precision ------------------------------------------------------------------------------------------------------------
def test_compute_precision_on_a_hand_made_ranking():
    m = 2100
    pairs = np.stack([np.arange(m), np.arange(m) + 1], axis=1).astype(np.uint32)
    score = -np.arange(m, dtype=np.float64)                      # pair i has rank i
    y = np.zeros(m, dtype=np.uint8)
    y[[0, 3, 9, 10, 50, 99, 100, 500, 999, 1000, 2000]] = 1
    perm = np.random.RandomState(4).permutation(m)               # the order given does not matter
    counts, curve = sbm_rank_precision(pairs[perm], score[perm], y[perm])
    assert counts == (3, 6, 9)                                   # cumulative: first 10, first 100, first 1000
    assert curve.tolist() == [[1, 1], [1000, 9], [2000, 10]]     # rank 1 and every 1000th
    # ties: broken by the ascending pair
    pairs = np.array([(5, 9), (2, 7), (2, 3), (1, 8)], dtype=np.uint32)
    counts, curve = sbm_rank_precision(pairs, [0.5, 0.5, 0.5, 0.1], [0, 0, 1, 1])
    assert counts == (2, 2, 2) and curve.tolist() == [[1, 1]]    # (2, 3) ranks first
    counts, curve = sbm_rank_precision(pairs, [0.5, 0.5, 0.5, 0.1], [1, 0, 0, 0])
    assert curve.tolist() == [[1, 0]] and counts == (1, 1, 1)


def test_engine_precision_counts():
    eng = SbmEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False, logl=True)
    eng.sweep()
    case = _engine_case(eng)
    ll = S.pair_loglik(eng.phi, eng.lam, eng.precision, np.ones(len(eng.precision), dtype=np.uint8))
    order = np.lexsort((eng.precision[:, 1], eng.precision[:, 0], -ll))
    y = case.y_of(eng.precision[order])
    assert eng.precision_counts() == (int(y[:10].sum()), int(y[:100].sum()), int(y[:1000].sum()))


# ---- the device library without a device ----------------------------------------------------------------------------------------
def test_library_answers_without_a_device():
    L = _svils.load()
    for name in ("svils_sbmelbo", "svils_sbmelbo_get_timing"):
        assert name in _svils.EXPORTS and hasattr(L, name)
    assert L.svils_abi_version() == 8
    out = (ctypes.c_double * 4)()
    assert L.svils_sbmelbo(None, out) == ERR_ARG and b"null handle" in L.svils_last_error()
    assert L.svils_sbmelbo_get_timing(None, out) == ERR_ARG


# ---- the command line -----------------------------------------------------------------------------------------------------------
def _run(args, cwd, timeout=300):
    return subprocess.run([SVINET] + args, capture_output=True, text=True, timeout=timeout, cwd=str(cwd))


@pytest.mark.parametrize("args,word", [
    (["-batch"], "-batch"),
    (["-batch-gpu"], "-batch"),
    (["-link-sampling"], "-link-sampling"),
    (["-rnode"], "-rnode"),
    (["-rpair"], "-rpair"),
    (["-stratified"], "-stratified"),
    (["-snode"], "-snode"),
    (["-infset"], "-infset"),
    (["-preprocess"], "-preprocess"),
    (["-orig"], "-orig"),
    (["-findk"], "-findk"),
    (["-gml"], "-gml"),
    (["-lcstats"], "-lcstats"),
    (["-ppc"], "-ppc"),
    (["-ppc-orig"], "-ppc-orig"),
    (["-gen"], "-gen"),
    (["-sparse-graph"], "-sparse-graph"),
    (["-logl"], "-logl"),
    (["-gpus", "2"], "-gpus"),
    (["-kshard"], "-kshard"),
    (["-minibatch", "10"], "-minibatch"),
    (["-scale", "2"], "-scale"),
    (["-load", "x/"], "-load"),
    (["-predict-pairs", "x"], "-predict-pairs"),
    (["-recommend", "3"], "-recommend"),
    (["-rank-pairs", "x"], "-rank-pairs"),
    (["-rank-heldout"], "-rank-heldout"),
    (["-adamic-adar"], "-adamic-adar"),
    (["-k", "257"], "SVILS_SBM_MAX_K"),
    (["-no-stop"], "-max-iterations"),
])
def test_cli_refusals_create_nothing(tmp_path, args, word):
    """everything -single is refused with, with and without -max-iterations; -no-stop alone: -single's message"""
    for more in ([], ["-max-iterations", "3"]):
        if word == "-max-iterations" and more:
            continue
        r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-single-logl"] + more + args, tmp_path)
        assert r.returncode == 2 and word in r.stderr and "-single" in r.stderr, (r.returncode, r.stderr)
        assert word in ("-max-iterations", "SVILS_SBM_MAX_K") or "-single-logl" in r.stderr   # (those two: -single's own messages)
        assert not list(tmp_path.iterdir())


def test_cli_single_with_logl_is_still_refused_and_the_new_flag_is_known(tmp_path):
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-single", "-logl", "-max-iterations", "3"], tmp_path)
    assert r.returncode == 2 and not list(tmp_path.iterdir())
    assert r.stderr == "error: -single is not available with -logl (an engine of its own: single GPU, its own output directory)\n"
    assert "-single-logl" in _run(["-help"], tmp_path).stdout


@pytest.fixture(scope="module")
def assort_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("sbm_logl")
    r = _run(ASSORT_ARGS + ["-single-logl", "-max-iterations", "1000"], d)
    assert r.returncode == 0, r.stderr
    return d


def test_cli_host_loops_run_ends_by_a_rule(assort_run):
    assert [p.name for p in assort_run.iterdir()] == ["n75-k4-mmsb-sbm"]
    d = assort_run / "n75-k4-mmsb-sbm"
    names = {p.name for p in d.iterdir()}
    rows = np.loadtxt(d / "logl.txt", ndmin=2)
    iters = rows.shape[0]
    print("ended after %d iterations; %s" % (iters, sorted(names & {"done.txt", "max.txt"})))
    assert 2 <= iters < 1000 and list(rows[:, 0]) == list(range(iters))      # one row per iteration, a rule below the cap
    assert len(names & {"done.txt", "max.txt"}) == 1
    eng = SbmEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False, logl=True)   # the library engine is the command line's
    while eng.stop_rule_verdict == 0:
        assert eng.iter < iters
        eng.sweep()
    assert eng.iter == iters and eng.logl_rows.shape == (iters, 2)
    assert ("max.txt" if eng.stop_rule_verdict == 1 else "done.txt") in names
    assert np.array_equal(eng.logl_rows[:, 0], rows[:, 0])
    np.testing.assert_allclose(rows[:, 2], eng.logl_rows[:, 1], rtol=0, atol=5.1e-6)   # %.5f
    for l in (d / "logl.txt").read_text().splitlines():
        assert len(l.split("\t")) == 3 and len(l.split("\t")[2].split(".")[1]) == 5
    if "done.txt" in names:
        done = (d / "done.txt").read_text().split("\t")
        assert int(done[0]) == iters - 1 and float(done[2]) == rows[-1, 2]
    else:
        mx = (d / "max.txt").read_text().split("\t")
        assert len(mx) == 10 and int(mx[0]) == iters - 1 and float(mx[2]) == rows[-1, 2] and float(mx[3]) == 0 and int(mx[9]) == 1
        assert float(mx[5]) == rows[:, 2].max()
    prec = np.loadtxt(d / "precision.txt", ndmin=2)
    assert prec.shape == (1, 5) and prec[0, 0] == iters - 1 and tuple(prec[0, 2:]) == eng.precision_counts()
    assert prec[0, 2] <= prec[0, 3] <= prec[0, 4] <= 10                        # the precision sample has 10 links
    hc = np.loadtxt(d / "hitcurve_0.txt", ndmin=2)
    assert hc.shape == (1, 2) and hc[0, 0] == 1 and hc[0, 1] in (0, 1)
    assert MODEL_FILES <= names
    assert np.loadtxt(d / "phi.txt").shape == (75, 6)
    np.testing.assert_allclose(np.loadtxt(d / "phi.txt")[:, 2:], eng.phi, atol=5.1e-6)
    for f in ("heldout.txt", "validation.txt"):                                # the constructor's row, one per iteration
        assert len((d / f).read_text().splitlines()) == iters + 1


def test_cli_without_the_flag_writes_what_it_wrote(assort_run, tmp_path):
    """the same run without -single-logl (capped where the rule ended it): an empty logl.txt, and none of the new files; with the
    flag and a cap below the rule's iteration: the rows, precision.txt and the hit curve, and no max.txt / done.txt"""
    with_flag = assort_run / "n75-k4-mmsb-sbm"
    iters = len((with_flag / "logl.txt").read_text().splitlines())
    r = _run(ASSORT_ARGS + ["-single", "-max-iterations", str(iters)], tmp_path)
    assert r.returncode == 0, r.stderr
    d = tmp_path / "n75-k4-mmsb-sbm"
    names = {p.name for p in d.iterdir()}
    assert names == {"convergence.txt", "gamma.txt", "heldout-pairs.txt", "heldout.txt", "infer.log", "lambda.txt", "logl.txt",
                     "modularity.txt", "network.dat", "param.txt", "phi.txt", "precision.txt", "time.txt", "validation-pairs.txt",
                     "validation.txt"}
    assert {p.name for p in with_flag.iterdir()} - names in ({"done.txt", "hitcurve_0.txt"}, {"max.txt", "hitcurve_0.txt"})
    assert (d / "logl.txt").read_text() == "" and (d / "precision.txt").read_text() == ""
    for f in ("phi.txt", "lambda.txt", "gamma.txt", "heldout-pairs.txt", "validation-pairs.txt"):   # the flag changes no iteration
        assert (d / f).read_bytes() == (with_flag / f).read_bytes(), f
    capped = tmp_path / "capped"
    capped.mkdir()
    r = _run(ASSORT_ARGS + ["-single-logl", "-no-stop", "-max-iterations", "2"], capped)
    assert r.returncode == 0, r.stderr
    c = capped / "n75-k4-mmsb-sbm"
    assert {p.name for p in c.iterdir()} == names | {"hitcurve_0.txt"}
    assert np.array_equal(np.loadtxt(c / "logl.txt")[:, [0, 2]], np.loadtxt(with_flag / "logl.txt")[:2, [0, 2]])   # (column 1: seconds)
    assert np.loadtxt(c / "precision.txt", ndmin=2).shape == (1, 5)
