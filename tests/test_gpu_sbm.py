"""-m gpu: the svils_sbm handle (-single, svinet_amd/csrc/svils_sbm.hip) against the numpy restatement of tests/sbm_cases.py,
which forms every sum directly over the trained pairs -- the split into column sums and corrections is the device's alone.

phi is held at rtol 1e-7 (atol 1e-200: an entry that small enters no double-precision sum the engine forms), pass counts
exactly, msum, gamma and lambda at rtol 1e-7.  tests/test_sbm.py asserts, on the restatement alone, that no pass of any case
used here has its msum within 10 % of the exit threshold and that the E-step does not amplify a 1e-13 perturbation."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sbm_cases as S
from conftest import ROOT
from svinet_amd import _svils
from svinet_amd.host_api import SbmEngine

pytestmark = pytest.mark.gpu

SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
ERR_ARG, ERR_UNSUPPORTED = -1, -4
B = _svils.sbm_variant(4)[1]
RTOL = 1e-7


def _handle(case, state=True):
    h = _svils.Sbm(case.n, case.K, S.ALPHA, case.eta)
    h.set_graph(case.links, case.skip)
    if state:
        h.set_state(case.phi, case.gamma, case.lam)
    return h


def _close(got, ref):
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=1e-200)


# ---- the E-step and whole iterations against the restatement ---------------------------------------------------------------
@pytest.mark.parametrize("case", S.estep_cases(B), ids=lambda c: c.name)
def test_estep_against_the_restatement(case):
    h = _handle(case)
    npass, ms = h.estep(1)                               # one pass
    rphi, rpass, rms = case.estep(1)
    assert npass == rpass == 1
    _close(ms, rms)
    _close(h.state()[0], rphi)
    h.set_state(case.phi, case.gamma, case.lam)          # the whole E-step
    npass, ms = h.estep()
    rphi, rpass, rms = case.estep()
    assert npass == rpass and h.stats()[:2] == (rpass, rpass)
    _close(ms, rms)
    _close(h.stats()[2], rms)
    phi, gamma, lam = h.state()
    _close(phi, rphi)
    assert np.array_equal(gamma, case.gamma) and np.array_equal(lam, case.lam)   # the E-step moves phi alone
    h.close()


@pytest.mark.parametrize("nkseed", S.ITER_CASES, ids=lambda t: "n%d-k%d" % t[:2])
def test_iterations_against_the_restatement(nkseed):
    case = S.planted_case(*nkseed)
    h = _handle(case)
    got = {}
    for niter in (1, 3):
        h.set_state(case.phi, case.gamma, case.lam)
        h.sweep(niter)
        rphi, rgamma, rlam, rpasses, rms = case.iterate(niter)
        phi, gamma, lam = h.state()
        last, total, ms = h.stats()
        assert last == rpasses[-1] and total == sum(rpasses)
        _close(ms, rms[-1])
        _close(phi, rphi)
        _close(gamma, rgamma)
        _close(lam, rlam)
        got[niter] = (phi, gamma, lam)
    h.set_state(case.phi, case.gamma, case.lam)          # three sweeps of 1 are bitwise one sweep of 3
    for _ in range(3):
        h.sweep(1)
    for a, b in zip(h.state(), got[3]):
        assert np.array_equal(a, b)
    h.close()


# ---- in-block dependences: the smallest shapes where the look-ahead can go wrong ------------------------------------------
@pytest.mark.parametrize("case", S.block_cases(B), ids=lambda c: c.name)
def test_in_block_dependences(case):
    h = _handle(case)
    npass, ms = h.estep()
    rphi, rpass, rms = case.estep()
    assert npass == rpass
    _close(ms, rms)
    phi = h.state()[0]
    _close(phi, rphi)
    h.set_plain_chain(True)                              # the plain chain: the same additions in the same order
    h.set_state(case.phi, case.gamma, case.lam)
    npass1, ms1 = h.estep()
    assert npass1 == npass and np.array_equal(ms1, ms) and np.array_equal(h.state()[0], phi)
    h.close()


# ---- launch cuts, run to run, two handles ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nkseed", [(130, 4, 2), (61, 65, 1)], ids=lambda t: "n%d-k%d" % t[:2])
def test_launch_cuts_change_no_bit(nkseed):
    case = S.planted_case(*nkseed)

    def run(h, nodes, plain=False):
        h.set_launch_nodes(nodes)
        h.set_plain_chain(plain)
        h.set_state(case.phi, case.gamma, case.lam)
        h.sweep(2)
        return h.state() + h.stats()[2:] + (np.array(h.stats()[:2]),)

    h = _handle(case)
    ref = run(h, 0)
    for nodes in (1, B, B + 3, case.n, 0):               # (0 again: run to run)
        for a, b in zip(run(h, nodes), ref):
            assert np.array_equal(a, b), nodes
    for a, b in zip(run(h, B + 3, plain=True), ref):
        assert np.array_equal(a, b)
    h2 = _handle(case)                                   # a second handle
    for a, b in zip(run(h2, 0), ref):
        assert np.array_equal(a, b)
    h.close()
    h2.close()


# ---- early exit --------------------------------------------------------------------------------------------------------------
def test_early_exit():
    case = S.planted_case(*S.EARLY, state="peaked")
    rphi, rpass, rms = case.estep()
    assert rpass == 2                                    # (the restatement's: the case converges in two passes)
    h = _handle(case)
    npass, ms = h.estep()                                # ten passes queued, two run
    assert npass == 2 and ms.shape == (2,)
    _close(ms, rms)
    phi10 = h.state()[0]
    _close(phi10, rphi)
    h.set_state(case.phi, case.gamma, case.lam)
    npass, ms2 = h.estep(2)                              # nothing queued behind the second pass
    assert npass == 2 and np.array_equal(ms2, ms)
    assert np.array_equal(h.state()[0], phi10)           # the eight passes queued behind the raised flag left phi untouched
    h.set_state(case.phi, case.gamma, case.lam)
    npass, ms1 = h.estep(1)                              # max_passes = 1 stops at 1, converged or not
    assert npass == 1 and ms1[0] == ms[0] and ms1[0] > S.THRESH
    _close(h.state()[0], case.estep(1)[0])
    h.close()


# ---- pair likelihoods ------------------------------------------------------------------------------------------------------------
def test_pair_loglik():
    case = S.planted_case(61, 7, 1)
    h = _handle(case)
    h.sweep(1)
    phi, gamma, lam = h.state()
    rng = np.random.RandomState(3)
    pairs = np.array([(p, q) for p, q in rng.randint(0, case.n, (300, 2)) if p != q], dtype=np.uint32)
    y = rng.randint(0, 2, pairs.shape[0]).astype(np.uint8)
    np.testing.assert_allclose(h.pair_loglik(pairs, y), S.pair_loglik(phi, lam, pairs, y), rtol=1e-9)
    h.close()
    # a pair clamped at 1e-30: both nodes surely in group 0, whose rate is 1e-40
    n, K = 4, 3
    phi = np.zeros((n, K))
    phi[:, 0] = 1.0
    phi[3] = (0.2, 0.3, 0.5)
    lam = np.array([(1e-40, 1.0), (2.0, 3.0), (1.0, 1.0), (0.5, 9.0)])
    h = _svils.Sbm(n, K, S.ALPHA, S.eta_of(K))
    h.set_graph([(0, 1)])
    h.set_state(phi, np.ones(K), lam)
    pairs, y = np.array([(0, 1), (3, 0), (2, 3), (3, 1)], dtype=np.uint32), np.array([1, 1, 1, 0], dtype=np.uint8)
    got, ref = h.pair_loglik(pairs, y), S.pair_loglik(phi, lam, pairs, y)
    assert ref[0] == np.log(1e-30) and np.all(ref[1:] > -5)
    np.testing.assert_allclose(got, ref, rtol=1e-9)
    h.close()


# ---- argument errors leave the state as it is -------------------------------------------------------------------------------------
def test_argument_errors_leave_the_state_untouched():
    L = _svils.load()
    case = S.planted_case(61, 7, 1)
    h = _handle(case)
    ref = case.estep()

    def refused(fn, word):
        with pytest.raises(_svils.SvilsError) as ei:
            fn()
        assert ei.value.code == ERR_ARG and word in str(ei.value), str(ei.value)

    assert L.svils_sbm_sweep(None, 1) == ERR_ARG and L.svils_sbm_estep(None, 1, None, None) == ERR_ARG   # null handle
    assert L.svils_sbm_get_state(None, None, None, None) == ERR_ARG
    refused(lambda: h.set_graph([(0, 61)]), "is not a pair p < q < n")                      # node >= n
    refused(lambda: h.set_graph([(5, 5)]), "is not a pair p < q < n")                       # self pair
    refused(lambda: h.set_graph(case.links, [(3, 2)]), "skipped pair 0")
    refused(lambda: h.set_graph(np.concatenate([case.links, case.links[:1]])), "is repeated")
    bad = case.phi.copy()
    bad[9, 0] += 1e-6
    refused(lambda: h.set_state(bad, case.gamma, case.lam), "row 9 of phi does not sum to 1")
    bad = case.phi.copy()
    bad[9, 0] = np.nan
    refused(lambda: h.set_state(bad, case.gamma, case.lam), "phi[9][0]")
    lam = case.lam.copy()
    lam[7, 1] = 0.0
    refused(lambda: h.set_state(case.phi, case.gamma, lam), "lambda[7][1]")
    refused(lambda: h.pair_loglik([(4, 4)], [1]), "is not a pair of two nodes")
    refused(lambda: h.estep(0), "max_passes")
    refused(lambda: h.estep(11), "max_passes")
    for a, b in zip(h.state(), (case.phi, case.gamma, case.lam)):                           # the state and the graph are as they were
        assert np.array_equal(a, b)
    npass, ms = h.estep()
    assert npass == ref[1]
    _close(h.state()[0], ref[0])
    h.close()
    out = ctypes.c_void_p()
    eta = S.eta_of(257)
    assert L.svils_sbm_create(0, 10, 257, 0.5, eta.ctypes.data, ctypes.byref(out)) == ERR_UNSUPPORTED and not out.value
    g = _svils.Sbm(10, 4, S.ALPHA, S.eta_of(4))
    refused(lambda: g.sweep(1), "set the graph and the state first")
    g.close()


# ---- the host engine and the command line on the device against -host-loops (LFR, n = 1000, K = 28) ------------------------------
def test_engine_on_the_device_against_host_loops(graph_files):
    dev = SbmEngine(graph_files["lfr"], 1000, 28, seed=S.LFR_SEED, on_device=True)
    host = SbmEngine(graph_files["lfr"], 1000, 28, seed=S.LFR_SEED, on_device=False)
    for name in ("heldout", "validation", "precision", "phi", "gamma", "lam"):
        assert np.array_equal(getattr(dev, name), getattr(host, name)), name
    for _ in range(2):
        dev.sweep()
        host.sweep()
        assert dev.passes == host.passes
        _close(dev.msums, host.msums)
    _close(dev.phi, host.phi)
    _close(dev.gamma, host.gamma)
    _close(dev.lam, host.lam)
    assert dev.rows.shape == host.rows.shape == (6, 8)
    _close(dev.rows, host.rows)
    dev.close()
    host.close()


def test_cli_on_the_device_against_host_loops(graph_files, tmp_path):
    out = {}
    for name, extra in (("dev", []), ("host", ["-host-loops"])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([SVINET, "-file", graph_files["lfr"], "-n", "1000", "-k", "28", "-single", "-max-iterations", "2", "-seed", str(S.LFR_SEED)] + extra,
                           capture_output=True, text=True, timeout=300, cwd=str(d))
        assert r.returncode == 0, r.stderr
        out[name] = d / ("n1000-k28-mmsb-seed%d-sbm" % S.LFR_SEED)
    for f in ("heldout-pairs.txt", "validation-pairs.txt"):                  # the same samples, byte for byte
        assert (out["dev"] / f).read_bytes() == (out["host"] / f).read_bytes() and (out["dev"] / f).stat().st_size > 10
    for f, cols in (("phi.txt", 30), ("gamma.txt", 2), ("lambda.txt", 3)):   # equal at the printed 5 decimals, up to one unit
        a, b = np.loadtxt(out["dev"] / f), np.loadtxt(out["host"] / f)
        assert a.shape == b.shape and a.shape[1] == cols
        assert np.max(np.abs(a - b)) <= 1.0001e-5, f
    for f in ("heldout.txt", "validation.txt"):
        a, b = np.loadtxt(out["dev"] / f), np.loadtxt(out["host"] / f)
        assert a.shape == b.shape == (3, 11)
        np.testing.assert_allclose(a[:, [2, 4, 6]], b[:, [2, 4, 6]], rtol=RTOL)
        assert np.array_equal(a[:, [0, 3, 5, 7, 8, 9, 10]], b[:, [0, 3, 5, 7, 8, 9, 10]])
