"""-m gpu: svils_sbmelbo (-single-logl, svinet_amd/csrc/svils_sbm.hip: k_sbm_elbo_rows, k_sbm_elbo_fold) against the numpy
restatement of tests/sbm_elbo_cases.py, which sums directly over the trained pairs -- the split into column sums and link / skip
corrections is the device's alone.

P, N, G and the total are held to 1e-9 A, A the sum of the absolute values of all addends of the total as the restatement
reports it (tests/sbm_elbo_cases.py derives the figure).  The restatement is evaluated at the state the DEVICE holds, so no
trajectory tolerance enters.  Repeated passes are held to equal bits."""
import os
import subprocess

import numpy as np
import pytest

import sbm_cases as S
import sbm_elbo_cases as E
from conftest import ROOT
from svinet_amd import _svils
from svinet_amd.host_api import SbmEngine

pytestmark = pytest.mark.gpu

SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
B = _svils.sbm_variant(4)[1]
PIECE = _svils.SBMELBO_PIECE_ROWS        # rows of one piece (= one partial sum, one wavefront) of k_sbm_elbo_rows


def _handle(case, state=None):
    h = _svils.Sbm(case.n, case.K, S.ALPHA, case.eta)
    h.set_graph(case.links, case.skip)
    h.set_state(*(state if state is not None else (case.phi, case.gamma, case.lam)))
    return h


def _check(h, case, what=""):
    """the four outputs against the restatement at the handle's own state -> (outputs, A)"""
    got = h.elbo()
    ref = E.case_elbo(case, h.state())
    print("%s %s: got %r ref %r A %.6e" % (case.name, what, got, ref[:4], ref[4]))
    assert got[0] == (got[1] + got[2]) + got[3]
    for name, g, r in zip(("total", "P", "N", "G"), got, ref):
        assert abs(g - r) <= E.RTOL_A * ref[4], (name, g, r, abs(g - r) / ref[4])
    return got, ref[4]


# ---- against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.estep_cases(B) + S.block_cases(B), ids=lambda c: c.name)
def test_against_the_restatement(case):
    h = _handle(case)
    assert h.elbo_timing() == -1.0
    _check(h, case, "start")
    h.sweep(1)
    _check(h, case, "after one iteration")
    assert h.elbo_timing() > 0
    h.close()


@pytest.mark.parametrize("K", [4, 65])
@pytest.mark.parametrize("n", [PIECE - 1, PIECE, PIECE + 1, 2 * PIECE - 1, 2 * PIECE, 2 * PIECE + 1])
def test_row_kernel_piece_edges(n, K):
    """n one below, at and above one and two pieces of the row kernel (_svils.SBMELBO_PIECE_ROWS rows each)"""
    case = S.planted_case(n, K, 4)
    h = _handle(case)
    _check(h, case)
    h.close()


def test_one_hot_phi():
    """phi exactly 0 and 1: finite, equal to the restatement, and the entropy part is 0 -- N is sum_p Elogpi[group of p]"""
    for n, K in ((61, 4), (33, 65)):
        case = S.planted_case(n, K, 1 if n == 61 else 4)
        phi, gamma, lam = E.one_hot_state(n, K)
        h = _handle(case, (phi, gamma, lam))
        got, A = _check(h, case, "one-hot")
        assert np.isfinite(got).all() and E.entropy(phi) == 0.0
        elogpi, _ = S.elog(gamma, lam)
        assert abs(got[2] - elogpi[S.groups_of(n, K)].sum()) <= E.RTOL_A * A
        h.close()


# ---- bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nkseed", [(130, 4, 2), (61, 65, 1)], ids=lambda t: "n%d-k%d" % t[:2])
def test_equal_bits(nkseed):
    case = S.planted_case(*nkseed)

    def run(h, nodes, plain=False):
        h.set_launch_nodes(nodes)
        h.set_plain_chain(plain)
        h.set_state(case.phi, case.gamma, case.lam)
        first = h.elbo()
        h.sweep(2)
        return first + h.elbo()

    h = _handle(case)
    ref = run(h, 0)
    assert h.elbo() == ref[4:] and h.elbo() == ref[4:]                   # run to run
    for nodes in (1, B, case.n, 0):                                      # every launch cut
        assert run(h, nodes) == ref, nodes
    assert run(h, B, plain=True) == ref                                  # the plain chain
    h2 = _handle(case)                                                   # a second handle
    assert run(h2, 0) == ref
    h.close()
    h2.close()


def test_a_pass_changes_nothing_a_sweep_reads():
    case = S.planted_case(130, 4, 2)
    h, g = _handle(case), _handle(case)
    for x in (h, g):
        x.sweep(1)
    before = h.state() + h.stats() + (h.timing(),)
    h.elbo()
    h.elbo()
    after = h.state() + h.stats() + (h.timing(),)
    for a, b in zip(before, after):                                      # phi, gamma, lambda, the stats, the timing
        assert np.array_equal(a, b)
    for x in (h, g):                                                     # a sweep after a pass = the sweep of a handle without
        x.sweep(1)
    for a, b in zip(h.state() + h.stats(), g.state() + g.stats()):
        assert np.array_equal(a, b)
    npass, ms = h.estep(1)                                               # ... and an E-step pass after one
    h.elbo()
    npass2, ms2 = g.estep(1)
    assert npass == npass2 and np.array_equal(ms, ms2) and np.array_equal(h.state()[0], g.state()[0])
    h.close()
    g.close()


# ---- monotone -------------------------------------------------------------------------------------------------------------------------
def test_estep_passes_do_not_lower_the_bound():
    case = S.planted_case(97, 7, 2)
    h = _handle(case)
    A = E.case_elbo(case)[4]
    prev = h.elbo()[0]
    for it in range(6):
        h.estep(1)
        cur = h.elbo()[0]
        print("pass %d: %.9f (step %.3e, A %.3e)" % (it, cur, cur - prev, A))
        assert cur - prev >= -E.RTOL_A * A
        prev = cur
    h.close()


# ---- the engine and the command line against -host-loops ----------------------------------------------------------------------------
def test_engine_rows_against_host_loops(graph_files):
    """two iterations on the LFR golden graph: the rows at the trajectory tolerance tests/test_gpu_sbm.py justifies"""
    dev = SbmEngine(graph_files["lfr"], 1000, 28, seed=S.LFR_SEED, on_device=True, logl=True)
    host = SbmEngine(graph_files["lfr"], 1000, 28, seed=S.LFR_SEED, on_device=False, logl=True)
    np.testing.assert_allclose(dev.elbo(), host.elbo(), rtol=1e-7)        # the start state: the same bits on both
    for _ in range(2):
        dev.sweep()
        host.sweep()
    print(dev.logl_rows, host.logl_rows)
    assert dev.logl_rows.shape == host.logl_rows.shape == (2, 2) and list(dev.logl_rows[:, 0]) == [0, 1]
    np.testing.assert_allclose(dev.logl_rows, host.logl_rows, rtol=1e-7)
    assert dev.stop_rule_verdict == host.stop_rule_verdict == 0
    c10, c100, c1000 = dev.precision_counts()                             # svils_sbm_pair_loglik with y = 1 for every pair
    assert 0 <= c10 <= c100 <= c1000 <= 10
    dev.close()
    host.close()


def test_cli_on_the_device_against_host_loops(graph_files, tmp_path):
    out = {}
    for name, extra in (("dev", []), ("host", ["-host-loops"])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([SVINET, "-file", graph_files["assort"], "-n", "75", "-k", "4", "-heldout-ratio", "0.1", "-single-logl",
                            "-max-iterations", "1000"] + extra, capture_output=True, text=True, timeout=300, cwd=str(d))
        assert r.returncode == 0, r.stderr
        out[name] = d / "n75-k4-mmsb-sbm"
    dev, host = (np.loadtxt(out[w] / "logl.txt", ndmin=2) for w in ("dev", "host"))
    print(dev, host)
    assert dev.shape == host.shape and dev.shape[0] < 1000                 # the same iteration ...
    rule = {w: sorted(p.name for p in out[w].iterdir() if p.name in ("done.txt", "max.txt")) for w in out}
    assert rule["dev"] == rule["host"] and len(rule["dev"]) == 1           # ... by the same rule
    assert np.array_equal(dev[:, 0], host[:, 0])
    assert np.max(np.abs(dev[:, 2] - host[:, 2])) <= 1.0001e-5             # the printed digits, up to one unit of the fifth
    for f, cols in (("precision.txt", 5), ("hitcurve_0.txt", 2)):          # (ranks of near-tied pairs may differ: the shapes only)
        a, b = np.loadtxt(out["dev"] / f, ndmin=2), np.loadtxt(out["host"] / f, ndmin=2)
        assert a.shape == b.shape == (1, cols) and a[0, 0] == b[0, 0]
    for f in ("phi.txt", "gamma.txt", "lambda.txt"):
        assert np.max(np.abs(np.loadtxt(out["dev"] / f) - np.loadtxt(out["host"] / f))) <= 1.0001e-5, f
