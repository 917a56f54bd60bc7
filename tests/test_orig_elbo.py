"""-orig -logl without a device: the restatement of the lower bound (tests/orig_elbo_cases.py) against its literal loops, the
host loops of the engine against the restatement (rtol 1e-9, the project's figure for -logl; the round
total exact), the one-orientation skip, the stop rules on made-up sequences, the command line (rows of logl.txt, a run that
ends by a rule, what is accepted and refused) and the null-handle / no-device answers of the new entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orig_cases as OC
import orig_elbo_cases as EC
from conftest import GOLDEN
from svinet_amd import _svils
from svinet_amd.host_api import OrigEngine, orig_stop_rule

ERR_ARG, ERR_DEVICE = -1, -2
RTOL = 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
ASSORT = os.path.join(GOLDEN, "graphs", "assort-75-4.txt")
GO, DROP, GAIN = 0, 1, 2


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _skip_of(e):
    return [tuple(int(x) for x in r) for r in e.heldout]


@pytest.mark.parametrize("k,n,seed,peaked", [(2, 9, 1, False), (3, 12, 2, True), (5, 11, 3, True), (17, 7, 4, False)])
def test_restatement_against_literal_loops(k, n, seed, peaked):
    links, gamma, beta = (OC.peaked_state if peaked else OC.plain_state)(seed, n, k)
    adj = OC.adjacency(n, links)
    skip = [(0, 1), (n - 1, 2)]
    r = EC.elbo(gamma, beta, adj, skip, 1.0 / k)
    total, P, N, rounds = EC.elbo_loops(gamma, beta, adj, skip, 1.0 / k)
    assert len(r["pair"]) == n * (n - 1) - 2 and int(r["rounds"].sum()) == rounds
    np.testing.assert_allclose([r["total"], r["P"], r["N"]], [total, P, N], rtol=1e-12)
    EC.check_conditions(r, beta, peaked=False)


def test_an_exact_zero_in_phi_adds_nothing():
    assert EC.xlogx(np.array([0.0, 1.0, 0.5])).tolist() == [0.0, 0.0, 0.5 * np.log(0.5)]


@pytest.mark.parametrize("k,seed", [(4, 41), (17, 42)])
def test_host_loops_against_the_restatement(k, seed):
    """the peaked states of tests/test_orig.py, before and after a sweep; the bound rises"""
    e = OrigEngine(ASSORT, 75, k, heldout_ratio=0.1, on_device=False)
    adj, skip = OC.adjacency(e.n, e.edges), _skip_of(e)
    _, gamma, beta = OC.peaked_state(seed, 75, k)
    e.set_state(gamma, beta)
    seen = []
    for it in range(2):
        r = EC.elbo(e.gamma, e.beta, adj, skip, 1.0 / k)
        EC.check_conditions(r, e.beta, peaked=it == 0)   # (after a sweep no pair need run to the cap)
        got = e.elbo()
        print("k %d: device-free engine %r restatement %r" % (k, got, (r["total"], r["P"], r["N"])))
        np.testing.assert_allclose(got, [r["total"], r["P"], r["N"]], rtol=RTOL)
        assert got[0] == got[1] + got[2]
        assert e.elbo_stats == (75 * 74 - len(set(skip)), int(r["rounds"].sum()))
        seen.append(got[0])
        e.sweep()
    assert seen[1] > seen[0]


def test_one_orientation_skips_leave_out_exactly_their_terms():
    one = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    both = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    skip = _skip_of(one)
    rev = sorted({(q, p) for p, q in skip if (q, p) not in skip})   # (a held-out pair drawn twice is listed twice)
    assert rev
    both.skip_also(rev)
    adj = OC.adjacency(one.n, one.edges)
    r = EC.elbo(one.gamma, one.beta, adj, skip, 0.25)
    p, q = OC.ordered_pairs(75, skip)
    idx = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(p, q))}
    left_out = sum(r["pair"][idx[pq]] for pq in rev)
    a, b = one.elbo(), both.elbo()
    assert one.elbo_stats[0] == both.elbo_stats[0] + len(rev)
    np.testing.assert_allclose(a[1] - b[1], left_out, rtol=1e-7)   # (a difference of two sums 1e3 times its size)
    assert a[2] == b[2]


def test_engine_rows_follow_the_reports():
    e = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False, logl=True)
    plain = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    assert e.logl_rows.shape == (1, 2) and plain.logl_rows.shape == (0, 2)
    assert e.logl_rows[0, 1] == e.elbo()[0]
    for _ in range(2):
        e.sweep()
        plain.sweep()
        e.report()
        plain.report()
    assert e.logl_rows[:, 0].tolist() == [0, 1, 2] and np.all(np.diff(e.logl_rows[:, 1]) > 0)
    assert np.array_equal(e.gamma, plain.gamma) and np.array_equal(e.rows, plain.rows)   # the bound changes nothing
    assert e.logl_rows[2, 1] == e.elbo()[0]


def test_stop_rule_drop():
    """s < max counts only past iteration 10; the fourth such report ends the run; a new maximum clears the count"""
    up = [(i, -100.0 + i) for i in range(1, 9)]                       # gains of 1 %: no gain rule
    assert orig_stop_rule(up) == [GO] * 8
    early = up + [(9, -95.0), (10, -96.0)]                            # below the maximum, iter <= 10: not counted
    assert orig_stop_rule(early + [(11, -97.0), (12, -98.0), (13, -99.0)]) == [GO] * 13
    assert orig_stop_rule(early + [(11, -97.0), (12, -98.0), (13, -99.0), (14, -99.5)]) == [GO] * 13 + [DROP]
    cleared = early + [(11, -97.0), (12, -98.0), (13, -99.0), (14, -80.0), (15, -85.0), (16, -86.0), (17, -87.0)]
    assert orig_stop_rule(cleared) == [GO] * 17
    assert orig_stop_rule(cleared + [(18, -88.0)]) == [GO] * 17 + [DROP]
    assert orig_stop_rule([(i, -50.0) for i in range(1, 30)]) == [GO] * 29   # s == max: neither branch


def test_stop_rule_gain():
    """s > prev, prev != 0, |(s - prev) / prev| < 1e-5"""
    assert orig_stop_rule([(0, -1000.0), (1, -999.0), (2, -998.995)]) == [GO, GO, GAIN]
    assert orig_stop_rule([(0, -1000.0), (1, -999.98)]) == [GO, GO]                 # 2e-5
    assert orig_stop_rule([(0, -1000.0), (1, -1000.001)]) == [GO, GO]               # a small LOSS is not a gain
    assert orig_stop_rule([(0, 0.0), (1, 1e-9)]) == [GO, GO]                        # prev == 0
    assert orig_stop_rule([(0, -1000.0)]) == [GO]                                   # the first row has no prev


def test_no_stop_turns_both_rules_off():
    seq = [(i, -100.0 + i) for i in range(1, 12)] + [(12, -95.0), (13, -96.0), (14, -97.0), (15, -98.0), (16, -98.0 + 1e-7)]
    assert orig_stop_rule(seq)[-1] == DROP and len(orig_stop_rule(seq)) == 15
    assert orig_stop_rule(seq, enabled=False) == [GO] * 16
    assert orig_stop_rule([(0, -1000.0), (1, -999.9999)], enabled=False) == [GO, GO]


def _run(args, cwd, timeout=300):
    return subprocess.run([SVINET] + args, capture_output=True, text=True, timeout=timeout, cwd=str(cwd))


BASE = ["-file", ASSORT, "-n", "75", "-k", "4", "-orig", "-heldout-ratio", "0.1"]


def test_cli_rows_against_the_engine(tmp_path):
    r = _run(BASE + ["-host-loops", "-max-iterations", "3", "-logl", "-no-stop"], tmp_path)
    assert r.returncode == 0, r.stderr
    d = tmp_path / "n75-k4-mmsb-U"
    rows = [l.split("\t") for l in (d / "logl.txt").read_text().splitlines()]
    assert [x[0] for x in rows] == ["0", "1", "2", "3"] and all(len(x) == 3 and len(x[2].split(".")[1]) == 5 for x in rows)
    assert r.stdout.count("approx. log likelihood = ") == 4
    e = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False, logl=True)
    for _ in range(3):
        e.sweep()
        e.report()
    assert [float(x[2]) for x in rows] == [float("%.5f" % s) for s in e.logl_rows[:, 1]]
    assert not (d / "max.txt").exists() and not (d / "done.txt").exists()
    # without -logl: the empty file of before, and exactly the files of before
    plain = tmp_path / "plain"
    plain.mkdir()
    r = _run(BASE + ["-host-loops", "-max-iterations", "3"], plain)
    assert r.returncode == 0, r.stderr
    p = plain / "n75-k4-mmsb-U"
    assert (p / "logl.txt").read_text() == "" and "approx. log likelihood" not in r.stdout
    assert {x.name for x in p.iterdir()} == {x.name for x in d.iterdir()}
    assert (p / "beta.txt").read_text() == (d / "beta.txt").read_text()


def test_cli_run_ends_by_a_rule(tmp_path):
    """-max-iterations 2000 is a guard only: a rule ends the run well before it (the default seed: see the printed sweep)"""
    r = _run(BASE + ["-host-loops", "-rfreq", "1", "-logl", "-max-iterations", "2000"], tmp_path)
    assert r.returncode == 0, r.stderr
    d = tmp_path / "n75-k4-mmsb-U"
    rows = [l.split("\t") for l in (d / "logl.txt").read_text().splitlines()]
    ended = [f for f in ("max.txt", "done.txt") if (d / f).exists()]
    print("rows %d, last iter %s, ended by %s" % (len(rows), rows[-1][0], ended))
    assert len(ended) == 1 and int(rows[-1][0]) < 1000
    cols = (d / ended[0]).read_text().split()
    assert len(cols) == (9 if ended[0] == "max.txt" else 3) and cols[0] == rows[-1][0]
    if ended[0] == "max.txt":
        s = [float(x[2]) for x in rows]
        assert abs(float(cols[2]) - max(s)) < 1e-4
        held = [l.split("\t") for l in (d / "heldout.txt").read_text().splitlines()]
        at = [h for h in held if h[0] == rows[int(np.argmax(s))][0]][-1]
        assert abs(float(cols[3]) - float(at[2])) < 1e-4
    beta = np.loadtxt(d / "beta.txt")
    assert beta.shape == (4, 4) and np.all((beta > 0) & (beta < 1))        # the model is saved
    assert np.loadtxt(d / "gamma.txt").shape == (75, 6)


def test_cli_accepts_logl_without_max_iterations_and_refuses_no_stop(tmp_path):
    ok = tmp_path / "ok"
    ok.mkdir()
    r = _run(BASE + ["-host-loops", "-logl"], ok)
    assert r.returncode == 0, r.stderr
    d = ok / "n75-k4-mmsb-U"
    assert (d / "beta.txt").exists() and ((d / "max.txt").exists() or (d / "done.txt").exists())
    for extra in (["-logl", "-no-stop"], []):
        no = tmp_path / ("no%d" % len(extra))
        no.mkdir()
        r = _run(BASE + ["-host-loops"] + extra, no)
        assert r.returncode == 2 and not list(no.iterdir())
        assert "error: -orig needs -max-iterations N: the reference's loop never ends and its stop rule is compiled out" in r.stderr


def test_help_says_what_logl_does_with_orig(tmp_path):
    r = _run(["-help"], tmp_path)
    text = r.stdout + r.stderr
    assert "With -orig: the bound of the K x K blockmodel" in text and "max.txt" in text and "done.txt" in text


def test_null_handles_and_no_device():
    L = _svils.load()
    null = ERR_ARG if _have_gpu() else ERR_DEVICE
    out = np.zeros(3)
    assert L.svils_orig_elbo(None, out.ctypes.data) == null
    assert L.svils_orig_elbo(None, None) == null
    assert L.svils_orig_get_elbo_stats(None, None, None, None, None) == null
    assert L.svils_orig_get_elbo_timing(None, None) == null
    if not _have_gpu():
        assert b"no CPU path" in L.svils_last_error()
        with pytest.raises(_svils.SvilsError) as ei:
            OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=True, logl=True)
        assert ei.value.code == ERR_DEVICE
