"""The link queries of -orig without a device: the three entry points are exported and declared, the command line refuses
every combination it cannot answer before anything is read or created, and -clean-holdout changes the host loops' skip
list to both orientations of both sets while the default stays the reference's one-orientation rule."""
import os
import re
import subprocess

import numpy as np
import pytest

import orig_cases as OC
from conftest import GOLDEN
from svinet_amd import _svils
from svinet_amd.host_api import OrigEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
ASSORT = os.path.join(GOLDEN, "graphs", "assort-75-4.txt")
RTOL = 1e-7
QUERIES = ("svils_orig_link_prob", "svils_orig_predict_links", "svils_orig_rank_links")


def test_entry_points_are_exported_and_declared():
    L = _svils.load()
    header = open(os.path.join(ROOT, "include", "svils.h")).read()
    for name in QUERIES:
        assert getattr(L, name) is not None
        assert re.search(r"^int %s\(svils_orig \*h, " % name, header, re.M), name
    assert _svils.load().svils_abi_version() == 8
    # a null handle answers as the other svils_orig_* calls do: "no HIP device" where there is none, else a bad argument
    import torch
    null = -1 if torch.cuda.is_available() else -2
    assert L.svils_orig_link_prob(None, None, 0, None) == null
    assert L.svils_orig_predict_links(None, None, 0, 1, None, None) == null
    assert L.svils_orig_rank_links(None, None, 0, None, None, None, None) == null
    assert L.svils_orig_get_query_timing(None, None) == null


def _run(args, cwd):
    return subprocess.run([SVINET] + args, capture_output=True, text=True, timeout=120, cwd=str(cwd))


PAIRS = os.path.join(GOLDEN, "graphs", "assort-75-4.txt")   # any readable file: a refusal comes before it is parsed
FLAGS = [(["-predict-pairs", PAIRS], "-predict-pairs"), (["-recommend", "3"], "-recommend"), (["-rank-pairs", PAIRS], "-rank-pairs"),
         (["-rank-heldout"], "-rank-heldout")]


@pytest.mark.parametrize("flag,word", FLAGS)
@pytest.mark.parametrize("more", [[], ["-clean-holdout", "-host-loops"]])
def test_cli_query_flags_need_clean_holdout_on_the_device(tmp_path, flag, word, more):
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-orig", "-max-iterations", "3"] + more + flag, tmp_path)
    assert r.returncode == 2 and word in r.stderr, (r.returncode, r.stderr)
    assert ("-host-loops" if more else "-clean-holdout") in r.stderr
    if not more:
        assert "reverse orientation" in r.stderr and "validation" in r.stderr   # the refusal says why
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("args,word", [
    (["-link-sampling", "-clean-holdout"], "-clean-holdout"),
    (["-batch", "-clean-holdout"], "-clean-holdout"),
    (["-orig", "-max-iterations", "3", "-clean-holdout", "-adamic-adar", "-rank-heldout"], "-adamic-adar"),
])
def test_cli_refusals_create_nothing(tmp_path, args, word):
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4"] + args, tmp_path)
    assert r.returncode == 2 and word in r.stderr, (r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


def _both_orientations(e):
    both = np.concatenate([e.heldout, e.validation]).astype(np.int64)
    return sorted({(p, q) for p, q in both.tolist()} | {(q, p) for p, q in both.tolist()})


def test_cli_host_loops_clean_holdout(tmp_path):
    """the skip test of the host loops holds both orientations of both sets with the flag, and the held-out pairs in the
    drawn orientation alone without it"""
    out = {}
    for which, extra in (("clean", ["-clean-holdout"]), ("plain", [])):
        d = tmp_path / which
        d.mkdir()
        r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-orig", "-host-loops", "-max-iterations", "2", "-heldout-ratio", "0.1"] + extra, d)
        assert r.returncode == 0, r.stderr
        out[which] = d / "n75-k4-mmsb-U"
    for f in ("heldout-edges.txt", "validation-edges.txt"):   # the sets are drawn exactly as before
        assert (out["clean"] / f).read_text() == (out["plain"] / f).read_text()
    e = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    adj = OC.adjacency(e.n, e.edges)
    one = [tuple(int(x) for x in r) for r in e.heldout]
    for which, skip in (("clean", _both_orientations(e)), ("plain", one)):
        g, b = e.gamma, e.beta
        for _ in range(2):
            g, b, _, bad = OC.sweep(g, b, adj, skip, 0.25)
            assert not bad.any()
        # gamma.txt carries five decimals, beta.txt twelve digits: the files against the restatement at what they can show
        np.testing.assert_allclose(np.loadtxt(out[which] / "gamma.txt")[:, 2:], g, rtol=RTOL, atol=6e-6)
        np.testing.assert_allclose(np.loadtxt(out[which] / "beta.txt"), b, rtol=RTOL)
    assert np.abs(np.loadtxt(out["clean"] / "beta.txt") / np.loadtxt(out["plain"] / "beta.txt") - 1).max() > 1e-5


def test_engine_host_loops_clean_holdout():
    """the same through the library engine, where gamma comes back in full precision"""
    clean = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False, clean_holdout=True)
    plain = OrigEngine(ASSORT, 75, 4, heldout_ratio=0.1, on_device=False)
    assert np.array_equal(clean.heldout, plain.heldout) and np.array_equal(clean.validation, plain.validation)
    adj = OC.adjacency(clean.n, clean.edges)
    g0, b0 = clean.gamma, clean.beta
    assert np.array_equal(g0, plain.gamma) and np.array_equal(b0, plain.beta)
    one = [tuple(int(x) for x in r) for r in plain.heldout]
    for e, skip in ((clean, _both_orientations(clean)), (plain, one)):
        g, b = g0, b0
        for _ in range(2):
            g, b, rounds, bad = OC.sweep(g, b, adj, skip, 0.25)
            e.sweep()
        assert not bad.any()
        np.testing.assert_allclose(e.gamma, g, rtol=RTOL)
        np.testing.assert_allclose(e.beta, b, rtol=RTOL)
        assert e.rounds_total == int(rounds.sum()) and len(rounds) == 75 * 74 - len(set(skip))
    assert len(set(_both_orientations(clean))) > 2 * len(set(one))
    with pytest.raises(_svils.SvilsError):       # the queries have no host path
        clean.link_prob([(0, 1)])
