"""CPU: the restatement tools/restate_ppc_orig.py (the K x K kind of svils_ppc) against its own plain
loops, the assortative restatement for a diagonal B and the closed forms the device is later held to
(tests/test_gpu_ppc_orig.py); what the two new entry points answer without a device; the command line of -ppc-orig."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np

from conftest import ROOT
import ppc_cases as PC
import ppc_orig_cases as OC
from ppc_cases import R
from ppc_orig_cases import RO

GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_array_draw_is_the_loop_draw():
    for K in (2, 5):
        pi, B = OC.random_model(9, K, 1)
        B = B / B.max()                              # dense enough at n = 9 to draw links
        for seed, r in PC.EQUALITY_DRAWS[:2]:
            a = RO.draw_loops(pi, B, seed, r)
            assert np.array_equal(a, RO.draw(pi, B, seed, r)) and len(a) > 5
        P, Q = R.all_pairs(9)
        assert np.array_equal(RO.pair_sums(pi, B, P, Q), [RO.pair_sum(pi[p], pi[q], B) for p, q in zip(P, Q)])
        assert np.array_equal(R.seq_sum(RO.terms(pi, B, P, Q)), RO.pair_sums(pi, B, P, Q))


def test_diagonal_rates_are_the_assortative_model_bit_for_bit():
    n, K = 65, 5
    pi, beta = PC.random_model(n, K, 1)
    B = np.diag(beta)
    P, Q = R.all_pairs(n)
    assert np.array_equal(RO.pair_sums(pi, B, P, Q).view(np.int64), R.pair_sums(pi, beta, P, Q).view(np.int64))
    for seed, r in PC.EQUALITY_DRAWS:
        links = R.draw(pi, beta, seed, r)
        assert np.array_equal(RO.draw(pi, B, seed, r), links) and len(links) > 100
        a, o = R.stats(links, pi, beta), RO.stats(links, pi, B)
        assert np.array_equal(o["colour"], a["colour"] * (K + 1)) and np.array_equal(o["join"], a["join"])
        assert np.array_equal(np.diag(o["bsize"]), a["size"]) and o["bsize"].sum() == a["size"].sum()
        assert np.array_equal(np.diag(o["blogpe"]).view(np.int64), a["logpe"].view(np.int64))
        assert not (o["blogpe"] - np.diag(np.diag(o["blogpe"]))).any() and o["offdiag_share"] == 0.0
        for name in ("ones", "max_deg", "argmax_deg", "triangles", "wedges", "transitivity", "clustering"):
            assert o[name] == a[name], name
        assert np.array_equal(o["deg"], a["deg"]) and np.array_equal(o["tri"], a["tri"])


def test_the_smaller_id_indexes_the_rows():
    n = 9
    pi, B = OC.parity_model(n, OC.ORIENTED)
    for seed, r in PC.EQUALITY_DRAWS:
        assert np.array_equal(RO.draw(pi, B, seed, r), OC.oriented_pairs(n))
    s = RO.stats(OC.oriented_pairs(n), pi, B)
    assert np.all(s["colour"] == 1) and np.all(s["join"]) and s["bsize"].tolist() == [[0, len(s["links"])], [0, 0]]
    assert s["offdiag_share"] == 1.0 and not s["blogpe"].any()


def test_complete_bipartite_in_closed_form():
    n = 9                                            # 5 even, 4 odd
    pi, B = OC.parity_model(n, OC.BIPARTITE)
    links = RO.draw(pi, B, 4, 1)
    assert np.array_equal(links, OC.bipartite_pairs(n)) and len(links) == 20
    s = RO.stats(links, pi, B)
    assert s["ones"] == 20 and s["triangles"] == 0 and s["transitivity"] == 0.0 and s["clustering"] == 0.0 and not s["tri"].any()
    assert np.array_equal(s["deg"], np.where(np.arange(n) % 2 == 0, 4, 5))
    assert s["offdiag_share"] == 1.0 and s["bsize"][0, 1] + s["bsize"][1, 0] == 20 and np.trace(s["bsize"]) == 0
    # colour = g K + h with g the class of the smaller id
    assert np.array_equal(s["colour"], np.where(links[:, 0] % 2 == 0, 1, 2))
    e = RO.stats(np.zeros((0, 2), np.int64), pi, B)
    assert e["ones"] == 0 and math.isnan(e["offdiag_share"]) and not e["bsize"].any()


def test_edge_model_meets_its_conditions():
    pi, B, want = OC.on_the_edge_model()             # asserts the band count itself
    assert np.all(pi.sum(1) == 1.0) and np.all((B >= 0) & (B <= 1))
    for (p, q), (g, h) in zip(OC.EDGE_PAIRS, ((0, 1), (2, 3), (4, 5))):
        assert RO.pair_sum(pi[p], pi[q], B) == B[g, h]
    have = set(map(tuple, RO.draw(pi, B, OC.EDGE_SEED, OC.EDGE_R).tolist()))
    for pq, y in want.items():
        assert (pq in have) == y


def test_band_covers_both_sums():
    """(K^2 + 2 K + 18) eps is twice the sum of the two rounding counts (K^2 + 1) + (K + k16 + 1), k16 <= K + 15, times eps / 2"""
    for K in (2, 5, 20, 64):
        k16 = (K + 15) // 16 * 16
        assert OC.band(K) >= 2 * ((K * K + 1) + (K + k16 + 1)) * PC.DBL_EPSILON / 2


def test_new_symbols_are_exported_and_the_abi_stays():
    from svinet_amd import _svils
    L = _svils.load()
    assert L.svils_abi_version() == 8
    for name in ("svils_ppc_set_params_orig", "svils_ppc_get_blocks"):
        assert hasattr(L, name) and name in open(os.path.join(ROOT, "include", "svils.h")).read()


def test_library_refusals_need_no_device():
    import torch
    from svinet_amd import _svils
    L = _svils.load()
    x = np.zeros(4)
    if not torch.cuda.is_available():
        for f, name in ((L.svils_ppc_set_params_orig, b"svils_ppc_set_params_orig"), (L.svils_ppc_get_blocks, b"svils_ppc_get_blocks")):
            assert f(None, x.ctypes.data, x.ctypes.data) == -2
            assert b"no CPU path" in L.svils_last_error() and name in L.svils_last_error()
    else:
        assert L.svils_ppc_set_params_orig(None, x.ctypes.data, x.ctypes.data) == -1
        assert L.svils_ppc_get_blocks(None, x.ctypes.data, x.ctypes.data) == -1


# ---- the command line ----

def _svinet(args, cwd):
    exe = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
    return subprocess.run([exe] + [str(a) for a in args], cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def _fit_directory(tmp_path):
    shutil.copy(os.path.join(GOLDEN, "ref_assort_batch", "gamma.txt"), str(tmp_path))
    (tmp_path / "beta.txt").write_text(OC.beta_text(OC.cli_rates()))
    return ["-file", OC.GRAPH, "-n", OC.CLI_N, "-k", OC.CLI_K]


def test_cli_refusals(tmp_path):
    graph = _fit_directory(tmp_path)
    cases = [(graph + ["-ppc-orig", "-gen"], "-gen"), (graph + ["-ppc-orig", "-ppc"], "-ppc"), (graph + ["-ppc-orig", "-orig"], "-orig"),
             (graph + ["-ppc-orig", "-infset"], "-infset"), (graph + ["-ppc-orig", "-preprocess"], "-preprocess"),
             (graph + ["-ppc-orig", "-batch-gpu"], "-batch"), (graph + ["-ppc-orig", "-load", "x"], "-load"),
             (graph + ["-ppc-orig", "-snode"], "-snode"),
             # the table of -ppc
             (graph + ["-ppc-orig", "-batch"], "-batch"), (graph + ["-ppc-orig", "-link-sampling"], "-link-sampling"),
             (graph + ["-ppc-orig", "-findk"], "-findk"), (graph + ["-ppc-orig", "-gml"], "-gml"), (graph + ["-ppc-orig", "-lcstats"], "-lcstats"),
             (graph + ["-ppc-orig", "-rnode"], "-rnode"), (graph + ["-ppc-orig", "-rpair"], "-rpair"),
             (graph + ["-ppc-orig", "-rpair", "-stratified"], "-rpair"), (graph + ["-ppc-orig", "-gpus", 2], "-gpus"),
             (graph + ["-ppc-orig", "-kshard"], "-kshard"), (graph + ["-ppc-orig", "-sharded"], "-sharded"),
             (graph + ["-ppc-orig", "-minibatch", 8], "-minibatch"), (graph + ["-ppc-orig", "-predict-pairs", "p.txt"], "-predict-pairs"),
             (graph + ["-ppc-orig", "-recommend", 3], "-recommend"), (graph + ["-ppc-orig", "-rank-pairs", "p.txt"], "-rank-pairs"),
             (graph + ["-ppc-orig", "-rank-heldout"], "-rank-heldout"), (graph + ["-ppc-orig", "-adamic-adar"], "-adamic-adar"),
             # the limits
             (graph[:4] + ["-k", 1, "-ppc-orig"], "-k 1"), (graph[:4] + ["-k", 65, "-ppc-orig"], "-k 65"),
             (graph[:2] + ["-n", 32769, "-k", 4, "-ppc-orig"], "-n 32769")]
    for args, word in cases:
        r = _svinet(args, tmp_path)
        assert r.returncode == 2 and word in r.stderr and "-ppc-orig" in r.stderr, (args, r.returncode, r.stderr)
        assert "unsupported option" not in r.stderr, r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["beta.txt", "gamma.txt"]      # refused before anything is created


def test_cli_names_a_missing_file(tmp_path):
    graph = _fit_directory(tmp_path)
    os.unlink(str(tmp_path / "beta.txt"))
    shutil.copy(os.path.join(GOLDEN, "ref_assort_batch", "lambda.txt"), str(tmp_path))   # the other model's file does not do
    r = _svinet(graph + ["-ppc-orig"], tmp_path)
    assert r.returncode == 2 and "beta.txt" in r.stderr, r.stderr
    os.unlink(str(tmp_path / "gamma.txt"))
    (tmp_path / "beta.txt").write_text(OC.beta_text(OC.cli_rates()))
    r = _svinet(graph + ["-ppc-orig"], tmp_path)
    assert r.returncode == 2 and "gamma.txt" in r.stderr, r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["beta.txt", "lambda.txt"]


def test_cli_names_the_line_of_a_malformed_rate_file(tmp_path):
    graph = _fit_directory(tmp_path)
    B = OC.cli_rates()
    rows = OC.beta_text(B).splitlines()
    bad = B.copy()
    bad[2, 1] = 1.5
    nan = OC.beta_text(B).replace("%.12g" % B[1, 3], "nan")
    for text, line in (("\n".join(rows[:3]) + "\n", "line 4"), ("\n".join(rows + rows[:1]) + "\n", "line 5"),
                       ("\n".join([rows[0], rows[1] + "\t0.5"] + rows[2:]) + "\n", "line 2"),
                       ("\n".join([rows[0].rsplit("\t", 1)[0]] + rows[1:]) + "\n", "line 1"), (OC.beta_text(bad), "line 3"),
                       (nan, "line 2"), (OC.beta_text(B).replace("\t", "\tx", 1), "line 1")):
        (tmp_path / "beta.txt").write_text(text)
        r = _svinet(graph + ["-ppc-orig", "-ppc-draws", 2], tmp_path)
        assert r.returncode not in (0, 2) and "beta.txt" in r.stderr and line in r.stderr, (text, r.returncode, r.stderr)
        assert "no CPU path" not in r.stderr
        assert sorted(os.listdir(str(tmp_path))) == ["beta.txt", "gamma.txt"]    # nothing is written


def test_cli_help_names_the_flag(tmp_path):
    r = _svinet(["-help"], tmp_path)
    assert r.returncode == 0 and "-ppc-orig" in r.stdout and "beta.txt" in r.stdout


def test_cli_needs_a_device(tmp_path):
    import torch
    if torch.cuda.is_available():
        return                                       # tests/test_gpu_ppc_orig.py runs it end to end
    graph = _fit_directory(tmp_path)
    for extra in ([], ["-ppc-hops"]):
        r = _svinet(graph + ["-ppc-orig", "-ppc-draws", 2] + extra, tmp_path)
        assert r.returncode not in (0, 2) and "no CPU path" in r.stderr and "unsupported option" not in r.stderr, r.stderr
