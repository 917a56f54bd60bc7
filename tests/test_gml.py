"""-gml / -lcstats without a device: the numpy restatement tools/restate_gml.py against the authors' shipped files, the
CLI's refusals and model checks, and the svils_lc_* entry points' behaviour without a device."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import restate_findk  # noqa: E402
import restate_gml as R  # noqa: E402

SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
ASSORT = os.path.join(ROOT, "tests", "golden", "graphs", "assort-75-4.txt")
BATCH = os.path.join(ROOT, "tests", "golden", "ref_assort_batch")


def _run(args, cwd):
    return subprocess.run([SVINET] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def test_restatement_reproduces_the_authors_files():
    links, seq2id = restate_findk.read_graph(ASSORT, 75)
    gamma, ids, lam = R.load_model(BATCH, 75, 4)
    assert np.array_equal(ids, seq2id)
    t = R.texts(R.link_communities(links, gamma, lam), links, seq2id)
    for mine, theirs in (("community_stats.txt", "obs_stats.txt"), ("node_bridgeness.txt", "obs_bridgeness.txt"),
                         ("node_influence.txt", "obs_influence.txt")):
        assert t[mine] == open(os.path.join(BATCH, theirs)).read(), mine
    # that revision did not write the closing "]\n" (src/mmsbgen.cc:957 does)
    assert t["network.gml"] == open(os.path.join(BATCH, "network.gml")).read() + "]\n"


def test_restatement_edge_cases():
    # K = 4; node 3's row puts everything on column 3, node 2's on column 2: the link 2-3 has x = 0 everywhere (NaN ratio:
    # joins community 0 and is a GML edge, colour 0); 0-1 ties on columns 0 and 1 (the first wins); community 3 is empty
    gamma = np.array([[2.0, 2.0, 0.0, 0.0], [2.0, 2.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    lam = np.array([[1.0, 1.0]] * 4)
    links = np.array([[0, 1], [2, 3]])
    r = R.link_communities(links, gamma, lam)
    assert r["colour"].tolist() == [0, 0] and np.isnan(r["ratio"][1])
    assert r["join"].tolist() == [True, True] and r["gml"].tolist() == [False, True]   # 0-1: ratio 0.5 exactly
    assert r["group"].tolist() == [0, 0, 2, 3]
    assert r["comm_nodes"].tolist() == [4, 0, 0, 0] and r["comm_argmax"].tolist() == [0, 0, 0, 0]
    t = R.texts(r, links, np.arange(4))
    assert t["community_stats.txt"].split("\n")[3] == "3\t-nan\t0.00000\t0\t0"


def test_pairwise_sums_decide_some_links_differently():
    """the reason for the sequential recheck: with np.sum's pairwise order a few near-threshold links flip"""
    from gml_models import near_threshold
    links, gamma, lam = near_threshold(64, 4000, seed=3)
    a = R.link_communities(links, gamma, lam)
    b = R.link_communities(links, gamma, lam, pairwise=True)
    assert (a["join"] != b["join"]).any() and (a["gml"] != b["gml"]).any()


@pytest.mark.parametrize("extra,needle", [
    (["-gpus", "2"], "-gpus N > 1"),
    (["-kshard"], "-kshard"),
    (["-sharded"], "-sharded"),
    (["-minibatch", "10"], "-minibatch"),
    (["-predict-pairs", "pairs.txt"], "-predict-pairs"),
    (["-recommend", "5"], "-recommend"),
])
@pytest.mark.parametrize("flag", ["-gml", "-lcstats"])
def test_cli_refusals(tmp_path, flag, extra, needle):
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", flag] + extra, str(tmp_path))
    assert r.returncode == 2 and needle in r.stderr and flag in r.stderr, (r.returncode, r.stderr)
    assert "unsupported option" not in r.stderr


def test_cli_needs_the_model_files(tmp_path):
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-gml"], str(tmp_path))
    assert r.returncode == 2 and "gamma.txt" in r.stderr, r.stderr
    shutil.copy(os.path.join(BATCH, "gamma.txt"), str(tmp_path))
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-lcstats"], str(tmp_path))
    assert r.returncode == 2 and "lambda.txt" in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "gml"))


@pytest.mark.parametrize("how,needle", [("short", "rows"), ("ids", "numbers it"), ("columns", "fewer than")])
def test_cli_refuses_a_model_of_another_network(tmp_path, how, needle):
    rows = open(os.path.join(BATCH, "gamma.txt")).read().split("\n")[:-1]
    if how == "short":
        rows = rows[:-1]
    elif how == "ids":
        f = rows[10].split("\t")
        f[1] = "999"
        rows[10] = "\t".join(f)
    else:
        rows[20] = "\t".join(rows[20].split("\t")[:4])
    open(str(tmp_path / "gamma.txt"), "w").write("\n".join(rows) + "\n")
    shutil.copy(os.path.join(BATCH, "lambda.txt"), str(tmp_path))
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-gml"], str(tmp_path))
    assert r.returncode != 0 and needle in r.stderr and "Abort" not in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(str(tmp_path / "gml" / "network.gml"))


def test_lcstats_names_the_directory_without_engine_and_makes_ppc(tmp_path):
    shutil.copy(os.path.join(BATCH, "gamma.txt"), str(tmp_path))
    shutil.copy(os.path.join(BATCH, "lambda.txt"), str(tmp_path))
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-lcstats"], str(tmp_path))
    assert "+ Output directory: n75-k4-mmsb\n" in r.stdout, r.stdout
    assert os.path.isdir(str(tmp_path / "ppc")) and os.path.isdir(str(tmp_path / "n75-k4-mmsb"))
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-gml"], str(tmp_path))
    assert "+ Output directory: gml\n" in r.stdout
    assert os.path.islink(str(tmp_path / "gml" / "network.dat")) and os.path.exists(str(tmp_path / "gml" / "param.txt"))


def test_usage_names_the_flags():
    r = subprocess.run([SVINET, "-help"], stdout=subprocess.PIPE, text=True, timeout=60)
    assert "\t-gml\t" in r.stdout and "\t-lcstats\t" in r.stdout


def test_entry_points_refuse_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from svinet_amd import _svils
    L = _svils.load()
    h = C.c_void_p()
    assert L.svils_lc_create(0, 10, 4, C.byref(h)) == -2
    assert b"no CPU path" in L.svils_last_error()
    ms = np.zeros(3)
    for rc in (L.svils_lc_set_graph(None, None, 0), L.svils_lc_set_model(None, None, None),
               L.svils_lc_run(None), L.svils_lc_get_nodes(None, None, None, None, None), L.svils_lc_get_degrees(None, None),
               L.svils_lc_get_pi(None, None), L.svils_lc_get_communities(None, None, None, None, None),
               L.svils_lc_get_links(None, None, None, None), L.svils_lc_get_gml(None, None, None),
               L.svils_lc_get_timing(None, ms.ctypes.data)):
        assert rc == -2
    assert L.svils_lc_destroy(None) == 0
