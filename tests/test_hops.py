"""CPU: the restatement tools/restate_hops.py against an independent route and closed forms, the
graphs the device is later compared on (tests/test_gpu_hops.py), and what the svils_ppc_hops family and `-ppc-hops`
answer without a device."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import hops_cases as HC
from hops_cases import H

NEW = ("svils_ppc_hops", "svils_ppc_get_hops", "svils_ppc_get_hop_nodes", "svils_ppc_get_hop_summary", "svils_ppc_set_hop_batch",
       "svils_ppc_get_hop_timing")


def test_restatement_against_matrix_powers():
    rng = np.random.default_rng(2025)
    seen = set()
    for case in range(30):
        n = int(rng.integers(2, 41))
        p = float(rng.choice([0.0, 0.03, 0.08, 0.2, 0.6]))
        iu = np.triu_indices(n, 1)
        keep = rng.random(len(iu[0])) < p
        links = np.stack([iu[0][keep], iu[1][keep]], 1)
        got = H.hops(links, n)
        D, ecc, comp = HC.matrix_power_route(links, n)
        assert got["D"].tolist() == D and got["ecc"].tolist() == ecc and got["comp"].tolist() == comp, case
        assert got["deg"].tolist() == HC.PC.degrees(links, n).tolist() if len(links) else not got["deg"].any()
        assert D[0] == n and (len(D) == 1 or D[1] == 2 * len(links))
        seen.add((len(set(comp)) > 1, len(D) > 3))
    assert len(seen) >= 3      # connected and not, short and long


@pytest.mark.parametrize("name", sorted(HC.closed_forms()))
def test_restatement_against_closed_forms(name):
    form = HC.closed_forms()[name]
    HC.check_closed_form(H.all_of(np.array(form[1], np.int64).reshape(-1, 2), form[0]), form)


def test_closed_forms_by_hand():
    f = HC.closed_forms()
    assert f["path-130"][2][:3] == [130, 258, 256] and len(f["path-130"][2]) == 130 and f["path-130"][3][:2] == [129, 128]
    assert sorted(set(f["three-cliques"][4])) == [0, 7, 27]
    s = H.all_of(np.array(f["three-cliques"][1]), 65)
    assert (s["components"], s["largest"], s["isolated"], s["diameter"], s["meandist"]) == (3, 38, 0, 1, 1.0)
    e = H.all_of(np.zeros((0, 2), np.int64), 65)
    assert (e["components"], e["largest"], e["isolated"], e["diameter"], e["reachable"]) == (65, 1, 65, 0, 0)
    assert math.isnan(e["meandist"]) and e["effdiam"] == 0.0


def test_effective_diameter_by_hand():
    assert H.effdiam([65]) == 0.0                                   # h* = 0: the empty graph
    assert H.effdiam([10, 0]) == 0.0
    # C = 2, 4: t = 3.6, h* = 1, (3.6 - 2) / 2
    assert H.effdiam([2, 2]) == 0.0 + (0.9 * 4.0 - 2.0) / 2.0 and abs(H.effdiam([2, 2]) - 0.8) < 1e-15
    # C = 10, 50, 90, 100: t = 90 is hit exactly at h* = 2: 1 + (90 - 50) / 40 = 2
    assert 0.9 * 100.0 == 90.0 and H.effdiam([10, 40, 40, 10]) == 2.0
    # C = 4, 10, 16, 20: t = 18, h* = 3: 2 + (18 - 16) / 4
    assert H.effdiam([4, 6, 6, 4]) == 2.5
    # the path on 4 nodes: D = 4, 6, 4, 2, C = 4, 10, 14, 16, t = 14.4, h* = 3: 2 + 0.4 / 2
    assert H.effdiam(H.hops([(0, 1), (1, 2), (2, 3)], 4)["D"]) == 2.0 + (0.9 * 16.0 - 14.0) / 2.0


def test_sparse_replicates_meet_their_conditions():
    for n in HC.REPLICATE_N:
        for seed, r in HC.SPARSE_DRAWS[n]:
            links, want = HC.replicate(n, HC.SPARSE_DEG, seed, r)
            big, isolated, diameter = HC.sparse_conditions(want)
            assert big >= 3 and isolated >= 1 and diameter >= 5, (n, seed, r, big, isolated, diameter)
            assert 0.75 <= 2 * len(links) / n <= 3.0, (n, len(links))
        for seed, r in HC.DENSE_DRAWS:
            links, want = HC.replicate(n, HC.DENSE_DEG, seed, r)
            assert 4.0 <= 2 * len(links) / n <= 8.0 and want["largest"] > n // 2, (n, len(links))
    pi, beta = HC.model(1100, HC.DENSE_DEG)
    assert np.all((beta >= 0) & (beta <= 1)) and np.allclose(pi.sum(1), 1.0, rtol=0, atol=1e-12)


def test_writers_by_hand():
    obs = H.all_of([(0, 1), (1, 2), (2, 3)], 5)
    reps = [H.all_of([(0, 1), (1, 2), (2, 3), (3, 4)], 5), H.all_of([], 5)]
    t = H.hops_texts(obs, reps)
    assert sorted(t) == ["obs-hop.txt", "ppc/hops-summary.txt", "ppc/obs-hops.txt", "ppc/ppc-hop.txt", "ppc/rep-hops.txt"]
    assert t["ppc/obs-hops.txt"] == "0\t5\t5\n1\t6\t11\n2\t4\t15\n3\t2\t17\n"
    assert t["obs-hop.txt"] == "%.5f\n" % (2.0 + (0.9 * 17.0 - 15.0) / 2.0)
    assert t["ppc/rep-hops.txt"].splitlines()[1] == "1\t0.00000\t0\tnan\t5\t1\t5"
    assert t["ppc/rep-hops.txt"].startswith("0\t") and t["ppc/ppc-hop.txt"].splitlines()[1] == "0.00000"
    rows = [l.split("\t") for l in t["ppc/hops-summary.txt"].splitlines()]
    assert [r[0] for r in rows] == list(H.STATISTICS) and all(len(r) == 5 for r in rows)
    assert rows[3] == ["components", "2.00000", "3.00000", "%.5f" % math.sqrt(8.0), "1.00000"]


# ---- the library and the command line without a device ----

def test_new_symbols_are_exported():
    from svinet_amd import _svils
    lib = _svils.load()
    for name in NEW:
        assert name in _svils.EXPORTS and hasattr(lib, name), name


def _calls(L, h):
    buf = (C.c_uint64 * 8)()
    val = (C.c_double * 2)()
    lev = C.c_uint32()
    return (("svils_ppc_hops", lambda: L.svils_ppc_hops(h)),
            ("svils_ppc_get_hops", lambda: L.svils_ppc_get_hops(h, C.byref(lev), buf, 8)),
            ("svils_ppc_get_hop_nodes", lambda: L.svils_ppc_get_hop_nodes(h, None, None)),
            ("svils_ppc_get_hop_summary", lambda: L.svils_ppc_get_hop_summary(h, buf, val)),
            ("svils_ppc_set_hop_batch", lambda: L.svils_ppc_set_hop_batch(h, 8, 8)),
            ("svils_ppc_get_hop_timing", lambda: L.svils_ppc_get_hop_timing(h, val)))


def test_null_handle_and_no_device():
    """a null handle is SVILS_ERR_ARG at every new entry point; without a HIP device each answers SVILS_ERR_DEVICE"""
    import torch
    from svinet_amd import _svils
    L = _svils.load()
    calls = _calls(L, None)
    assert [c[0] for c in calls] == list(NEW)
    for name, call in calls:
        if torch.cuda.is_available():
            assert call() == -1 and b"null handle" in L.svils_last_error(), name
        else:
            assert call() == -2 and b"no CPU path" in L.svils_last_error() and name.encode() in L.svils_last_error(), name


def _svinet(args, cwd):
    exe = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
    return subprocess.run([exe] + [str(a) for a in args], cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_cli_refusals(tmp_path):
    golden = os.path.join(ROOT, "tests", "golden")
    for m in ("gamma.txt", "lambda.txt"):
        shutil.copy(os.path.join(golden, "ref_assort_batch", m), str(tmp_path))
    graph = ["-file", os.path.join(golden, "graphs", "assort-75-4.txt"), "-n", 75, "-k", 4]
    cases = [(graph + ["-ppc-hops"], "-ppc runs"), (["-n", 65, "-k", 4, "-gen", "-ppc-hops"], "-gen"),
             (graph + ["-ppc", "-gen", "-ppc-hops"], "-gen")]
    for flag in (["-link-sampling"], ["-batch"], ["-batch-gpu"], ["-findk"], ["-gml"], ["-lcstats"], ["-rnode"], ["-rpair"],
                 ["-snode"], ["-infset"], ["-preprocess"], ["-orig"], ["-gpus", 2], ["-kshard"], ["-sharded"], ["-minibatch", 8],
                 ["-recommend", 5], ["-rank-heldout"], ["-adamic-adar"], ["-load", "x/"]):
        word = "-batch" if flag[0] == "-batch-gpu" else flag[0]      # -batch-gpu sets -batch, which the table names first
        cases += [(graph + flag + ["-ppc-hops"], word), (graph + ["-ppc", "-ppc-hops"] + flag, word)]
    for args, word in cases:
        r = _svinet(args, tmp_path)
        assert r.returncode == 2 and "-ppc-hops" in r.stderr and word in r.stderr, (args, r.returncode, r.stderr)
        assert "unsupported option" not in r.stderr, r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["gamma.txt", "lambda.txt"]      # refused before anything is created
    assert "-ppc-hops" in _svinet(["-help"], tmp_path).stdout
