"""-findk without a device: the numpy restatement (tools/restate_findk.py) hand-checked on tiny inputs, the CLI's
refusals and output directory name, and the svils_findk_* entry points' behaviour without a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import restate_findk as R  # noqa: E402

SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
ASSORT = os.path.join(ROOT, "tests", "golden", "graphs", "assort-75-4.txt")


def _run(args, cwd):
    return subprocess.run([SVINET] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def test_count_ties_keep_ascending_label_order():
    # node 0 sees labels 7, 3, 7, 3, 5: counts 3:2, 7:2, 5:1 -> (3, 7, 5); node 1 sees 9 x 3 and 2 x 1; node 2 nothing
    src = np.array([0, 0, 0, 0, 0, 1, 1, 1, 1])
    lab = np.array([7, 3, 7, 3, 5, 9, 9, 2, 9])
    top, cnt, d = R.count_top(3, src, lab)
    assert top[0].tolist() == [3, 7, 5, -1, -1] and cnt[0].tolist() == [2, 2, 1, 0, 0]
    assert top[1].tolist() == [9, 2, -1, -1, -1] and cnt[1].tolist() == [3, 1, 0, 0, 0]
    assert d.tolist() == [3, 2, 0]
    # six distinct labels with equal counts: the five smallest, ascending
    top, cnt, d = R.count_top(1, np.zeros(6, int), np.array([40, 10, 50, 20, 60, 30]))
    assert top[0].tolist() == [10, 20, 30, 40, 50] and d.tolist() == [6]


def test_padding_rejects_counted_labels_but_keeps_duplicate_pads():
    n, alpha = 10, 0.25
    labels = np.array([[0, 1, 2, 3, 4], [1, 2, 3, 4, 5]])
    values = np.array([[1.5, .1, .2, .3, .4], [1.6, .5, .6, .7, .8]])
    top = np.array([[3, 7, -1, -1, -1], [-1] * 5])
    cnt = np.array([[2, 1, 0, 0, 0], [0] * 5])
    d = np.array([2, 0])
    draws = iter([3, 9, 7, 9, 4])   # 3 and 7 are counted labels of node 0: redrawn; 9 twice is kept twice
    seen = []

    def draw(m):
        assert m == n
        v = next(draws)
        seen.append(v)
        return v
    lab, val = R.set_gamma(labels, values, top, cnt, d, alpha, draw, n)
    assert seen == [3, 9, 7, 9, 4]
    assert lab[0].tolist() == [3, 7, 9, 9, 4]
    assert val[0].tolist() == [2.25, 1.25, 0.5, 0.5, 0.5]
    assert lab[1].tolist() == labels[1].tolist() and val[1].tolist() == values[1].tolist()   # no count: slots kept
    pi = R.estimate_pi(val, n, alpha)
    assert pi[0, 0] == 2.25 / (2.25 + 1.25 + 0.5 + 0.5 + 0.5 + 5 * 0.25)


def test_node_with_every_link_held_out_keeps_its_slots():
    """links 0-1, 1-2, 2-0, 3-4, 4-0 with 3-4 held out: node 3 has no training link (no count, no pads)"""
    edges = np.array([[0, 1], [1, 2], [0, 2], [3, 4], [0, 4]])
    fk = R.FindK(edges, np.arange(5), 5, 2, heldout_ratio=0)
    fk.train = np.array([True, True, True, False, True])
    lab0, val0 = fk.labels.copy(), fk.values.copy()
    fk.step()
    assert fk.labels[3].tolist() == lab0[3].tolist() and fk.values[3].tolist() == val0[3].tolist()
    # node 4's only training neighbour is node 0 (label 0 before the step): one count, 4 pads
    assert fk.labels[4, 0] == 0 and fk.values[4, 0] == 1 + 0.5 and np.all(fk.values[4, 1:] == 1.0)


def test_groups_drop_the_65535_label_and_count_unlikely_entries():
    n = 70000
    labels = np.zeros((n, 5), np.int64)
    labels[:] = np.arange(5) + 100
    labels[0] = [65535, 1, 2, 3, 4]
    labels[1] = [65535, 11, 12, 13, 14]     # 0-1 share only 65535: likely, but dropped
    labels[2] = [7, 20, 21, 22, 23]
    labels[3] = [7, 30, 31, 32, 33]          # 2-3 share 7
    labels[4] = [40, 41, 42, 43, 44]
    labels[5] = [50, 51, 52, 53, 54]         # 4-5 share nothing: unlikely both ways
    pi = np.full((n, 5), 0.1)
    edges = np.array([[0, 1], [2, 3], [4, 5]])
    bad, mem = R.groups(labels, pi, edges, 0.5)
    assert bad == 2
    assert (mem >> 32).tolist() == [7, 7] and (mem & 0xFFFFFFFF).tolist() == [2, 3]
    # a split: 2-3 share 7 and 20 with equal products -> max / sum = 0.5; below 0.9 both directions are unlikely
    labels[3] = [7, 20, 31, 32, 33]
    bad, mem = R.groups(labels, pi, edges, 0.9)
    assert bad == 4 and len(mem) == 0
    # ties: the first strict maximum wins (k1 outer, k2 inner) -- from 2's side 7 (its slot 0), from 3's side also 7
    bad, mem = R.groups(labels, pi, edges, 0.5)
    assert bad == 2 and (mem >> 32).tolist() == [7, 7]


def test_restatement_iteration_count_and_empty_heldout_rows():
    edges, seq2id = R.read_graph(ASSORT, 75)
    fk = R.FindK(edges, seq2id, 75, 4, heldout_ratio=0).run()
    assert fk.iter == 2                       # floor(log10 75) + 1
    assert fk.heldout_text().split("\n")[0].split("\t")[2] == "-nan"
    fk2 = R.FindK(edges, seq2id, 75, 4).run()
    assert fk2.rows[0][2] == int(0.01 * len(edges)) // 2 * 2


@pytest.mark.parametrize("extra,needle", [
    (["-gpus", "2"], "-gpus N > 1"),
    (["-kshard"], "-kshard"),
    (["-sharded"], "-sharded"),
    (["-minibatch", "10"], "-minibatch"),
    (["-predict-pairs", "pairs.txt"], "-predict-pairs"),
    (["-recommend", "5"], "-recommend"),
])
def test_cli_refusals(tmp_path, extra, needle):
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-findk"] + extra, str(tmp_path))
    assert r.returncode == 2 and needle in r.stderr and "-findk" in r.stderr, (r.returncode, r.stderr)


def test_cli_no_engine_message_and_rnode(tmp_path):
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4"], str(tmp_path))
    assert r.returncode == 2 and "only the -link-sampling and -batch engines" in r.stderr
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-link-sampling", "-rnode"], str(tmp_path))
    assert r.returncode == 2 and "-rnode" in r.stderr
    r = _run(["-file", ASSORT, "-n", "75", "-k", "4", "-findk", "-rnode"], str(tmp_path))
    assert r.returncode == 2 and "-rnode" in r.stderr


def test_cli_usage_names_findk(tmp_path):
    r = _run(["-help"], str(tmp_path))
    assert "-findk" in r.stdout


@pytest.mark.parametrize("extra,name", [
    ([], "n75-k75-mmsb-findk"),
    (["-seed", "5"], "n75-k75-mmsb-seed5-findk"),
    (["-batch"], "n75-k75-mmsb-batch"),
    (["-link-sampling"], "n75-k75-mmsb-linksampling"),
])
def test_cli_output_directory(tmp_path, extra, name):
    """src/env.hh:503-528: -batch / -link-sampling take precedence in the name; -k up to n is accepted"""
    r = _run(["-file", ASSORT, "-n", "75", "-k", "75", "-findk"] + extra, str(tmp_path))
    assert os.path.isdir(os.path.join(str(tmp_path), name)), (os.listdir(str(tmp_path)), r.stderr)
    assert "+ Estimating communities" in r.stdout
    d = os.path.join(str(tmp_path), name)
    assert open(os.path.join(d, "heldout-edges.txt")).read() == "\n"
    for f in ("validation-edges.txt", "training-edges.txt", "stats.txt", "time.txt", "convergence.txt", "cmap.txt",
              "validation.txt", "training.txt", "logl.txt", "modularity.txt", "uncolored-links.txt", "heldout.txt"):
        assert os.path.exists(os.path.join(d, f)), f


def test_abi_additions_without_a_device_or_handle():
    from svinet_amd import _svils
    lib = _svils.load()
    names = [e for e in _svils.EXPORTS if e.startswith("svils_findk_")]
    assert len(names) == 10 and lib.svils_abi_version() == 8
    hdr = open(os.path.join(ROOT, "include", "svils.h")).read()
    for e in names:
        assert e + "(" in hdr
    h = C.c_void_p()
    rc = lib.svils_findk_create(0, 10, 0.1, 0.5, C.byref(h))
    if rc == 0:   # a device: a null handle is an argument error
        assert lib.svils_findk_destroy(h) == 0
        assert lib.svils_findk_count(None, None) == -1 and b"null handle" in lib.svils_last_error()
        return
    assert rc == -2 and b"no CPU path" in lib.svils_last_error()
    calls = {"svils_findk_set_graph": (None, None, 0, None, None, 0), "svils_findk_init_state": (None, None, None),
             "svils_findk_count": (None, None), "svils_findk_pad_requests": (None, None, None, None),
             "svils_findk_apply": (None, None), "svils_findk_report": (None, None, None, None, None),
             "svils_findk_get_state": (None, None, None, None), "svils_findk_get_timing": (None, None)}
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -2, name
        assert b"no CPU path" in lib.svils_last_error(), name
