"""Link prediction (svils_link_prob / svils_predict_links, -predict-pairs / -recommend): what can be checked without a
device -- the entry points exist and refuse a null handle, the CLI refuses the flags where they do not apply, and the
pairs file is read and checked before anything touches the device."""
import os
import subprocess

import pytest

from conftest import ROOT

SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")


def _run(args, cwd):
    return subprocess.run([SVINET] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def test_null_handle_is_refused():
    from svinet_amd import _svils
    lib = _svils.load()
    assert "svils_link_prob" in _svils.EXPORTS and "svils_predict_links" in _svils.EXPORTS
    assert lib.svils_link_prob(None, None, 0, None) == -1
    assert b"null handle" in lib.svils_last_error()
    assert lib.svils_predict_links(None, None, 0, 10, None, None) == -1
    assert _svils.PREDICT_MAX_TOPK == 256


def test_header_declares_the_limit():
    hdr = open(os.path.join(ROOT, "include", "svils.h")).read()
    assert "#define SVILS_PREDICT_MAX_TOPK 256" in hdr
    assert "src/linksampling.hh:240-256" in hdr


@pytest.mark.parametrize("extra,needle", [
    (["-link-sampling", "-recommend", "0"], "-recommend wants a count of 1 .. 256"),
    (["-link-sampling", "-recommend", "257"], "-recommend wants a count of 1 .. 256"),
    (["-link-sampling", "-recommend", "5", "-gpus", "2"], "-gpus N > 1"),
    (["-link-sampling", "-recommend", "5", "-gpus", "2", "-kshard"], "-gpus N > 1"),
    (["-link-sampling", "-recommend", "5", "-kshard"], "-kshard"),
    (["-link-sampling", "-recommend", "5", "-sharded"], "-sharded"),
    (["-batch", "-recommend", "5"], "-batch"),
    (["-link-sampling", "-predict-pairs", "/nonexistent/pairs.txt"], "cannot read -predict-pairs file"),
])
def test_cli_rejections(graph_files, tmp_path, extra, needle):
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "4"] + extra, str(tmp_path))
    assert r.returncode == 2 and needle in r.stderr, (r.returncode, r.stderr)


def test_cli_rejects_column_tiled_k(graph_files, tmp_path):
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "2100", "-link-sampling", "-recommend", "3"], str(tmp_path))
    assert r.returncode == 2 and "-k > 2048" in r.stderr


def test_cli_unknown_pair_id_fails_before_the_device(graph_files, tmp_path):
    """the pairs file is read in the constructor, before any device work: an unknown external id is reported as such
    (on a box without a GPU, before the 'no HIP device' failure)"""
    f = tmp_path / "pairs.txt"
    f.write_text("0\t1\n999999\t2\n")
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-link-sampling", "-predict-pairs", str(f)], str(tmp_path))
    assert r.returncode == 2 and "not found" in r.stderr and "no HIP device" not in r.stderr, r.stderr
    g = tmp_path / "pairs_self.txt"
    g.write_text("3\t3\n")
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-link-sampling", "-predict-pairs", str(g)], str(tmp_path))
    assert r.returncode == 2 and "one node" in r.stderr and "no HIP device" not in r.stderr, r.stderr


def test_cli_without_the_flags_writes_no_prediction_files(graph_files, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by tests/test_gpu_predict.py")
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-link-sampling"], str(tmp_path))
    assert r.returncode != 0 and "no HIP device" in r.stderr
    for d in tmp_path.iterdir():
        if d.is_dir():
            assert not (d / "link-prob.txt").exists() and not (d / "recommendations.txt").exists()


def test_usage_lists_the_flags(tmp_path):
    r = _run(["-help"], str(tmp_path))
    assert r.returncode == 0 and "-predict-pairs" in r.stdout and "-recommend" in r.stdout
