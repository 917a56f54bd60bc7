"""Neighbourhood baselines of link ranks (svils_nbr_score / svils_nbr_rank, -adamic-adar): what can be checked without a
device -- the entry points exist and refuse a null handle, the CLI takes the flag where it applies and refuses it where it
does not, and a run without it writes none of the new files."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
FILES = ("link-nbr.txt", "link-ranks-aa.txt", "heldout-ranks-aa.txt", "link-ranks-baselines.txt")


def _run(args, cwd):
    return subprocess.run([SVINET] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def test_entry_points_are_exported_and_declared():
    from svinet_amd import _svils
    hdr = open(os.path.join(ROOT, "include", "svils.h")).read()
    assert "svils_nbr_score" in _svils.EXPORTS and "svils_nbr_rank" in _svils.EXPORTS
    assert re.search(r"^int svils_nbr_score\(svils_handle \*h, int measure, const uint32_t \*pairs, uint64_t npairs, "
                     r"double \*score, uint32_t \*common\);", hdr, re.M)
    assert re.search(r"^int svils_nbr_rank\(svils_handle \*h, int measure, const uint32_t \*pairs, uint64_t npairs,", hdr, re.M)
    assert re.search(r"SVILS_NBR_CN = 0, SVILS_NBR_AA = 1, SVILS_NBR_RA = 2 \} svils_nbr_measure;", hdr)
    assert hasattr(_svils.Engine, "nbr_score") and hasattr(_svils.Engine, "nbr_rank")
    assert (_svils.NBR_CN, _svils.NBR_AA, _svils.NBR_RA) == (0, 1, 2)


def test_null_handle_is_refused():
    from svinet_amd import _svils
    lib = _svils.load()
    assert lib.svils_nbr_score(None, 1, None, 0, None, None) == -1
    assert b"null handle" in lib.svils_last_error() and b"svils_nbr_score" in lib.svils_last_error()
    assert lib.svils_nbr_rank(None, 1, None, 0, None, None, None, None) == -1
    assert b"null handle" in lib.svils_last_error() and b"svils_nbr_rank" in lib.svils_last_error()
    assert lib.svils_abi_version() == 8


def test_the_new_unit_is_built_into_the_library():
    from svinet_amd import build
    assert os.path.join(build.CSRC, "svils_nbr.hip") in build._svils_sources()


def test_cli_flag_alone_is_refused(graph_files, tmp_path):
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-link-sampling", "-adamic-adar"], str(tmp_path))
    assert r.returncode == 2 and "-adamic-adar belongs to" in r.stderr and "-rank-heldout" in r.stderr, (r.returncode, r.stderr)
    assert not [d for d in tmp_path.iterdir() if d.is_dir()]          # refused before anything is created


@pytest.mark.parametrize("mode,needle", [
    (["-batch", "-rank-heldout"], "-batch"),
    (["-link-sampling", "-gpus", "2", "-rank-heldout"], "-gpus N > 1"),
    (["-link-sampling", "-kshard", "-rank-heldout"], "-kshard"),
    (["-link-sampling", "-sharded", "-rank-heldout"], "-sharded"),
    (["-findk"], "is not available with -findk"),
    (["-gml"], "is not available with -gml"),
    (["-link-sampling", "-minibatch", "100", "-rank-heldout"], "-minibatch"),
])
def test_cli_rejections(graph_files, tmp_path, mode, needle):
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "4"] + mode + ["-adamic-adar"], str(tmp_path))
    assert r.returncode == 2 and needle in r.stderr and "-adamic-adar" in r.stderr, (r.returncode, r.stderr)
    assert "unsupported option" not in r.stderr


def test_cli_minibatch_refusal_says_why(graph_files, tmp_path):
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-link-sampling", "-minibatch", "20", "-rank-heldout",
              "-adamic-adar"], str(tmp_path))
    assert r.returncode == 2 and "relabelled" in r.stderr and "order" in r.stderr, r.stderr


def test_cli_rejects_column_tiled_k(graph_files, tmp_path):
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "2100", "-link-sampling", "-rank-heldout", "-adamic-adar"],
             str(tmp_path))
    assert r.returncode == 2 and "-k > 2048" in r.stderr and "-adamic-adar" in r.stderr


def test_cli_flag_is_no_longer_an_unsupported_option(graph_files, tmp_path):
    """with a device the run completes, without one it ends at the missing device: the flag itself is taken"""
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-link-sampling", "-no-stop", "-max-iterations", "3",
              "-rank-heldout", "-adamic-adar"], str(tmp_path))
    assert "unsupported option" not in r.stderr and "only the -link-sampling" not in r.stderr
    assert r.returncode == 0 or "no HIP device" in r.stderr, r.stderr


def test_cli_without_the_flag_writes_none_of_the_files(graph_files, tmp_path):
    f = tmp_path / "pairs.txt"
    f.write_text("2\t1\n6\t10\n")
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-link-sampling", "-no-stop", "-max-iterations", "3",
              "-rank-heldout", "-predict-pairs", str(f)], str(tmp_path))
    assert r.returncode == 0 or "no HIP device" in r.stderr, r.stderr
    dirs = [d for d in tmp_path.iterdir() if d.is_dir()]
    assert dirs
    for d in dirs:
        for name in FILES:
            assert not (d / name).exists()


def test_usage_lists_the_flag(tmp_path):
    r = _run(["-help"], str(tmp_path))
    assert r.returncode == 0 and "-adamic-adar" in r.stdout and "link-ranks-baselines.txt" in r.stdout
