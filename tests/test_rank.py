"""Ranks of given links (svils_rank_links, -rank-pairs / -rank-heldout): what can be checked without a device -- the entry
point exists and refuses a null handle, the CLI refuses the flags where they do not apply, and the pairs file is read and
checked before anything touches the device."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
FILES = ("link-ranks.txt", "heldout-ranks.txt", "link-ranks-summary.txt")


def _run(args, cwd):
    return subprocess.run([SVINET] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def test_entry_point_is_exported_and_declared():
    from svinet_amd import _svils
    hdr = open(os.path.join(ROOT, "include", "svils.h")).read()
    assert "svils_rank_links" in _svils.EXPORTS
    assert re.search(r"^int svils_rank_links\(svils_handle \*h, const uint32_t \*pairs, uint64_t npairs,", hdr, re.M)
    assert hasattr(_svils.Engine, "rank_links")


def test_null_handle_is_refused():
    from svinet_amd import _svils
    lib = _svils.load()
    assert lib.svils_rank_links(None, None, 0, None, None, None, None) == -1
    assert b"null handle" in lib.svils_last_error()
    assert lib.svils_abi_version() == 8


@pytest.mark.parametrize("flag", [["-rank-heldout"], ["-rank-pairs", "PAIRS"]])
@pytest.mark.parametrize("mode,needle", [
    (["-link-sampling", "-gpus", "2"], "-gpus N > 1"),
    (["-link-sampling", "-kshard"], "-kshard"),
    (["-link-sampling", "-sharded"], "-sharded"),
    (["-batch"], "-batch"),
    (["-findk"], "is not available with -findk"),
    (["-gml"], "is not available with -gml"),
    (["-lcstats"], "is not available with -lcstats"),
])
def test_cli_rejections(graph_files, tmp_path, flag, mode, needle):
    f = tmp_path / "pairs.txt"
    f.write_text("0\t1\n")
    flag = [str(f) if x == "PAIRS" else x for x in flag]
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "4"] + mode + flag, str(tmp_path))
    assert r.returncode == 2 and needle in r.stderr and flag[0] in r.stderr, (r.returncode, r.stderr)


@pytest.mark.parametrize("flag", [["-rank-heldout"], ["-rank-pairs", "/dev/null"]])
def test_cli_rejects_column_tiled_k(graph_files, tmp_path, flag):
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "2100", "-link-sampling"] + flag, str(tmp_path))
    assert r.returncode == 2 and "-k > 2048" in r.stderr and flag[0] in r.stderr


def test_cli_unreadable_pairs_file(graph_files, tmp_path):
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-link-sampling", "-rank-pairs", "/nonexistent/pairs.txt"],
             str(tmp_path))
    assert r.returncode == 2 and "cannot read -rank-pairs file" in r.stderr


def test_cli_unknown_pair_id_fails_before_the_device(graph_files, tmp_path):
    """like -predict-pairs: the file is read in the constructor, so a bad line is reported as such and not as the missing
    device of a box without a GPU"""
    f = tmp_path / "pairs.txt"
    f.write_text("0\t1\n999999\t2\n")
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-link-sampling", "-rank-pairs", str(f)], str(tmp_path))
    assert r.returncode == 2 and "-rank-pairs" in r.stderr and "not found" in r.stderr and "no HIP device" not in r.stderr, r.stderr
    g = tmp_path / "pairs_self.txt"
    g.write_text("3\t3\n")
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-link-sampling", "-rank-pairs", str(g)], str(tmp_path))
    assert r.returncode == 2 and "one node" in r.stderr and "no HIP device" not in r.stderr, r.stderr


def test_cli_without_the_flags_writes_no_rank_files(graph_files, tmp_path):
    """with a device the run completes, without one it ends at the missing device: neither leaves one of the three files"""
    r = _run(["-file", graph_files["assort"], "-n", "75", "-k", "4", "-link-sampling", "-no-stop", "-max-iterations", "3"],
             str(tmp_path))
    assert r.returncode == 0 or "no HIP device" in r.stderr, r.stderr
    dirs = [d for d in tmp_path.iterdir() if d.is_dir()]
    assert dirs
    for d in dirs:
        for name in FILES:
            assert not (d / name).exists()


def test_usage_lists_the_flags(tmp_path):
    r = _run(["-help"], str(tmp_path))
    assert r.returncode == 0 and "-rank-pairs" in r.stdout and "-rank-heldout" in r.stdout
