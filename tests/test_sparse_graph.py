"""-sparse-graph without a device: svils_batch_create_sparse repeats the argument checks of svils_batch_create and has
no SVILS_BATCH_MAX_N check, the command line lets the sampled engines past the -n cap with the flag and refuses the flag
everywhere else, before anything is read or created."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from svinet_amd import _svils, host_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
ERR_ARG, ERR_DEVICE, ERR_UNSUPPORTED = -1, -2, -4


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _cli(args, tmp, timeout=120, cwd=None):
    return subprocess.run([SVINET] + args + ["-outdir", str(tmp)], capture_output=True, text=True, timeout=timeout, cwd=cwd)


def test_create_sparse_repeats_the_argument_checks_and_has_no_n_cap():
    L = _svils.load()
    assert "svils_batch_create_sparse" in _svils.EXPORTS and L.svils_abi_version() == 8
    h = C.c_void_p()
    create = lambda n, k, alpha=0.25, eta0=1.0, eta1=1.0, eps=1e-30: L.svils_batch_create_sparse(0, n, k, alpha, eta0, eta1, eps, C.byref(h))
    assert create(1, 4) == ERR_ARG and b"svils_batch_create_sparse" in L.svils_last_error()
    assert create(10, 1) == ERR_ARG
    assert create(10, 4, alpha=0.0) == ERR_ARG and create(10, 4, eta1=-1.0) == ERR_ARG and create(10, 4, eps=0.0) == ERR_ARG
    assert create(10, 4, eps=1.0) == ERR_ARG
    assert L.svils_batch_create_sparse(0, 10, 4, 0.25, 1.0, 1.0, 1e-30, None) == ERR_ARG
    assert create(10, 257) == ERR_UNSUPPORTED and b"SVILS_BATCH_MAX_K" in L.svils_last_error()
    assert h.value is None
    # above the cap of the dense form: past every argument check, as far as the device
    rc = create(_svils.BATCH_MAX_N + 1, 4)
    if _have_gpu():
        assert rc == 0 and h.value
        assert L.svils_batch_destroy(h) == 0
    else:
        assert rc == ERR_DEVICE and b"no CPU path" in L.svils_last_error() and h.value is None
    # the dense form keeps its cap and its message
    d = C.c_void_p()
    assert L.svils_batch_create(0, _svils.BATCH_MAX_N + 1, 4, 0.25, 1.0, 1.0, 1e-30, C.byref(d)) == ERR_UNSUPPORTED
    assert b"svils_batch_create: n = 32769 exceeds SVILS_BATCH_MAX_N" in L.svils_last_error() and d.value is None


def test_python_classes_take_the_flag():
    if not _have_gpu():
        with pytest.raises(_svils.SvilsError) as ei:
            _svils.Batch(_svils.BATCH_MAX_N + 1, 4, 0.25, (1.0, 1.0), sparse=True)
        assert ei.value.code == ERR_DEVICE and "no CPU path" in str(ei.value)
    from conftest import GOLDEN
    path = os.path.join(GOLDEN, "graphs", "assort-75-4.txt")
    # the all-pairs engine, the host loops and the lower bound have no sparse form
    with pytest.raises(ValueError):
        host_api.BatchEngine(path, 75, 4, on_device=True, sparse_graph=True)
    with pytest.raises(ValueError):
        host_api.StratNodeEngine(path, 75, 4, on_device=False, sparse_graph=True)
    with pytest.raises(ValueError):
        host_api.SampledEngine(path, 75, 4, "rnode", on_device=True, logl=True, sparse_graph=True)
    if not _have_gpu():
        with pytest.raises(_svils.SvilsError) as ei:
            host_api.StratNodeEngine(path, 75, 4, on_device=True, heldout_ratio=0.1, sparse_graph=True)
        assert ei.value.code == ERR_DEVICE and "no CPU path" in str(ei.value)


def _ring_file(tmp_path, n=300):
    rng = np.random.RandomState(5)
    pairs = {(i, (i + 1) % n) for i in range(n)} | {tuple(rng.randint(0, n, 2)) for _ in range(3 * n)}
    path = tmp_path / "ring.txt"
    path.write_text("".join("%d\t%d\n" % (a + 1, b + 1) for a, b in sorted(pairs) if a != b))
    return str(path)


def test_cli_flag_lifts_the_n_cap(tmp_path):
    """-n 40000 is refused without the flag (today's refusal, the limit and the engine named) and passes the limits with it:
    without a GPU the run then fails after the host set-up, as the -n 75 case does.  -n is the declared size: the file
    has 300 nodes, so the engine and its handle are made at n = 300 -- this test is about the limit check of the command
    line alone.  A handle above the cap is made in the GPU tier (tests/test_gpu_sparse_graph.py, n = 33 025)"""
    graph, out = _ring_file(tmp_path), tmp_path / "out"
    out.mkdir()
    size = ["-file", graph, "-n", "40000", "-k", "4", "-heldout-ratio", "0.1", "-max-iterations", "30"]
    r = _cli(size + ["-snode"], out)
    assert r.returncode == 2 and "32768" in r.stderr and "-snode" in r.stderr and not list(out.iterdir())
    r = _cli(size + ["-snode", "-sparse-graph"], out)
    run = out / "n40000-k4-mmsb-SUrnode"
    assert (run / "heldout-pairs.txt").exists(), (r.returncode, r.stderr, list(out.iterdir()))
    if _have_gpu():
        assert r.returncode == 0, r.stderr
        assert len((run / "gamma.txt").read_text().splitlines()) == 300
    else:
        assert r.returncode != 0 and "no CPU path" in r.stderr
        assert not list(out.rglob("gamma.txt")) and not list(out.rglob("heldout.txt"))
    # the K cap stays, with the flag too
    for engine in (["-snode"], ["-infset"], ["-rnode"], ["-rpair"], ["-rpair", "-stratified"]):
        r = _cli(["-file", "x", "-n", "40000", "-k", "300", "-sparse-graph"] + engine, tmp_path / "none", timeout=60)
        assert r.returncode == 2 and "256" in r.stderr and engine[0] in r.stderr, (engine, r.stderr)
        r = _cli(["-file", "x", "-n", "40000", "-k", "4"] + engine, tmp_path / "none", timeout=60)
        assert r.returncode == 2 and "32768" in r.stderr and engine[0] in r.stderr and "-sparse-graph" in r.stderr, (engine, r.stderr)
    assert not (tmp_path / "none").exists()


REFUSED_BESIDE = [("-batch", []), ("-batch-gpu", []), ("-logl", []), ("-orig", []), ("-ppc", []), ("-ppc-orig", []), ("-gen", []),
                  ("-link-sampling", []), ("-findk", []), ("-gml", []), ("-lcstats", []), ("-preprocess", []), ("-host-loops", [])]


@pytest.mark.parametrize("other,extra", REFUSED_BESIDE)
@pytest.mark.parametrize("engine", [[], ["-snode"], ["-infset"], ["-rnode"], ["-rpair"]])
def test_cli_refusals(tmp_path, other, extra, engine):
    for flags in (["-sparse-graph"] + engine + [other] + extra, [other] + extra + engine + ["-sparse-graph"]):
        r = _cli(["-file", "x", "-n", "75", "-k", "4"] + flags, tmp_path, timeout=60)
        assert r.returncode == 2 and "-sparse-graph" in r.stderr and other in r.stderr, (flags, r.returncode, r.stderr)
        assert other != "-batch" or "-batch-gpu" not in r.stderr
    assert not list(tmp_path.iterdir())


def test_cli_refuses_the_flag_alone_and_shows_it_in_the_usage(tmp_path):
    r = _cli(["-file", "x", "-n", "75", "-k", "4", "-sparse-graph"], tmp_path, timeout=60)
    assert r.returncode == 2 and "-sparse-graph" in r.stderr and "-snode" in r.stderr and "-infset" in r.stderr
    assert not list(tmp_path.iterdir())
    r = _cli(["-help"], tmp_path)
    assert r.returncode == 0 and "\t-sparse-graph\t" in r.stdout
    for row in ("\t-rnode\t", "\t-snode\t", "\t-infset\t"):   # the capped engines point at the flag
        at = r.stdout.index(row)
        assert "unless -sparse-graph" in r.stdout[at:at + 700], row
