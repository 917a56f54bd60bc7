"""The device backend of the -batch engine without a device: the instantiation table of the pair kernel
(svils_batch_variant), the argument checks of svils_batch_create / svils_batch_set_graph, and -batch-gpu on a box
without a GPU -- it fails with the library's message and never runs the host engine instead."""
import ctypes as C
import os
import subprocess

import pytest

from svinet_amd import _svils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
ERR_ARG, ERR_DEVICE, ERR_UNSUPPORTED = -1, -2, -4


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def test_variant_table_covers_every_k():
    L = _svils.load()
    seen = set()
    for k in range(2, _svils.BATCH_MAX_K + 1):
        w, v = _svils.batch_variant(k)
        assert w * v >= k and 64 % w == 0 and v >= 1, (k, w, v)
        seen.add((w, v))
    assert 2 <= len(seen) <= 16
    w, v = C.c_uint32(), C.c_uint32()
    assert L.svils_batch_variant(257, C.byref(w), C.byref(v)) == ERR_UNSUPPORTED
    assert b"SVILS_BATCH_MAX_K" in L.svils_last_error()
    for k in (0, 1):
        assert L.svils_batch_variant(k, C.byref(w), C.byref(v)) == ERR_ARG
    assert L.svils_batch_variant(4, None, None) == ERR_ARG


def test_argument_checks_do_not_need_a_device():
    L = _svils.load()
    h = C.c_void_p()
    create = lambda n, k, alpha=0.25, eta0=1.0, eta1=1.0, eps=1e-30: L.svils_batch_create(0, n, k, alpha, eta0, eta1, eps, C.byref(h))
    assert create(1, 4) == ERR_ARG and create(10, 1) == ERR_ARG
    assert create(10, 4, alpha=0.0) == ERR_ARG and create(10, 4, eta1=-1.0) == ERR_ARG and create(10, 4, eps=0.0) == ERR_ARG
    assert L.svils_batch_create(0, 10, 4, 0.25, 1.0, 1.0, 1e-30, None) == ERR_ARG
    assert create(10, 257) == ERR_UNSUPPORTED and b"SVILS_BATCH_MAX_K" in L.svils_last_error()
    assert create(_svils.BATCH_MAX_N + 1, 4) == ERR_UNSUPPORTED and b"SVILS_BATCH_MAX_N" in L.svils_last_error()
    assert h.value is None
    # a null handle answers as the other tool handles do: "no HIP device" where there is none, else a bad argument
    null = ERR_ARG if _have_gpu() else ERR_DEVICE
    assert L.svils_batch_set_graph(None, None, 0, None, 0) == null
    assert L.svils_batch_sweep(None, 1) == null
    assert L.svils_batch_get_timing(None, None) == null
    if not _have_gpu():
        assert b"no CPU path" in L.svils_last_error()


def test_no_cpu_fallback():
    if _have_gpu():
        pytest.skip("GPU present")
    with pytest.raises(_svils.SvilsError) as ei:
        _svils.Batch(10, 4, 0.25, (1.0, 1.0))
    assert ei.value.code == ERR_DEVICE and "no CPU path" in str(ei.value)
    from conftest import GOLDEN
    from svinet_amd.host_api import BatchEngine
    with pytest.raises(_svils.SvilsError) as ei:
        BatchEngine(os.path.join(GOLDEN, "graphs", "assort-75-4.txt"), 75, 4, heldout_ratio=0.1, on_device=True)
    assert ei.value.code == ERR_DEVICE and "no CPU path" in str(ei.value)


def test_cli_batch_gpu_without_a_gpu_fails_and_writes_no_model(graph_files, tmp_path):
    if _have_gpu():
        pytest.skip("GPU present")
    r = subprocess.run([SVINET, "-file", graph_files["assort"], "-n", "75", "-k", "4", "-batch-gpu", "-heldout-ratio", "0.1",
                        "-outdir", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "no CPU path" in r.stderr
    assert not list(tmp_path.rglob("gamma.txt")) and not list(tmp_path.rglob("heldout.txt"))


def test_cli_batch_gpu_refuses_sizes_above_the_limits(graph_files, tmp_path):
    for size, limit in ((["-n", "75", "-k", "300"], "256"), (["-n", "40000", "-k", "4"], "32768")):
        r = subprocess.run([SVINET, "-file", graph_files["assort"]] + size + ["-batch-gpu", "-outdir", str(tmp_path)],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and limit in r.stderr, r.stderr
    assert not list(tmp_path.iterdir())
