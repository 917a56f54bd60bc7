"""-m gpu: the device memory of the standalone tool handles (svils_findk_*, svils_lc_*; csrc/svils_tool.h).  After a warm-up
cycle, three cycles of create -> set_graph (a refused one on the way, then a graph of another size) -> state / model -> run ->
destroy leave the device's free memory where the warm-up left it: both allocation scopes, the handle's and the graph's,
come back.  So does a sweep handle's held-out set when svils_set_validation replaces it."""
import ctypes as C

import numpy as np
import pytest

from svinet_amd import _svils

pytestmark = pytest.mark.gpu

SLACK = 2 << 20   # bytes
ERR_ARG = -1


def _links(n, m, hub, seed):
    """about m distinct links p < q < n, plus node 0 linked to nodes 1 .. hub (a hub above the LDS hash of -findk)"""
    rng = np.random.default_rng(seed)
    p, q = rng.integers(0, n, m), rng.integers(0, n, m)
    p, q = np.minimum(p, q), np.maximum(p, q)
    key = np.concatenate([p[p < q].astype(np.uint64) * n + q[p < q], np.arange(1, hub + 1, dtype=np.uint64)])
    key = np.unique(key)
    return np.ascontiguousarray(np.stack([key // n, key % n], axis=1).astype(np.uint32))


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def _findk_run(L, h, n):
    m = C.c_uint32()
    _svils._chk(L.svils_findk_count(h, C.byref(m)))
    nodes, nd, lab = np.zeros(m.value, np.uint32), np.zeros(m.value, np.uint32), np.zeros((m.value, 4), np.uint32)
    _svils._chk(L.svils_findk_pad_requests(h, nodes.ctypes.data, nd.ctypes.data, lab.ctypes.data))
    pads = np.zeros((m.value, 4), np.uint32)
    _svils._chk(L.svils_findk_apply(h, pads.ctypes.data))
    tll, unlikely = C.c_double(), C.c_uint32()
    sums, masks = np.zeros(3), np.zeros(n, np.uint32)
    _svils._chk(L.svils_findk_report(h, C.byref(tll), sums.ctypes.data, C.byref(unlikely), masks.ctypes.data))
    assert np.isfinite(tll.value) and np.all(np.isfinite(sums))


def _findk_cycle(L, n, sizes, seed):
    h = C.c_void_p()
    _svils._chk(L.svils_findk_create(0, n, 0.25, 0.5, C.byref(h)))
    try:
        rng = np.random.default_rng(seed)
        labels = ((np.arange(n)[:, None] + np.arange(5)[None, :]) % n).astype(np.uint32)
        values = rng.uniform(0.5, 2.0, (n, 5))
        for i, (m, hub) in enumerate(sizes):
            links = _links(n, m, hub, seed + i)
            held = np.zeros(len(links), np.uint8)
            held[:100] = 1
            pairs = np.ascontiguousarray(np.concatenate([links[:100], np.ones((100, 1), np.uint32)], axis=1))
            if i == 0:
                bad = links.copy()
                bad[-1] = (bad[-1, 0], n)   # names a node >= n: refused, the handle stays as it was
                assert L.svils_findk_set_graph(h, bad.ctypes.data, len(bad), None, None, 0) == ERR_ARG
            _svils._chk(L.svils_findk_set_graph(h, links.ctypes.data, len(links), held.ctypes.data, pairs.ctypes.data, len(pairs)))
            _svils._chk(L.svils_findk_init_state(h, labels.ctypes.data, values.ctypes.data))
            _findk_run(L, h, n)
    finally:
        assert L.svils_findk_destroy(h) == 0


def _lc_cycle(L, n, k, sizes, seed):
    h = C.c_void_p()
    _svils._chk(L.svils_lc_create(0, n, k, C.byref(h)))
    try:
        rng = np.random.default_rng(seed)
        lam = np.ascontiguousarray(rng.uniform(0.5, 2.0, (k, 2)))
        for i, (m, hub) in enumerate(sizes):
            links = _links(n, m, hub, seed + i)
            links = np.ascontiguousarray(links[rng.permutation(len(links))])   # the caller's order is not (p, q)
            if i == 0:
                bad = links.copy()
                bad[-1] = (bad[-1, 1], bad[-1, 0])   # p > q: refused, the handle stays as it was
                assert L.svils_lc_set_graph(h, bad.ctypes.data, len(bad)) == ERR_ARG
            _svils._chk(L.svils_lc_set_graph(h, links.ctypes.data, len(links)))
            gamma = np.ascontiguousarray(rng.uniform(0.1, 5.0, (n, k)))
            _svils._chk(L.svils_lc_set_model(h, gamma.ctypes.data, lam.ctypes.data))
            _svils._chk(L.svils_lc_run(h))
            count = C.c_uint64()
            _svils._chk(L.svils_lc_get_gml(h, C.byref(count), None))
            assert count.value <= len(links)
    finally:
        assert L.svils_lc_destroy(h) == 0


# per cycle: the handle's n, then the graphs it is given in turn as (links drawn, hub degree)
CYCLES = [(40000, [(300000, 3000), (500000, 0)]),
          (60000, [(600000, 5000), (200000, 2500)]),
          (50000, [(400000, 0), (700000, 4000)])]


@pytest.mark.parametrize("tool", ["findk", "lc"])
def test_tool_handles_give_back_device_memory(tool):
    L = _svils.load()

    def cycle(i):
        n, sizes = CYCLES[i % len(CYCLES)]
        if tool == "findk":
            _findk_cycle(L, n, sizes, 100 * i)
        else:
            _lc_cycle(L, n, 24 + i, sizes, 100 * i)

    cycle(0)   # warm-up: code objects, runtime pools
    warm = _free_bytes()
    for i in range(3):
        cycle(i)
        free = _free_bytes()
        assert free >= warm - SLACK, (tool, i, warm - free)


def test_set_validation_gives_back_the_set_it_replaces(graph_files):
    """svils_set_validation three times with sets of the same size: the device's free memory stays where the first call left it"""
    from svinet_amd.host_api import Setup
    setup = Setup(graph_files["lfr"], 1000, 28)
    eng = setup.engine(use_validation_stop=False)
    rng = np.random.default_rng(7)
    nv = 2000000   # 40 MB of pairs and values per set
    p = rng.integers(0, 999, nv)
    pairs = np.stack([p, rng.integers(p + 1, 1000), rng.integers(0, 2, nv)], axis=1).astype(np.uint32)
    eng.set_validation(pairs)
    warm = _free_bytes()
    for i in range(2):
        eng.set_validation(pairs)
        free = _free_bytes()
        assert free >= warm - SLACK, (i, warm - free)
    eng.set_validation(setup.validation_sorted)   # ... and the handle sweeps on the set it holds
    eng.sweep(2)
    eng.synchronize()
    assert eng.rows().shape == (2, 10) and np.all(np.isfinite(eng.rows()))
