"""-m gpu: `svinet -findk` (svils_findk_*) against the numpy restatement tools/restate_findk.py -- communities.txt,
communities_size.txt and uncolored-links.txt byte for byte, heldout.txt to 1e-10 relative with the wall-clock column
ignored -- and the Python API's state against the restatement's exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import restate_findk as R  # noqa: E402

pytestmark = pytest.mark.gpu

SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")


def _cli(path, n, k, cwd, extra=()):
    r = subprocess.run([SVINET, "-file", path, "-n", str(n), "-k", str(k), "-findk"] + list(extra), cwd=cwd,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    dirs = [d for d in os.listdir(cwd) if d.endswith("-findk")]
    assert len(dirs) == 1, dirs
    return os.path.join(cwd, dirs[0])


def _rows(text):
    return [[float(v) for j, v in enumerate(line.split("\t")) if j != 1] for line in text.strip("\n").split("\n") if line]


def _check(d, fk):
    for name in ("communities.txt", "communities_size.txt"):
        want = fk.communities[-1] if name == "communities.txt" else fk.sizes[-1]
        assert open(os.path.join(d, name)).read() == want, name
    assert open(os.path.join(d, "uncolored-links.txt")).read() == "".join("%d\n" % u for u in fk.unlikely)
    got, want = _rows(open(os.path.join(d, "heldout.txt")).read()), _rows(fk.heldout_text())
    assert len(got) == len(want)
    np.testing.assert_allclose(np.array(got), np.array(want), rtol=1e-10, atol=0, equal_nan=True)
    assert open(os.path.join(d, "aggregate.txt")).read() == ""
    assert open(os.path.join(d, "heldout-edges.txt")).read() == "\n"


_CACHE = {}


def _restated(path, n, k, **kw):
    key = (path, n, k, tuple(sorted(kw.items())))
    if key not in _CACHE:
        edges, seq2id = R.read_graph(path, n)
        _CACHE[key] = R.FindK(edges, seq2id, len(seq2id), k, **kw).run()
    return _CACHE[key]


@pytest.fixture(scope="module")
def big_graphs(tmp_path_factory):
    from svinet_amd import mmsbgen_sparse
    d = tmp_path_factory.mktemp("findk_graphs")
    out = {}
    pairs = mmsbgen_sparse.generate(200000, 64, 24)
    out["mmsb"] = str(d / "mmsb_n200k.txt")
    mmsbgen_sparse.write_pairs(out["mmsb"], pairs)
    # one hub of degree 30000 over degree-1 leaves, a few of them in a ring with each other, and a clique of 80
    n_leaf = 30000
    hub = [(0, i) for i in range(1, n_leaf + 1)]
    ring = [(i, i + 1) for i in range(1, 2000, 2)]
    base = n_leaf + 1
    clique = [(base + a, base + b) for a in range(80) for b in range(a + 1, 80)]
    with open(str(d / "hub.txt"), "w") as f:
        for p, q in hub + ring + clique + [(base, 5)]:
            f.write("%d\t%d\n" % (p, q))
    out["hub"] = str(d / "hub.txt")
    out["hub_n"] = base + 80
    return out


@pytest.mark.parametrize("name,n,k,extra,kw", [
    ("assort", 75, 4, [], {}),
    ("lfr", 1000, 28, [], {}),
    ("lfr", 1000, 1000, [], {}),
    ("lfr", 1000, 28, ["-link-thresh", "0.9"], {"link_thresh": 0.9}),
    ("lfr", 1000, 28, ["-heldout-ratio", "0"], {"heldout_ratio": 0.0}),
    ("lfr", 1000, 28, ["-seed", "5"], {}),
    ("astroph", 17903, 20, [], {}),
])
def test_cli_matches_restatement(graph_files, tmp_path, name, n, k, extra, kw):
    d = _cli(graph_files[name], n, k, str(tmp_path), extra)
    if "-seed" in extra:
        assert os.path.basename(d) == "n%d-k%d-mmsb-seed5-findk" % (n, k)
    _check(d, _restated(graph_files[name], n, k, **kw))


def test_cli_large_and_hub_graphs(big_graphs, tmp_path):
    """n = 2e5 (labels above 65535, the uint32 total_pairs wraps) and a hub of degree 30000 (the global-hash path)"""
    fk = _restated(big_graphs["mmsb"], 200000, 64)
    assert np.any(fk.labels > 65535)
    os.makedirs(str(tmp_path / "a"))
    os.makedirs(str(tmp_path / "b"))
    _check(_cli(big_graphs["mmsb"], 200000, 64, str(tmp_path / "a")), fk)
    n = big_graphs["hub_n"]
    _check(_cli(big_graphs["hub"], n, 10, str(tmp_path / "b")), _restated(big_graphs["hub"], n, 10))


def test_two_runs_are_identical(graph_files, tmp_path):
    outs = []
    for run in ("a", "b"):
        os.makedirs(str(tmp_path / run))
        d = _cli(graph_files["astroph"], 17903, 20, str(tmp_path / run))
        outs.append({f: open(os.path.join(d, f)).read() for f in ("communities.txt", "communities_size.txt",
                                                                   "uncolored-links.txt")})
        outs[-1]["heldout"] = [r for r in _rows(open(os.path.join(d, "heldout.txt")).read())]
    assert outs[0] == outs[1]


def test_python_state_equals_restatement(graph_files, big_graphs):
    from svinet_amd.host_api import FindK
    for path, n, k in ((graph_files["lfr"], 1000, 28), (big_graphs["hub"], big_graphs["hub_n"], 10)):
        ref = _restated(path, n, k)
        fk = FindK(path, n, k)
        rows = fk.run()
        lab, val, masks = fk.state()
        assert fk.iter == ref.iter
        assert np.array_equal(lab.astype(np.int64), ref.labels) and np.array_equal(val, ref.values)
        assert fk.unlikely == ref.unlikely[-1]
        np.testing.assert_allclose(rows[:, 2], [r[1] for r in ref.rows], rtol=1e-10)
        # masks: the members of every community are the nodes with a set bit naming it
        bad, mem = R.groups(ref.labels, ref.pi, ref.edges, 0.5)
        got = set()
        for i in np.nonzero(masks)[0]:
            for b in range(5):
                if masks[i] >> b & 1:
                    got.add((int(lab[i, b]), int(i)))
        assert got == set(zip((mem >> 32).tolist(), (mem & 0xFFFFFFFF).tolist()))
        t = fk.timing()
        assert t["count_ms"] > 0 and t["groups_ms"] > 0
        fk.close()


def test_link_sampling_engine_unaffected(graph_files):
    from svinet_amd.host_api import FindK, Setup
    setup = Setup(graph_files["lfr"], 1000, 28)
    before = setup.engine(use_validation_stop=False, device=0)
    before.sweep(5)
    g0, l0, c0 = before.state()
    fk = FindK(graph_files["lfr"], 1000, 28)
    fk.run()
    fk.close()
    after = setup.engine(use_validation_stop=False, device=0)
    after.sweep(5)
    g1, l1, c1 = after.state()
    assert np.array_equal(g0, g1) and np.array_equal(l0, l1) and np.array_equal(c0, c1)
    before.sweep(2)
    after.sweep(2)
    assert np.array_equal(before.state()[0], after.state()[0])
