"""-m gpu: `svinet -gml` / `-lcstats` (svils_lc_*) against the authors' shipped files and the numpy restatement
tools/restate_gml.py -- every output file byte for byte -- and host_api.LinkCommunities' arrays against the
restatement's bitwise, on adversarial models (ratios a few ulps from the thresholds, ties, NaN ratios, empty
communities, K = 2 / odd / 2100, a 30 000-degree hub, an n = 2e5 K = 512 MMSB graph)."""
import gzip
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import gml_models as M

sys.path.insert(0, os.path.join(ROOT, "tools"))
import restate_findk  # noqa: E402
import restate_gml as R  # noqa: E402

pytestmark = pytest.mark.gpu

SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BATCH = os.path.join(GOLDEN, "ref_assort_batch")
FILES = ("community_stats.txt", "node_bridgeness.txt", "node_influence.txt", "number_of_memberships.txt", "network.gml")


def _cli(args, cwd, timeout=900):
    r = subprocess.run([SVINET] + [str(a) for a in args], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r


def _restated_texts(path, n, k, mdir):
    links, seq2id = restate_findk.read_graph(path, n)
    gamma, ids, lam = R.load_model(mdir, len(seq2id), k)
    assert np.array_equal(ids, seq2id)
    return R.texts(R.link_communities(links, gamma, lam), links, seq2id)


def _check_dir(d, want, names=FILES):
    for name in names:
        assert open(os.path.join(d, name)).read() == want[name], name


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _check_arrays(got, r, links):
    assert np.array_equal(got["group"], r["group"])
    assert _same_bits(got["bridgeness"], r["bridgeness"])
    assert np.array_equal(got["memberships"], r["memberships"]) and np.array_equal(got["influence"], r["influence"])
    assert np.array_equal(got["deg_c"], r["deg_c"])
    for a, b in (("comm_nodes", "comm_nodes"), ("comm_degsum", "comm_degsum"), ("comm_max", "comm_max"), ("comm_argmax", "comm_argmax")):
        assert np.array_equal(got[a].astype(np.int64), r[b].astype(np.int64)), a
    assert np.array_equal(got["colour"], r["colour"])
    assert np.array_equal(got["join"], r["join"]) and np.array_equal(got["gml"], r["gml"])
    assert got["unlikely"] == r["unlikely"]
    links = np.asarray(links, np.int64)
    order = np.lexsort((links[:, 1], links[:, 0]))
    order = order[r["gml"][order]]
    want = np.stack([links[order, 0], links[order, 1], r["colour"][order]], axis=1)
    assert np.array_equal(got["gml_edges"].astype(np.int64), want)


def _lc(links, gamma, lam):
    from svinet_amd.host_api import LinkCommunities
    return LinkCommunities(links, gamma, lam)


def test_assort_matches_the_authors_files(tmp_path):
    for m in ("gamma.txt", "lambda.txt"):
        shutil.copy(os.path.join(BATCH, m), str(tmp_path))
    _cli(["-file", os.path.join(GOLDEN, "graphs", "assort-75-4.txt"), "-n", 75, "-k", 4, "-gml"], str(tmp_path))
    d = str(tmp_path / "gml")
    for mine, theirs in (("community_stats.txt", "obs_stats.txt"), ("node_bridgeness.txt", "obs_bridgeness.txt"),
                         ("node_influence.txt", "obs_influence.txt")):
        assert open(os.path.join(d, mine)).read() == open(os.path.join(BATCH, theirs)).read(), mine
    assert open(os.path.join(d, "network.gml")).read() == open(os.path.join(BATCH, "network.gml")).read() + "]\n"


def test_lfr_k28_matches_restatement(graph_files, tmp_path):
    with gzip.open(os.path.join(GOLDEN, "ref_lfr_k28", "gamma.txt.gz"), "rb") as f, open(str(tmp_path / "gamma.txt"), "wb") as g:
        g.write(f.read())
    shutil.copy(os.path.join(GOLDEN, "ref_lfr_k28", "lambda.txt"), str(tmp_path))
    _cli(["-file", graph_files["lfr"], "-n", 1000, "-k", 28, "-gml"], str(tmp_path))
    _check_dir(str(tmp_path / "gml"), _restated_texts(graph_files["lfr"], 1000, 28, str(tmp_path)))


def test_astroph_tutorial_chain(graph_files, tmp_path):
    path = graph_files["astroph"]
    _cli(["-file", path, "-n", 17903, "-k", 20, "-link-sampling", "-max-iterations", 30], str(tmp_path))
    fit = [d for d in os.listdir(str(tmp_path)) if d.endswith("-linksampling")]
    assert len(fit) == 1, fit
    fit = str(tmp_path / fit[0])
    want = _restated_texts(path, 17903, 20, fit)
    r = _cli(["-file", path, "-n", 17903, "-k", 20, "-gml"], fit)
    assert "+ Done writing GML file" in r.stdout
    _check_dir(os.path.join(fit, "gml"), want)
    _cli(["-file", path, "-n", 17903, "-k", 20, "-lcstats"], fit)
    _check_dir(os.path.join(fit, "n17903-k20-mmsb"), want, FILES[:4])
    assert not os.path.exists(os.path.join(fit, "n17903-k20-mmsb", "network.gml"))
    assert os.path.isdir(os.path.join(fit, "ppc"))


def _cli_on_model(tmp_path, pairs, gamma_by_id, lam):
    """the model's pairs as a network file (ids = the model's row numbers), gamma.txt in the reader's numbering"""
    d = str(tmp_path)
    net = os.path.join(d, "net.txt")
    np.savetxt(net, pairs, fmt="%d", delimiter="\t")
    links, seq2id = restate_findk.read_graph(net, gamma_by_id.shape[0])
    M.write_model(d, gamma_by_id[seq2id], lam, seq2id)
    k = gamma_by_id.shape[1]
    _cli(["-file", net, "-n", len(seq2id), "-k", k, "-gml"], d)
    _check_dir(os.path.join(d, "gml"), _restated_texts(net, len(seq2id), k, d))


def test_adversarial_models_cli(tmp_path):
    links, gamma, lam = M.mixed(8)
    os.makedirs(str(tmp_path / "mixed"))
    _cli_on_model(tmp_path / "mixed", links, gamma, lam)
    assert "\t-nan\t" in open(str(tmp_path / "mixed" / "gml" / "community_stats.txt")).read()
    links, gamma, lam = M.random_model(3000, 2, 20000)
    os.makedirs(str(tmp_path / "k2"))
    _cli_on_model(tmp_path / "k2", links, gamma, lam)


def test_near_threshold_links_need_the_recheck():
    links, gamma, lam = M.near_threshold(64, 4000, seed=3)
    r = R.link_communities(links, gamma, lam)
    rp = R.link_communities(links, gamma, lam, pairwise=True)
    assert (r["join"] != rp["join"]).any() and (r["gml"] != rp["gml"]).any()
    got = _lc(links, gamma, lam)
    _check_arrays(got, r, links)
    assert got["n_rechecked"] > 0 and got["rechecked"].sum() == got["n_rechecked"]


@pytest.mark.parametrize("name", ["mixed", "k2", "k75", "k2100", "hub"])
def test_python_arrays_equal_restatement(name):
    links, gamma, lam = {"mixed": lambda: M.mixed(8), "k2": lambda: M.random_model(5000, 2, 30000),
                         "k75": lambda: M.random_model(2000, 75, 20000), "k2100": lambda: M.random_model(3000, 2100, 20000),
                         "hub": lambda: M.hub_model()}[name]()
    _check_arrays(_lc(links, gamma, lam), R.link_communities(links, gamma, lam), links)


def test_mmsb_n200k_k512():
    from svinet_amd import mmsbgen_sparse
    pairs, (comm, w, beta) = mmsbgen_sparse.generate(200000, 512, 24, return_truth=True)
    n, K = 200000, 512
    rng = np.random.default_rng(7)
    gamma = np.full((n, K), 0.01) + rng.gamma(0.05, 0.1, size=(n, K))
    rows = np.repeat(np.arange(n), comm.shape[1])
    np.add.at(gamma, (rows, comm.reshape(-1)), 100.0 * w.reshape(-1))
    lam = np.stack([beta * 100 + 1e-3, (1 - beta) * 100 + 1e-3], axis=1)
    links = np.asarray(pairs, np.int64)
    got = _lc(links, gamma, lam)
    _check_arrays(got, R.link_communities(links, gamma, lam), links)
    assert got["timing_ms"]["link"] > 0


def test_two_runs_are_identical(graph_files, tmp_path):
    outs = []
    for run in ("a", "b"):
        d = tmp_path / run
        os.makedirs(str(d))
        with gzip.open(os.path.join(GOLDEN, "ref_lfr_k28", "gamma.txt.gz"), "rb") as f, open(str(d / "gamma.txt"), "wb") as g:
            g.write(f.read())
        shutil.copy(os.path.join(GOLDEN, "ref_lfr_k28", "lambda.txt"), str(d))
        _cli(["-file", graph_files["lfr"], "-n", 1000, "-k", 28, "-gml"], str(d))
        outs.append({f: open(str(d / "gml" / f), "rb").read() for f in FILES})
    assert outs[0] == outs[1]
    links, gamma, lam = M.near_threshold(64, 4000, seed=5)
    a, b = _lc(links, gamma, lam), _lc(links, gamma, lam)
    for key in ("deg_c", "colour", "join", "gml", "gml_edges", "bridgeness", "comm_argmax"):
        assert np.array_equal(a[key], b[key]), key
