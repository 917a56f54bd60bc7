"""-m gpu: svils_batch_elbo, the variational lower bound of -logl on the device (k_batch_elbo<W,V>, k_batch_elbo_nodes,
k_batch_elbo_reduce in csrc/svils_batch.hip).

The reference is the numpy restatement of tests/elbo_cases.py; total, G, P and N are each held at rtol 1e-9 (the bound the
project holds its likelihood rows to on the HIP path), the round total exactly -- every state passes
assert_exits_are_clear, so no exit test is within 1e-4 of the threshold and a last-bit difference cannot move an exit.
Every state also passes check_conditions: exits at >= 3 distinct rounds (n = 3 has too few pairs for that), every pair
and node term < 0 (G, P and N cannot cancel), every phi > 0 except in the states built for exact zeros."""
import os
import subprocess

import numpy as np
import pytest

import batch_cases as BC
import elbo_cases as EC
from svinet_amd import _svils, host_api
from svinet_amd.host_api import BatchEngine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
ERR_ARG, ERR_UNSUPPORTED = -1, -4
KS = [2, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256]


def _device(n, k, links, skip, gamma=None, lam=None):
    d = _svils.Batch(n, k, 1.0 / k, (1.0, 1.0))
    d.set_graph(links, sorted(skip))
    if gamma is not None:
        d.set_state(gamma, lam)
    return d


def _restated(n, k, kind, gamma=None, lam=None):
    links, skip, adj, g0, l0 = EC.case(n, k, kind)
    gamma, lam = (g0, l0) if gamma is None else (gamma, lam)
    e = EC.Elbo(gamma, lam, adj, skip, 1.0 / k, (1.0, 1.0))
    return links, skip, adj, gamma, lam, e


def _check_case(n, k, kind):
    links, skip, adj, gamma, lam, e = _restated(n, k, kind)
    EC.check_conditions(e, exact_zeros=kind == "zeros", min_exit_rounds=1 if n == 3 else 3)
    e.assert_exits_are_clear()
    d = _device(n, k, links, skip, gamma, lam)
    parts, pairs_done, rounds_total = d.elbo()
    print("n %d k %d %s: device %r restated %r rel %r" % (n, k, kind, parts, e.parts, np.abs(parts / e.parts - 1)))
    EC.assert_parts(parts, e)
    assert abs(parts[0] - (parts[1] + parts[2] + parts[3])) <= 1e-12 * abs(parts[0])
    assert pairs_done == len(e.rounds) == n * (n - 1) // 2 - len(skip)
    assert rounds_total == e.rounds_total
    assert d.stats() == (0, 0, 0, 0)          # the sweep's counters are not the pass's
    assert d.timing()[0] > 0 and d.timing()[1] == d.timing()[2] == -1
    d.close()


@pytest.mark.parametrize("kind", ["plain", "peaked"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", [3, 37, 96])
def test_every_instantiation_at_the_tile_edges(n, k, kind):
    """every (W, V) at both ends of its k range; n = 3: one pair tile; 37: a partial tile; 96: tiles on both sides of
    column 64, skipped pairs at rows and columns 63 / 64, a node without links, a node whose pairs are all skipped"""
    _check_case(n, k, kind)


@pytest.mark.parametrize("n,k", [(37, 4), (37, 9), (37, 33), (37, 129), (96, 9), (96, 65)])
def test_phi_entries_that_are_exactly_zero(n, k):
    """gamma entries of 1e-3 beside entries of 50: some phi underflow to exactly 0, every normaliser stays > 0; such an
    entry adds 0 (the reference's log(phi) * phi is NaN there) -- finite, and equal to the restatement"""
    _check_case(n, k, "zeros")


@pytest.mark.parametrize("k", [9, 129])
def test_launch_cuts_do_not_change_a_bit(k):
    """n = 96: 3 tiles at k = 9 (64 rows each), 10 at k = 129 (16 rows each). One, two and (the default) all tiles per launch: the same bits"""
    links, skip, adj, gamma, lam, e = _restated(96, k, "peaked")
    d = _device(96, k, links, skip, gamma, lam)
    out = []
    for tiles in (1, 2, 0):
        d.set_elbo_tiles(tiles)
        parts, pairs_done, rounds_total = d.elbo()
        out.append((parts.tobytes(), pairs_done, rounds_total))
    assert out[0] == out[1] == out[2]
    EC.assert_parts(np.frombuffer(out[0][0]), e)
    d.close()


def test_two_handles_give_the_same_bits():
    links, skip, adj, gamma, lam, e = _restated(96, 17, "plain")
    a, b = _device(96, 17, links, skip, gamma, lam), _device(96, 17, links, skip, gamma, lam)
    pa, pb = a.elbo(), b.elbo()
    assert pa[0].tobytes() == pb[0].tobytes() and pa[1:] == pb[1:]
    assert a.elbo()[0].tobytes() == pa[0].tobytes()
    a.close()
    b.close()


def test_the_pass_has_no_side_effects():
    """sweep, elbo, sweep = sweep, sweep bit for bit; the expectations and the sweep's counters are as before the call"""
    links, skip, adj, gamma, lam, _ = _restated(96, 9, "plain")
    a, b = _device(96, 9, links, skip, gamma, lam), _device(96, 9, links, skip, gamma, lam)
    a.sweep()
    b.sweep()
    stats, (ep, eb), (g1, l1) = a.stats(), a.expectations(), a.state()
    parts = a.elbo()[0]
    assert a.stats() == stats
    ep2, eb2 = a.expectations()
    assert ep2.tobytes() == ep.tobytes() and eb2.tobytes() == eb.tobytes()
    g2, l2 = a.state()
    assert g2.tobytes() == g1.tobytes() and l2.tobytes() == l1.tobytes()
    EC.assert_parts(parts, EC.Elbo(g1, l1, adj, skip, 1.0 / 9, (1.0, 1.0)))
    a.sweep()
    b.sweep()
    (ga, la), (gb, lb) = a.state(), b.state()
    assert ga.tobytes() == gb.tobytes() and la.tobytes() == lb.tobytes()
    assert a.stats() == b.stats()
    a.close()
    b.close()


def test_the_value_after_steps_is_that_of_the_state_read_back():
    """svils_batch_step_node / _pairs / _star keep Elogpi row by row: the pass after them reads what they left"""
    n, k = 37, 9
    links, skip, adj, gamma, lam, _ = _restated(n, k, "plain")
    d = _device(n, k, links, skip, gamma, lam)

    def check():
        g, l = d.state()
        e = EC.Elbo(g, l, adj, skip, 1.0 / k, (1.0, 1.0))
        parts, pairs_done, _ = d.elbo()
        EC.assert_parts(parts, e)
        assert pairs_done == len(e.rounds)
        g2, l2 = d.state()
        assert g2.tobytes() == g.tobytes() and l2.tobytes() == l.tobytes()

    d.step_node([3, 20], n / 2.0, [0.3, 0.25], [0.2, -1.0])
    check()
    trained = [(int(a), int(b)) for a, b in zip(*EC.trained_pairs(n, skip))]
    d.step_pairs([trained[5:25], trained[100:110]], [30.0, 60.0], [0.3, 0.2], [0.1, 0.1])
    check()
    partners = [j for j in range(n) if j != 2 and (min(2, j), max(2, j)) not in skip][:12]
    d.step_star([dict(start=2, partner=partners, y=[adj[2, j] for j in partners], rho_partner=[0.2] * len(partners), rho_start=0.3,
                      scale=n / 2.0, rho_lambda=0.1)])
    check()
    d.sweep()
    check()
    d.close()


def test_errors():
    n, k = 37, 4
    links, skip, adj, gamma, lam, _ = _restated(n, k, "peaked")
    L = _svils.load()
    d = _device(n, k, links, skip)
    parts = np.zeros(4)
    assert L.svils_batch_elbo(d._h, parts.ctypes.data, None, None) == ERR_ARG and b"state" in L.svils_last_error()   # no state
    d.set_state(gamma, lam)
    assert L.svils_batch_elbo(d._h, None, None, None) == ERR_ARG and b"null" in L.svils_last_error()
    assert L.svils_batch_set_elbo_tiles(d._h, 2049) == ERR_ARG and b"2048" in L.svils_last_error()
    assert L.svils_batch_set_elbo_tiles(d._h, 2048) == 0 and L.svils_batch_set_elbo_tiles(d._h, 0) == 0
    assert L.svils_batch_elbo(d._h, parts.ctypes.data, None, None) == 0 and np.all(parts < 0)      # null counters are fine
    nograph = _svils.Batch(n, k, 1.0 / k, (1.0, 1.0))
    nograph.set_state(gamma, lam)
    assert L.svils_batch_elbo(nograph._h, parts.ctypes.data, None, None) == ERR_ARG and b"graph" in L.svils_last_error()
    nograph.close()
    # a node whose Elogpi is below log(DBL_MIN) everywhere: the normaliser of its pairs is 0 -- the sweep's answer
    bad = gamma.copy()
    bad[2] = 5e-4
    with pytest.raises(AssertionError):
        EC.Elbo(bad, lam, adj, skip, 1.0 / k, (1.0, 1.0))
    d.set_state(bad, lam)
    kept = parts.copy()
    assert L.svils_batch_elbo(d._h, parts.ctypes.data, None, None) == ERR_UNSUPPORTED
    assert b"phi normaliser underflow" in L.svils_last_error() and np.array_equal(parts, kept)
    g, _ = d.state()                       # the pass's underflow count is its own: the state is still served
    assert np.array_equal(g, bad)
    d.close()


def test_engine_on_the_device_matches_the_restatement(graph_files):
    e = BatchEngine(graph_files["assort"], 75, 4, heldout_ratio=0.1, on_device=True, logl=True)
    for _ in range(2):
        e.sweep()
        e.report()
    skip = {tuple(int(x) for x in r) for r in e.heldout} | {tuple(int(x) for x in r) for r in e.validation}
    r = EC.Elbo(e.gamma, e.lam, BC.adjacency(e.n, e.edges), skip, 0.25, e.eta)
    EC.check_conditions(r)
    EC.assert_parts(e.elbo(), r)
    assert e.logl_rows.shape == (3, 2) and e.logl_rows[-1, 1] == e.elbo()[0]
    e.close()


def _cli(args, tmp, cwd=None):
    return subprocess.run([SVINET] + args + ["-outdir", str(tmp)], capture_output=True, text=True, timeout=600, cwd=cwd)


def _rows(path):
    return [line.split("\t") for line in open(path).read().splitlines()]


@pytest.mark.parametrize("device,host,run,name", [
    (["-batch-gpu"], ["-batch"], ["-max-iterations", "1"], "batch"),
    (["-rnode"], ["-rnode", "-host-loops"], ["-rfreq", "2", "-max-iterations", "3"], "Urnode"),
    (["-infset"], ["-infset", "-host-loops"], ["-rfreq", "2", "-max-iterations", "3"], "infset"),
])
def test_cli_rows_on_the_device_equal_the_host_loops(graph_files, tmp_path, device, host, run, name):
    """LFR n = 1000, k = 28, three rows per run: equal at %.5f, or within 1e-9 relative where the last digit differs"""
    work = tmp_path / "work"
    work.mkdir()
    if name == "infset":
        host_api.preprocess(graph_files["lfr"], 1000, str(work / "neighbors.bin"))
    rows = {}
    for tag, flags in (("dev", device), ("host", host)):
        out = tmp_path / tag
        out.mkdir()
        r = _cli(["-file", graph_files["lfr"], "-n", "1000", "-k", "28", "-logl", "-no-stop"] + run + flags, out, cwd=str(work))
        assert r.returncode == 0, r.stderr
        rows[tag] = _rows(out / ("n1000-k28-mmsb-" + name) / "logl.txt")
        assert r.stdout.count("approx. log likelihood = ") == 3
    assert len(rows["dev"]) == len(rows["host"]) == 3
    for a, b in zip(rows["dev"], rows["host"]):
        print(a, b)
        assert a[0] == b[0] and len(a) == len(b) == 3
        assert a[2] == b[2] or abs(float(a[2]) - float(b[2])) <= 1e-9 * abs(float(b[2])), (a, b)
