"""-m gpu: product mode of the lane-per-link layout (K <= 32, option lpl_product; svinet_amd/csrc/svils_lpl.hip:
k_phi_lpl<.., PROD>, k_finalize_lpl<.., PROD>; the gate: svinet_amd/csrc/svils_api.hip: lpl_product_gate).

In product mode the finalise pass stores exp(Elogpi) rows instead of Elogpi and the phi pass multiplies them; the exp
form stays as it was.  Every test runs on the LFR fixture (n = 1000) against the oracle, both forms side by side where
the form matters.  Bar: gamma / lambda to 1e-9 relative; flags, link-branch counts, the likelihood rows' stop decision and
the member tags exactly.  Each test prints the errors it found before it asserts them."""
import importlib.util
import os

import numpy as np
import pytest

import matrix_cases as MC
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1000
RTOL = 1e-9
FORMS = (0, 1)

_cache = {}


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _net(graph_files):
    if "net" not in _cache:
        _cache["net"] = O.Network(graph_files["lfr"], N)
    return _cache["net"]


def _snap(ref):
    return dict(gamma=ref.gamma, lam=ref.lam, conv=ref.converged, counts=ref.link_counts(), iter=ref.iter,
                annealing=ref.annealing, rows=ref.rows[1:], member=ref.communities())


def _natural(graph_files, k, sweeps, **kw):
    """the oracle's run of `sweeps` sweeps from its own initialisation, computed once per (k, sweeps, options):
    -> (inputs, snapshot)"""
    key = (k, sweeps, tuple(sorted(kw.items())))
    if key not in _cache:
        net = _net(graph_files)
        ref = O.LinkSampling(net, k, use_validation_stop=False, **kw)
        inputs = dict(links=ref.links, validation=ref.validation_sorted, gamma0=ref.gamma, lam0=ref.lam, ones=net.ones,
                      ones_prob=ref.ones_prob, eta=ref.eta, test_sorted=ref.test_sorted if kw.get("test_pairs") is not None else None)
        for _ in range(sweeps):
            assert ref.sweep() == 0
        _cache[key] = (inputs, _snap(ref))
    return _cache[key]


def _engine(inputs, k, form, **kw):
    eng = MC.engine_on(inputs, N, k, options={"lpl_product": form}, **kw)
    assert eng.get_option("lpl_product") == form, (k, form)
    return eng


def _check(tag, eng, want, rows=True):
    g, lam, conv = eng.state()
    err = (_rel(g, want["gamma"]), _rel(lam, want["lam"]))
    print("%s: gamma rel err %.3e, lambda rel err %.3e" % (tag, err[0], err[1]))
    assert err[0] < RTOL and err[1] < RTOL, (tag, err)
    assert np.array_equal(conv, want["conv"]), tag
    c = eng.control()
    assert (c.links_dense, c.links_sparse, c.links_shortcut) == tuple(want["counts"]), tag
    assert (c.iter, bool(c.annealing)) == (want["iter"], want["annealing"]), tag       # the stop rule / annealing switch decided alike
    if rows:
        got = eng.rows()
        assert np.array_equal(got[:, 0], want["rows"][:, 0]), tag
        np.testing.assert_allclose(got[:, 1:], want["rows"][:, 1:], rtol=1e-8, atol=1e-12, err_msg=str(tag))
    assert np.array_equal(eng.communities(), want["member"]), tag


# K = 28 over 101 sweeps crosses the annealing switch and reaches the converged-node shortcuts; the others are one
# instantiation of every KC shape of K <= 32 (KC = 4, 10, 12, 16; 28 is KC = 14)
@pytest.mark.parametrize("k,sweeps", [(28, 101), (4, 12), (20, 12), (24, 12), (32, 12)])
def test_both_forms_against_oracle(graph_files, k, sweeps):
    inputs, want = _natural(graph_files, k, sweeps)
    if sweeps > 100:
        assert not want["annealing"] and want["counts"][2] > 0, want["counts"]
    for form in FORMS:
        eng = _engine(inputs, k, form)
        eng.sweep(sweeps)
        assert eng.get_option("lpl_product") == form
        _check(("K=%d" % k, "product=%d" % form), eng, want)
        eng.close()


def _planted(graph_files, k):
    """tools/make_config5_digest.py::planted_state on the LFR fixture: the memberships are the strongest community of
    every node after 40 oracle sweeps -> (inputs, state, snapshot after four sweeps from _iter = 999, counts per sweep)"""
    key = ("planted", k)
    if key in _cache:
        return _cache[key]
    spec = importlib.util.spec_from_file_location("make_config5_digest", os.path.join(ROOT, "tools", "make_config5_digest.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    inputs, warm = _natural(graph_files, k, 40)
    comm = np.argmax(warm["gamma"], 1).astype(np.int64)[:, None]
    pairs = np.asarray(inputs["links"], dtype=np.int64)
    state = tool.planted_state(pairs, (comm, np.ones((N, 1)), None), N, k)
    ref = O.LinkSampling(_net(graph_files), k, use_validation_stop=False)
    g, lam, conv = state
    ref.set_gamma(g); ref.set_lambda(lam); ref.set_converged(conv); ref.refresh()
    ref.annealing = False
    ref.iter = 999
    counts = []
    for _ in range(4):
        assert ref.sweep() == 0
        counts.append(ref.link_counts())
    _cache[key] = (inputs, state, _snap(ref), counts)
    return _cache[key]


def test_active_set_list_from_planted_state(graph_files):
    """four sweeps from the planted state at _iter = 999, annealing off (set_control): two dense ones with shortcuts,
    then two past _iter = 1000 whose class-1 list takes the product form over the union columns"""
    k = 20
    inputs, (g, lam, conv), want, counts = _planted(graph_files, k)
    assert counts[0][1] == 0 and counts[0][2] > 0 and counts[3][1] > 0 and counts[3][0] > 0, counts
    for form in FORMS:
        eng = _engine(inputs, k, form)
        eng.set_state(g, lam, conv)
        eng.set_control(iter=999, annealing=0)
        assert eng.get_option("lpl_product") == form       # the planted state is inside the bound
        eng.sweep(4)
        st = eng.sweep_stats(0, 4)
        assert [tuple(int(x) for x in r) for r in st] == counts
        _check(("planted", "product=%d" % form), eng, want, rows=False)
        eng.close()


def test_phase_split_sweeps(graph_files):
    """eight sweeps through svils_sweep_phase (the four-launch form, K-vectors through k_colreduce)"""
    k = 20
    inputs, want = _natural(graph_files, k, 8)
    eng = _engine(inputs, k, 1)
    MC.phase_split_sweeps(eng)(8)
    _check(("phases", "product=1"), eng, want)
    eng.close()


def test_full_window_unit_step_is_a_sweep(graph_files):
    """tests/test_gpu_stochastic.py's anchor on product-mode handles: a mini-batch step over all nodes with step size 1
    (k_finalize_lpl<.., STOCH, .., PROD>) is a full sweep"""
    k, steps = 20, 12
    inputs, want = _natural(graph_files, k, steps)
    a, b = _engine(inputs, k, 1), _engine(inputs, k, 1)
    b.set_stochastic(batch_nodes=0, tau0=1.0, kappa=0.0)
    a.sweep(steps)
    b.step(steps)
    ga, la, ca = a.state()
    gb, lb, cb = b.state()
    print("step vs sweep: gamma %.3e lambda %.3e" % (_rel(gb, ga), _rel(lb, la)))
    np.testing.assert_allclose(gb, ga, rtol=1e-9)
    np.testing.assert_allclose(lb, la, rtol=1e-9)
    assert np.array_equal(ca, cb) and np.array_equal(a.communities(), b.communities())
    np.testing.assert_allclose(b.rows(), a.rows(), rtol=1e-9, atol=1e-12)
    _check(("steps", "product=1"), b, want, rows=False)
    assert a.get_option("lpl_product") == 1 and b.get_option("lpl_product") == 1
    a.close()
    b.close()


def test_handle_with_a_test_set(graph_files):
    """-load-test: the handle keeps four launches and adds a test row per sweep"""
    k = 20
    net = _net(graph_files)
    tp = MC.test_pairs_of(O.LinkSampling(net, k, use_validation_stop=False).links)
    ref = O.LinkSampling(net, k, use_validation_stop=False, test_pairs=tp)
    inputs = dict(links=ref.links, validation=ref.validation_sorted, gamma0=ref.gamma, lam0=ref.lam, ones=net.ones,
                  ones_prob=ref.ones_prob, eta=ref.eta, test_sorted=ref.test_sorted)
    for _ in range(8):
        assert ref.sweep() == 0
    eng = _engine(inputs, k, 1)
    eng.sweep(8)
    _check(("testset", "product=1"), eng, _snap(ref))
    tr = eng.test_rows(0, ref.test_rows.shape[0])
    assert np.array_equal(tr[:, 0], ref.test_rows[:, 0])
    np.testing.assert_allclose(tr[:, 1:], ref.test_rows[:, 1:], rtol=1e-8, atol=1e-12)
    eng.close()


def test_elogpi_view(graph_files):
    """svils_get_aux(0) on a handle that stores no Elogpi rows (computed at the call) against the stored rows of an
    exp-mode handle after the same five sweeps"""
    k = 20
    inputs, want = _natural(graph_files, k, 5)
    views = []
    for form in FORMS:
        eng = _engine(inputs, k, form)
        eng.sweep(5)
        views.append(eng.aux(0))
        eng.close()
    err = _rel(views[1], views[0])
    print("Elogpi view, product against exp handle: rel err %.3e" % err)
    assert np.isfinite(views[1]).all() and (views[1] < 0).all()
    assert err < 1e-12


@pytest.mark.parametrize("kw,k,expect", [(dict(), 20, 1), (dict(), 32, 1), (dict(eta=(1e-3, 1.0)), 32, 0),
                                         (dict(link_thresh=0.3), 20, 0), (dict(), 33, 0)])
def test_host_gate(graph_files, kw, k, expect):
    """a forced 1 that fails a condition reads back 0: eta0 below the bound (3.5e-3 at K = 32 on this graph would still
    pass: 1 / eta0 = 1000 does not), link_thresh < 1/2, K above 32.  No kernel runs."""
    from svinet_amd._svils import Engine
    net = _net(graph_files)
    ref = O.LinkSampling(net, 20, use_validation_stop=False)
    eng = Engine(N, k, ones=net.ones, ones_prob=ref.ones_prob, use_validation_stop=False, options={"lpl_product": 1}, **kw)
    assert eng.get_option("lpl_product") == 1
    eng.set_graph(ref.links)
    assert eng.get_option("lpl_product") == expect, (kw, k)
    auto = Engine(N, k, ones=net.ones, ones_prob=ref.ones_prob, use_validation_stop=False, **kw)
    assert auto.get_option("lpl_product") == -1
    auto.set_graph(ref.links)
    assert auto.get_option("lpl_product") in (0, expect)      # auto never goes where a forced 1 may not
    eng.close()
    auto.close()


def test_state_outside_the_bound_takes_the_exp_kernels(graph_files):
    """a state that arrives with gamma entries far below alpha (psi = -2000: the product of two such factors is beyond
    the gate's 1e-250) turns the mode off for the handle; the sweep that follows matches the oracle"""
    k = 20
    inputs, _ = _natural(graph_files, k, 5)
    ref = O.LinkSampling(_net(graph_files), k, use_validation_stop=False)
    g = np.full((N, k), 5e-4)
    g[np.arange(N), np.arange(N) % k] = 50.0
    lam = np.tile([3.0, 2.0], (k, 1))
    ref.set_gamma(g); ref.set_lambda(lam); ref.refresh()
    eng = _engine(inputs, k, 1)
    eng.set_state(g, lam)
    assert eng.get_option("lpl_product") == 0
    ref.sweep()
    eng.sweep(1)
    gg, ll, conv = eng.state()
    assert np.isfinite(gg).all() and np.isfinite(ll).all()
    np.testing.assert_allclose(gg, ref.gamma, rtol=1e-7)
    np.testing.assert_allclose(ll, ref.lam, rtol=1e-7)
    assert np.array_equal(conv, ref.converged)
    eng.close()


def test_two_product_runs_are_bit_identical(graph_files):
    k = 20
    inputs, _ = _natural(graph_files, k, 5)
    outs = []
    for _ in range(2):
        eng = _engine(inputs, k, 1)
        eng.sweep(20)
        outs.append(eng.state() + (eng.rows(), eng.communities(), eng.aux(2)))
        eng.close()
    for x, y in zip(*outs):
        assert np.array_equal(x, y)
