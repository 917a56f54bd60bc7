"""-m gpu: deferred exp(Elogpi) rows of product-mode three-launch sweeps (option lpl_defer_epi;
svinet_amd/csrc/svils_lpl.hip: k_finalize_lpl<.., PROD = 2>, lpl_epi_rows_role in k_s3_lpl<.., DEFER>).

With the option on, the finalise pass stops after the flags and the s3 launch forms the rows from the stored gamma rows,
chunk by chunk off a queue, in whichever of its blocks has nothing else left to do.  The rows come from the same doubles
by the same operations in the same order, so EVERY comparison here is np.array_equal between a handle with the option
off (the rows formed by the finalise pass) and one with it on: gamma, lambda, the exp(Elogpi) buffer (svils_get_aux 6),
the converged flags, the likelihood rows, the member tags.  No tolerance anywhere except where the Elogpi VIEW
(svils_get_aux 0, computed from gamma by another kernel) is set against the rows.

Inputs: the LFR fixture (n = 1000) and ca-AstroPh (n = 17 903 = 8 * 2237 + 7: the last chunk of the queue is partial)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LFR, N_ASTRO = 1000, 17903
_setups = {}


def _setup(graph_files, which, k):
    from svinet_amd.host_api import Setup
    key = (which, k)
    if key not in _setups:
        _setups[key] = Setup(graph_files[which], N_LFR if which == "lfr" else N_ASTRO, k)
    return _setups[key]


def _engine(setup, defer, expect=None, **kw):
    opts = {"lpl_product": 1, "lpl_defer_epi": defer}
    opts.update(kw.pop("options", {}))
    kw.setdefault("use_validation_stop", False)
    eng = setup.engine(options=opts, **kw)
    assert eng.get_option("lpl_defer_epi") == (defer if expect is None else expect), (opts, kw)
    return eng


def _outputs(eng):
    """everything a sweep leaves behind that the rows could show in"""
    g, lam, conv = eng.state()
    return dict(gamma=g, lam=lam, conv=conv, epi=eng.aux(6), rows=eng.rows(), member=eng.communities())


def _same(tag, a, b):
    for key in a:
        same = np.array_equal(a[key], b[key])
        diff = 0.0 if same or a[key].shape != b[key].shape else float(np.max(np.abs(a[key].astype(np.float64) - b[key].astype(np.float64))))
        print("%s: %s %s (max abs difference %.3e)" % (tag, key, "equal" if same else "DIFFERS", diff))
    for key in a:
        assert np.array_equal(a[key], b[key]), (tag, key)


# K = 4 .. 32: NC = 1 .. 4 communities per lane of the finalise layout; K = 4, 20, 28 leave a slot idle (psi(row sum) rides in
# it), K = 8, 16, 24, 32 fill the row (psi(row sum) is a call of its own); KC = 4 .. 16, the 1024-thread (K <= 20) and
# 512-thread (K > 20) s3 shapes, both finalise shapes (576 and 512 threads).  K = 28 for 101 sweeps crosses the annealing
# switch and reaches the shortcut links.
@pytest.mark.parametrize("k,sweeps", [(4, 12), (8, 12), (16, 12), (20, 12), (24, 12), (28, 12), (32, 12), (28, 101)])
def test_both_forms_same_bits(graph_files, k, sweeps):
    setup = _setup(graph_files, "lfr", k)
    outs = []
    for defer in (0, 1):
        eng = _engine(setup, defer)
        assert eng.get_option("lpl_product") == 1
        eng.sweep(sweeps)
        outs.append(_outputs(eng))
        c = eng.control()
        assert c.sweeps_done == sweeps
        if sweeps > 100:
            assert not c.annealing and c.links_shortcut > 0, (c.annealing, c.links_shortcut)
        eng.close()
    assert (outs[0]["epi"] > 0).all() and (outs[0]["epi"] <= 1).all()
    _same("K=%d, %d sweeps" % (k, sweeps), outs[0], outs[1])


@pytest.mark.parametrize("replay", [True, False])
def test_no_chunk_skipped_sweep_by_sweep(graph_files, replay):
    """ca-AstroPh at K = 20, six sweeps taken one at a time: after each the rows are those of the other form.  A chunk nobody
    took would still hold the rows of the sweep before, which differ from this sweep's by many orders above rounding (checked:
    the buffer changes from sweep to sweep in every chunk of 8 nodes)."""
    k = 20
    setup = _setup(graph_files, "astroph", k)
    opts = {} if replay else {"graph_after": 1 << 30}
    engs = [_engine(setup, defer, options=dict(opts)) for defer in (0, 1)]
    if replay:
        for eng in engs:
            eng.prepare_graphs(8)      # the graphs of 1 and 8 sweeps exist: single sweeps replay the first
    prev = engs[0].aux(6)
    for sweep in range(1, 7):
        for eng in engs:
            eng.sweep(1)
        a, b = engs[0].aux(6), engs[1].aux(6)
        pad = (-N_ASTRO) % 8
        moved = np.abs(np.pad(a - prev, ((0, pad), (0, 0)))).reshape(-1, 8 * k).max(axis=1)
        print("sweep %d (%s): smallest change of a chunk %.3e, rows equal: %s" % (sweep, "replay" if replay else "eager", moved.min(), np.array_equal(a, b)))
        assert moved.min() > 1e-9              # the comparison below would see a stale chunk
        assert np.array_equal(a, b), sweep
        assert np.array_equal(a[-7:], b[-7:])  # the partial last chunk (n mod 8 = 7)
        prev = a
    _same("ca-AstroPh K=20 after six single sweeps", _outputs(engs[0]), _outputs(engs[1]))
    for eng in engs:
        eng.close()


def test_run_to_its_stop(graph_files):
    """LFR K = 28 with the validation stop on: the same stop sweep, the same state and rows at the stop (both launches of
    the sweeps behind it return at once: the rows stay those of the last completed sweep), and the Elogpi view agrees with
    the rows.  The view is psi(gamma_k) - psi(row sum) from another kernel's digamma (2e-15 relative each, svils_devutil.h):
    where a community dominates, the two psi are O(ln row sum) < 10 and their difference is off by < 1e-13 absolute; where
    gamma_k is tiny, psi(gamma_k) = -1 / gamma_k is the difference itself, off by 4e-15 relative.  Bar: 1e-12 of both."""
    setup = _setup(graph_files, "lfr", 28)
    outs, stops = [], []
    for defer in (0, 1):
        eng = _engine(setup, defer, use_validation_stop=True)
        eng.sweep(400)
        c = eng.control()
        assert c.stopped == 1 and c.sweeps_done < 395, (c.stopped, c.sweeps_done)
        stops.append((c.sweeps_done, c.iter, c.why if hasattr(c, "why") else 0))
        outs.append(_outputs(eng))
        view = eng.aux(0)
        epi = outs[-1]["epi"]
        assert (epi > 0).all()
        err = np.abs(np.log(epi) - view) / np.maximum(np.abs(view), 1.0)
        print("defer=%d: stopped after %d sweeps; log(rows) against the Elogpi view: %.3e" % (defer, c.sweeps_done, err.max()))
        assert err.max() < 1e-12
        eng.close()
    assert stops[0] == stops[1], stops
    _same("LFR K=28 at the stop", outs[0], outs[1])


def test_decision_reads_back(graph_files):
    """1 on the headline shape (ca-AstroPh, K = 20), forced and by default; 0 -- and the bits of the other form -- where a
    condition fails: three-launch sweeps forced off, product mode off, a handle with a test set"""
    head = _setup(graph_files, "astroph", 20)
    for opts in ({"lpl_defer_epi": 1}, {}):
        eng = head.engine(use_validation_stop=False, options=opts)
        assert eng.get_option("lpl_product") == 1 and eng.get_option("lpl_defer_epi") == 1, opts
        eng.close()
    setup = _setup(graph_files, "lfr", 20)

    def run(eng, product=True):
        eng.sweep(8)
        g, lam, conv = eng.state()
        out = dict(gamma=g, lam=lam, conv=conv, rows=eng.rows(), member=eng.communities())
        if product:
            out["epi"] = eng.aux(6)
        eng.close()
        return out

    for tag, opts in (("fused3=0", {"fused3": 0}), ("lpl_product=0", {"lpl_product": 0})):
        a = _engine(setup, 0, options=dict(opts))
        b = _engine(setup, 1, expect=0, options=dict(opts))     # a forced 1 that fails a condition falls back to 0
        _same(tag, run(a, "lpl_product" not in opts), run(b, "lpl_product" not in opts))
    tp = np.concatenate([setup.links[7::997], [[3, 900], [999, 4]]]).astype(np.uint32)
    tp = np.column_stack([tp, np.array([1] * (tp.shape[0] - 2) + [0, 0], dtype=np.uint32)])
    outs = []
    for defer in (0, 1):
        eng = _engine(setup, defer)
        eng.set_test(tp)
        assert eng.get_option("lpl_defer_epi") == 0
        outs.append(run(eng))
    _same("test set", outs[0], outs[1])
    eng = _engine(setup, 1)
    eng.set_test(tp)
    eng.set_test(tp[:0])                        # the test set goes: the form comes back
    assert eng.get_option("lpl_defer_epi") == 1
    eng.close()


def test_small_device_keeps_the_rows_in_the_finalise_pass(graph_files, tmp_path):
    """the TESTING build pretends a device of 16 CUs (option assume_cus): the handle keeps four launches, hence the rows where
    they were; a forced 1 reads back 0 and the bits are those of a forced 0"""
    lib = os.path.join(ROOT, "svinet_amd", "lib", "libsvils_testing.so")
    if not os.path.exists(lib):
        from svinet_amd import build
        build.build_testing()
    out = str(tmp_path / "small.npz")
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r)\n"
        "from svinet_amd.host_api import Setup\n"
        "s = Setup(%r, 1000, 20)\n"
        "res = {}\n"
        "for defer in (0, 1):\n"
        "    e = s.engine(use_validation_stop=False, options={'lpl_product': 1, 'lpl_defer_epi': defer})\n"
        "    res['opt%%d' %% defer] = e.get_option('lpl_defer_epi')\n"
        "    e.sweep(8)\n"
        "    g, lam, conv = e.state()\n"
        "    res.update({'g%%d' %% defer: g, 'lam%%d' %% defer: lam, 'conv%%d' %% defer: conv, 'epi%%d' %% defer: e.aux(6), 'rows%%d' %% defer: e.rows()})\n"
        "    e.close()\n"
        "np.savez(%r, **res)\n"
    ) % (ROOT, graph_files["lfr"], out)
    env = dict(os.environ, SVILS_ASSUME_CUS="16", SVILS_LIB=lib)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert int(z["opt0"]) == 0 and int(z["opt1"]) == 0
    for key in ("g", "lam", "conv", "epi", "rows"):
        assert np.array_equal(z[key + "0"], z[key + "1"]), key


def test_two_deferred_runs_are_bit_identical(graph_files):
    """which wavefront takes which chunk differs from run to run; no output may show it"""
    setup = _setup(graph_files, "astroph", 20)
    outs = []
    for _ in range(2):
        eng = _engine(setup, 1)
        eng.sweep(20)
        outs.append(_outputs(eng))
        eng.close()
    _same("two deferred runs", outs[0], outs[1])
