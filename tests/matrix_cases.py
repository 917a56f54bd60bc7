"""Helpers the two kernel matrices share (test infrastructure): test_gpu_small_k_matrix.py (lane-per-link kernels) and
test_gpu_rpw_matrix.py (row-per-wavefront kernels).  A case is two phases, each compared with the oracle in full:

  (a) `nat` natural sweeps from the reference initialisation (annealing, every link on the full softmax);
  (b) `reg` sweeps from a seeded state (seed_state) -- one at the natural _iter, whose prune() derives the active sets,
      then the others at _iter = 1500 with annealing off: converged-node shortcuts, the active-set branch and the full
      softmax side by side.

trajectory() runs the oracle through both and keeps what compare() needs; two_phases() drives handles through the same
steps.  The drivers of the modes (sweeps split at their exchange points, node blocks on one GPU) are here too."""
import numpy as np

from oracle import oracle as O


def seed_state(n, k, lam):
    """The state phase (b) starts from.  Nineteen nodes in twenty are concentrated on community 0 and dominate: a
    link with one of them puts all of its phi there (their rows are the smallest off their own community).  Pairs of ring neighbours
    (nodes 20 i + 5, 20 i + 6) share one of the other communities, so that every community keeps mass.  After one sweep
    without the annealing scale the majority nodes have one active community (prune() marks them converged), the others a
    few: links between two majority nodes take the active-set branch, links with one converged end the shortcuts, and
    links among the rest the full softmax.  A quarter of the nodes carries its community as converged flag from the
    start (community K among them: quirk Q2)."""
    rng = np.random.default_rng(4000 + k)
    home = np.zeros(n, dtype=np.int64)
    minor = np.zeros(n, dtype=bool)
    if k > 1:
        first = np.arange(5, n - 1, 20)
        home[first] = home[first + 1] = 1 + np.arange(first.size) % (k - 1)
        minor[first] = minor[first + 1] = True
    g = np.where(minor[:, None], 0.02, 0.005) * np.ones((n, k))
    g[np.arange(n), home] = rng.uniform(20.0, 60.0, size=n)
    conv = np.zeros(n, dtype=np.uint32)
    idx = rng.choice(n, size=n // 4, replace=False)
    conv[idx] = home[idx] + 1
    return g, np.array(lam), conv


def snapshot(ref, counts, test=False):
    return dict(gamma=ref.gamma, lam=ref.lam, conv=ref.converged, counts=list(counts), rows=ref.rows[1:],
                member=ref.communities(), mphi=ref.mphi, iter=ref.iter, annealing=ref.annealing,
                test_rows=ref.test_rows if test else None)


def test_pairs_of(ref_links):
    """a test set: some training links, two non-links (one unordered)"""
    return np.concatenate([ref_links[7::997], [[3, 900], [999, 4]]]).astype(np.uint32)


test_pairs_of.__test__ = False


def trajectory(n, pairs, k, nat, reg, test=False, seed=None, **ref_kw):
    """the oracle's trajectory of one (graph, K): its inputs, the seeded state and a snapshot after each phase; the link
    counts of every sweep are in the snapshots (dense, active-set, shortcut).  seed(n, k, lam) -> (gamma, lambda, flags):
    the state phase (b) starts from (seed_state when None); "b1" is the snapshot after the first sweep from it, "row0" the
    constructor's likelihood row."""
    net = O.Network(n=n, pairs=pairs)
    tp = None
    if test:
        tp = test_pairs_of(O.LinkSampling(net, k, use_validation_stop=False, **ref_kw).links)
    ref = O.LinkSampling(net, k, use_validation_stop=False, test_pairs=tp, **ref_kw)
    rec = dict(links=ref.links, validation=ref.validation_sorted, gamma0=ref.gamma, lam0=ref.lam, ones=net.ones,
               ones_prob=ref.ones_prob, eta=ref.eta, test_sorted=ref.test_sorted if test else None, row0=ref.rows[0])
    counts = []

    def sweeps(m):
        for _ in range(m):
            assert ref.sweep() == 0
            counts.append(ref.link_counts())

    sweeps(nat)
    rec["a"] = snapshot(ref, counts, test)
    rec["seed"] = g, lam, conv = (seed or seed_state)(n, k, ref.lam)
    ref.set_gamma(g); ref.set_lambda(lam); ref.set_converged(conv); ref.refresh()
    ref.annealing = False
    sweeps(1)
    rec["b1"] = snapshot(ref, counts, test)
    ref.iter = 1500
    sweeps(reg - 1)
    rec["b"] = snapshot(ref, counts, test)
    assert np.isfinite(rec["b"]["gamma"]).all() and (rec["b"]["gamma"] > 0).all()
    return rec


def engine_on(rec, n, k, **kw):
    """a handle on the oracle's inputs (its links, held-out pairs and initial state)"""
    from svinet_amd._svils import Engine
    eng = Engine(n, k, ones=rec["ones"], ones_prob=rec["ones_prob"], eta=rec["eta"], use_validation_stop=False, **kw)
    eng.set_graph(rec["links"])
    eng.set_validation(rec["validation"])
    eng.set_state(rec["gamma0"], rec["lam0"])
    if rec["test_sorted"] is not None:
        eng.set_test(rec["test_sorted"])
    return eng


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def compare(tag, want, eng, tol, lo=0, hi=None, counts=True):
    """the state of `eng` against an oracle snapshot; [lo, hi): the rows the handle owns (tags, stored indicators).
    -> the relative errors it found (gamma, lambda, likelihood rows, stored indicators over max(|m|, 1e-9))"""
    g, lam, conv = eng.state()
    rows = eng.rows()
    mphi = eng.aux(2)[lo:hi]
    wm = want["mphi"][lo:hi]
    err = (rel(g, want["gamma"]), rel(lam, want["lam"]))
    assert err[0] < tol["state"] and err[1] < tol["state"], (tag, err)
    assert np.array_equal(conv, want["conv"]), tag
    assert eng.control().iter == want["iter"], tag
    if counts:
        st = eng.sweep_stats(0, len(want["counts"]))
        assert [tuple(int(x) for x in r) for r in st] == want["counts"], tag
    assert np.array_equal(rows[:, 0], want["rows"][:, 0]), tag
    np.testing.assert_allclose(rows[:, 1:], want["rows"][:, 1:], rtol=tol["rows_rtol"], atol=tol["rows_atol"], err_msg=str(tag))
    assert np.array_equal(eng.communities()[lo:hi], want["member"][lo:hi]), tag
    np.testing.assert_allclose(mphi, wm, rtol=tol["mphi_rtol"], atol=tol["mphi_atol"], err_msg=str(tag))
    if want["test_rows"] is not None:
        tr = eng.test_rows(0, want["test_rows"].shape[0])
        assert np.array_equal(tr[:, 0], want["test_rows"][:, 0]), tag
        np.testing.assert_allclose(tr[:, 1:], want["test_rows"][:, 1:], rtol=tol["rows_rtol"], atol=tol["rows_atol"], err_msg=str(tag))
    wr = want["rows"][:, 1:]
    err_rows = float(np.max(np.abs(rows[:, 1:] - wr) / np.maximum(np.abs(wr), 1e-300))) if rows.size else 0.0
    err_m = float(np.max(np.abs(mphi - wm) / np.maximum(np.abs(wm), 1e-9))) if wm.size else 0.0
    return dict(gamma=err[0], lam=err[1], rows=err_rows, mphi=err_m)


def two_phases(rec, engines, sweep, check, reg, seed=None):
    """phases (a) and (b) on `engines` (every handle of a run), `sweep(m)` running m sweeps on all of them;
    seed(engine, gamma, lambda, flags) puts the seeded state on a handle (set_state when None: a handle of all columns)"""
    sweep(len(rec["a"]["counts"]))
    check("a", rec["a"])
    g, lam, conv = rec["seed"]
    for e in engines:
        if seed is None:
            e.set_state(g, lam, conv)
        else:
            seed(e, g, lam, conv)
        e.set_control(annealing=0)
    sweep(1)
    for e in engines:
        e.set_control(iter=1500)
    sweep(reg - 1)
    check("b", rec["b"])


# --------------------------------------------------------------------------------------------------------- the modes
def phase_split_sweeps(eng):
    """-> sweep(m): sweeps split at their exchange points (svils_sweep_phase)"""
    from svinet_amd import _svils

    def sweep(m):
        for _ in range(m):
            for ph in (_svils.PHASE_A, _svils.PHASE_B, _svils.PHASE_EXPAND, _svils.PHASE_C, _svils.PHASE_D):
                eng.sweep_phase(ph)
    return sweep


def exchange_sum(ts):
    tot = ts[0].clone()
    for t in ts[1:]:
        tot += t
    for t in ts:
        t.copy_(tot)


def node_blocks(setup, bounds, **engine_kw):
    """one handle per node block of `bounds`, all on GPU 0 -> (shards, sync)"""
    import torch
    from svinet_amd.sharded import HipShard
    world = len(bounds) - 1
    shards = [HipShard(setup, r, world, 0, bounds=bounds, use_validation_stop=False, **engine_kw) for r in range(world)]
    assert list(shards[0].bounds.astype(np.int64)) == list(bounds)

    def sync():
        for s in shards:
            s.engine.synchronize()
        torch.cuda.synchronize()
    return shards, sync


def staged_block_sweeps(shards, sync):
    """-> sweep(m): node-block sweeps with the two exchanges done in process (tests/test_gpu_sharded.py): the light
    finalise pass, the staged rows copied to every rank, k_expand_all"""
    from svinet_amd import _svils
    world, bm = len(shards), shards[0].bmax

    def sweep(m):
        for _ in range(m):
            for s in shards:
                s.phase(_svils.PHASE_A)
                s.phase(_svils.PHASE_B_LIGHT)
            sync()
            exchange_sum([s.kvec_a for s in shards])
            for dst in range(world):
                for src in range(world):
                    if src != dst:
                        shards[dst].gstage[src * bm:(src + 1) * bm].copy_(shards[src].gstage[src * bm:(src + 1) * bm])
            sync()
            for s in shards:
                s.phase(_svils.PHASE_EXPAND_ALL)
                s.phase(_svils.PHASE_C)
            sync()
            exchange_sum([s.kvec_c for s in shards])
            sync()
            for s in shards:
                s.phase(_svils.PHASE_D)
        sync()
    return sweep


def compare_blocks(tag, want, shards, tol):
    """every rank against the snapshot: a rank tags and stores indicators for its own rows and counts the links of its
    own rows (each link with the rank that owns its first end) -- the ranks' counts add up to the oracle's"""
    bounds = shards[0].bounds.astype(np.int64)
    states = [s.engine.state() for s in shards]
    errs = [compare(tag + ("block%d" % r,), want, s.engine, tol, lo=int(bounds[r]), hi=int(bounds[r + 1]), counts=False)
            for r, s in enumerate(shards)]
    nsw = len(want["counts"])
    tot = sum(s.engine.sweep_stats(0, nsw).astype(np.int64) for s in shards)
    assert [tuple(int(x) for x in row) for row in tot] == want["counts"], tag
    for g, lam, conv in states[1:]:
        assert np.array_equal(g, states[0][0]) and np.array_equal(lam, states[0][1])
    return {key: max(e[key] for e in errs) for key in errs[0]}


# ------------------------------------------------------------------------------------------------- column slices
def compare_slices(tag, want, shards, tol, skip=0):
    """K-sharded ranks (svinet_amd/ksharded.py: every rank the columns [k0, k1) of all rows) against a snapshot: gamma,
    lambda and the communities put together from the slices, the stored mean indicators slice by slice; flags, _iter,
    the annealing flag, sweeps_done, the per-sweep link counts and the likelihood rows are replicated -- all of them on
    every rank.  skip: sweeps of the snapshot these handles did not run (a fresh handle set to the seeded state).
    -> the relative errors, as compare(), and under "ranks" those of every rank's own columns (gamma, lambda, indicators)"""
    states = [s.engine.state() for s in shards]
    g = np.concatenate([st[0] for st in states], 1)
    lam = np.concatenate([st[1] for st in states], 0)
    err = (rel(g, want["gamma"]), rel(lam, want["lam"]))
    assert err[0] < tol["state"] and err[1] < tol["state"], (tag, err)
    nsw = len(want["counts"]) - skip
    wr = want["rows"][skip:]
    err_rows = err_m = 0.0
    ranks = []
    for s, st in zip(shards, states):
        who = tag + ("rank%d" % s.rank,)
        assert np.array_equal(st[2], want["conv"]), who
        c = s.engine.control()
        assert (c.iter, bool(c.annealing), c.sweeps_done) == (want["iter"], want["annealing"], nsw), who
        stats = s.engine.sweep_stats(0, nsw)
        assert [tuple(int(x) for x in r) for r in stats] == want["counts"][skip:], who
        rows = s.engine.rows()
        assert np.array_equal(rows[:, 0], wr[:, 0]), who
        np.testing.assert_allclose(rows[:, 1:], wr[:, 1:], rtol=tol["rows_rtol"], atol=tol["rows_atol"], err_msg=str(who))
        mphi, wm = s.engine.aux(2), want["mphi"][:, s.k0:s.k1]
        np.testing.assert_allclose(mphi, wm, rtol=tol["mphi_rtol"], atol=tol["mphi_atol"], err_msg=str(who))
        err_rows = max(err_rows, float(np.max(np.abs(rows[:, 1:] - wr[:, 1:]) / np.maximum(np.abs(wr[:, 1:]), 1e-300))))
        ranks.append((rel(st[0], want["gamma"][:, s.k0:s.k1]), rel(st[1], want["lam"][s.k0:s.k1]),
                      float(np.max(np.abs(mphi - wm) / np.maximum(np.abs(wm), 1e-9)))))
        err_m = max(err_m, ranks[-1][2])
    member = np.concatenate([s.engine.communities() for s in shards], 1)
    assert np.array_equal(member, want["member"]), tag
    return dict(gamma=err[0], lam=err[1], rows=err_rows, mphi=err_m, ranks=ranks)
