"""-m gpu: every instantiation of the lane-per-link kernels (svinet_amd/csrc/svils_lpl.hip, K <= 56) against the
oracle, on graphs that put every size switch of that path on both sides, plus K = 57 (the first row-per-wavefront K).

The K list holds both edges of every tier of LPL_DISPATCH (k_phi_lpl / k_s3_lpl) and FIN_DISPATCH (k_finalize_lpl); the
lower edge of a tier is where its padding columns are most.  The graphs are the hub-bearing synthetic family of
tests/test_gpu_properties.py (split hub rows, wave-items that straddle node runs) at three sizes:

  S  3 000 nodes,  ~25 000 links: below every switch -- one-round grids, 8-wave finalise, 512 / 1024-thread s3, three launches
  M 20 000 nodes, ~160 000 links: 768-thread s3 at K = 21..32, 12-wave finalise at four communities per lane
                                  (K = 25..32, 49..56), blocks that loop, still three launches at K <= 32
  L 40 000 nodes, ~320 000 links: more than 512 classification tiles -- K <= 32 keeps four launches (upper tier edges only)

Every case asserts the side of each switch its graph is on (the library's formulas restated below, with the device's CU
count), and what the handle's launch counters show of it.  A case is two phases, each compared with the oracle in full:

  (a) 4 natural sweeps from the reference initialisation (annealing, every link on the full softmax);
  (b) 5 sweeps from a seeded state (matrix_cases.seed_state) -- one at the natural _iter, whose prune() derives the active sets, then four at
      _iter = 1500 with annealing off: converged-node shortcuts, the active-set branch and the full softmax side by side.

The oracle's own link counts must show that (b) reached those branches, or the case fails before any kernel runs.

The largest error each tier showed on an MI355X is recorded beside TOL below."""
import numpy as np
import pytest

import matrix_cases as MC
from test_gpu_properties import _synthetic

pytestmark = pytest.mark.gpu

# both edges of every tier of LPL_DISPATCH and of FIN_DISPATCH (svinet_amd/csrc/svils_lpl.hip), and 57 = use_lpl's edge + 1:
# whoever adds a tier to either macro adds its two edges here
KS = [1, 8, 9, 16, 17, 20, 21, 24, 25, 28, 29, 32, 33, 36, 37, 40, 41, 48, 49, 56, 57]
L_KS = [8, 16, 20, 24, 28, 32]                 # size L: the upper tier edges of the K that can take three launches
MODE_KS = [9, 20, 25, 33, 41, 49, 56]          # every FIN_DISPATCH tier, both fold regimes
SIZES = {"S": 3000, "M": 20000, "L": 40000}    # nodes; mean degree 16 plus a hub of 3000 links
# which side of the size switches a graph must be on, on the device the suite runs on (256 CUs)
EXPECT = {"S": dict(s3_768=False, fin12=False, three=True),
          "M": dict(s3_768=True, fin12=True, three=True),
          "L": dict(s3_768=True, fin12=True, three=False)}
NAT, REG = 4, 5                                # sweeps of phase (a), of phase (b) (the first one before _iter is seeded)

# Tolerances: those of tests/test_gpu_properties.py::test_midsize_parity_with_hubs (this graph family, this size, a few
# sweeps) and of the stored-indicator test for aux(2).  Flags, counts and communities are exact.
# Largest relative errors measured against the oracle on an MI355X (256 CUs), by LPL_DISPATCH tier, over all sizes,
# modes and both phases -- gamma / lambda / likelihood rows:
#   K <=  8: 4.1e-11 / 1.9e-12 / 3.0e-13      K <= 32: 1.5e-12 / 2.2e-13 / 1.1e-11
#   K <= 16: 1.2e-11 / 7.4e-13 / 6.3e-12      K <= 36: 2.1e-13 / 1.1e-13 / 1.8e-11
#   K <= 20: 9.4e-13 / 1.9e-13 / 4.5e-12      K <= 40: 5.1e-13 / 9.3e-14 / 1.8e-11
#   K <= 24: 7.0e-13 / 1.2e-13 / 5.9e-12      K <= 48: 6.0e-13 / 1.2e-13 / 1.0e-11
#   K <= 28: 9.3e-13 / 1.6e-13 / 2.5e-11      K <= 56: 6.7e-13 / 1.4e-13 / 3.0e-11      K = 57: 6.7e-13 / 1.2e-13 / 2.2e-11
# (stored mean indicators: at most 7e-9 of max(|m|, 1e-9)): no case needs more than the 1e-8 it is given.
TOL = dict(state=1e-8, rows_rtol=1e-8, rows_atol=1e-13, mphi_rtol=1e-6, mphi_atol=1e-15)

TIMED = (1 << 1) | (1 << 5) | (1 << 6)         # reduce_sum, reduce_s, tail

_graphs, _records = {}, {}


def _pairs(size):
    if size not in _graphs:
        _graphs[size] = _synthetic(SIZES[size], 16, 11)
    return _graphs[size]


def _oracle(k, size, test=False):
    """the oracle's trajectory of one (K, size): computed once, kept for the K the modes share"""
    key = (k, size, test)
    if key in _records:
        return _records[key]
    rec = MC.trajectory(SIZES[size], _pairs(size), k, NAT, REG, test=test)
    # the condition on the seeded state, from the oracle alone: phase (b) reached the branches it is there for
    reg = rec["b"]["counts"][NAT:]
    assert any(c[0] > 0 for c in reg) and any(c[2] > 0 for c in reg), reg
    if k >= 20:
        assert any(c[1] > 0 for c in reg), reg
    if size == "M" and k in MODE_KS:
        _records[key] = rec
    return rec


def _engine(rec, k, size, **kw):
    """a handle on the oracle's inputs (its links, held-out pairs and initial state)"""
    return MC.engine_on(rec, SIZES[size], k, **kw)


def _compare(tag, want, eng, lo=0, hi=None, counts=True):
    """the state of `eng` against an oracle snapshot; [lo, hi): the rows the handle owns (tags, stored indicators)"""
    MC.compare(tag, want, eng, TOL, lo=lo, hi=hi, counts=counts)


def _two_phases(rec, engines, sweep, check):
    """phases (a) and (b) on `engines` (every handle of a run), `sweep(m)` running m sweeps on all of them"""
    MC.two_phases(rec, engines, sweep, check, REG)


def _block_shapes(k, nodes, links, cus):
    """lpl_s3_threads and lpl_finalize_waves (svils_lpl.hip) restated: the s3 block of a handle that owns `links` links,
    the waves per finalise block of one that owns `nodes` nodes -- the whole graph, or a rank's node block"""
    s3_threads = 1024 if k <= 20 else (768 if k <= 32 and links > 192 * 512 else 512)
    nc4 = k <= 56 and (25 <= k <= 32 or k > 48)      # (the row-per-wavefront finalise has no such shapes)
    w = 512 // 64 if nc4 else 576 // 64
    group = 8 if k <= 32 else 16
    return s3_threads, (12 if nc4 and nodes > w * (64 // group) * cus else w)


def _switches(k, n, nlinks, cus):
    """the library's size switches for a whole-graph handle (_block_shapes; svils_api.hip: cls_ntiles;
    svils_sweep.hip: d.fold, d.fused3), restated"""
    lpl = k <= 56
    s3_threads, fin_waves = _block_shapes(k, n, nlinks, cus)
    assert 2 * nlinks <= 1024 * 2048                       # classification tiles of 1024 entries
    ntiles = (2 * nlinks + 1023) // 1024
    fold = lpl and k <= 32
    return dict(lpl=lpl, s3_768=s3_threads == 768, fin12=fin_waves == 12, ntiles=ntiles, fold=fold,
                three=fold and ntiles <= 512)


def _assert_switch_sides(k, size, nlinks):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sw = _switches(k, SIZES[size], nlinks, cus)
    exp = EXPECT[size]
    assert sw["lpl"] == (k <= 56)
    assert sw["s3_768"] == (exp["s3_768"] and 21 <= k <= 32), (k, size, nlinks)
    assert sw["fin12"] == (exp["fin12"] and (25 <= k <= 32 or 49 <= k <= 56)), (k, size, cus)
    assert (sw["ntiles"] <= 512) == exp["three"], (size, nlinks, sw["ntiles"])
    assert sw["three"] == (exp["three"] and k <= 32)
    if size == "M":
        assert nlinks > 192 * 512
    return sw


CASES = [(k, "S") for k in KS] + [(k, "M") for k in KS] + [(k, "L") for k in L_KS]


@pytest.mark.parametrize("k,size", CASES, ids=["%s-K%d" % (s, k) for k, s in CASES])
def test_tier_against_oracle(k, size):
    """one (K, size) cell: switch sides asserted, launch counters checked, both phases against the oracle.  Phase (a)
    runs with the tail and reduce launches timed (eager sweeps), phase (b) untimed (its last four sweeps replay a graph)."""
    rec = _oracle(k, size)
    nlinks = rec["links"].shape[0]
    sw = _assert_switch_sides(k, size, nlinks)
    eng = _engine(rec, k, size)
    eng.enable_timing(TIMED)

    def check(phase, want):
        if phase == "a":
            eng.synchronize()
            t = eng.timing()
            # three launches: no k_tail, only the likelihood flush that ends the call; four: one k_tail per sweep
            assert t["tail"][1] == (1 if sw["three"] else NAT), (t["tail"], sw)
            # K <= 32 folds the partial rows in the consumers; above, k_colreduce launches leave the K-vectors
            assert t["reduce_sum"][1] == (0 if sw["fold"] else NAT) and t["reduce_s"][1] == (0 if sw["fold"] else NAT), t
            eng.enable_timing(0)
        _compare((k, size, "sweep", phase), want, eng)

    _two_phases(rec, [eng], eng.sweep, check)
    eng.close()


# ---------------------------------------------------------------------------------------------------- modes, at size M
@pytest.mark.parametrize("k,option,value", [(k, "fused3", 0) for k in MODE_KS if k <= 32] +
                         [(k, "wt", v) for k in MODE_KS for v in (0, 1)])
def test_forced_options_against_oracle(k, option, value):
    """four launches where three would do (K <= 32), and the row stores of the phi / finalise passes both ways"""
    rec = _oracle(k, "M")
    eng = _engine(rec, k, "M", options={option: value})
    assert eng.get_option(option) == value
    eng.enable_timing(1 << 6)

    def check(phase, want):
        if phase == "a":
            eng.synchronize()
            three = k <= 32 and option != "fused3"
            assert eng.timing()["tail"][1] == (1 if three else NAT)   # the flush that ends the call / one k_tail per sweep
            eng.enable_timing(0)
        _compare((k, "M", "%s=%d" % (option, value), phase), want, eng)

    _two_phases(rec, [eng], eng.sweep, check)
    eng.close()


@pytest.mark.parametrize("k", MODE_KS)
def test_phase_split_sweeps_against_oracle(k):
    """sweeps split at their exchange points (svils_sweep_phase): K-vectors through k_colreduce at every K, the stored
    mean indicators in the s3 pass, a stand-alone classification per sweep"""
    rec = _oracle(k, "M")
    eng = _engine(rec, k, "M")
    sweep = MC.phase_split_sweeps(eng)
    _two_phases(rec, [eng], sweep, lambda phase, want: _compare((k, "M", "phases", phase), want, eng))
    eng.close()


@pytest.mark.parametrize("k", MODE_KS)
def test_full_window_unit_steps_against_oracle(k):
    """mini-batch steps over all nodes with step size 1 are full sweeps (k_finalize_lpl<.., STOCH = true>): against the
    oracle itself"""
    rec = _oracle(k, "M")
    eng = _engine(rec, k, "M")
    eng.set_stochastic(batch_nodes=0, tau0=1.0, kappa=0.0)
    _two_phases(rec, [eng], eng.step, lambda phase, want: _compare((k, "M", "step", phase), want, eng))
    eng.close()


# node blocks of the M graph: a handle shapes its finalise launch by the nodes, its s3 launch by the links of ITS block, so
# rank 0 is cut large enough for the 12-wave light finalise (more than 8 * 8 * 256 nodes at K = 25..32, 8 * 4 * 256 at
# K = 49..56) and the 768-thread s3 (more than 192 * 512 links, K = 21..32); ranks 1 and 2 stay below both
BLOCK_BOUNDS = [0, 17000, 18500, 20000]


@pytest.mark.parametrize("k", MODE_KS)
def test_three_virtual_node_blocks_against_oracle(k):
    """three node blocks (BLOCK_BOUNDS) on the one GPU, the two exchanges done in process (tests/test_gpu_sharded.py):
    the light finalise pass (k_finalize_lpl<.., LIGHT = true>) in its 12-wave form on rank 0 at K = 25, 49 and 56 and in
    its 8- / 9-wave forms elsewhere, rows staged and expanded by every rank, s3 over a rank's share of the links
    (768 threads on rank 0 at K = 25), K-vectors through k_colreduce at every K (caller-driven phases do not fold).
    Each rank's side of the two switches is asserted from its block, and the ranks' link counts add up to the oracle's."""
    import torch
    from svinet_amd.host_api import Setup
    rec = _oracle(k, "M")
    setup = Setup(n=SIZES["M"], k=k, pairs=_pairs("M"))
    assert np.array_equal(setup.links, rec["links"]) and np.array_equal(setup.gamma, rec["gamma0"])
    shards, sync = MC.node_blocks(setup, BLOCK_BOUNDS)
    world, bounds = len(shards), shards[0].bounds.astype(np.int64)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for r in range(world):
        lo, hi = int(bounds[r]), int(bounds[r + 1])
        owned = int(np.count_nonzero((rec["links"][:, 0] >= lo) & (rec["links"][:, 0] < hi)))   # links by their first end
        s3_threads, fin_waves = _block_shapes(k, hi - lo, owned, cus)
        assert (fin_waves == 12) == (r == 0 and k in (25, 49, 56)), (k, r, hi - lo, cus)
        assert s3_threads == (1024 if k <= 20 else 768 if (r == 0 and k == 25) else 512), (k, r, owned)
    sweep = MC.staged_block_sweeps(shards, sync)

    def check(phase, want):
        MC.compare_blocks((k, "M", phase), want, shards, TOL)

    _two_phases(rec, [s.engine for s in shards], sweep, check)
    for s in shards:
        s.engine.close()


@pytest.mark.parametrize("k", [25, 49])
def test_handle_with_a_test_set_against_oracle(k):
    """-load-test: the test pairs leave the training links, the handle keeps four launches at any K <= 32 and adds a test
    row per sweep (the validation kernel over the test pairs)"""
    rec = _oracle(k, "M", test=True)
    assert rec["links"].shape[0] < _oracle(k, "M")["links"].shape[0] and rec["test_sorted"].shape[0] > 100
    eng = _engine(rec, k, "M")
    eng.enable_timing(1 << 6)

    def check(phase, want):
        if phase == "a":
            eng.synchronize()
            assert eng.timing()["tail"][1] == NAT
            eng.enable_timing(0)
        _compare((k, "M", "testset", phase), want, eng)

    _two_phases(rec, [eng], eng.sweep, check)
    eng.close()


@pytest.mark.parametrize("k", [41, 49])
def test_two_engines_are_bit_identical(k):
    """no floating-point atomics in k_phi_lpl<24 / 28>, k_s3_lpl<24 / 28>, k_finalize_lpl<16, 3 / 4> either: two handles on
    the same inputs end both phases with the same bits (the claim itself is about two engine runs)"""
    rec = _oracle(k, "M")
    a, b = _engine(rec, k, "M"), _engine(rec, k, "M")

    def sweep(m):
        a.sweep(m)
        b.sweep(m)

    def check(phase, want):
        for x, y in zip(a.state(), b.state()):
            assert np.array_equal(x, y), (k, phase)
        assert np.array_equal(a.rows(), b.rows()) and np.array_equal(a.communities(), b.communities())
        assert np.array_equal(a.aux(2), b.aux(2)) and np.array_equal(a.sweep_stats(), b.sweep_stats())

    _two_phases(rec, [a, b], sweep, check)
    a.close()
    b.close()
