"""-m gpu: every device kernel of -findk (svinet_amd/csrc/svils_findk.hip) on planted states, tier by tier, against the
plain reference of tests/findk_cases.py (tests/test_findk_cases.py holds that reference against the numpy restatement
and proves the planted cases are what they claim).  Integer-exact or bit-exact, but for the logarithms:

  * a per-pair likelihood is held to the CORRECTLY ROUNDED log of the reference's sum, within LOG_ULP = 1.5 ulp: the HIP
    math API documents the double-precision log of the ROCm device library at 1 ulp from the true value, and the
    correctly rounded one lies within 1/2 ulp of it.  Largest measured on an MI355X: 0.0 ulp -- all 95 values equal the
    correctly rounded ones (profiles/r23a_findk_matrix.md);
  * a sum is held to math.fsum of the reference's terms within findk_cases.sum_bound: (D + c) 2^-53 sum |term|, D the
    addition depth of k_part_sum for the size at hand and c = LOG_C the per-term allowance above (1.5 ulp <= 3 x 2^-53
    relative; the reference's terms are the correctly rounded logs).
"""
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import findk_cases as F  # noqa: E402

pytestmark = pytest.mark.gpu

S = F.S
LOG_ULP = 1.5
LOG_C = 3


def _run_steps(case, steps=2, thresh=0.5):
    """`steps` rounds of count -> pad requests -> apply on a fresh handle with the reference's pads; per round the
    request rows and the state"""
    ref = F.case_steps(case, steps)
    h = F.Handle(case.n, case.alpha, thresh)
    try:
        h.ok(h.set_graph(case.links, case.held, case.pairs))
        h.ok(h.init_state(case.labels, case.values))
        out = []
        for r in range(steps):
            out.append(h.step(ref[r][2]) + h.state())
        return out
    finally:
        h.close()


@pytest.fixture(scope="module")
def ladder_run():
    return _run_steps(F.ladder())


@pytest.fixture(scope="module")
def hubs_run():
    return _run_steps(F.hubs())


def _check_centre(case, run, ref, name):
    """the counted slots of one centre after the first apply: labels the top 5, values - alpha the counts; its request row"""
    node = case.centres[name][0]
    nodes, nd, req, lab, val, _ = run
    ranked = ref[0].get(node, [])
    got = [(int(lab[node, j]), val[node, j]) for j in range(min(len(ranked), S))]
    want = [(label, float(c) + case.alpha) for label, c in ranked[:S]]
    assert got == want, (name, got, want)
    at = np.searchsorted(nodes, node)
    asked = at < len(nodes) and nodes[at] == node
    assert asked == (1 <= len(ranked) < S), name
    if asked:
        assert nd[at] == len(ranked) and req[at].tolist() == [label for label, _ in ranked] + [F.NONE] * (4 - len(ranked)), name


# ---- count and top 5 -----------------------------------------------------------------------------------------------------

def test_planted_degrees_cover_every_bin_and_both_sides_of_every_tier():
    lad, hub = F.ladder(), F.hubs()
    deg = F.ref_degrees(lad.links, lad.held)
    planted = sorted(set(deg[node] for node, _ in lad.centres.values()) | set(d for _, d in hub.centres.values()))
    assert all(deg[node] == d for node, d in lad.centres.values())
    bins = set(F.bin_of(d) for d in planted)
    assert bins == {None, "wave", "lds", "hub"}
    for below in (F.WAVE_MAX, F.LDS_SLOTS // 2, F.LDS_SLOTS):
        assert below in planted and below + 1 in planted
    assert F.bin_of(64) == "wave" and F.bin_of(65) == "lds" and F.bin_of(2048) == "lds" and F.bin_of(2049) == "hub"
    assert F.table_size(4096) == 8192 and F.table_size(4097) == 16384
    assert set(F.RUNGS) <= set(planted) and hub.n - 1 in planted
    # every pattern sits on both sides of every boundary
    for p in F.PATTERNS:
        for d in (64, 65, 2048, 2049, 4096):
            assert "%s_%d" % (p, d) in lad.centres, (p, d)
    assert sum(1 for p in F.PATTERNS if "%s_4097" % p in lad.centres) >= len(F.PATTERNS) - 1   # 4097 = 17 x 241 ties too


@pytest.mark.parametrize("d", F.RUNGS)
def test_count_of_every_pattern_on_the_rung(ladder_run, d):
    lad = F.ladder()
    ref = F.case_steps(lad)[0]
    names = ["%s_%d" % (p, d) for p in F.PATTERNS if "%s_%d" % (p, d) in lad.centres]
    assert len(names) >= 3
    for name in names:
        _check_centre(lad, ladder_run[0], ref, name)


@pytest.mark.parametrize("name", [c[0] for c in F.CHAINS])
def test_count_through_a_probe_chain_that_wraps(ladder_run, name):
    _check_centre(F.ladder(), ladder_run[0], F.case_steps(F.ladder())[0], name)


@pytest.mark.parametrize("name", ["held_65_is_64", "held_66_is_65", "held_2049_is_2048", "all_held"])
def test_heldout_links_leave_the_count_and_the_bins(ladder_run, name):
    lad = F.ladder()
    ref = F.case_steps(lad)[0]
    _check_centre(lad, ladder_run[0], ref, name)
    node = lad.centres[name][0]
    if name == "all_held":       # no training link: the planted slots stay
        assert np.array_equal(ladder_run[0][3][node], lad.labels[node]) and np.array_equal(ladder_run[0][4][node], lad.values[node])
    else:
        assert len(ref[0][node]) == 2 and ladder_run[0][1][np.searchsorted(ladder_run[0][0], node)] == 2


def test_hubs_of_degree_n_minus_one(hubs_run):
    hub = F.hubs()
    for name in hub.centres:
        _check_centre(hub, hubs_run[0], F.case_steps(hub)[0], name)


@pytest.mark.parametrize("which", ["ladder", "hubs"])
def test_pad_requests_ascend_and_equal_the_reference(ladder_run, hubs_run, which):
    case, run = (F.ladder(), ladder_run) if which == "ladder" else (F.hubs(), hubs_run)
    for r in range(2):
        nodes, nd, req = run[r][:3]
        want = F.case_steps(case)[r][1]
        assert np.all(np.diff(nodes.astype(np.int64)) > 0)
        assert nodes.tolist() == [w[0] for w in want] and nd.tolist() == [w[1] for w in want]
        assert np.array_equal(req, np.array([w[2] for w in want], np.uint32).reshape(-1, 4))
    if which == "ladder":
        assert len(run[0][0]) > 4096 and set(run[0][1].tolist()) == {1, 2, 3, 4}


# ---- apply, pads, pi -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["ladder", "hubs"])
def test_state_after_one_and_two_rounds_is_the_references_bit_for_bit(ladder_run, hubs_run, which):
    """the second round reads the labels the first one wrote (a Jacobi step: all counts from the previous labels)"""
    case, run = (F.ladder(), ladder_run) if which == "ladder" else (F.hubs(), hubs_run)
    for r in range(2):
        count, _, pads, lab, val, pi = F.case_steps(case)[r]
        got_lab, got_val, got_pi = run[r][3:]
        bad = np.nonzero(np.any(got_lab != lab, axis=1) | np.any(got_val != val, axis=1))[0]
        assert len(bad) == 0, (r, bad[:8].tolist(), got_lab[bad[:2]].tolist(), lab[bad[:2]].tolist(), got_val[bad[:2]].tolist())
        assert np.array_equal(got_pi.view(np.uint64), pi.view(np.uint64)), r
        for i, p in list(pads.items())[::97]:                     # the sent pads, in order, with 2 alpha
            d = len(count[i])
            assert got_lab[i, d:].tolist() == p and np.all(got_val[i, d:] == case.alpha + case.alpha)
    idle = np.setdiff1d(np.arange(case.n), np.array(sorted(F.case_steps(case)[0][0])))
    if which == "ladder":
        assert len(idle) > 1000
    assert np.array_equal(run[1][3][idle], case.labels[idle]) and np.array_equal(run[1][4][idle], case.values[idle])


@pytest.mark.parametrize("n", [2, 3, 4])
def test_fewer_than_five_nodes(n):
    """(n - 5) wraps in uint32, as the reference's does"""
    case = F.tiny(n)
    run = _run_steps(case)
    for r in range(2):
        _, requests, _, lab, val, pi = F.case_steps(case)[r]
        assert run[r][0].tolist() == [w[0] for w in requests] and run[r][2].tolist() == [w[2] for w in requests]
        assert np.array_equal(run[r][3], lab) and np.array_equal(run[r][4], val)
        assert np.array_equal(run[r][5].view(np.uint64), pi.view(np.uint64))
        assert np.all(pi < 1e-8)                                  # the wrap happened


# ---- likelihoods ---------------------------------------------------------------------------------------------------------

def _ulps(got, want):
    return abs(got - want) / math.ulp(max(abs(got), abs(want)))


def test_per_pair_likelihoods_against_the_correctly_rounded_log():
    names, n, alpha, labels, values = F.pair_cases()
    pi = F.ref_pi(values, n, alpha)
    h = F.Handle(n, alpha)
    worst = 0.0
    try:
        h.ok(h.init_state(labels, values))
        assert np.array_equal(h.state()[2].view(np.uint64), pi.view(np.uint64))
        for c, (name, y) in enumerate(names):
            p, q = 2 * c, 2 * c + 1
            want = F.log_cr(F.ref_pair_sums(labels, pi, [(p, q, y)])[0])
            if name.startswith(("disjoint_y1", "all_one_label_y0", "below_floor")):
                assert want == F.log_cr(1e-30), name
            links, held = ([(p, q)], [1]) if y else ([(0, 1)], [0])
            h.ok(h.set_graph(links, held, [(p, q, y)]))
            t, hs, _, _ = h.report()
            got = [hs[0], hs[1 + y]] + ([t] if y else [])
            assert hs[2 - y] == 0.0, name                          # the other selection is empty
            for g in got:
                worst = max(worst, _ulps(g, want))
                assert _ulps(g, want) <= LOG_ULP, (name, g, want)
    finally:
        h.close()
    print("per-pair likelihoods: largest error %.2f ulp of the correctly rounded log (bound %.1f)" % (worst, LOG_ULP))


def test_per_pair_likelihoods_with_fewer_than_five_nodes():
    n, alpha = 3, 0.25
    labels = np.array([[0, 1, 2, 0, 1], [2, 2, 0, 1, 1], [1, 1, 1, 1, 1]], np.uint32)
    values = np.array([[1.5, 0.25, 0.75, 0.5, 1.0], [0.3, 0.7, 1.1, 0.9, 0.2], [1, 2, 3, 4, 5.0]])
    pi = F.ref_pi(values, n, alpha)
    h = F.Handle(n, alpha)
    try:
        h.ok(h.init_state(labels, values))
        h.ok(h.set_graph([(0, 1), (1, 2)], [0, 1], [(0, 2, 0), (1, 2, 1)]))
        t, hs, unlikely, masks = h.report()
    finally:
        h.close()
    s = F.ref_pair_sums(labels, pi, [(0, 1, 1), (1, 2, 1), (0, 2, 0)])
    assert s[2] > 1e-30 and s[0] > 1e-30
    for got, want in ((hs[1], F.log_cr(s[2])), (hs[2], F.log_cr(s[1]))):
        assert _ulps(got, want) <= LOG_ULP
    assert abs(t - (F.log_cr(s[0]) + F.log_cr(s[1])) / 2) <= 4 * math.ulp(t)
    want_u, member = F.ref_groups(labels, pi, [(0, 1), (1, 2)], 0.5)
    assert unlikely == want_u and F.decode_masks(masks, labels) == member


SUM_SIZES = [(1, 1), (4095, 4097), (4096, 4095), (4097, 4096), (F.SUM_BIG_E, 4097)]


@pytest.fixture(scope="module")
def sums_handle():
    labels, values, alpha = F.sums_state()
    h = F.Handle(F.SUM_N, alpha)
    h.ok(h.init_state(labels, values))
    yield h
    h.close()


@pytest.mark.parametrize("E,H", SUM_SIZES)
def test_sums_against_fsum_within_the_depth_of_the_tree(sums_handle, E, H):
    labels, values, alpha = F.sums_state()
    pi = F.ref_pi(values, F.SUM_N, alpha)
    links, held, pairs = F.sums_graph(E, H)
    sums_handle.ok(sums_handle.set_graph(links, held, pairs))
    t, hs, _, _ = sums_handle.report(groups=False)
    terms = F.sums_terms(labels, pi, links)
    bound = F.sum_bound(E, math.fsum(abs(v) for v in terms), LOG_C)
    # training_ll is the sum over E: one more rounding (the division)
    want = math.fsum(terms)
    err = abs(t * E - want)
    print("E = %d: |sum - fsum| = %.3e, bound %.3e" % (E, err, bound + abs(want) * 2.0 ** -52))
    assert err <= bound + abs(want) * 2.0 ** -52
    hterms = F.sums_terms(labels, pi, pairs)
    y = pairs[:, 2].tolist()
    for k, sel in enumerate((None, 0, 1)):
        chosen = [v for v, yy in zip(hterms, y) if sel is None or yy == sel]
        bound = F.sum_bound(H, math.fsum(abs(v) for v in chosen), LOG_C)     # the tree is H wide whatever is selected
        err = abs(hs[k] - math.fsum(chosen))
        print("H = %d, y = %s: %d terms, |sum - fsum| = %.3e, bound %.3e" % (H, sel, len(chosen), err, bound))
        assert err <= bound, (sel, hs[k], math.fsum(chosen))
        if not chosen:
            assert hs[k] == 0.0
    if H > 1:
        assert 0 < sum(y) < H


def test_two_handles_give_the_same_bits():
    labels, values, alpha = F.sums_state()
    links, held, pairs = F.sums_graph(3 * F.SUM_CHUNK + 77, 4097)
    outs = []
    for _ in range(2):
        h = F.Handle(F.SUM_N, alpha)
        try:
            h.ok(h.init_state(labels, values))
            h.ok(h.set_graph(links, held, pairs))
            rc, m = h.count()
            h.ok(rc)
            rc, nodes, nd, req = h.pad_requests(m)
            h.ok(h.apply((nodes[:, None] + np.arange(1, 5)[None, :]) % F.SUM_N))
            t, hs, u, masks = h.report()
            outs.append((np.float64(t).tobytes(), hs.tobytes(), u, masks.tobytes(), nodes.tobytes(), req.tobytes()) +
                        tuple(a.tobytes() for a in h.state()))
        finally:
            h.close()
    assert outs[0] == outs[1]


# ---- groups --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("thresh", [0.5, 0.9])
def test_groups_on_planted_pairs(thresh):
    links, labels, values, named = F.groups_case()
    pi = F.ref_pi(values, F.GROUPS_N, F.GROUPS_ALPHA)
    h = F.Handle(F.GROUPS_N, F.GROUPS_ALPHA, thresh)
    try:
        h.ok(h.init_state(labels, values))
        assert np.array_equal(h.state()[2].view(np.uint64), pi.view(np.uint64))
        got = {}
        # every named pair alone (its own unlikely count), then the whole graph
        for name, (i, m) in named.items():
            if name in ("hub", "two_slots"):
                continue
            h.ok(h.set_graph([(i, m)]))
            _, _, u, masks = h.report()
            want_u, member = F.ref_groups(labels, pi, [(i, m)], thresh)
            got[name] = u
            assert (u, F.decode_masks(masks, labels)) == (want_u, member), name
        h.ok(h.set_graph(links))
        _, _, u, masks = h.report()
    finally:
        h.close()
    want_u, member = F.ref_groups(labels, pi, links, thresh)
    assert u == want_u and F.decode_masks(masks, labels) == member
    hub, leaf = named["hub"]
    assert masks[hub] == 1 << 2 and masks[leaf] == 1                 # 5000 links, one bit
    assert masks[named["two_slots"][0]] == (1 | 1 << 2)
    assert got["sentinel_wins"] == 0 and got["sum_zero"] == 2 and got["tie"] == (0 if thresh == 0.5 else 2)
    assert [got["thresh_%g_%+d" % (thresh, s)] for s in (-1, 0, 1)] == [2, 0, 0]
    i, m = named["sentinel_wins"]
    assert masks[i] == 0 and masks[m] == 0
    if thresh == 0.5:
        assert F.decode_masks(masks, labels)[named["tie"][0]] == {100}
        assert F.decode_masks(masks, labels)[named["sharp_second_larger"][0]] == {100}
        assert F.decode_masks(masks, labels)[named["sharp_first_larger"][0]] == {200}


# ---- refusals ------------------------------------------------------------------------------------------------------------

def test_refusals():
    n = 6
    labels, values = F._filler_state(n, 5)
    h = F.Handle(n, 0.5)
    try:
        rc, m = h.count()
        assert rc == -1 and "set the graph and the state first" in h.error()
        h.ok(h.set_graph([(0, 1), (1, 2)]))
        rc, m = h.count()
        assert rc == -1 and "set the graph and the state first" in h.error()          # the graph alone
        h2 = F.Handle(n, 0.5)
        try:
            h2.ok(h2.init_state(labels, values))
            assert h2.count()[0] == -1 and "set the graph and the state first" in h2.error()   # the state alone
        finally:
            h2.close()
        bad = labels.copy()
        bad[3, 2] = n
        assert h.init_state(bad, values) == -1 and "label 6 >= n = 6" in h.error()
        h.ok(h.init_state(labels, values))
        assert h.pad_requests(1)[0] == -1 and "no svils_findk_count" in h.error()
        assert h.apply(np.zeros((1, 4), np.uint32)) == -1 and "no svils_findk_count" in h.error()
        rc, m = h.count()
        h.ok(rc)
        assert m == 3
        pads = np.zeros((m, 4), np.uint32)
        pads[1, 2] = n                       # node 1 has two distinct labels: pads 0 .. 2 are read
        assert h.apply(pads) == -1 and "pad label of record 1 >= n" in h.error()
        pads[1, 2], pads[1, 3] = 0, n        # the fourth is not
        h.ok(h.apply(pads))
        assert h.pad_requests(m)[0] == -1 and h.apply(pads) == -1                      # the count is spent
        rc, m = h.count()
        h.ok(rc)
        h.ok(h.init_state(labels, values))                                              # a new state spends it too
        assert h.apply(pads) == -1 and "no svils_findk_count" in h.error()
        rc, m = h.count()
        h.ok(rc)
        h.ok(h.set_graph([(0, 1)]))                                                     # and so does a new graph
        assert h.pad_requests(m)[0] == -1
        assert h.set_graph([(0, 6)]) == -1 and h.set_graph([(2, 2)]) == -1
        assert h.set_graph([(0, 1)], None, [(0, 6, 1)]) == -1
    finally:
        h.close()
