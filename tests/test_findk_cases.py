"""The planted -findk cases without a device (tests/findk_cases.py): the plain reference and the numpy restatement
(tools/restate_findk.py) hold each other exactly, on random states and on every planted case, and the planted cases are
what their names say -- degrees, shared home slots, ties, the sharp products, the ratios around link_thresh."""
import fractions
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import restate_findk as R  # noqa: E402
import findk_cases as F  # noqa: E402

S = F.S


def _restated_count(case_n, links, held, labels):
    tr = np.asarray(links, np.int64)[np.asarray(held) == 0] if held is not None else np.asarray(links, np.int64)
    lab0 = np.asarray(labels, np.int64)[:, 0]
    src = np.concatenate([tr[:, 0], tr[:, 1]])
    lab = np.concatenate([lab0[tr[:, 1]], lab0[tr[:, 0]]])
    return R.count_top(case_n, src, lab)


def _check_steps(case, steps=2):
    """count_top, set_gamma (scripted draws) and estimate_pi against the plain reference, round after round"""
    labels, values = case.labels.astype(np.int64), case.values.copy()
    for count, requests, pads, ref_lab, ref_val, ref_pi in F.case_steps(case, steps):
        top_lab, top_cnt, d = _restated_count(case.n, case.links, case.held, labels)
        want_lab, want_cnt, want_nd = F.ref_top(count, case.n)
        assert np.array_equal(d, want_nd)
        assert np.array_equal(np.where(top_lab < 0, F.NONE, top_lab), want_lab) and np.array_equal(top_cnt, want_cnt)
        assert [r[0] for r in requests] == np.nonzero((d > 0) & (d < S))[0].tolist()
        stream = iter([p for i in sorted(pads) for p in pads[i]])
        labels, values = R.set_gamma(labels, values, top_lab, top_cnt, d, case.alpha, lambda m: next(stream), case.n)
        assert next(stream, None) is None
        assert np.array_equal(labels, ref_lab) and np.array_equal(values, ref_val)
        assert np.array_equal(R.estimate_pi(values, case.n, case.alpha), ref_pi)


def _check_likelihoods(labels, pi, pairs):
    pairs = np.asarray(pairs, np.int64)
    y = pairs[:, 2] if pairs.shape[1] > 2 else np.ones(len(pairs), np.int64)
    sums = np.array(F.ref_pair_sums(labels, pi, pairs))
    # the same positions through the same numpy log: equal bits if and only if the sums are
    assert np.array_equal(R.edge_ll(np.asarray(labels, np.int64), pi, pairs[:, 0], pairs[:, 1], y), np.log(sums))


def _check_groups(labels, pi, links, thresh):
    bad, mem = R.groups(np.asarray(labels, np.int64), pi, np.asarray(links, np.int64), thresh)
    unlikely, member = F.ref_groups(labels, pi, links, thresh)
    assert bad == unlikely
    assert set(mem.tolist()) == set((lab << 32) | i for i, labs in member.items() for lab in labs)


def test_tier_constants_are_the_units():
    src = open(os.path.join(ROOT, "svinet_amd", "csrc", "svils_findk.hip")).read()
    for name, want in (("S", F.S), ("WAVE_MAX", F.WAVE_MAX), ("LDS_SLOTS", F.LDS_SLOTS), ("SUM_CHUNK", F.SUM_CHUNK),
                       ("SENTINEL", F.SENTINEL)):
        m = re.search(r"constexpr uint32_t %s = (\d+);" % name, src)
        assert m and int(m.group(1)) == want, name
    assert "(lab * %du) & mask" % F.HASH_MUL in src and "if (s < 1e-30) s = 1e-30;" in src


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_plain_reference_equals_restatement_on_random_states(seed):
    rs = np.random.RandomState(seed)
    n, E = 300, 1500 * seed
    pq = rs.randint(0, n, (4 * E, 2))
    pq = np.unique(np.sort(pq[pq[:, 0] != pq[:, 1]], axis=1), axis=0)[:E]
    held = (rs.random_sample(len(pq)) < 0.1).astype(np.uint8)
    labels = rs.randint(0, 12 * seed, (n, S)).astype(np.uint32)       # few labels: ties and duplicates inside a node
    values = 0.05 + 2.95 * rs.random_sample((n, S))
    non = rs.randint(0, n, (200, 2))
    pairs = np.concatenate([np.column_stack([pq[held == 1], np.ones(int(held.sum()), np.int64)]),
                            np.column_stack([non, np.zeros(200, np.int64)])])
    case = F.Case(n, 1.0 / (seed + 2), pq.astype(np.uint32), held, pairs, labels, values, {})
    _check_steps(case, 3)
    for _, _, _, lab, val, pi in F.case_steps(case, 3):
        _check_likelihoods(lab, pi, pq)
        _check_likelihoods(lab, pi, pairs)
        for thresh in (0.5, 0.9):
            _check_groups(lab, pi, pq, thresh)


@pytest.mark.parametrize("name", ["ladder", "hubs", "tiny2", "tiny3", "tiny4"])
def test_plain_reference_equals_restatement_on_planted_counts(name):
    case = F.tiny(int(name[4])) if name.startswith("tiny") else getattr(F, name)()
    _check_steps(case)
    if name != "ladder":
        lab, val, pi = F.case_steps(case)[-1][3:]
        _check_likelihoods(lab, pi, case.links)
        _check_groups(lab, pi, case.links, 0.5)
        if len(case.pairs):
            _check_likelihoods(lab, pi, case.pairs)


def test_plain_reference_equals_restatement_on_planted_likelihoods_and_groups():
    names, n, alpha, labels, values = F.pair_cases()
    pi = F.ref_pi(values, n, alpha)
    assert np.array_equal(pi, R.estimate_pi(values, n, alpha))
    _check_likelihoods(labels, pi, [(2 * c, 2 * c + 1, y) for c, (_, y) in enumerate(names)])
    labels, values, alpha = F.sums_state()
    pi = F.ref_pi(values, F.SUM_N, alpha)
    links, held, pairs = F.sums_graph(4097, 4096)
    _check_likelihoods(labels, pi, links)
    _check_likelihoods(labels, pi, pairs)
    terms = F.sums_terms(labels, pi, pairs)
    assert terms == [F.log_cr(s) for s in F.ref_pair_sums(labels, pi, pairs)]      # the memo changes nothing
    links, labels, values, named = F.groups_case()
    pi = F.ref_pi(values, F.GROUPS_N, F.GROUPS_ALPHA)
    assert np.array_equal(pi, R.estimate_pi(values, F.GROUPS_N, F.GROUPS_ALPHA))
    for thresh in (0.5, 0.9):
        _check_groups(labels, pi, links, thresh)


# ---- preconditions of the planted cases ----------------------------------------------------------------------------------

def test_every_centre_has_the_degree_its_name_says():
    for case in (F.ladder(), F.hubs()):
        deg = F.ref_degrees(case.links, case.held)
        for name, (node, d) in case.centres.items():
            assert deg[node] == d, name
            assert name.rsplit("_", 1)[-1] == str(d) or name.startswith(("chain", "held", "all_held", "hub")), name
    lad = F.ladder()
    assert len(np.unique(lad.links, axis=0)) == len(lad.links) and np.all(lad.links[:, 0] < lad.links[:, 1])
    total = F.ref_degrees(lad.links, None)
    for name, tot in (("held_65_is_64", 65), ("held_66_is_65", 66), ("held_2049_is_2048", 2049)):
        node, d = lad.centres[name]
        assert total[node] == tot and d == tot - 1
    assert total[lad.centres["all_held"][0]] == 2 and lad.centres["all_held"][0] not in F.ref_degrees(lad.links, lad.held)
    assert F.hubs().centres["hub_a"][1] == F.hubs().n - 1
    # every rung carries every pattern that fits it
    for d in F.RUNGS:
        for p in F.PATTERNS:
            assert (("%s_%d" % (p, d)) in lad.centres) == (F.pattern_counts(p, d, 0) is not None)
    assert lad.n <= 10 ** 6 and int(lad.labels.max()) < lad.n


def test_patterns_are_what_their_names_say():
    lad = F.ladder()
    count = F.case_steps(lad)[0][0]
    for d in F.RUNGS:
        for k in (2, 3, 4, 5, 6):
            if d >= k:
                ranked = count[lad.centres["k%d_%d" % (k, d)][0]]
                assert len(ranked) == k and sum(c for _, c in ranked) == d
        assert len(count[lad.centres["one_%d" % d][0]]) == 1
        ranked = count[lad.centres["distinct_%d" % d][0]]
        assert len(ranked) == d and [lab for lab, _ in ranked] == sorted(lab for lab, _ in ranked)
        assert all(lab > 65535 for lab, _ in count[lad.centres["big_%d" % d][0]])
        if d >= 6:
            ranked = count[lad.centres["tie56_%d" % d][0]]
            assert len(ranked) == 6 and ranked[4][1] == ranked[5][1] and ranked[4][0] < ranked[5][0]
        if "alltied_%d" % d in lad.centres:
            ranked = count[lad.centres["alltied_%d" % d][0]]
            assert len(set(c for _, c in ranked)) == 1 and len(ranked) >= 2
        if d >= 2:
            ranked = count[lad.centres["dominant_%d" % d][0]]
            assert all(c == 1 for _, c in ranked[1:]) and len(ranked) == min(d - 1, 37) + 1
    # tie order and count order disagree somewhere: a tied 5th place whose label was planted after the 6th's
    glab = F.group_labels()
    assert any(glab.index(count[lad.centres["tie56_%d" % d][0]][4][0]) > glab.index(count[lad.centres["tie56_%d" % d][0]][5][0])
               for d in F.RUNGS if d >= 6)
    assert len(F.case_steps(lad)[0][1]) > 4096                  # thousands of nodes ask for pads ...
    assert set(r[1] for r in F.case_steps(lad)[0][1]) == {1, 2, 3, 4}     # ... of every ndistinct


def test_group_labels_sit_in_the_threads_and_wavefronts_they_are_chosen_for():
    g = F.group_labels()
    assert len(set(g)) == len(g) and not set(g) & set(F.single_label(j) for j in range(F.RUNGS[-1]))
    for T in (4096, 8192, 16384):
        slots = [F.home_slot(v, T) for v in g[:6]]
        assert len(set(slots)) == 6                              # no displacement: each sits in its home slot
        thread = [s % 256 for s in slots]
        assert thread[0] == thread[1] and [t // 64 for t in thread[:5]] == [0, 0, 1, 2, 3]
    assert g[1] > 65535 and g[4] > 65535 and g[5] == 65535 and list(g[:5]) != sorted(g[:5])


def test_chained_labels_share_the_last_slot_of_their_table():
    lad = F.ladder()
    count = F.case_steps(lad)[0][0]
    for name, d, first, stride, cnt in F.CHAINS:
        T = F.table_size(d)
        assert T == stride and F.bin_of(d) == ("lds" if T == 4096 else "hub")
        labs = F.chain_labels(first, stride, cnt)
        assert set(F.home_slot(v, T) for v in labs) == {T - 1}    # the chain starts in the last slot and wraps to 0
        ranked = count[lad.centres[name][0]]
        assert sorted(lab for lab, _ in ranked) == labs
        mult = [c for _, c in ranked]
        assert len(set(mult)) > 3 and len(set(mult)) < len(mult)  # unequal, with ties
    assert F.table_size(4096) == 8192 and F.table_size(4097) == 16384 and F.table_size(2049) == 8192


def test_sharp_products_round_equal_and_differ_exactly():
    Fr = fractions.Fraction
    links, labels, values, named = F.groups_case()
    pi = F.ref_pi(values, F.GROUPS_N, F.GROUPS_ALPHA)
    for name, first_smaller in (("sharp_second_larger", True), ("sharp_first_larger", False)):
        i, m = named[name]
        assert labels[i, 0] == labels[m, 0] and labels[i, 1] == labels[m, 1]
        assert pi[i, 0] * pi[m, 0] == pi[i, 1] * pi[m, 1]
        e0, e1 = Fr(pi[i, 0]) * Fr(pi[m, 0]), Fr(pi[i, 1]) * Fr(pi[m, 1])
        assert e0 != e1 and (e0 < e1) == first_smaller
        # a fused multiply-add compares the exact product: fma(a, b, -mx) > 0 where the rounded u > mx is false
        assert (e1 > Fr(pi[i, 0] * pi[m, 0])) == first_smaller


def test_ties_and_threshold_cases_sit_where_intended():
    links, labels, values, named = F.groups_case()
    pi = F.ref_pi(values, F.GROUPS_N, F.GROUPS_ALPHA)
    _, _, entries = F.ref_groups(labels, pi, links, 0.5, detail=True)
    at = {tuple(l): x for x, l in enumerate(links.tolist())}
    i, m = named["tie"]
    assert pi[i, 0] * pi[m, 0] == pi[i, 1] * pi[m, 1] and \
        fractions.Fraction(pi[i, 0]) * fractions.Fraction(pi[m, 0]) == fractions.Fraction(pi[i, 1]) * fractions.Fraction(pi[m, 1])
    assert entries[2 * at[(i, m)]][0] == labels[i, 0] == entries[2 * at[(i, m)] + 1][0]
    for thresh in (0.5, 0.9):
        for side in (-1, 0, 1):
            x = at[named["thresh_%g_%+d" % (thresh, side)]]
            want = thresh if side == 0 else math.nextafter(thresh, 2.0 * side)
            assert entries[2 * x][1] == want and entries[2 * x + 1][1] == want
    assert entries[2 * at[named["sum_zero"]]][3] == 0.0
    assert entries[2 * at[named["sentinel_wins"]]][:2] == (F.SENTINEL, 1.0)
    assert F.GROUPS_N > 65536 and len(links) > 4096


def test_sums_graphs_are_unique_links_with_an_interleaved_heldout_list():
    for E, H in ((1, 1), (4095, 4097), (4096, 4095), (4097, 4096), (F.SUM_BIG_E, 4097)):
        links, held, pairs = F.sums_graph(E, H)
        assert len(links) == E and len(pairs) == H
        key = links[:, 0].astype(np.int64) * F.SUM_N + links[:, 1]
        assert len(np.unique(key)) == E and np.all(links[:, 0] < links[:, 1])
        y = pairs[:, 2]
        assert int(held.sum()) == int(y.sum())
        pk = pairs[:, 0].astype(np.int64) * F.SUM_N + pairs[:, 1]
        assert np.array_equal(np.isin(pk, key), y == 1) and set(pk[y == 1].tolist()) == set(key[held == 1].tolist())
        if H > 4096:   # both selections on both sides of the chunk edge
            assert set(y[:4096].tolist()) == {0, 1} and set(y[4090:4096].tolist()) == {0, 1} and len(y[4096:]) >= 1
    assert F.SUM_BIG_E > 256 * F.SUM_CHUNK
