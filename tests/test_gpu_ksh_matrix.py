"""-m gpu: every instantiation of the K-sharded kernels (svinet_amd/csrc/svils_ksh.h) against the oracle, built like
tests/test_gpu_small_k_matrix.py and tests/test_gpu_rpw_matrix.py on the machinery of tests/matrix_cases.py.  All ranks are
virtual ranks in one process on one GPU (svinet_amd/ksharded.py: KShard, init_virtual, sweep_virtual, step_virtual).

The width of a rank's column slice selects its kernels (pick_layout: V doubles per lane; slices of <= 64 columns take the
16-lane kernels k_phi_ksh16 / k_s3_ksh16 / k_fin*_ksh<16, 4> in the product form and k_phi_ksh<1, ., true> in the log
form); k_total only sets the oracle's cost and the default form (log above 700).  So the cases are a few runs with UNEQUAL
slices (KShard(bounds=...)) -- the LADDERS below hold both edges of every tier, ranks of different tiers exchange with each
other, and the 16-lane kernels run next to the 64-lane ones.  The graphs are those of the row-per-wavefront matrix (W and
N: rows split into slotted items at training degrees 33, 64 and 65, a hub, phi blocks that loop over items -- asserted for
every rank from its own V; the one rank that cannot loop is named at LOOP_EXEMPT).  One ladder (1, 3, 17, 64, 65, 128, 129,
256) would hold all tiers up to V = 4, but at k_total = 663 on graph W the ORACLE's own likelihood rows are off by 1.2e-8
(its K^2 loop, _oracle_row_error), more than the 1e-8 they are held to: hence A and G, and F = (513, 3).

A case is the two phases of matrix_cases (NAT natural sweeps, REG sweeps from the seeded state), each compared with the
oracle in full on every rank (matrix_cases.compare_slices).  The seeded state additionally plants converged flags at the
slice edges (_edge_seed): for every inner bound b the flags b and b + 1 -- quirk Q2 reads column pc and adds into column
pc - 1, so flag b crosses the edge through q2v[K0 - 1] and flag b + 1 is the first that does not -- and flag k_total (Q2
with pc == K reads nothing); the neighbours of the flagged nodes get mass in that column, so that what Q2 reads is of order
0.1.  From the oracle alone, before any kernel runs: phase (b) reached the dense, active-set and shortcut branches, every
planted flag has links with exactly one converged end whose other end has a mean indicator above 0.01 in the column read,
and the oracle's own likelihood rows are good to the tolerance (against an extended-precision evaluation of the same pairs).

Forms (what selects them is confirmed on the handles, ksh_log_domain(), before the sweeps):

  default    the product form on A, G and F (k_total <= 700), the log form on B-E
  log        forced on A, G and F: k_phi_ksh<V, 0|1|2, true> at V = 1, 2, 4, 12 (V = 8: B by default), k_fin2_ksh<16, 4> and
             <64, V>; the state differs in bits from the product run
  product    forced on B-E, phase (b) only, from fresh handles set to the seed: k_phi_ksh<V, 1|2, false> at V >= 8, the fused
             k_fin1_ksh and k_flags_ksh.  (The natural first sweep underflows in this form -- `underflow`, on B: the library
             must say so.)  Restated on the CPU from the oracle's states WITH the row-sum shift of k_fin1_ksh (the exp(Elogpi)
             rows of a sweep are shifted by psi of the row sums of the state before the previous one): on the first natural
             sweep 1477 (B), 677 (C), 2332 (D and E: the same natural sweeps) links have a denominator below 1e-280; from the seed the smallest
             denominator is 2.8e-25 (sweep 1 of phase (b)), then 0.47 and 1.1e-4 -- the shift makes them larger, not smaller,
             since the row sums grow from ~50 to ~n.  No link of the active-set branch has a masked sum of exactly 0 on any
             ladder (neither an empty union nor one that underflowed: every union here holds community 0, where both rows
             have mass), so the `sparse && s == 0` clause of k_phi_ksh is not reached by these states.
  lowt       link_thresh < 1/2 (the arg-max tagging: ksh_lowt, the MIN exchange of SVILS_KSH_EARG), lt_min_deg 0 on every
             ladder and 2 on A, G, C and E, on oracle trajectories of their own whose communities differ from the 1/2 run's
  steps      full-window unit steps (k_fin1_ksh<., ., true>) in the ladder's default form; steps_log: forced log on A and G

then mini-batch windows against svils_step on one plain handle (A, G, F and the bounds [0, 1025, 2048]), and exact ties of the
maximum whose columns lie on different ranks (A, C, E).  The likelihood row of a state between two sweeps (phase VDOT:
k_vdot_ksh<V> alone, ksharded.validation_row_virtual) is compared right after init_virtual with the oracle's constructor row
and after the first sweep with that sweep's row.

The whole file -- 44 cases -- takes 35 s on an MI355X host (slowest case 3.0 s, B, of which the oracle is most; on a slower
CPU the oracle side alone is about 70 s); the largest errors are recorded beside TOL."""
import types

import numpy as np
import pytest

import matrix_cases as MC
import test_gpu_rpw_matrix as R

pytestmark = pytest.mark.gpu

# ladder -> (slice widths, graph of tests/test_gpu_rpw_matrix.py).  Whoever adds a tier to pick_layout adds its two edges
# (test_ladders_cover_every_instantiation fails until then).
LADDERS = {"A": ((1, 3, 17, 64, 65, 128), "W"),                # k_total  278: product by default
           "G": ((3, 129, 256), "W"),                          #          388: product by default
           "B": ((257, 512, 513), "W"),                        #         1282
           "C": ((768, 769), "N"),                             #         1537
           "D": ((1024, 1025), "N"),                           #         2049
           "E": ((2048, 1), "N"),                              #         2049 (see LOW_THRESH)
           "F": ((513, 3), "W")}                               #          516: the default product form at V = 12
TIERS = {1: (1, 64), 2: (65, 128), 4: (129, 256), 8: (257, 512), 12: (513, 768), 16: (769, 1024), 32: (1025, 2048)}
NAT, REG = R.NAT, R.REG
FORMS = {"A": ("default", "log", "lowt_min0", "lowt_min2", "steps", "steps_log"),
         "B": ("default", "product", "underflow", "lowt_min0", "steps"),
         "C": ("default", "product", "lowt_min0", "lowt_min2", "steps"),
         "D": ("default", "product", "lowt_min0", "steps"),
         "E": ("default", "product", "lowt_min0", "lowt_min2", "steps"),
         "F": ("default", "log", "lowt_min0", "steps"),
         "G": ("default", "log", "lowt_min0", "lowt_min2", "steps", "steps_log")}
CASES = [(l, f) for l in LADDERS for f in FORMS[l]]
# link_thresh of the arg-max cases: at 0.3 the oracle's communities differ from the 1/2 run's of the ladder in one of the
# phases (_lowt_oracle asserts it on the CPU, before any kernel runs).  Next to a slice of 2048 columns the margin is thin:
# with k_total = 2051 or 2050 (slices (3, 2048), (2, 2048), (4, 2047)) no threshold down to 0.0004 changes a single tag at
# lt_min_deg = 0 -- every link that is tagged has a phi above 1/2 there -- which is why ladder E is (2048, 1): at k_total =
# 2049 ONE link differs.  A change to graph N or to the seed can flip that; the assertion then fails on the CPU and says so.
LOW_THRESH = 0.3
# E's slice of one column: its phi grid is sized by k_phi<1, false, false> (8 blocks of 4 wave-items per CU), which graph N
# (2 655 items) cannot fill on any device of 83 CUs or more -- no graph of N's size can.  k_phi_ksh16 and k_phi_ksh<1, ., true>
# have the same four-items-per-block loop and do loop on A, G and F (graph W: 8 482 items against 8 x 4 x 256 = 8 192 on
# 256 CUs -- a margin of 3.5 %: on a device with more than 265 CUs the precondition fails and graph W must grow); here they
# run next to the V = 32 kernels, which is what this ladder is for.
LOOP_EXEMPT = {("E", 1)}

# Tolerances: those of the two other matrices.  Flags, counts, _iter, sweeps_done and tags are exact.
# Largest relative errors measured against the oracle on an MI355X (256 CUs), over both phases, of the columns a rank of
# that tier holds -- gamma / lambda / stored mean indicators (over max(|m|, 1e-9)); profiles/r16a_ksh_matrix.md has the forms:
#   16-lane and V = 1 log (<= 64 columns): 4.3e-13 / 7.0e-14 / 1.1e-10      V = 12: 1.4e-12 / 2.6e-13 / 5.4e-11
#   V =  2: 4.7e-13 / 4.6e-14 / 1.1e-10                                      V = 16: 1.7e-12 / 1.3e-12 / 2.7e-11
#   V =  4: 6.9e-13 / 8.2e-14 / 1.1e-10                                      V = 32: 1.7e-12 / 1.3e-12 / 2.7e-11
#   V =  8: 1.4e-12 / 2.6e-13 / 2.7e-11
# (the forms agree to the digits shown but for the log form at V = 12, ladder F: 6.4e-13 / 1.1e-13; the forced product form,
# phase (b) alone: <= 1.7e-14 / 9.0e-15 / 1.8e-14; windows against the plain engine: gamma <= 2.6e-13, lambda <= 1.6e-13,
# rows <= 6.1e-15; ties: gamma <= 1.3e-13, lambda <= 2.5e-13).
# Likelihood rows, by ladder (k_total) -- every form of a ladder shows the same figure, which is the ORACLE's own error to
# the digits shown (_oracle_row_error; the device's rows agree with the extended-precision evaluation):
#   A (278) 2.4e-9   G (388) 3.3e-10   F (516) 5.9e-9   |   B (1282) 5.0e-8   C (1537) 1.6e-8   D, E (2049) 4.0e-8
TOL = R.TOL
ROWS_RTOL_WIDE = R.ROWS_RTOL_V32    # likelihood rows where k_total > 1024: the oracle's own K^2 rounding (test_gpu_rpw_matrix.py)

_records, _members, _base_bits = {}, {}, {}


def _bounds(ladder):
    return [0] + [int(x) for x in np.cumsum(LADDERS[ladder][0])]


def _family(width, log):
    """the kernels of a slice, restated from launch_ksh_phase: (family, V)"""
    v = R._layout_v(width)
    if width <= 64:
        return ("V=1 log", 1) if log else ("16-lane", 1)
    return ("64-lane", v)


def _default_log(ladder):
    return _bounds(ladder)[-1] > 700


def _runs():
    """(ladder, form name, log form?, arg-max?, steps?) of every run of CASES"""
    out = []
    for ladder, form in CASES:
        if form == "underflow":
            continue
        lowt = form.startswith("lowt")
        log = lowt or form in ("log", "steps_log") or (form in ("default", "steps") and _default_log(ladder))
        out.append((ladder, form, log, lowt, form.startswith("steps")))
    return out


def test_ladders_cover_every_instantiation():
    """the ladders and forms together reach every (kernel family, V, form), both edges of every tier among the slices"""
    reached, widths = set(), {}
    for ladder, form, log, lowt, steps in _runs():
        for w in LADDERS[ladder][0]:
            fam, v = _family(w, log)
            reached.add((fam, v, "log" if log else "product", "lowt" if lowt else "", "steps" if steps else ""))
            widths.setdefault((fam, v), set()).add(w)
    for v, (lo, hi) in TIERS.items():
        for fam in (("16-lane", "V=1 log") if v == 1 else ("64-lane",)):
            assert {lo, hi} <= widths[(fam, v)], (fam, v, sorted(widths[(fam, v)]))
    assert all(R._layout_v(lo) == v == R._layout_v(hi) and (lo == 1 or R._layout_v(lo - 1) != v) for v, (lo, hi) in TIERS.items())
    assert max(_bounds(l)[-1] for l in LADDERS) <= 2051
    have = lambda fam, v, form, lowt="", steps="": (fam, v, form, lowt, steps) in reached
    for v in (2, 4, 8, 12, 16, 32):
        assert have("64-lane", v, "log") and have("64-lane", v, "product"), v          # every V in both forms
        assert have("64-lane", v, "log", "lowt"), v                                     # the arg-max tagging
        assert have("64-lane", v, "log", "", "steps") or have("64-lane", v, "product", "", "steps"), v   # k_fin1_ksh<64, V, true>
    assert have("16-lane", 1, "product") and have("16-lane", 1, "product", "", "steps")
    assert have("V=1 log", 1, "log") and have("V=1 log", 1, "log", "lowt") and have("V=1 log", 1, "log", "", "steps")
    # ranks of different tiers in one run, the 16-lane kernels next to the 64-lane ones
    assert all(len({_family(w, False) for w in LADDERS[l][0]}) > 1 for l in LADDERS)
    assert any(min(LADDERS[l][0]) <= 64 < max(LADDERS[l][0]) for l in LADDERS)


def _planted(bounds):
    """the flag values planted at the slice edges"""
    return sorted({x for b in bounds[1:-1] for x in (b, b + 1)} | {bounds[-1]})


def _planted_nodes(bounds):
    """value -> its three nodes: majority nodes of seed_state (20 i + 12 is neither a minor node, 20 i + 5 / + 6, nor wired)"""
    return {v: [20 * (3 * j + c) + 12 for c in range(3)] for j, v in enumerate(_planted(bounds))}


def _edge_seed(bounds):
    """seed_state plus the flags at the slice edges.  Q2 adds mphi[q][v] of a flagged node's unconverged neighbour q into
    s3[v - 1]; that is nothing unless q has mass in community v, which needs a link of q whose BOTH ends have it.  So the
    two ring neighbours 20 i + 13 and 20 i + 14 of every flagged node 20 i + 12 get gamma = 30 in column v (beside their
    20..60 in column 0) and no flag: the link between them puts a share of its phi there, and the link (20 i + 12,
    20 i + 13) is a shortcut link whose Q2 term is of order 0.1 -- for v = an inner bound it crosses the slice edge."""
    def seed(n, k, lam):
        g, lam, conv = MC.seed_state(n, k, lam)
        for v, nodes in _planted_nodes(bounds).items():
            assert max(nodes) + 2 < n and not set(nodes) & set(R.WIRED)
            conv[nodes] = v
            for p in nodes:
                conv[[p + 1, p + 2]] = 0
                if v < k:
                    g[[p + 1, p + 2], v] = 30.0
        return g, lam, conv
    return seed


def _oracle_row_error(rec):
    """what the ORACLE's last likelihood row is off by (its mean over the held-out non-links, relative): the reference scores
    a non-link with a K^2 loop that adds pi_p[z] pi_q[z'] to a running sum near 1 (src/linksampling.hh:258-292); in the
    seeded state nearly all of those products are the same tiny number, every addition rounds the same way and the error
    grows like K^2 eps / 2 (tests/test_gpu_rpw_matrix.py).  Here the same sum is evaluated from the oracle's own gamma and
    lambda in extended precision, in the collapsed form (sum pi_p)(sum pi_q)(1 - eps) - sum_z pi_p[z] pi_q[z] (beta_z - eps)."""
    ld = np.longdouble
    g, lam = rec["b"]["gamma"].astype(ld), rec["b"]["lam"].astype(ld)
    pi = g / g.sum(1, keepdims=True)
    beta = lam[:, 0] / (lam[:, 0] + lam[:, 1])
    eps = ld(1e-30)
    zeros = rec["validation"][rec["validation"][:, 2] == 0]
    pp, pq = pi[zeros[:, 0]], pi[zeros[:, 1]]
    s = pp.sum(1) * pq.sum(1) * (1 - eps) - (pp * pq * (beta - eps)).sum(1)
    mean0 = np.log(np.maximum(s, ld(1e-30))).mean()
    return float(abs(ld(rec["b"]["rows"][-1, 3]) - mean0) / abs(mean0))


def _oracle(ladder, link_thresh=0.5, lt_min_deg=0):
    """the oracle's trajectory of one (ladder, link_thresh, lt_min_deg), kept while the cases of that ladder run (CASES go
    ladder by ladder), with the conditions on the seeded state asserted from the oracle alone"""
    key = (ladder, link_thresh, lt_min_deg)
    if key in _records:
        return _records[key]
    for old in [o for o in _records if o[0] != ladder]:
        del _records[old]
    bounds, size = _bounds(ladder), LADDERS[ladder][1]
    n, k = R.SIZES[size], bounds[-1]
    rec = MC.trajectory(n, R._pairs(size), k, NAT, REG, seed=_edge_seed(bounds), link_thresh=link_thresh, lt_min_deg=lt_min_deg)
    rec["items"] = R._graph_facts(size, rec["links"])
    reg = rec["b"]["counts"][NAT:]
    assert all(any(c[j] > 0 for c in reg) for j in range(3)), reg             # dense, active-set and shortcut branches
    assert reg[0][0] > 0 and reg[0][2] > 0, reg                               # dense links and shortcuts in its first sweep
    conv = rec["seed"][2]
    p, q = rec["links"].T
    for v, nodes in _planted_nodes(bounds).items():
        assert (conv[nodes] == v).all()
        one_end = ((conv[p] == v) & (conv[q] == 0)) | ((conv[q] == v) & (conv[p] == 0))
        assert one_end.sum() >= 3, (ladder, v, int(one_end.sum()))             # Q2 reads column v for each of them
        if v < k:
            # ... and finds something there: the neighbour's mean indicator in column v after the first sweep from the seed
            assert all(rec["b1"]["mphi"][x + 1, v] > 0.01 for x in nodes), (ladder, v, [rec["b1"]["mphi"][x + 1, v] for x in nodes])
    # the oracle's own rows must be good to the tolerance they are compared at (a ladder of k_total = 663 on graph W is
    # not: 1.2e-8, and every form of it then misses the 1e-8 by the same 1.2e-8 -- hence ladders A and G instead of one)
    rec["row_error"] = _oracle_row_error(rec)
    print("KSH-ORACLE ladder=%s K=%d link_thresh %.2f: the oracle's mean0 is off by %.1e" % (ladder, k, link_thresh, rec["row_error"]))
    assert rec["row_error"] < 0.8 * _tol(k)["rows_rtol"], (ladder, rec["row_error"])
    if key == (ladder, 0.5, 0):
        _members[ladder] = tuple(np.packbits(rec[ph]["member"]) for ph in "ab")
    _records[key] = rec
    return rec


def _lowt_oracle(ladder, lt_min_deg):
    """the low-threshold trajectory of a ladder, with the assertion that its communities are not those of the 1/2 run"""
    if ladder not in _members:
        _oracle(ladder)
    rec = _oracle(ladder, LOW_THRESH, lt_min_deg)
    differ = [int(np.count_nonzero(np.unpackbits(_members[ladder][i])[:rec[ph]["member"].size] != rec[ph]["member"].ravel()))
              for i, ph in enumerate("ab")]
    assert max(differ) > 0, (ladder, differ)
    return rec


def _setup(rec, n, k, link_thresh=0.5, lt_min_deg=0):
    """what KShard reads of a host_api.Setup, from the oracle's inputs"""
    return types.SimpleNamespace(n=n, k=k, links=rec["links"], validation_sorted=rec["validation"], gamma=rec["gamma0"],
                                 lam=rec["lam0"], ones=rec["ones"], ones_prob=rec["ones_prob"], eta=rec["eta"],
                                 link_thresh=link_thresh, lt_min_deg=lt_min_deg)


def _shards(rec, n, bounds, log_domain=None, **setup_kw):
    from svinet_amd.ksharded import KShard
    world = len(bounds) - 1
    setup = _setup(rec, n, bounds[-1], **setup_kw)
    shards = [KShard(setup, r, world, 0, log_domain=log_domain, bounds=bounds, use_validation_stop=False) for r in range(world)]
    assert [(s.k0, s.k1) for s in shards] == list(zip(bounds, bounds[1:]))
    return shards


def _close(shards):
    for s in shards:
        s.engine.close()


def _tol(k):
    return TOL if k <= 1024 else dict(TOL, rows_rtol=ROWS_RTOL_WIDE)


def _blocks_loop(ladder, phi_items):
    """every rank's phi grid is rpw_resident_blocks of ITS slice's layout: more items than that and its blocks loop"""
    cus = R._cus()
    for r, w in enumerate(LADDERS[ladder][0]):
        if (ladder, r) not in LOOP_EXEMPT:
            R._blocks_loop(w, phi_items, cus)


def _report(ladder, form, phase, err):
    """one line per comparison: the whole state, then gamma / lambda / indicators of every rank's own columns by its V"""
    by_rank = " ".join("w%d(V%d):%.1e/%.1e/%.1e" % ((w, R._layout_v(w)) + e) for w, e in zip(LADDERS[ladder][0], err["ranks"]))
    print("KSH-ERR ladder=%s K=%d %s %s gamma %.1e lambda %.1e rows %.1e mphi %.1e | %s"
          % (ladder, _bounds(ladder)[-1], form, phase, err["gamma"], err["lam"], err["rows"], err["mphi"], by_rank))


def _slice_seed(shards):
    """-> the seed function of MC.two_phases for column slices; the row sums cross the ranks again afterwards (marked)"""
    by_engine = {id(s.engine): s for s in shards}
    pending = []

    def seed(e, g, lam, conv):
        s = by_engine[id(e)]
        e.set_state(np.ascontiguousarray(g[:, s.k0:s.k1]), np.ascontiguousarray(lam[s.k0:s.k1]), conv)
        pending.append(e)
    return seed, pending


def _check_vrow(tag, shards, want_row, tol):
    from svinet_amd.ksharded import validation_row_virtual
    row = validation_row_virtual(shards)
    np.testing.assert_allclose(row[1:], want_row[1:], rtol=tol["rows_rtol"], atol=tol["rows_atol"], err_msg=str(tag))


def _run(rec, ladder, form, shards, steps=False):
    """both phases on the ranks of one run -> (gamma, lambda) after phase (b), put together"""
    from svinet_amd.ksharded import init_virtual, step_virtual, sweep_virtual
    k = _bounds(ladder)[-1]
    tol = _tol(k)
    seed, pending = _slice_seed(shards)
    done = [0]
    init_virtual(shards)
    _check_vrow((ladder, form, "constructor row"), shards, rec["row0"], tol)      # k_vdot_ksh<V> alone

    def sweep(m):
        if pending:
            del pending[:]
            init_virtual(shards)
        for _ in range(m):
            (step_virtual if steps else sweep_virtual)(shards, 1)
            done[0] += 1
            if done[0] == 1:                                                      # between two sweeps
                _check_vrow((ladder, form, "row between two sweeps"), shards, rec["a"]["rows"][0], tol)

    def check(phase, want):
        _report(ladder, form, phase, MC.compare_slices((ladder, form, phase), want, shards, tol))

    MC.two_phases(rec, [s.engine for s in shards], sweep, check, REG, seed=seed)
    states = [s.engine.state() for s in shards]
    _close(shards)
    return np.concatenate([st[0] for st in states], 1), np.concatenate([st[1] for st in states], 0)


def _base(ladder, rec):
    """the state after phase (b) of the default run, for the cases that show another form ran"""
    if ladder not in _base_bits:
        _base_bits.clear()
        shards = _shards(rec, R.SIZES[LADDERS[ladder][1]], _bounds(ladder))
        assert all(s.log_domain == _default_log(ladder) and s.engine.ksh_log_domain() == s.log_domain for s in shards)
        _base_bits[ladder] = _run(rec, ladder, "default", shards)
    return _base_bits[ladder]


@pytest.mark.parametrize("ladder,form", CASES, ids=["%s-%s" % c for c in CASES])
def test_form_against_oracle(ladder, form):
    """one (ladder, form) cell: the form confirmed on every handle, blocks that loop asserted for every rank, both phases
    against the oracle on every rank.  The forms of a ladder at one link_thresh share one oracle trajectory."""
    from svinet_amd import _svils
    from svinet_amd.ksharded import init_virtual, sweep_virtual
    bounds, n = _bounds(ladder), R.SIZES[LADDERS[ladder][1]]
    k = bounds[-1]
    if form.startswith("lowt"):
        min_deg = int(form[-1])
        rec = _lowt_oracle(ladder, min_deg)
        _blocks_loop(ladder, rec["items"][0])
        shards = _shards(rec, n, bounds, link_thresh=LOW_THRESH, lt_min_deg=min_deg)
        assert all(s.engine.ksh_log_domain() for s in shards)         # forced: the log-domain exchange carries the maximum
        assert all(s.buf[_svils.KSH_EARG] is not None for s in shards)
        _run(rec, ladder, form, shards)
        return
    rec = _oracle(ladder)
    _blocks_loop(ladder, rec["items"][0])
    if form == "default":
        _base_bits.pop(ladder, None)
        _base(ladder, rec)
    elif form == "log":
        assert not _default_log(ladder)
        base = _base(ladder, rec)
        shards = _shards(rec, n, bounds, log_domain=True)
        assert all(s.engine.ksh_log_domain() for s in shards)
        got = _run(rec, ladder, form, shards)
        # exp(a + b + c - max) / sum instead of e^a e^b e^c / sum: another rounding of every phi
        assert not np.array_equal(got[0], base[0])
    elif form in ("steps", "steps_log"):
        log = True if form == "steps_log" else None
        shards = _shards(rec, n, bounds, log_domain=log)
        assert all(s.engine.ksh_log_domain() == (_default_log(ladder) or form == "steps_log") for s in shards)
        for s in shards:
            s.engine.set_stochastic(batch_nodes=0, tau0=1.0, kappa=0.0)
        _run(rec, ladder, form, shards, steps=True)
    elif form == "product":
        # phase (b) alone, on fresh handles set to the seed (the natural sweeps underflow in this form: `underflow`)
        assert _default_log(ladder)
        shards = _shards(rec, n, bounds, log_domain=False)
        assert not any(s.engine.ksh_log_domain() for s in shards)
        seed, pending = _slice_seed(shards)
        for s in shards:
            seed(s.engine, *rec["seed"])
            s.engine.set_control(iter=NAT, annealing=0, write_comm=1)             # where the oracle stands after phase (a)
        init_virtual(shards)
        sweep_virtual(shards, 1)
        err = MC.compare_slices((ladder, form, "b1"), rec["b1"], shards, _tol(k), skip=NAT)
        _report(ladder, form, "b1", err)
        for s in shards:
            s.engine.set_control(iter=1500)
        sweep_virtual(shards, REG - 1)
        _report(ladder, form, "b", MC.compare_slices((ladder, form, "b"), rec["b"], shards, _tol(k), skip=NAT))
        _close(shards)
    else:
        # the natural first sweep in the forced product form: hundreds of links whose denominator is below 1e-280 (rows of
        # psi(1 / k_total) < -745 off a node's few communities) -- an error code read from the control block, not a fault
        assert form == "underflow" and _default_log(ladder)
        shards = _shards(rec, n, bounds, log_domain=False)
        assert not any(s.engine.ksh_log_domain() for s in shards)
        init_virtual(shards)
        with pytest.raises(_svils.SvilsError, match="underflowed"):
            sweep_virtual(shards, 1)       # the first host entry that looks at the control block reports it
            shards[0].engine.control()
        for s in shards:                   # every rank saw the same summed denominators
            with pytest.raises(_svils.SvilsError, match="underflowed"):
                s.engine.control()
        _close(shards)


def test_vdot_inside_an_open_step_is_refused():
    """phase VDOT reads the row sums of a finished state: inside an open mini-batch step (the step's first phase has run,
    STOP has not) svils_ksweep_phase refuses it with an argument error; between two steps it runs"""
    from oracle import oracle as O
    from svinet_amd import _svils
    from svinet_amd.ksharded import init_virtual, step_virtual, validation_row_virtual
    bounds, n = _bounds("G"), R.SIZES["N"]
    ref = O.LinkSampling(O.Network(n=n, pairs=R._pairs("N")), bounds[-1], use_validation_stop=False)
    rec = dict(links=ref.links, validation=ref.validation_sorted, gamma0=ref.gamma, lam0=ref.lam, ones=ref.net.ones,
               ones_prob=ref.ones_prob, eta=ref.eta)
    shards = _shards(rec, n, bounds)
    for s in shards:
        s.engine.set_stochastic(batch_nodes=(n + 2) // 3, tau0=4.0, kappa=0.6)
    init_virtual(shards)
    step_virtual(shards, 1)
    assert np.isfinite(validation_row_virtual(shards)).all()           # between two steps
    assert not shards[0].engine.ksh_log_domain()
    shards[0].engine.ksweep_phase(_svils.KPHASE_DEN)                    # opens the next step
    with pytest.raises(_svils.SvilsError, match="VDOT belongs between two steps") as err:
        shards[0].engine.ksweep_phase(_svils.KPHASE_VDOT)
    assert err.value.code == -1                                         # SVILS_ERR_ARG
    _close(shards)


WINDOW_CASES = [("A", None), ("G", None), ("F", None), ("X", [0, 1025, 2048])]


@pytest.mark.parametrize("ladder,bounds", WINDOW_CASES, ids=[c[0] for c in WINDOW_CASES])
def test_windows_equal_the_plain_engine(ladder, bounds):
    """windows of n / 3 nodes with damped steps on unequal slices: put together, the ranks equal svils_step on ONE plain
    handle with the same windows and step sizes (state, flags, likelihood rows, tags, _iter), as
    tests/test_gpu_ksharded.py::test_ksharded_minibatch_windows_equal_the_plain_engine does for even slices.  A plain handle
    stops at 2048 columns, so the widest case is the pair (1025, 1023) on graph N."""
    from oracle import oracle as O
    from svinet_amd.ksharded import init_virtual, step_virtual
    size = LADDERS[ladder][1] if bounds is None else "N"
    bounds = bounds or _bounds(ladder)
    n, k, steps = R.SIZES[size], bounds[-1], 7                  # two passes over the three windows and one step more
    ref = O.LinkSampling(O.Network(n=n, pairs=R._pairs(size)), k, use_validation_stop=False)
    rec = dict(links=ref.links, validation=ref.validation_sorted, gamma0=ref.gamma, lam0=ref.lam, ones=ref.net.ones,
               ones_prob=ref.ones_prob, eta=ref.eta, test_sorted=None)
    kw = dict(batch_nodes=(n + 2) // 3, tau0=4.0, kappa=0.6, node_tau0=2.0, node_kappa=0.5)
    shards = _shards(rec, n, bounds)
    assert all(s.engine.ksh_log_domain() == (k > 700) for s in shards)
    for s in shards:
        s.engine.set_stochastic(**kw)
    init_virtual(shards)
    step_virtual(shards, steps)
    plain = MC.engine_on(rec, n, k)
    plain.set_stochastic(**kw)
    plain.step(steps)
    pg, pl, pc = plain.state()
    states = [s.engine.state() for s in shards]
    g = np.concatenate([st[0] for st in states], 1)
    lam = np.concatenate([st[1] for st in states], 0)
    err = (MC.rel(g, pg), MC.rel(lam, pl))
    rows = plain.rows()
    tol = _tol(k)
    err_rows = 0.0
    for s, st in zip(shards, states):
        assert np.array_equal(st[2], pc), s.rank
        got = s.engine.rows()
        assert got.shape == rows.shape and np.array_equal(got[:, 0], rows[:, 0])
        np.testing.assert_allclose(got[:, 1:], rows[:, 1:], rtol=TOL["rows_rtol"], atol=TOL["rows_atol"])
        err_rows = max(err_rows, float(np.max(np.abs(got[:, 1:] - rows[:, 1:]) / np.abs(rows[:, 1:]))))
        assert s.engine.control().iter == steps == plain.control().iter
    print("KSH-ERR ladder=%s K=%d windows gamma %.1e lambda %.1e rows %.1e mphi 0" % (ladder, k, err[0], err[1], err_rows))
    assert err[0] < tol["state"] and err[1] < tol["state"], err
    assert np.array_equal(np.concatenate([s.engine.communities() for s in shards], 1), plain.communities())
    _close(shards)
    plain.close()


# ladder -> (tied columns, link_thresh): the tied columns lie in three slices (two where the ladder has two), the smallest
# is not the first column of its slice and, where a lane holds more than one value, not a lane's first; on A it is not on
# rank 0 (on C and E the lower of two slices is rank 0)
TIE_CASES = [("A", (30, 100, 200), 0.3), ("C", (131, 700, 1000), 0.2), ("E", (131, 1500, 2048), 0.2)]


@pytest.mark.parametrize("ladder,tied,thresh", TIE_CASES, ids=[c[0] for c in TIE_CASES])
def test_first_of_tied_maxima_across_ranks_is_tagged(ladder, tied, thresh):
    """Exact ties of a link's maximum whose columns lie on DIFFERENT ranks, built like
    tests/test_gpu_rpw_matrix.py::test_first_of_tied_maxima_is_tagged (its _tie_record, on graph N): one natural sweep,
    then gamma rows of 1.0 with the three columns `tied` at 40.0 and lambda (3, 2), then one sweep.  Every rank that holds
    a tied column publishes it (SVILS_KSH_EARG); the MIN over the ranks must leave the smallest global column, tagged on
    the rank that holds it and nowhere else."""
    from svinet_amd.ksharded import init_virtual, sweep_virtual
    bounds = _bounds(ladder)
    k, n = bounds[-1], R.SIZES["N"]
    rank_of = lambda c: int(np.searchsorted(bounds, c, side="right")) - 1
    ranks = [rank_of(c) for c in tied]
    assert len(set(ranks)) == min(3, len(bounds) - 1), ranks
    first = min(tied)
    r0 = rank_of(first)
    width, local = bounds[r0 + 1] - bounds[r0], first - bounds[r0]
    assert local != 0
    if width > 64:
        assert R._kmap_inverse(local, R._layout_v(width))[1] != 0
    if ladder == "A":
        assert r0 != 0
    t = R._tie_record(k, tied, thresh)     # (asserts on the CPU: the set of maxima does not depend on the order of additions,
    #                                         the maximum clears the threshold and stays below 1/2, only min(tied) is tagged)
    shards = _shards(t["rec"], n, bounds, link_thresh=thresh)
    init_virtual(shards)
    sweep_virtual(shards, 1)
    g, lam, conv = t["state"]
    for s in shards:
        s.engine.set_state(np.ascontiguousarray(g[:, s.k0:s.k1]), np.ascontiguousarray(lam[s.k0:s.k1]), conv)
    init_virtual(shards)
    sweep_virtual(shards, 1)
    states = [s.engine.state() for s in shards]
    for s, st in zip(shards, states):
        member = s.engine.communities()
        assert np.array_equal(member, t["member"][:, s.k0:s.k1]), s.rank
        assert member.any() == (s.rank == r0)
        assert np.array_equal(st[2], t["conv"]) and s.engine.control().iter == t["iter"]
    err = (MC.rel(np.concatenate([st[0] for st in states], 1), t["gamma"]),
           MC.rel(np.concatenate([st[1] for st in states], 0), t["lam"]))
    print("KSH-ERR ladder=%s K=%d ties b gamma %.1e lambda %.1e rows 0 mphi 0" % (ladder, k, err[0], err[1]))
    assert err[0] < TOL["state"] and err[1] < TOL["state"], err
    _close(shards)
