"""-m gpu: every instantiation of the row-per-wavefront kernels (svinet_amd/csrc/svils_device.hip, K >= 57) against the
oracle, built like tests/test_gpu_small_k_matrix.py (the machinery both share is tests/matrix_cases.py).

The K list holds both edges of every tier of pick_layout (V = 1, 2, 4, 8, 12, 16, 32 doubles per lane); the lower edge of
a tier is where its padding columns are most.  The oracle costs O(K L) per sweep, so the graphs have many nodes and few
links -- a ring, n / 4 random links, one hub with links to min(3000, n) random nodes -- plus four nodes wired to the
training degrees 32, 33, 64 and 65 (the chunk limit of a work item is 32 neighbours: one unsplit item; two, two and three
slotted items whose partial rows and tag counts the finalise pass merges).  Two sizes:

  W  8 400 nodes, ~13 100 links, K <= 512: more phi items than 32 x CUs (8 blocks of 4 waves per CU is the most a CU holds)
  N  2 600 nodes,  ~5 050 links, K >= 513: more phi items than 4 x PHI_BLOCKS_PER_CU[V] x CUs

so that the blocks of the phi launch loop over items at every K (asserted per case from chunk_row restated below; the s3
grid may hold twice the resident blocks and takes these graphs in one round).  A case is the two phases of matrix_cases
(NAT natural sweeps, REG sweeps from the seeded state), each compared with the oracle in full: gamma, lambda, converged
flags, _iter, per-sweep link counts, likelihood rows, communities and the stored mean indicators.  The oracle's own link
counts must show that phase (b) reached the dense, active-set and shortcut branches, or the case fails before any kernel
runs.

What selects a kernel is confirmed on the handle (get_option) before the sweeps:

  base         k_phi<V, false, true> (product form), k_finalize<64, V, false>, k_s3<64, V, true>, k_tail<64, V, false>
  log          SVILS_EPI_MAX_MB=0: k_phi<V, false, false>
  two_launch   SVILS_SKIP_ELOGPI=1, K <= 512: k_phi<V, false, true, 1> then <.., 2> (the state does not underflow: the redo
               launch returns at once here; tests/test_gpu_fuzz.py::test_softmax_rows_that_underflow makes it redo)
  stored_m     SVILS_DERIVE_M=0: k_s3<64, V, false> in whole sweeps
  phases       sweeps split at their exchange points
  steps        full-window unit steps: k_finalize<64, V, true>, k_tail<64, V, true>
  blocks       three node blocks, rows staged: k_finalize<64, V, false, true>, k_expand_all
  blocks_gamma three node blocks, gamma rows and packed flags exchanged after the full finalise pass: k_expand<64, V>
  link_thresh < 1/2: k_phi<V, true, false> (the arg-max form of the tagging rule)

The largest error each tier and form showed on an MI355X is recorded beside TOL below."""
import numpy as np
import pytest

import matrix_cases as MC

pytestmark = pytest.mark.gpu

# both edges of every tier of pick_layout (svinet_amd/csrc/svils_device.hip) above use_lpl's K = 56:
# whoever adds a tier there adds its two edges here
KS = [57, 64, 65, 128, 129, 256, 257, 512, 513, 768, 769, 1024, 1025, 2048]
MODE_KS = [64, 128, 256, 512, 768, 1024, 2048]      # one K per V: the upper edge of each tier
SIZES = {"W": 8400, "N": 2600}                      # nodes
NAT, REG = 2, 3                                     # sweeps of phase (a), of phase (b) (the first one before _iter is seeded)
WIRED = {100: 32, 200: 33, 300: 64, 400: 65}        # node -> its degree in the oracle's training links
CHUNK = 32                                          # neighbours per work item (svils_api.hip: ch = 32 * (64 / W), W = 64)

# Blocks of 256 threads a CU holds, k_phi<V, false, false> (the instantiation rpw_resident_blocks sizes the phi grid by)
# and k_s3<64, V, false> (the s3 grid: up to twice as many), from the compiler's kernel-resource-usage remarks for gfx950
# (Occupancy [waves/SIMD]; a block is one wave per SIMD).  The launch bounds ask for 2, 2 and 1 at V = 12, 16, 32:
#   k_phi<12,false,false>  228 VGPRs, no spill      -> 2      k_s3<64,12,false>   98 VGPRs -> 4
#   k_phi<16,false,false>  256 VGPRs, 68 spilled    -> 2      k_s3<64,16,false>  124 VGPRs -> 4
#   k_phi<32,false,false>  256 + 256 AGPRs, 128 sp. -> 1      k_s3<64,32,false>  250 VGPRs -> 2
# (the other phi forms of these V have the same occupancy; profiles/r14a_rpw_matrix.md has the remarks)
PHI_BLOCKS_PER_CU = {12: 2, 16: 2, 32: 1}

# Tolerances: those of tests/test_gpu_small_k_matrix.py (the project's bar for this graph family).  Flags, counts, _iter
# and communities are exact.
# Largest relative errors measured against the oracle on an MI355X (256 CUs), by pick_layout tier, over every form, mode
# and both phases -- gamma / lambda / likelihood rows / stored mean indicators (over max(|m|, 1e-9)):
#   V =  1 (K <=   64): 8.3e-13 / 2.3e-14 / 1.5e-10 / 8.7e-10      V = 12 (K <=  768): 6.9e-13 / 2.5e-13 / 2.3e-09 / 5.4e-11
#   V =  2 (K <=  128): 8.8e-13 / 2.8e-14 / 1.6e-10 / 4.3e-10      V = 16 (K <= 1024): 1.1e-12 / 1.7e-13 / 3.6e-09 / 5.4e-11
#   V =  4 (K <=  256): 7.3e-13 / 1.8e-13 / 2.4e-09 / 2.2e-10      V = 32 (K <= 2048): 1.3e-12 / 5.5e-13 / 2.3e-08 / 2.7e-11
#   V =  8 (K <=  512): 7.2e-13 / 1.1e-13 / 7.4e-09 / 1.1e-10
# The phi forms do not differ in this (product, log, two-launch and arg-max form agree to the digits shown but for gamma at
# V = 12 / 16: 6.1e-13 / 1.1e-12 product, 6.9e-13 / 9.7e-13 log and arg-max); the likelihood-row figure is the oracle's own
# rounding (below) and grows with K^2.
TOL = dict(state=1e-8, rows_rtol=1e-8, rows_atol=1e-13, mphi_rtol=1e-6, mphi_atol=1e-15)
# V = 32 (K = 1025..2048), likelihood rows only: the 1e-7 tests/test_gpu_fuzz.py::test_large_k_layouts grants these K.  Not the
# kernels' error but the oracle's: the reference scores a held-out non-link with a K^2 loop that adds pi_p[z] pi_q[z'] to a
# running sum near 1 (src/linksampling.hh:258-292).  In the seeded state of phase (b) all but a few of those 4.2e6 products
# are the same tiny number, so every addition rounds the same way and the error grows like K^2 eps / 2 = 4.7e-10 at
# K = 2048 instead of averaging out -- on a mean log-likelihood of -5.7e-3 that is up to 8e-8.  Against an
# extended-precision evaluation of the same pairs from the oracle's own gamma and lambda, the oracle's mean0 is off by
# 2.3e-8 at K = 2048 (2.1e-9 at K = 1024, inside the 1e-8), the collapsed K-term form k_tail uses by 2e-14.
ROWS_RTOL_V32 = 1e-7

_graphs, _records, _members, _base_bits = {}, {}, {}, {}


def _layout_v(k):
    """pick_layout restated: doubles per lane"""
    for edge, v in ((64, 1), (128, 2), (256, 4), (512, 8), (768, 12), (1024, 16)):
        if k <= edge:
            return v
    return 32


def _size(k):
    return "W" if k <= 512 else "N"


def _chunk_row(length, slotted=True):
    """chunk_row (svils_api.hip) restated -> [(neighbours, has a slot)]: a row of more than CHUNK entries is cut into
    ceil(length / CHUNK) items of nearly equal length; the phi pass gives each a slot (its partial row and tag counts)"""
    if length == 0:
        return []
    nch = (length + CHUNK - 1) // CHUNK
    if nch <= 1:
        return [(length, False)]
    base, rem = divmod(length, nch)
    return [(base + (1 if c < rem else 0), slotted) for c in range(nch)]


def _draw(n, extra):
    rng = np.random.default_rng(11)
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n], 1)
    plain = np.setdiff1d(np.arange(1, n), list(WIRED))
    rand = rng.choice(plain, size=(n // 4, 2))
    hub = np.stack([np.zeros(min(3000, n), dtype=np.int64), rng.choice(plain, size=min(3000, n))], 1)
    far = np.setdiff1d(plain, [s + d for s in WIRED for d in (-1, 1)])
    wired = [np.stack([np.full(d - 2 + extra[s], s), rng.choice(far, size=d - 2 + extra[s], replace=False)], 1)
             for s, d in WIRED.items()]
    return np.concatenate([ring, rand, hub] + wired).astype(np.int32)


def _pairs(size):
    """the graph of a size.  The random links and the hub avoid the WIRED nodes, which get their two ring links and as many
    more as their degree asks for; the oracle then holds some links out (the same ones at every K: they are drawn before
    gamma), so a wired node that lost links is given that many more until the training degrees are exact."""
    if size in _graphs:
        return _graphs[size]
    from oracle import oracle as O
    n = SIZES[size]
    extra = {s: 0 for s in WIRED}
    for _ in range(10):
        pairs = _draw(n, extra)
        deg = _degrees(n, O.LinkSampling(O.Network(n=n, pairs=pairs), 2, use_validation_stop=False).links)
        if all(deg[s] == d for s, d in WIRED.items()):
            break
        for s, d in WIRED.items():
            extra[s] += d - int(deg[s])
    _graphs[size] = pairs
    return pairs


def _degrees(n, links):
    return np.bincount(links.ravel(), minlength=n)


def _graph_facts(size, links):
    """what the graph is there for, from the oracle's training links and chunk_row restated -> (phi items, s3 items)"""
    n = SIZES[size]
    deg = _degrees(n, links)
    assert [int(deg[s]) for s in WIRED] == list(WIRED.values()), deg[list(WIRED)]
    assert _chunk_row(32) == [(32, False)] and _chunk_row(33) == [(17, True), (16, True)]
    assert _chunk_row(64) == [(32, True), (32, True)] and _chunk_row(65) == [(22, True), (22, True), (21, True)]
    assert deg[0] > 1000 and deg.min() >= 1                    # the hub: a row of dozens of slotted items
    upper = np.bincount(links.min(1), minlength=n)             # the s3 pass walks the upper half of a row
    phi_items = sum(len(_chunk_row(int(x))) for x in deg)
    s3_items = sum(len(_chunk_row(int(x), False)) for x in upper)
    assert 13000 <= links.shape[0] <= 14000 if size == "W" else 4500 <= links.shape[0] <= 5500, links.shape
    return phi_items, s3_items


def _blocks_loop(k, phi_items, cus):
    """the phi grid is one resident round of blocks (svils_api.hip: nb_a) of four wave-items each: more items than that
    and blocks loop"""
    v = _layout_v(k)
    per_cu = 8 if v <= 8 else PHI_BLOCKS_PER_CU[v]             # V <= 8: no more than 8 blocks of 4 waves fit a CU anyway
    assert phi_items > 4 * per_cu * cus, (k, v, phi_items, cus)


def _oracle(k, link_thresh=0.5, lt_min_deg=0):
    """the oracle's trajectory of one (K, link_thresh, lt_min_deg), kept while the cases of that K run (the parametrised
    lists below go K by K); the communities of every link_thresh = 0.5 run stay, packed, for the low-threshold cases"""
    key = (k, link_thresh, lt_min_deg)
    if key in _records:
        return _records[key]
    for old in [o for o in _records if o[0] != k]:
        del _records[old]
    size = _size(k)
    rec = MC.trajectory(SIZES[size], _pairs(size), k, NAT, REG, link_thresh=link_thresh, lt_min_deg=lt_min_deg)
    rec["items"] = _graph_facts(size, rec["links"])
    # the condition on the seeded state, from the oracle alone: phase (b) reached the branches it is there for
    reg = rec["b"]["counts"][NAT:]
    assert all(any(c[j] > 0 for c in reg) for j in range(3)), reg
    if k >= 129:
        assert reg[0][0] > 0 and reg[0][2] > 0, reg            # dense links and shortcuts side by side in its first sweep
    if key == (k, 0.5, 0):
        _members[k] = tuple(np.packbits(rec[ph]["member"]) for ph in "ab")
    _records[key] = rec
    return rec


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _engine(rec, k, env=None, monkeypatch=None, **kw):
    """a handle on the oracle's inputs; env: creation-time options, read from the environment by svils_create"""
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    eng = MC.engine_on(rec, SIZES[_size(k)], k, **kw)
    for name in env or {}:
        monkeypatch.delenv(name)
    return eng


def _report(k, form, phase, err):
    print("RPW-ERR V=%d K=%d %s %s gamma %.1e lambda %.1e rows %.1e mphi %.1e"
          % (_layout_v(k), k, form, phase, err["gamma"], err["lam"], err["rows"], err["mphi"]))


def _tol(k):
    return TOL if k <= 1024 else dict(TOL, rows_rtol=ROWS_RTOL_V32)


def _run(rec, k, form, eng, sweep=None):
    """both phases on one handle -> (gamma, lambda) after phase (b)"""
    def check(phase, want):
        _report(k, form, phase, MC.compare((k, form, phase), want, eng, _tol(k)))

    MC.two_phases(rec, [eng], sweep or eng.sweep, check, REG)
    g, lam, _ = eng.state()
    eng.close()
    return g, lam


def _same_bits(k, form, got, base):
    same = np.array_equal(got[0], base[0]), np.array_equal(got[1], base[1])
    print("RPW-BITS K=%d %s gamma identical=%s lambda identical=%s" % ((k, form) + same))
    return all(same)


def _base_gamma(k, rec):
    """gamma after phase (b) on the default handle (product form), for the cases that show another kernel ran"""
    if k not in _base_bits:
        _base_bits.clear()
        eng = MC.engine_on(rec, SIZES[_size(k)], k)
        assert (eng.get_option("epi_max_mb"), eng.get_option("skip_elogpi"), eng.get_option("derive_m")) == (-1, -1, 1)
        _base_bits[k] = _run(rec, k, "base", eng)
    return _base_bits[k]


FORMS = ["base", "log", "two_launch"]
MODES = ["stored_m", "phases", "steps", "blocks", "blocks_gamma"]
FORM_CASES = [(k, f) for k in KS for f in FORMS + (MODES if k in MODE_KS else []) if f != "two_launch" or k <= 512]
BLOCK_BOUNDS = {"W": [0, 5000, 7000, 8400], "N": [0, 1500, 2100, 2600]}   # the hub and the wired nodes in block 0


@pytest.mark.parametrize("k,form", FORM_CASES, ids=["K%d-%s" % c for c in FORM_CASES])
def test_form_against_oracle(k, form, monkeypatch):
    """one (K, form) cell at link_thresh = 1/2: the option that selects the form confirmed, blocks that loop asserted,
    both phases against the oracle.  All forms of a K share one oracle trajectory."""
    rec = _oracle(k)
    _blocks_loop(k, rec["items"][0], _cus())
    if form == "base":
        _base_bits.pop(k, None)
        _base_gamma(k, rec)
        return
    base = _base_gamma(k, rec)
    if form == "log":
        eng = _engine(rec, k, {"SVILS_EPI_MAX_MB": "0"}, monkeypatch)
        assert eng.get_option("epi_max_mb") == 0
        got = _run(rec, k, form, eng)
        # exp(a + b + c) instead of e^a e^b e^c: another rounding of every phi
        assert not _same_bits(k, form, got, base)
    elif form == "two_launch":
        eng = _engine(rec, k, {"SVILS_SKIP_ELOGPI": "1"}, monkeypatch)
        assert eng.get_option("skip_elogpi") == 1
        got = _run(rec, k, form, eng)
        # (the fast launch computes what the product form computes and nothing here underflows: the same bits as base)
        _same_bits(k, form, got, base)
    elif form == "stored_m":
        eng = _engine(rec, k, {"SVILS_DERIVE_M": "0"}, monkeypatch)
        assert eng.get_option("derive_m") == 0
        got = _run(rec, k, form, eng)
        # (the two forms of the mean indicators agree to the last bits of s3, which lambda[k][1] mostly absorbs: gamma
        # comes out identical at every K here, lambda at some -- nothing to assert)
        _same_bits(k, form, got, base)
    elif form == "phases":
        eng = _engine(rec, k)
        got = _run(rec, k, form, eng, MC.phase_split_sweeps(eng))
        _same_bits(k, form, got, base)          # (as stored_m: the same kernels, launched one phase at a time)
    elif form == "steps":
        eng = _engine(rec, k)
        eng.set_stochastic(batch_nodes=0, tau0=1.0, kappa=0.0)
        got = _run(rec, k, form, eng, eng.step)
        # s1 / s2 are running totals updated by (new - old) of every row: another rounding of lambda, then of gamma
        assert not _same_bits(k, form, got, base)
    else:
        _node_blocks(rec, k, form)


def _gamma_block_sweeps(shards, sync):
    """-> sweep(m): node-block sweeps that exchange the finished rows -- the full finalise pass on a rank's own rows (it
    needs the all-reduced `sum` first), then every rank's gamma rows and packed flags (SVILS_BUF_XFLAGS) copied to the
    others, whose k_expand re-derives Elogpi and the mean indicators of the rows they do not own"""
    from svinet_amd import _svils
    bounds = shards[0].bounds.astype(np.int64)

    def sweep(m):
        for _ in range(m):
            for s in shards:
                s.phase(_svils.PHASE_A)
            sync()
            MC.exchange_sum([s.kvec_a for s in shards])
            sync()
            for s in shards:
                s.phase(_svils.PHASE_B)
            sync()
            for src, s in enumerate(shards):
                lo, hi = int(bounds[src]), int(bounds[src + 1])
                for dst in shards:
                    if dst is not s:
                        dst.rows[0][lo:hi].copy_(s.rows[0][lo:hi])
                        dst.xflags[lo:hi].copy_(s.xflags[lo:hi])
            sync()
            for s in shards:
                s.phase(_svils.PHASE_EXPAND)
                s.phase(_svils.PHASE_C)
            sync()
            MC.exchange_sum([s.kvec_c for s in shards])
            sync()
            for s in shards:
                s.phase(_svils.PHASE_D)
        sync()
    return sweep


def _node_blocks(rec, k, form):
    """three node blocks on the one GPU, the exchanges done in process; a rank's phi launch covers its own rows (block 0
    has the split rows), its s3 launch a share of the links"""
    from svinet_amd.host_api import Setup
    size = _size(k)
    setup = Setup(n=SIZES[size], k=k, pairs=_pairs(size))
    assert np.array_equal(setup.links, rec["links"]) and np.array_equal(setup.gamma, rec["gamma0"])
    shards, sync = MC.node_blocks(setup, BLOCK_BOUNDS[size])
    sweep = (MC.staged_block_sweeps if form == "blocks" else _gamma_block_sweeps)(shards, sync)

    def check(phase, want):
        _report(k, form, phase, MC.compare_blocks((k, form, phase), want, shards, _tol(k)))

    MC.two_phases(rec, [s.engine for s in shards], sweep, check, REG)
    # another partition of every sum over the nodes: lambda differs in the last bits from the whole-graph handle's at
    # every K (gamma too up to K = 768; at K = 1024 and 2048 it comes out identical)
    assert not _same_bits(k, form, shards[0].engine.state()[:2], _base_gamma(k, rec))
    for s in shards:
        s.engine.close()


def _lowt_oracle(k, lt_min_deg):
    """the link_thresh = 0.3 trajectory of a K, with the assertion that its communities are not those of the 1/2 run"""
    if k not in _members:
        _oracle(k)
    rec = _oracle(k, 0.3, lt_min_deg)
    differ = [int(np.count_nonzero(np.unpackbits(_members[k][i])[:rec[ph]["member"].size] != rec[ph]["member"].ravel()))
              for i, ph in enumerate("ab")]
    assert max(differ) > 0, (k, differ)
    return rec


LOWT_CASES = [(k, 0) for k in KS] + [(k, 2) for k in MODE_KS]


@pytest.mark.parametrize("k,lt_min_deg", LOWT_CASES, ids=["K%d-min%d" % c for c in LOWT_CASES])
def test_low_link_thresh_against_oracle(k, lt_min_deg):
    """link_thresh = 0.3: several phi of a link may exceed it, the tag goes to the first strict maximum over all columns
    -- k_phi<V, true, false>, on an oracle trajectory of its own whose communities differ from the link_thresh = 1/2
    run's of this K (so the >= 1/2 kernels cannot pass for it); lt_min_deg = 2: a tag needs more than two such links"""
    rec = _lowt_oracle(k, lt_min_deg)
    _blocks_loop(k, rec["items"][0], _cus())
    eng = _engine(rec, k, link_thresh=0.3, lt_min_deg=lt_min_deg)
    _run(rec, k, "lowt_min%d" % lt_min_deg, eng)


def _kmap_inverse(k, v_total):
    """kmap (svils_devutil.h) inverted: column k -> (lane, v).  V = 1: lane k; else the double2 chunk c = k / 2 sits in
    lane c % 64 as the lane's chunk c / 64"""
    if v_total == 1:
        return k, 0
    c = k >> 1
    return c % 64, 2 * (c // 64) + (k & 1)


TIE_CASES = [(130, (5, 70, 129), 0.3), (700, (3, 130, 699), 0.25), (2048, (129, 1024, 2047), 0.2)]


def _tie_record(k, tied, thresh):
    """the oracle through the tie sequence (see the test) -> the inputs and the state after the tied sweep, checked"""
    from oracle import oracle as O
    n = SIZES["N"]
    out = {}
    for lt in (thresh, 0.5):
        ref = O.LinkSampling(O.Network(n=n, pairs=_pairs("N")), k, use_validation_stop=False, link_thresh=lt)
        rec = dict(links=ref.links, validation=ref.validation_sorted, gamma0=ref.gamma, lam0=ref.lam, ones=ref.net.ones,
                   ones_prob=ref.ones_prob, eta=ref.eta, test_sorted=None)
        assert ref.sweep() == 0 and not ref.communities().any()       # write_comm is still off on the first sweep
        g = np.ones((n, k))
        g[:, list(tied)] = 40.0
        lam = np.tile([3.0, 2.0], (k, 1))
        conv = np.zeros(n, dtype=np.uint32)
        ref.set_gamma(g); ref.set_lambda(lam); ref.set_converged(conv); ref.refresh()
        if lt != 0.5:
            # the kernel adds (Elogpi_p + Elogbeta) + Elogpi_q, the reference (Elogpi_p + Elogpi_q) + Elogbeta: the set of
            # maximal columns of every link must not depend on that, and the maximum must clear the threshold
            ep, eb = ref.elogpi, ref.elogbeta[:, 0]
            for lo in range(0, rec["links"].shape[0], 1024):
                p, q = rec["links"][lo:lo + 1024].T
                x_ref = (ep[p] + ep[q]) + eb
                x_dev = (ep[p] + eb) + ep[q]
                top_ref, top_dev = x_ref == x_ref.max(1, keepdims=True), x_dev == x_dev.max(1, keepdims=True)
                assert np.array_equal(top_ref, top_dev)
                assert (top_ref.sum(1) == 3).all() and top_ref[:, list(tied)].all()
                phi_max = 1.0 / np.exp(x_ref - x_ref.max(1, keepdims=True)).sum(1)
                assert (phi_max > lt).all() and (phi_max < 0.5).all()
        assert ref.sweep() == 0
        member = ref.communities()
        if lt == 0.5:
            assert not member.any()                                    # no phi reaches 1/2: the >= 1/2 kernels tag nothing
        else:
            linked = _degrees(n, rec["links"]) > 0
            want = np.zeros((n, k), dtype=np.uint8)
            want[linked, min(tied)] = 1
            assert np.array_equal(member, want)                        # the first of the tied maxima and nothing else
            out = dict(rec=rec, state=(g, lam, conv), gamma=ref.gamma, lam=ref.lam, conv=ref.converged, member=member,
                       iter=ref.iter)
    return out


@pytest.mark.parametrize("k,tied,thresh", TIE_CASES, ids=["K%d" % c[0] for c in TIE_CASES])
def test_first_of_tied_maxima_is_tagged(k, tied, thresh):
    """Exact ties: the first strict maximum must win on the device as it does in the reference.  One natural sweep (the
    reference writes no tags on the first sweep), then gamma rows of 1.0 with the three columns `tied` at 40.0 and lambda
    (3, 2) in every row, then one sweep at link_thresh = thresh: every link has a three-way tied maximum above the
    threshold.  In the kernel's column order the smallest tied column is never a lane's first value and the tied columns
    sit in more than one lane; at K = 130 the smallest is not in lane 0 either while another one is -- a reduction that
    takes the wrong end, the first value or the lowest lane tags another column."""
    v = _layout_v(k)
    where = [_kmap_inverse(c, v) for c in tied]
    assert where[0][1] != 0 and len({lane for lane, _ in where}) > 1, where
    if k == 130:
        assert where[0][0] != 0 and any(lane == 0 for lane, _ in where[1:]), where
    t = _tie_record(k, tied, thresh)
    eng = MC.engine_on(t["rec"], SIZES["N"], k, link_thresh=thresh)
    eng.sweep(1)
    eng.set_state(*t["state"])
    eng.sweep(1)
    g, lam, conv = eng.state()
    assert np.array_equal(eng.communities(), t["member"])
    err = (MC.rel(g, t["gamma"]), MC.rel(lam, t["lam"]))
    print("RPW-ERR V=%d K=%d ties b gamma %.1e lambda %.1e rows 0 mphi 0" % (v, k, err[0], err[1]))
    assert err[0] < TOL["state"] and err[1] < TOL["state"], err
    assert np.array_equal(conv, t["conv"]) and eng.control().iter == t["iter"]
    eng.close()
