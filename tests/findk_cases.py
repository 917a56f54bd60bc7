"""Planted states for the -findk device kernels (svinet_amd/csrc/svils_findk.hip) -- TEST INFRASTRUCTURE, not collected.

Three parts:

  * a PLAIN reference of every operation the unit runs on the device: collections.Counter, Python loops, math.fsum.
    It shares no code with tools/restate_findk.py (whole-array numpy); tests/test_findk_cases.py holds the two against
    each other, tests/test_gpu_findk_matrix.py holds the device against this one;
  * a thin ctypes wrapper over svils_findk_* (Handle);
  * builders of planted cases: stars whose leaves carry the planted slot-0 labels, so that a centre's count is known by
    construction.  ladder() holds every degree rung x label pattern and the hash collision chains in one graph; hubs(),
    tiny(n), pair_cases(), sums_graph(), groups_case() the rest.

The constants below restate the tiers of the unit; test_findk_cases.py asserts them against its source text.
"""
import collections
import ctypes as C
import decimal
import fractions
import functools
import math

import numpy as np

S = 5
NONE = 0xFFFFFFFF
SENTINEL = 65535
WAVE_MAX = 64            # training degree <= this: k_top_wave
LDS_SLOTS = 4096         # hash slots in LDS; degree <= LDS_SLOTS / 2: k_top_block<true>
SUM_CHUNK = 4096         # items per partial sum
HASH_MUL = 2654435761
FLOOR = 1e-30

RUNGS = (1, 2, 5, 6, 63, 64, 65, 66, 255, 256, 257, 2047, 2048, 2049, 4096, 4097)
PATTERNS = ("one", "k2", "k3", "k4", "k5", "k6", "distinct", "tie56", "alltied", "dominant", "big")


def bin_of(d):
    return None if d == 0 else "wave" if d <= WAVE_MAX else "lds" if d <= LDS_SLOTS // 2 else "hub"


def table_size(d):
    """slots of the hash a node of training degree d > 64 is counted in"""
    if d <= LDS_SLOTS // 2:
        return LDS_SLOTS
    T = 1
    while T < 2 * d:
        T <<= 1
    return T


def home_slot(label, T):
    return ((label * HASH_MUL) & 0xFFFFFFFF) & (T - 1)


# ----------------------------------------------------------------------------------------------------------------------
# the plain reference
# ----------------------------------------------------------------------------------------------------------------------

def ref_count(links, held, labels):
    """{node: [(label, count), ...]} over the slot-0 labels of the node's training neighbours, sorted by (-count, label);
    nodes without a training link are absent"""
    lab0 = [int(v) for v in np.asarray(labels)[:, 0].tolist()]
    nb = collections.defaultdict(list)
    for x, (p, q) in enumerate(np.asarray(links).reshape(-1, 2).tolist()):
        if held is not None and held[x]:
            continue
        nb[p].append(q)
        nb[q].append(p)
    out = {}
    for i, js in nb.items():
        c = collections.Counter(lab0[j] for j in js)
        out[i] = sorted(c.items(), key=lambda kv: (-kv[1], kv[0]))
    return out


def ref_degrees(links, held):
    deg = collections.Counter()
    for x, (p, q) in enumerate(np.asarray(links).reshape(-1, 2).tolist()):
        if held is None or not held[x]:
            deg[p] += 1
            deg[q] += 1
    return deg


def ref_top(count, n):
    """(top labels [n][5] with NONE past the distinct ones, counts [n][5], ndistinct [n]) as the device holds them"""
    lab = np.full((n, S), NONE, np.uint32)
    cnt = np.zeros((n, S), np.uint32)
    nd = np.zeros(n, np.uint32)
    for i, ranked in count.items():
        nd[i] = len(ranked)
        for j, (label, c) in enumerate(ranked[:S]):
            lab[i, j] = label
            cnt[i, j] = c
    return lab, cnt, nd


def ref_pad_requests(count):
    """rows (node, ndistinct, [labels then NONE] x 4) of the nodes with 1 .. 4 distinct labels, nodes ascending"""
    rows = []
    for i in sorted(count):
        d = len(count[i])
        if 1 <= d < S:
            rows.append((i, d, [label for label, _ in count[i]] + [NONE] * (4 - d)))
    return rows


def make_pads(count, n):
    """pads of the test's choosing: {node: [5 - ndistinct labels]}, none of them a counted label of the node (so that
    set_gamma's redraw rule never fires and a scripted draw stream reproduces them), ascending from a start of the node's own"""
    pads = {}
    for i in sorted(count):
        d = len(count[i])
        if d >= S:
            continue
        have = set(label for label, _ in count[i])
        out, x = [], (i * 48271 + 11) % n
        while len(out) < S - d:
            if x not in have:
                out.append(x)
            x = (x + 1) % n
        pads[i] = out
    return pads


def ref_apply(labels, values, count, alpha, pads):
    """set_gamma: counted slots (label, count + alpha), then the pads with 2 alpha; other nodes keep their slots"""
    labels, values = np.array(labels, dtype=np.uint32), np.array(values, dtype=np.float64)
    for i, ranked in count.items():
        d = len(ranked)
        for j in range(min(d, S)):
            labels[i, j] = ranked[j][0]
            values[i, j] = float(ranked[j][1]) + alpha
        for j in range(d, S):
            labels[i, j] = pads[i][j - d]
            values[i, j] = alpha + alpha
    return labels, values


def ref_pi(values, n, alpha):
    """estimate_all_pi: the five values summed in slot order, then (n - 5) alpha with n - 5 in uint32"""
    tail = float((n - S) & 0xFFFFFFFF) * alpha
    out = np.empty((len(values), S), np.float64)
    for i, row in enumerate(np.asarray(values).tolist()):
        s = 0.0
        for v in row:
            s += v
        s += tail
        out[i] = [v / s for v in row]
    return out


def ref_edge_sum(lp, lq, pp, pq, y):
    """the sum edge_likelihood takes the log of, floored: 5 x 5, k1 outer, products and sums one by one"""
    s = 0.0
    for k1 in range(S):
        for k2 in range(S):
            if (lp[k1] == lq[k2]) == bool(y):
                s += pp[k1] * pq[k2]
    if s < FLOOR:
        s = FLOOR
    return s


def ref_edge_ll(lp, lq, pp, pq, y):
    return math.log(ref_edge_sum(lp, lq, pp, pq, y))


def log_cr(s):
    """the correctly rounded natural logarithm of the double s (60 digits, then one rounding)"""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        return float(decimal.Decimal(s).ln())


def ref_pair_sums(labels, pi, pairs):
    """the floored sums of pairs [m][2 or 3] ((p, q) with y = 1, or (p, q, y))"""
    L, P = np.asarray(labels).tolist(), np.asarray(pi).tolist()
    out = []
    for r in np.asarray(pairs).tolist():
        p, q, y = r[0], r[1], (r[2] if len(r) > 2 else 1)
        out.append(ref_edge_sum(L[p], L[q], P[p], P[q], y))
    return out


def ref_groups(labels, pi, links, thresh, detail=False):
    """compute_and_log_groups over both directions of every link: (unlikely, {node: set of labels it is a member of});
    detail: also the (max_k, ratio, mx, sum) of every directed entry, links outer, direction inner"""
    L, P = np.asarray(labels).tolist(), np.asarray(pi).tolist()
    unlikely, member, entries = 0, collections.defaultdict(set), []
    for p, q in np.asarray(links).reshape(-1, 2).tolist():
        for i, m in ((p, q), (q, p)):
            max_k, mx, sm = SENTINEL, 0.0, 0.0
            for k1 in range(S):
                for k2 in range(S):
                    if L[i][k1] == L[m][k2]:
                        u = P[i][k1] * P[m][k2]
                        sm += u
                        if u > mx:
                            mx, max_k = u, L[i][k1]
            ratio = mx / sm if sm > 0.0 else 0.0
            entries.append((max_k, ratio, mx, sm))
            if ratio < thresh:
                unlikely += 1
                continue
            if max_k != SENTINEL:
                member[i].add(max_k)
                member[m].add(max_k)
    if detail:
        return unlikely, dict(member), entries
    return unlikely, dict(member)


def decode_masks(masks, labels):
    """{node: set of labels} from the device's 5-bit membership masks and the labels they index"""
    out = {}
    for i in np.nonzero(masks)[0].tolist():
        out[i] = set(int(labels[i, b]) for b in range(S) if int(masks[i]) >> b & 1)
    return out


def sum_bound(m, abs_sum, c):
    """|device sum - exact sum| over m terms, each within c * 2^-53 (relative) of the reference's: the depth of
    k_part_sum is 16 sequential additions per thread and 8 tree levels per chunk, then ceil(partials / 256) sequential
    additions and 8 levels in the final block; gamma_D = D u / (1 - D u) of a summation in which no term passes more
    than D additions"""
    partials = -(-m // SUM_CHUNK)
    D = 16 + 8 + -(-partials // 256) + 8
    u = 2.0 ** -53
    return (D + c) * u / (1 - (D + c) * u) * abs_sum


# ----------------------------------------------------------------------------------------------------------------------
# the device, through the C ABI
# ----------------------------------------------------------------------------------------------------------------------

class Handle:
    """svils_findk_* as the tests drive it; every call returns the ABI's return code unless it says otherwise"""

    def __init__(self, n, alpha, thresh=0.5, device=0):
        from svinet_amd import _svils
        self.lib, self._svils = _svils.load(), _svils
        self.n, self.alpha, self.thresh = n, alpha, thresh
        self.h = C.c_void_p()
        self.ok(self.lib.svils_findk_create(device, n, alpha, thresh, C.byref(self.h)))

    def ok(self, rc):
        self._svils._chk(rc)

    def error(self):
        return self.lib.svils_last_error().decode("utf-8", "replace")

    def set_graph(self, links, held=None, pairs=None):
        links = np.ascontiguousarray(links, dtype=np.uint32).reshape(-1, 2)
        held = None if held is None else np.ascontiguousarray(held, dtype=np.uint8)
        pairs = np.zeros((0, 3), np.uint32) if pairs is None else np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 3)
        return self.lib.svils_findk_set_graph(self.h, links.ctypes.data if len(links) else None, len(links),
                                              None if held is None else held.ctypes.data,
                                              pairs.ctypes.data if len(pairs) else None, len(pairs))

    def init_state(self, labels, values):
        labels = np.ascontiguousarray(labels, dtype=np.uint32)
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert labels.shape == (self.n, S) and values.shape == (self.n, S)
        return self.lib.svils_findk_init_state(self.h, labels.ctypes.data, values.ctypes.data)

    def count(self):
        """(rc, number of pad records)"""
        m = C.c_uint32(0xDEAD)
        rc = self.lib.svils_findk_count(self.h, C.byref(m))
        return rc, m.value

    def pad_requests(self, m):
        nodes, nd, lab = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros((m, 4), np.uint32)
        rc = self.lib.svils_findk_pad_requests(self.h, nodes.ctypes.data, nd.ctypes.data, lab.ctypes.data)
        return rc, nodes, nd, lab

    def apply(self, pads):
        pads = np.ascontiguousarray(pads, dtype=np.uint32).reshape(-1, 4)
        return self.lib.svils_findk_apply(self.h, pads.ctypes.data if len(pads) else None)

    def step(self, pads_of):
        """count, the pad requests, apply with pads_of[node]; returns (nodes, ndistinct, request labels)"""
        rc, m = self.count()
        self.ok(rc)
        rc, nodes, nd, lab = self.pad_requests(m)
        self.ok(rc)
        pads = np.zeros((m, 4), np.uint32)
        for x, i in enumerate(nodes.tolist()):
            p = pads_of.get(i, [])          # a node the reference does not pad: the comparison of the rows will say so
            pads[x, :len(p)] = p
        self.ok(self.apply(pads))
        return nodes, nd, lab

    def state(self):
        lab, val, pi = np.zeros((self.n, S), np.uint32), np.zeros((self.n, S)), np.zeros((self.n, S))
        self.ok(self.lib.svils_findk_get_state(self.h, lab.ctypes.data, val.ctypes.data, pi.ctypes.data))
        return lab, val, pi

    def report(self, groups=True):
        """(training_ll, held-out sums [all, y = 0, y = 1], unlikely, masks)"""
        t, hs, u = C.c_double(), np.zeros(3), C.c_uint32()
        masks = np.zeros(self.n, np.uint32)
        self.ok(self.lib.svils_findk_report(self.h, C.byref(t), hs.ctypes.data, C.byref(u) if groups else None,
                                            masks.ctypes.data if groups else None))
        return t.value, hs, (u.value if groups else None), (masks if groups else None)

    def close(self):
        if self.h:
            self.lib.svils_findk_destroy(self.h)
            self.h = C.c_void_p()


# ----------------------------------------------------------------------------------------------------------------------
# planted cases
# ----------------------------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "n alpha links held pairs labels values centres")
# centres: {name: (node, training degree the name promises)}


def _filler_state(n, seed):
    """labels (i + j) % n and values in (0.05, 3): what every node holds unless a builder plants something else"""
    rs = np.random.RandomState(seed)
    labels = ((np.arange(n)[:, None] + np.arange(S)[None, :]) % n).astype(np.uint32)
    values = 0.05 + 2.95 * rs.random_sample((n, S))
    return labels, values


def _split_unequal(d, k):
    """k counts >= 1 summing to d, about halving"""
    counts, r = [1] * k, d - k
    for i in range(k - 1):
        take = r - r // 2
        counts[i] += take
        r -= take
    counts[k - 1] += r
    return counts


N_GROUPS = 24
GROUP_BIG = 6                 # groups 0 .. 5 have a leaf for every degree of the ladder; the others 256


@functools.lru_cache(maxsize=None)
def group_labels():
    """the labels of the leaf groups.  Groups 0 .. 4 are chosen by their home slot modulo 256, which is the thread of
    k_top_block that scans the slot (in every table size): 0 and 1 belong to ONE thread (its private top 5 then holds two
    of the global five), 0, 2, 3, 4 to the four wavefronts.  1 and 4 are above 65535, 5 is 65535 itself; the labels do not
    ascend with the group number, so that count order and label order disagree."""
    def thread(label):
        return home_slot(label, LDS_SLOTS) % 256
    small = [v for v in range(900, 10, -1)]
    big = [v for v in range(131000, 90000, -1)]
    g0 = next(v for v in small if thread(v) // 64 == 0 and v < 720)
    g1 = next(v for v in big if thread(v) == thread(g0) and home_slot(v, LDS_SLOTS) != home_slot(g0, LDS_SLOTS))
    g2 = next(v for v in small if thread(v) // 64 == 1 and v < 300)
    g3 = next(v for v in small if thread(v) // 64 == 2 and v > 750)
    g4 = next(v for v in big if thread(v) // 64 == 3 and v < 120000)
    rest = [10001 + 13 * g if g % 2 else 80001 + 17 * g for g in range(GROUP_BIG, N_GROUPS)]
    return tuple([g0, g1, g2, g3, g4, SENTINEL] + rest)


def single_label(j):
    """the label of single leaf j: all different, the odd ones above 65535"""
    return 66001 + 2 * j if j % 2 else 1000 + 2 * j


def pattern_counts(name, d, r):
    """the neighbour labels of the centre (pattern name, degree d, rung number r): ({group: count}, [single leaves]),
    or None where the pattern does not fit the degree"""
    rot = lambda k: [(g + r) % k for g in range(k)]
    if name == "one":
        return {r % GROUP_BIG: d}, []
    if name in ("k2", "k3", "k4", "k5", "k6"):
        k = int(name[1])
        if d < k:
            return None
        return dict(zip(rot(k), _split_unequal(d, k))), []
    if name == "distinct":
        return {}, list(range(d))
    if name == "tie56":
        if d < 6:
            return None
        t = max(1, d // 12)
        return dict(zip(rot(6), _split_unequal(d - 2 * t, 4) + [t, t])), []
    if name == "alltied":
        ks = [k for k in (6, 5, 4, 3, 2) if d % k == 0] + [k for k in range(7, N_GROUPS + 1) if d % k == 0]
        if not ks:
            return None            # 1, or a prime above 24: the same as `one` / `distinct`
        return {g: d // ks[0] for g in range(ks[0])}, []
    if name == "dominant":
        if d < 2:
            return None
        m = min(d - 1, 37)
        return {r % GROUP_BIG: d - m}, list(range(3 * r, 3 * r + m))
    if name == "big":
        if d == 1:
            return {}, [1]
        m = min(d // 3, 20)
        rest = d - m
        groups = {1: rest} if rest < 2 else dict(zip((1, 4) if r % 2 else (4, 1), _split_unequal(rest, 2)))
        return groups, [2 * j + 1 for j in range(m)]
    raise KeyError(name)


CHAINS = (("chain_lds_1500", 1500, 175, 4096, 40), ("chain_lds_2048", 2048, 175, 4096, 40),
          ("chain_hub_2049", 2049, 4271, 8192, 20), ("chain_hub_4097", 4097, 4271, 16384, 10))


def chain_labels(first, stride, count):
    return [first + stride * j for j in range(count)]


def chain_multiplicities(d, count):
    """unequal multiplicities summing to d; two of them tie"""
    w = [1 + (j * 7) % 6 for j in range(count)]
    m = [max(1, d * v // sum(w)) for v in w]
    m[0] += d - sum(m)
    assert m[0] >= 1 and sum(m) == d
    return m


@functools.lru_cache(maxsize=None)
def ladder():
    """every rung x pattern of the degree ladder, the four collision chains and the held-out cases in one graph.
    Leaves are shared: a centre takes the first leaves of each group it needs."""
    n, alpha = 170000, 1.0 / 7.0
    labels, values = _filler_state(n, 23)
    glab = group_labels()
    at = 0
    group_leaves = []
    for g in range(N_GROUPS):
        size = RUNGS[-1] if g < GROUP_BIG else 256
        group_leaves.append(list(range(at, at + size)))
        labels[at:at + size, 0] = glab[g]
        at += size
    singles = list(range(at, at + RUNGS[-1]))
    for j, i in enumerate(singles):
        labels[i, 0] = single_label(j)
    at += len(singles)
    links, held, centres = [], [], {}
    centre_labels = (5, 70007, 9, SENTINEL, 5, 12, 131071, 9, 5, 70007)

    def centre(name, d, leaves, held_leaves=()):
        nonlocal at
        c = at
        at += 1
        labels[c, 0] = centre_labels[len(centres) % len(centre_labels)]
        for leaf in leaves:
            links.append((leaf, c))
            held.append(0)
        for leaf in held_leaves:
            links.append((leaf, c))
            held.append(1)
        assert name not in centres
        centres[name] = (c, d)
        return c

    def leaves_of(groups, single_ids):
        out = []
        for g, cnt in sorted(groups.items()):
            out += group_leaves[g][:cnt]
        return out + [singles[j] for j in single_ids]

    for r, d in enumerate(RUNGS):
        for name in PATTERNS:
            pc = pattern_counts(name, d, r)
            if pc is not None:
                centre("%s_%d" % (name, d), d, leaves_of(*pc))
    for name, d, first, stride, cnt in CHAINS:
        mult = chain_multiplicities(d, cnt)
        leaves = list(range(at, at + d))
        at += d
        x = 0
        for lab, m in zip(chain_labels(first, stride, cnt), mult):
            labels[leaves[x:x + m], 0] = lab
            x += m
        centre(name, d, leaves)
    # held-out links leave the count: total degree 65 counted as 64 (and 66 as 65, 2049 as 2048).  The held-out leaf
    # carries a label of its own: counted, it would be a third distinct label and change the pad request.
    for name, d in (("held_65_is_64", 64), ("held_66_is_65", 65), ("held_2049_is_2048", 2048)):
        lv = group_leaves[0][:d // 2] + group_leaves[2][:d - d // 2]
        centre(name, d, lv, held_leaves=[singles[7]])
    # a node whose every link is held out: no training link, it keeps its slots
    centre("all_held", 0, [], held_leaves=group_leaves[3][:2])
    assert at < n and max(int(labels[:, 0].max()), 0) < n
    pairs = [(p, q, 1) for (p, q), h in zip(links, held) if h]
    pairs += [(0, 1, 0), (2, n - 1, 0)]
    pairs.sort()
    return Case(n, alpha, np.array(links, np.uint32), np.array(held, np.uint8), np.array(pairs, np.uint32), labels, values,
                centres)


@functools.lru_cache(maxsize=None)
def hubs():
    """two hubs of training degree n - 1 (every other node), over leaves with a skewed label mix and a ring"""
    n, alpha = 6000, 0.1
    labels, values = _filler_state(n, 29)
    for j in range(n):
        labels[j, 0] = (j % 40) if j % 3 else (j % 2000)
    links = [(0, j) for j in range(1, n)] + [(1, j) for j in range(2, n)] + [(j, j + 1) for j in range(2, 400, 2)]
    centres = {"hub_a": (0, n - 1), "hub_b": (1, n - 1)}
    return Case(n, alpha, np.array(links, np.uint32), np.zeros(len(links), np.uint8), np.zeros((0, 3), np.uint32), labels,
                values, centres)


@functools.lru_cache(maxsize=None)
def tiny(n):
    """n = 2, 3, 4: (n - 5) wraps in uint32"""
    assert 2 <= n <= 4
    labels, values = _filler_state(n, 31 + n)
    links = [(i, i + 1) for i in range(n - 1)] + ([(0, 3)] if n == 4 else [])
    held = [0] * len(links)
    pairs = []
    if n == 4:
        held[1] = 1
        pairs = [(0, 2, 0), (1, 2, 1)]
    return Case(n, 0.25, np.array(links, np.uint32), np.array(held, np.uint8), np.array(pairs, np.uint32).reshape(-1, 3),
                labels, values, {})


def case_steps(case, steps=2):
    """the reference's states of `steps` count -> apply rounds: [(count, requests, pads, labels, values, pi)]"""
    key = id(case)
    if key not in _STEPS:
        out, labels, values = [], case.labels, case.values
        for _ in range(steps):
            count = ref_count(case.links, case.held, labels)
            pads = make_pads(count, case.n)
            labels, values = ref_apply(labels, values, count, case.alpha, pads)
            out.append((count, ref_pad_requests(count), pads, labels, values, ref_pi(values, case.n, case.alpha)))
        _STEPS[key] = (case, out)
    return _STEPS[key][1]


_STEPS = {}


# ---- per-pair likelihoods ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pair_cases():
    """[(name, y)] and one state: case c is the pair (2 c, 2 c + 1)"""
    rs = np.random.RandomState(37)
    cases = []

    def add(name, y, lp, lq, vp=None, vq=None):
        cases.append((name, y, lp, lq, vp if vp is not None else (0.05 + 2.95 * rs.random_sample(S)).tolist(),
                      vq if vq is not None else (0.05 + 2.95 * rs.random_sample(S)).tolist()))

    for y in (1, 0):
        add("one_match_y%d" % y, y, [1, 2, 3, 4, 5], [9, 8, 3, 7, 6])
        add("all_match_y%d" % y, y, [1, 2, 3, 4, 5], [5, 4, 3, 2, 1])
        add("disjoint_y%d" % y, y, [1, 2, 3, 4, 5], [6, 7, 8, 9, 10])           # y = 1: the floor
        add("all_one_label_y%d" % y, y, [3, 3, 3, 3, 3], [3, 3, 3, 3, 3])        # y = 0: the floor
        add("duplicates_y%d" % y, y, [3, 3, 4, 1, 1], [3, 1, 1, 3, 9])
        add("tiny_values_y%d" % y, y, [1, 2, 3, 4, 5], [1, 2, 3, 4, 5], [1e-9, 2e-12, 3e-7, 1e-10, 5e-8],
            [3e-11, 1e-9, 4e-12, 2e-8, 1e-10])
        add("below_floor_y%d" % y, y, [1, 2, 3, 4, 5], [1, 12, 13, 14, 15] if y else [1, 1, 1, 1, 1],
            [1e-14, 1., 1., 1., 1.] if y else [1., 1e-16, 1e-16, 1e-16, 1e-16], [1e-14, 1., 1., 1., 1.] if y else [1e-16] * 5)
    for x in range(24):
        lp, lq = rs.randint(0, 7, S).tolist(), rs.randint(0, 7, S).tolist()
        add("random%d_y%d" % (x, x % 2), x % 2, lp, lq)
    n = 2 * len(cases)
    labels, values = np.zeros((n, S), np.uint32), np.zeros((n, S))
    for c, (_, _, lp, lq, vp, vq) in enumerate(cases):
        labels[2 * c], labels[2 * c + 1], values[2 * c], values[2 * c + 1] = lp, lq, vp, vq
    return [(c[0], c[1]) for c in cases], n, 0.25, labels, values


# ---- sums ------------------------------------------------------------------------------------------------------------

SUM_N, SUM_CLASSES = 2048, 37
SUM_BIG_E = 256 * SUM_CHUNK + 18       # 257 partial sums: the final block's strided loop


@functools.lru_cache(maxsize=None)
def sums_state():
    """n = 2048 nodes in 37 classes (node i: class i % 37) over a pool of 12 labels, so that a term depends on the two
    classes alone; class 36 holds labels nobody else has (links with it take the floor)"""
    rs = np.random.RandomState(41)
    cl = rs.randint(0, 12, (SUM_CLASSES, S)).astype(np.uint32)
    cl[SUM_CLASSES - 1] = [100, 101, 102, 103, 104]
    cv = 0.05 + 2.95 * rs.random_sample((SUM_CLASSES, S))
    idx = np.arange(SUM_N) % SUM_CLASSES
    return cl[idx], cv[idx], 0.1


@functools.lru_cache(maxsize=None)
def _all_pairs():
    """every pair p < q of the 2048 nodes, by difference: (0, 1), (1, 2), ..., (0, 2), (1, 3), ... -- all unique"""
    out = []
    for delta in range(1, SUM_N):
        p = np.arange(SUM_N - delta, dtype=np.uint32)
        out.append(np.stack([p, p + delta], axis=1))
    return np.concatenate(out)


def sums_graph(E, H):
    """(links [E][2], held flags, held-out pairs [H][3]): unique links; the held-out list interleaves y = 0 (pairs that are
    no link) and y = 1 (links, flagged held out) irregularly, so that both selections cross the 4096-item chunk edges"""
    ap = _all_pairs()
    links = ap[:E]
    y = [((x * HASH_MUL) >> 9) & 1 for x in range(H)]
    n1 = sum(y)
    if n1 > E:
        raise ValueError("more held-out links than links")
    step = max(1, E // max(n1, 1))
    held = np.zeros(E, np.uint8)
    ones = [k * step for k in range(n1)]
    held[ones] = 1
    zeros = ap[len(ap) - (H - n1):] if H - n1 else ap[:0]
    pairs, i0, i1 = np.zeros((H, 3), np.uint32), 0, 0
    for x in range(H):
        if y[x]:
            pairs[x] = (links[ones[i1]][0], links[ones[i1]][1], 1)
            i1 += 1
        else:
            pairs[x] = (zeros[i0][0], zeros[i0][1], 0)
            i0 += 1
    return links, held, pairs


def sums_terms(labels, pi, pairs):
    """the reference's terms of pairs over the class state -- the correctly rounded log of the plain sum -- with one plain
    evaluation per (class, class, y)"""
    L, P = np.asarray(labels[:SUM_CLASSES]).tolist(), np.asarray(pi[:SUM_CLASSES]).tolist()
    memo = {}
    out = []
    for r in np.asarray(pairs).tolist():
        key = (r[0] % SUM_CLASSES, r[1] % SUM_CLASSES, r[2] if len(r) > 2 else 1)
        if key not in memo:
            memo[key] = log_cr(ref_edge_sum(L[key[0]], L[key[1]], P[key[0]], P[key[1]], key[2]))
        out.append(memo[key])
    return out


# ---- groups ----------------------------------------------------------------------------------------------------------

GROUPS_N = 65541                 # n - 5 = 2^16 and alpha = 2^-16: (n - 5) alpha = 1, and values summing to 3 give pi = v / 4
GROUPS_ALPHA = 2.0 ** -16


def _pi_of(values):
    return ref_pi(np.array([values]), GROUPS_N, GROUPS_ALPHA)[0].tolist()


@functools.lru_cache(maxsize=None)
def sharp_products():
    """a fractions.Fraction search for pi values a, b, c, d with fl(a b) == fl(c d) and a b != c d exactly: the values
    (v_i, v_m) of two nodes whose slots 0 hold (a, b) and slots 1 hold (c, d), the exact product of the slots 1 being the
    LARGER.  Candidates are m^2 - 49 = (m - 7)(m + 7) against m^2 for 30-bit m: 60-bit products, 49 units apart where
    a double keeps one in 128."""
    F = fractions.Fraction
    rs = np.random.RandomState(43)
    for _ in range(1000):
        m = int(rs.randint(1 << 29, 640000000)) | 1
        a, b, c, d = (m - 7) / 2.0 ** 31, (m + 7) / 2.0 ** 31, m / 2.0 ** 31, m / 2.0 ** 31
        vi = [4 * a, 4 * c, 0.25, 0.25, 3 - 4 * a - 4 * c - 0.5]
        vm = [4 * b, 4 * d, 0.25, 0.25, 3 - 4 * b - 4 * d - 0.5]
        if min(vi) <= 0 or min(vm) <= 0:
            continue
        pi_i, pi_m = _pi_of(vi), _pi_of(vm)
        r = pi_i[0] * pi_m[0]
        # the rounded product strictly between the two exact ones: a fused compare of either against it is decided
        if r == pi_i[1] * pi_m[1] and F(pi_i[0]) * F(pi_m[0]) < F(r) < F(pi_i[1]) * F(pi_m[1]):
            return vi, vm
    raise AssertionError("no sharp product found")


THRESH_VM = [1.0, 1.0, 0.5, 0.25, 0.25]


def threshold_values(thresh, side):
    """the values of a node i whose entry against a node of values (1, 1, 1/2, 1/4, 1/4) has max / sum one ulp below
    (side -1), equal to (0) or one ulp above (+1) thresh: a search over the last bits of one value, judged by the plain
    reference's own arithmetic.  Two shared labels reach ratios from 1/2 up; three reach below 1/2."""
    want = thresh if side == 0 else math.nextafter(thresh, 2.0 * side)
    for j in range(0, 17):
        for k in range(-256, 257):
            if thresh == 0.5:
                x = 1.0 + k * (2.0 ** -52 if k > 0 else 2.0 ** -53)
                vi = [1.0 - j * 2.0 ** -53, 0.5, x, 0.25, 0.25]    # slots 0, 1, 2 shared: products 1, 1/2, x/2 (over 16)
                shared = 3
            else:
                lo = 1.0 - thresh
                vi = [thresh + (j - 8) * math.ulp(thresh), lo + k * math.ulp(lo), 0.5, 0.75, 0.75]   # slots 0, 1 shared
                shared = 2
            pi_i, pi_m = _pi_of(vi), _pi_of(THRESH_VM)
            us = [pi_i[q] * pi_m[q] for q in range(shared)]
            sm = 0.0
            for u in us:
                sm += u
            if us[0] == max(us) and us[0] / sm == want:
                return vi, shared
    raise AssertionError("no values for ratio %r" % want)



@functools.lru_cache(maxsize=None)
def groups_case():
    """one graph (n = 65541) holding every planted groups case as a pair of nodes of its own, plus a hub.  Returns
    (links, labels, values, named: {name: (i, m)})."""
    n = GROUPS_N
    labels, values = _filler_state(n, 47)
    values[:] = [1.0, 0.5, 0.5, 0.5, 0.5]
    at = [10]
    links, named = [], {}
    fresh = [20000]

    def private(k):
        out = list(range(fresh[0], fresh[0] + k))
        fresh[0] += k
        return out

    def pair(name, li, lm, vi, vm):
        i, m = at[0], at[0] + 1
        at[0] += 2
        labels[i], labels[m], values[i], values[m] = li, lm, vi, vm
        links.append((i, m))
        named[name] = (i, m)

    A, B, Cc = 100, 200, 300
    x = private(12)
    # exact tie of u: A gives 3/16 x 1/8, B gives 1/8 x 3/16; A is the first in both nodes, so both directions keep A
    pair("tie", [A, B, x[0], x[1], x[2]], [A, B, x[3], x[4], x[5]], [0.75, 0.5, 0.5, 0.5, 0.75], [0.5, 0.75, 0.5, 0.5, 0.75])
    vi, vm = sharp_products()
    x = private(6)
    pair("sharp_second_larger", [A, B, x[0], x[1], x[2]], [A, B, x[3], x[4], x[5]], vi, vm)
    pair("sharp_first_larger", [B, A, x[0], x[1], x[2]], [B, A, x[3], x[4], x[5]], [vi[1], vi[0]] + vi[2:], [vm[1], vm[0]] + vm[2:])
    x = private(8)
    pair("sentinel_wins", [SENTINEL, x[0], x[1], x[2], x[3]], [x[4], SENTINEL, x[5], x[6], x[7]], [2.0, 0.25, 0.25, 0.25, 0.25],
         [0.25, 2.0, 0.25, 0.25, 0.25])
    # 65535 shared but a larger product elsewhere: an ordinary member of A
    pair("sentinel_loses", [SENTINEL, A, x[1], x[2], x[3]], [A, SENTINEL, x[5], x[6], x[7]], [0.5, 1.5, 0.25, 0.5, 0.25],
         [1.5, 0.5, 0.25, 0.5, 0.25])
    x = private(10)
    pair("sum_zero", x[:5], x[5:], [1.0, 0.5, 0.5, 0.5, 0.5], [1.0, 0.5, 0.5, 0.5, 0.5])
    for thresh in (0.5, 0.9):
        for side in (-1, 0, 1):
            vi, shared = threshold_values(thresh, side)
            x = private(10)
            li = [A, B, Cc][:shared] + x[:S - shared]
            lm = [A, B, Cc][:shared] + x[5:10 - shared]
            pair("thresh_%g_%+d" % (thresh, side), li, lm, vi, THRESH_VM)
    # a member through two slots: its slot 0 wins against one neighbour, its slot 2 against the other
    x = private(12)
    i = at[0]
    at[0] += 3
    labels[i], values[i] = [A, x[0], B, x[1], x[2]], [1.0, 0.5, 1.0, 0.25, 0.25]
    labels[i + 1], values[i + 1] = [A, x[3], x[4], x[5], x[6]], [1.0, 0.5, 0.5, 0.5, 0.5]
    labels[i + 2], values[i + 2] = [x[7], x[8], x[9], B, x[10]], [0.5, 0.5, 0.5, 1.0, 0.5]
    links += [(i, i + 1), (i, i + 2)]
    named["two_slots"] = (i, i + 1)
    # a hub whose every link sets bit 2 of its mask (and bit 0 of the leaf's)
    hub = at[0]
    at[0] += 1
    nleaf = 5000
    x = private(4)
    labels[hub], values[hub] = [x[0], x[1], Cc, x[2], x[3]], [0.25, 0.25, 2.0, 0.25, 0.25]
    leaves = np.arange(at[0], at[0] + nleaf)
    at[0] += nleaf
    labels[leaves, 0] = Cc
    labels[leaves, 1:] = (30000 + 4 * np.arange(nleaf)[:, None] + np.arange(4)[None, :])
    values[leaves] = [1.0, 0.5, 0.5, 0.5, 0.5]
    links += [(hub, int(leaf)) for leaf in leaves]
    named["hub"] = (hub, int(leaves[0]))
    assert at[0] < 20000 and fresh[0] < 30000
    return np.array(links, np.uint32), labels, values, named
