"""-m gpu: the neighbourhood baselines of link ranks (svils_nbr_score / svils_nbr_rank, -adamic-adar).

The reference is a restatement written here from the definition: Python sets for the neighbourhoods, the weight of a
common neighbour z from its training degree d -- 1.0 (CN), 1.0 / math.log(d) (AA), 1.0 / d (RA) -- and Python-float adds
over sorted(N(p) & N(q)).  The library builds its weights on the host with the same two expressions and adds them in
ascending z, so scores are compared BITWISE, `common` exactly, and above / tied / ncand exactly against counts the
restatement makes from its own scores over all n candidates (every node but p, p's training neighbours and q)."""
import glob
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pair_cases import _bits, _lfr_setup, _random_pairs, _same, _state_bits

pytestmark = pytest.mark.gpu

SVINET = os.path.join(ROOT, "svinet_amd", "bin", "svinet")
CN, AA, RA = 0, 1, 2
MEASURES = (CN, AA, RA)


def _weight(measure, d):
    if d < 2:
        return 0.0
    return 1.0 if measure == CN else 1.0 / math.log(d) if measure == AA else 1.0 / d


class Restatement:
    def __init__(self, n, links):
        self.n = n
        self.nb = [set() for _ in range(n)]
        for p, q in np.asarray(links).tolist():
            self.nb[p].add(q)
            self.nb[q].add(p)
        self.w = {m: [_weight(m, len(x)) for x in self.nb] for m in MEASURES}
        self._rows = {}

    def score(self, measure, p, q):
        w = self.w[measure]
        z = sorted(self.nb[p] & self.nb[q])
        s = 0.0
        for x in z:
            s += w[x]
        return s, len(z)

    def row(self, measure, p):
        """the score of (p, c) for every c != p (None at p), computed once per (measure, p)"""
        key = (measure, p)
        if key not in self._rows:
            self._rows[key] = [None if c == p else self.score(measure, p, c)[0] for c in range(self.n)]
        return self._rows[key]

    def rank(self, measure, p, q):
        row = self.row(measure, p)
        s = row[q]
        above = tied = ncand = 0
        for c in range(self.n):
            if c == p or c == q or c in self.nb[p]:
                continue
            ncand += 1
            above += row[c] > s
            tied += row[c] == s
        return above, tied, ncand, s

    def check_scores(self, eng, pairs):
        for m in MEASURES:
            score, common = eng.nbr_score(m, pairs)
            want = [self.score(m, p, q) for p, q in pairs.tolist()]
            assert np.array_equal(score.view(np.uint64), np.array([w[0] for w in want]).view(np.uint64)), m
            assert np.array_equal(common, [w[1] for w in want]), m
            if m == CN:
                assert np.array_equal(score, common.astype(np.float64))

    def check_ranks(self, eng, pairs, measures=MEASURES):
        for m in measures:
            above, tied, ncand, score = eng.nbr_rank(m, pairs)
            want = np.array([self.rank(m, p, q) for p, q in pairs.tolist()], dtype=object)
            assert np.array_equal(above, want[:, 0].astype(np.int64)), m
            assert np.array_equal(tied, want[:, 1].astype(np.int64)), m
            assert np.array_equal(ncand, want[:, 2].astype(np.int64)), m
            assert np.array_equal(score.view(np.uint64), want[:, 3].astype(np.float64).view(np.uint64)), m
            assert np.array_equal(score.view(np.uint64), eng.nbr_score(m, pairs)[0].view(np.uint64)), m


def _random_links(rng, n, m):
    a = rng.integers(0, n, size=3 * m)
    b = rng.integers(0, n, size=3 * m)
    e = np.stack([np.minimum(a, b), np.maximum(a, b)], 1)
    e = e[e[:, 0] != e[:, 1]]
    e = np.unique(e, axis=0)
    e = e[rng.permutation(len(e))[:m]]
    return np.ascontiguousarray(e[np.lexsort((e[:, 1], e[:, 0]))], dtype=np.uint32)


def _graph_engine(n, links, k=2):
    """a handle with a graph and NO state"""
    from svinet_amd import _svils
    eng = _svils.Engine(n, k, ones=len(links), ones_prob=len(links) / (n * (n - 1) / 2), use_validation_stop=False)
    eng.set_graph(links)
    return eng


def _both(pairs):
    pairs = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    return np.ascontiguousarray(np.stack([pairs, pairs[:, ::-1]], 1).reshape(-1, 2))   # p -> q, q -> p, ...


@pytest.fixture(scope="module")
def small():
    """n = 300, 1500 links among the nodes 0 .. 298: node 299 has degree 0"""
    n = 300
    links = _random_links(np.random.default_rng(5), n - 1, 1500)
    assert len(links) == 1500
    return n, links, Restatement(n, links), _graph_engine(n, links)


@pytest.fixture(scope="module")
def hubbed():
    """n = 3000, 9000 links, 700 of them at the hub 1500 (ids 0 and n - 1 among its neighbours): a row of eleven 64-entry
    chunks, searched over ten levels"""
    n, hub = 3000, 1500
    rng = np.random.default_rng(6)
    others = sorted({0, n - 1} | set(rng.choice(np.setdiff1d(np.arange(n), [hub]), size=698, replace=False).tolist()))
    extra = np.array([(min(hub, x), max(hub, x)) for x in others], dtype=np.uint32)
    e = np.unique(np.concatenate([_random_links(rng, n, 8400), extra]), axis=0)
    links = np.ascontiguousarray(e[np.lexsort((e[:, 1], e[:, 0]))], dtype=np.uint32)
    r = Restatement(n, links)
    assert 8900 <= len(links) <= 9100 and 690 <= len(r.nb[hub]) <= 720
    return n, hub, links, r, _graph_engine(n, links)


LIST_CAP = 2048      # svils_nbr.hip: candidates a block lists in LDS before its wavefronts score them


@pytest.fixture(scope="module")
def big_hub():
    """n = 8000, 32000 random links and a hub of degree 1500: more than twice LIST_CAP candidates two steps from the hub that
    are not its neighbours, so the list of a query from the hub is drained several times in the middle of the walk"""
    n, hub = 8000, 4000
    rng = np.random.default_rng(9)
    others = rng.choice(np.setdiff1d(np.arange(n), [hub]), size=1500, replace=False).tolist()
    extra = np.array([(min(hub, x), max(hub, x)) for x in others], dtype=np.uint32)
    e = np.unique(np.concatenate([_random_links(rng, n, 32000), extra]), axis=0)
    links = np.ascontiguousarray(e[np.lexsort((e[:, 1], e[:, 0]))], dtype=np.uint32)
    r = Restatement(n, links)
    listed = set().union(*(r.nb[z] for z in r.nb[hub])) - r.nb[hub] - {hub}
    assert len(r.nb[hub]) >= 1500 and len(listed) > 2 * LIST_CAP + 256, (len(r.nb[hub]), len(listed))
    return n, hub, links, r, _graph_engine(n, links)


def _disconnected_pairs(r, rng, count):
    """pairs without a common neighbour"""
    out = []
    while len(out) < count:
        p, q = rng.choice(r.n, size=2, replace=False).tolist()
        if not (r.nb[p] & r.nb[q]):
            out.append((p, q))
    return out


def test_small_graph_every_kind_of_pair(small):
    n, links, r, eng = small
    rng = np.random.default_rng(1)
    lone = n - 1
    assert not r.nb[lone]
    pairs = _both(np.concatenate([_random_pairs(rng, n - 1, 60), links[:20].astype(np.uint32),      # random pairs, training links
                                  np.array(_disconnected_pairs(r, rng, 10), dtype=np.uint32),       # no common neighbour
                                  np.array([[lone, 0], [lone, 17]], dtype=np.uint32)]))             # a node of degree 0
    r.check_scores(eng, pairs)
    r.check_ranks(eng, pairs)
    above, tied, ncand, score = eng.nbr_rank(AA, np.array([[lone, 0]], dtype=np.uint32))
    assert (above[0], tied[0], ncand[0], score[0]) == (0, n - 2, n - 2, 0.0)       # every candidate ties at 0
    p, q = _disconnected_pairs(r, rng, 1)[0]
    above, tied, ncand, score = eng.nbr_rank(CN, np.array([[p, q]], dtype=np.uint32))
    zero = sum(1 for c in range(n) if c not in (p, q) and c not in r.nb[p] and not (r.nb[p] & r.nb[c]))
    assert score[0] == 0.0 and tied[0] == zero and above[0] == ncand[0] - zero
    a, b = links[0].tolist()                                                       # q a training neighbour of p
    nc = eng.nbr_rank(RA, np.array([[a, b]], dtype=np.uint32))[2][0]
    assert nc == n - 1 - len(r.nb[a])


def test_hub_as_p_as_q_and_as_common_neighbour(hubbed):
    n, hub, links, r, eng = hubbed
    rng = np.random.default_rng(2)
    hn = sorted(r.nb[hub])
    strangers = [x for x in rng.permutation(n).tolist() if x != hub and x not in r.nb[hub]][:6]
    with_hub = [(hub, x) for x in [0, n - 1, hn[1], hn[350]] + strangers]          # the hub as p and (reversed) as q
    via_hub = [(hn[i], hn[j]) for i, j in ((0, 1), (5, 600), (100, 699), (64, 65))]   # the hub as a common neighbour
    assert all(hub in (r.nb[a] & r.nb[b]) for a, b in via_hub)
    pairs = _both(np.array(with_hub + via_hub + _random_pairs(rng, n, 10).tolist(), dtype=np.uint32))
    r.check_scores(eng, pairs)
    r.check_ranks(eng, pairs)
    assert eng.nbr_score(CN, np.array([[hub, strangers[0]]]))[1][0] == len(r.nb[hub] & r.nb[strangers[0]])


def test_a_query_whose_candidates_overflow_the_list(big_hub):
    """the hub as p: its listed candidates are scored in several drains, and the counters, the list and the claimed bits
    carry over from one to the next"""
    n, hub, links, r, eng = big_hub
    rng = np.random.default_rng(4)
    hn = sorted(r.nb[hub])
    strangers = [x for x in rng.permutation(n).tolist() if x != hub and x not in r.nb[hub]][:5]
    lonely = [x for x in strangers if not (r.nb[x] & r.nb[hub])][:1]             # s == 0 where one is found: the unseen tie
    pairs = _both(np.array([(hub, x) for x in [hn[0], hn[700]] + strangers + lonely], dtype=np.uint32))
    pairs = np.concatenate([pairs, pairs[:4]])                                    # the hub again, behind other queries
    r.check_scores(eng, pairs)
    r.check_ranks(eng, pairs)
    whole = _bits(eng.nbr_rank(AA, pairs))
    for a, b in zip(whole, _bits(eng.nbr_rank(AA, pairs[::-1]))):
        assert np.array_equal(a, b[::-1])


def test_a_pair_does_not_depend_on_the_call_it_is_in(small):
    """more directed pairs than the kernel has workgroups (four per CU): every workgroup serves several pairs from one
    bitmap, so a bit left behind by one pair shows in the next"""
    n, links, r, eng = small
    import torch
    blocks = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    pairs = _both(_random_pairs(np.random.default_rng(3), n, blocks // 2 + 150))
    assert len(pairs) > blocks
    whole = _bits(eng.nbr_rank(AA, pairs))
    r.check_ranks(eng, pairs[:200], measures=(AA,))
    back = _bits(eng.nbr_rank(AA, pairs[::-1]))
    for a, b in zip(whole, back):
        assert np.array_equal(a, b[::-1])
    single = [_bits(eng.nbr_rank(AA, pairs[i:i + 1])) for i in range(len(pairs))]
    for j, a in enumerate(whole):
        assert np.array_equal(a, np.concatenate([s[j] for s in single]))
    for a, b in zip(whole, _bits(eng.nbr_rank(AA, pairs))):
        assert np.array_equal(a, b)
    for m in (CN, RA):                                    # another measure leaves the first one's table alone
        eng.nbr_rank(m, pairs[:10])
    for a, b in zip(whole, _bits(eng.nbr_rank(AA, pairs))):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("which", ["small", "hubbed"])
def test_full_rows_agree_with_the_pair_scores(which, request):
    """for a few p: the counts made from svils_nbr_score(p, c) over all c are svils_nbr_rank's"""
    fx = request.getfixturevalue(which)
    n, r, eng = fx[0], fx[-2], fx[-1]
    ps = [0, 7, n - 1] + ([fx[1]] if which == "hubbed" else [])
    for m in MEASURES:
        for p in ps:
            cs = np.array([c for c in range(n) if c != p], dtype=np.uint32)
            row = np.stack([np.full(len(cs), p, dtype=np.uint32), cs], 1)
            score = eng.nbr_score(m, row)[0]
            cand = np.array([c not in r.nb[p] for c in cs.tolist()])
            qs = cs[:: max(1, len(cs) // 40)]
            above, tied, ncand, s = eng.nbr_rank(m, np.stack([np.full(len(qs), p, dtype=np.uint32), qs], 1))
            for i, q in enumerate(qs.tolist()):
                sq = score[cs == q][0]
                others = cand & (cs != q)
                assert s[i] == sq
                assert (above[i], tied[i], ncand[i]) == (np.sum(score[others] > sq), np.sum(score[others] == sq), np.sum(others))


def test_arguments_and_null_outputs(small):
    from svinet_amd import _svils
    n, links, r, eng = small
    lib = _svils.load()
    pairs = _both(_random_pairs(np.random.default_rng(8), n, 5))
    for bad in ([[4, 4]], [[0, n]], [[n, 0]]):
        for call in (eng.nbr_score, eng.nbr_rank):
            with pytest.raises(_svils.SvilsError) as ei:
                call(AA, bad)
            assert ei.value.code == -1
    for measure in (3, -1):
        for call in (eng.nbr_score, eng.nbr_rank):
            with pytest.raises(_svils.SvilsError) as ei:
                call(measure, pairs)
            assert ei.value.code == -1 and "measure" in str(ei.value)
    assert lib.svils_nbr_score(eng._h, AA, pairs.ctypes.data, len(pairs), None, None) == 0
    assert lib.svils_nbr_rank(eng._h, AA, pairs.ctypes.data, len(pairs), None, None, None, None) == 0
    only = np.zeros(len(pairs), dtype=np.uint32)
    assert lib.svils_nbr_rank(eng._h, AA, pairs.ctypes.data, len(pairs), None, only.ctypes.data, None, None) == 0
    assert np.array_equal(only, eng.nbr_rank(AA, pairs)[1])
    assert lib.svils_nbr_rank(eng._h, AA, None, 0, None, None, None, None) == 0
    assert all(len(x) == 0 for x in eng.nbr_rank(AA, np.zeros((0, 2), dtype=np.uint32)))
    bare = _svils.Engine(n, 2, ones=len(links), ones_prob=0.01)
    with pytest.raises(_svils.SvilsError) as ei:
        bare.nbr_score(AA, pairs)
    assert ei.value.code == -1 and "graph" in str(ei.value)


def test_the_calls_do_not_disturb_the_sweeps(graph_files):
    s = _lfr_setup(graph_files)
    a, b = s.engine(use_validation_stop=False), s.engine(use_validation_stop=False)
    a.sweep(10)
    before = _state_bits(a)
    v1 = s.validation_accept[s.validation_accept[:, 2] == 1][:, :2]
    pairs = _both(v1)
    r = Restatement(s.n, s.links)
    r.check_scores(a, pairs[:40])
    r.check_ranks(a, pairs[:40], measures=(AA,))
    for m in MEASURES:
        a.nbr_rank(m, pairs)
    _same(before, _state_bits(a))
    a.sweep(10)
    b.sweep(10)
    b.sweep(10)
    _same(_state_bits(a), _state_bits(b))


def test_refusals(graph_files):
    from svinet_amd import _svils
    s = _lfr_setup(graph_files)
    ksh = _svils.Engine(s.n, 28, ones=s.ones, ones_prob=s.ones_prob, eta=s.eta, use_validation_stop=False, k_slice=(0, 28))
    ksh.set_graph(s.links)
    block = s.engine(use_validation_stop=False, node_block=(250, 700))
    for eng, needle in ((ksh, "K-sharded"), (block, "node-block")):
        for call, name in ((eng.nbr_score, "svils_nbr_score"), (eng.nbr_rank, "svils_nbr_rank")):
            with pytest.raises(_svils.SvilsError) as ei:
                call(AA, [[0, 1]])
            assert ei.value.code == -4 and needle in str(ei.value) and name in str(ei.value)


def _summary(above, tied, ncand):
    """the columns of link-ranks-summary.txt, from the definitions: sequential double sums in the given order"""
    auc = mrr = chance = 0.0
    h = [0, 0, 0]
    for a, t, c in zip(above, tied, ncand):
        mid = a + 0.5 * t
        auc += 1.0 - mid / c
        mrr += 1.0 / (mid + 1.0)
        chance += 10.0 / c
        for j, lim in enumerate((1, 10, 100)):
            h[j] += a + t < lim
    m = float(len(above)) if len(above) else 1.0
    return [len(above), auc / m, mrr / m, h[0] / m, h[1] / m, h[2] / m, chance / m]


@pytest.mark.parametrize("graph,n,k", [("assort", 75, 4), ("lfr", 1000, 28)])
def test_cli_baseline_files(graph_files, tmp_path, graph, n, k):
    from svinet_amd.host_api import Setup
    s = Setup(graph_files[graph], n, k)
    rng = np.random.default_rng(2)
    pp = [(s.seq2id[p], s.seq2id[q]) for p, q, _ in s.validation_sorted[:30]]
    pp += [(s.seq2id[p], s.seq2id[q]) for p, q in s.links[:10]]          # training links: y = 1, not in the summary
    for _ in range(20):
        p, q = rng.choice(s.n, size=2, replace=False)
        pp.append((s.seq2id[p], s.seq2id[q]))
    f = tmp_path / "pairs.txt"
    f.write_text("".join("%d\t%d\n" % x for x in pp))

    def run(sub, flags):
        (tmp_path / sub).mkdir()
        r = subprocess.run([SVINET, "-file", graph_files[graph], "-n", str(n), "-k", str(k), "-link-sampling", "-no-stop",
                            "-max-iterations", "20"] + flags, cwd=str(tmp_path / sub), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=900)
        assert r.returncode == 0, r.stderr
        d = glob.glob(str(tmp_path / sub / ("n%d-k%d-*" % (n, k))))
        assert len(d) == 1
        return d[0]

    flags = ["-rank-heldout", "-rank-pairs", str(f), "-predict-pairs", str(f)]
    d = run("with", flags + ["-adamic-adar"])
    plain = run("without", flags)
    for name in ("link-ranks-summary.txt", "heldout-ranks.txt", "link-ranks.txt", "link-prob.txt", "gamma.txt"):
        assert open(os.path.join(d, name), "rb").read() == open(os.path.join(plain, name), "rb").read(), name
    for name in ("link-nbr.txt", "link-ranks-aa.txt", "heldout-ranks-aa.txt", "link-ranks-baselines.txt"):
        assert not os.path.exists(os.path.join(plain, name))

    ext = np.loadtxt(os.path.join(d, "gamma.txt"))[:, 1].astype(np.int64)
    seq = {int(e): i for i, e in enumerate(ext)}
    edges = set()
    for line in open(graph_files[graph]):
        a = line.split()
        if len(a) >= 2 and not a[0].startswith("#") and a[0] != a[1]:      # the network drops a node's link to itself
            edges.add((int(a[0]), int(a[1])))
            edges.add((int(a[1]), int(a[0])))
    val = np.loadtxt(os.path.join(d, "validation-edges.txt"), dtype=np.int64).reshape(-1, 3)
    held = {(int(a), int(b)) for a, b, _ in val} | {(int(b), int(a)) for a, b, _ in val}
    train = sorted({(min(seq[a], seq[b]), max(seq[a], seq[b])) for a, b in edges if (a, b) not in held})
    r = Restatement(len(ext), train)

    rows = [l.split("\t") for l in open(os.path.join(d, "link-nbr.txt")).read().splitlines()]
    assert len(rows) == len(pp)
    for (a, b), row in zip(pp, rows):
        sc, common = r.score(AA, seq[a], seq[b])
        assert row == [str(a), str(b), "1" if (a, b) in edges else "0", str(common), "%.9e" % sc], row

    def check(name, model_name, want_pairs):
        """-> the restatement's (above, tied, ncand) per measure over the directed pairs the summary counts"""
        rows = [l.split("\t") for l in open(os.path.join(d, name)).read().splitlines()]
        model = [l.split("\t") for l in open(os.path.join(d, model_name)).read().splitlines()]
        assert len(rows) == len(want_pairs) == len(model) and all(len(x) == 8 for x in rows)
        counted = {m: [] for m in MEASURES}
        for (a, b), row, mrow in zip(want_pairs, rows, model):
            y = 1 if (a, b) in edges else 0
            assert row[:3] == [str(a), str(b), str(y)] == mrow[:3]
            assert row[3] == "%.9e" % r.score(AA, seq[a], seq[b])[0]
            for (p, q), mid, nc, mnc in (((seq[a], seq[b]), row[4], row[5], mrow[5]), ((seq[b], seq[a]), row[6], row[7], mrow[7])):
                above, tied, ncand, _ = r.rank(AA, p, q)
                assert (mid, nc) == ("%.3f" % (above + 0.5 * tied + 1.0), str(ncand)) and nc == mnc
                if y == 1 and (a, b) in held and ncand:
                    for m in MEASURES:
                        counted[m].append(r.rank(m, p, q)[:3])
        return counted

    check("link-ranks-aa.txt", "link-ranks.txt", pp)
    v1 = [(int(a), int(b)) for a, b, y in val if y == 1]
    assert len(v1) > 0
    counted = check("heldout-ranks-aa.txt", "heldout-ranks.txt", v1)        # both flags: the summaries are the held-out file's
    lines = [l.split("\t") for l in open(os.path.join(d, "link-ranks-baselines.txt")).read().splitlines()]
    assert lines[0] == ["measure", "pairs", "auc", "mrr", "hits1", "hits10", "hits100", "chance10"]
    assert [l[0] for l in lines[1:]] == ["model", "cn", "aa", "ra"]
    summary = open(os.path.join(d, "link-ranks-summary.txt")).read().splitlines()
    assert "\t".join(lines[1][1:]) == summary[1] and "\t".join(lines[0][1:]) == summary[0]
    for line, m in zip(lines[2:], MEASURES):
        want = _summary(*zip(*counted[m])) if counted[m] else _summary([], [], [])
        assert int(line[1]) == want[0] == int(lines[1][1]) > 0
        assert [float(x) for x in line[2:]] == want[1:], (line, want)       # the same sums in the same order: the same doubles
        print("%s K = %d, %s: %s" % (graph, k, line[0], " ".join(line[1:])))
    print("%s K = %d, model: %s" % (graph, k, " ".join(lines[1][1:])))
