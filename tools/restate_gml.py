"""An INDEPENDENT numpy restatement of `svinet -gml` / `-lcstats` (MMSBGen::gml / get_lc_stats, src/mmsbgen.cc:181-193,
230-285, 418-499, 700-729, 911-961) -- TEST INFRASTRUCTURE.  Written from the reference text, not from
svinet_amd/host/lcstats.cc or svils_lc.hip.  Every sum the reference takes in k order is taken here in k order too, one
column at a time over all rows (never np.sum, which sums pairwise); the arg-maxes are the reference's "first strict
maximum, starting from 0" scans, column by column.  Counts come from np.add.at / np.unique instead of std::map walks.

    python tools/restate_gml.py <edge list> <n> <k> <dir with gamma.txt, lambda.txt> <outdir> [--lcstats]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from restate_findk import read_graph  # noqa: E402  (Network::read)


def load_model(d, n, k):
    """gamma.txt ("seq id g0 .. gK-1" rows) and lambda.txt ("k l0 l1" rows); returns gamma [n][k], ids [n], lam [k][2]"""
    g = np.loadtxt(os.path.join(d, "gamma.txt"), dtype=np.float64, ndmin=2)
    lam = np.loadtxt(os.path.join(d, "lambda.txt"), dtype=np.float64, ndmin=2)
    if g.shape[0] != n or g.shape[1] < k + 2 or lam.shape[0] != k:
        raise ValueError("model shape %s / %s does not fit n = %d, k = %d" % (g.shape, lam.shape, n, k))
    return g[:, 2:k + 2].copy(), g[:, 1].astype(np.int64), lam[:, 1:3].copy()


def seq_sum(cols):
    """sum over the columns of a [m][k] array in k order"""
    s = np.zeros(cols.shape[0])
    for c in range(cols.shape[1]):
        s = s + cols[:, c]
    return s


def first_strict_max(cols):
    """(max, index) of every row: the first k with v > max, max starting from 0 (index 0 when nothing beats 0)"""
    u = np.zeros(cols.shape[0])
    idx = np.zeros(cols.shape[0], np.int64)
    for c in range(cols.shape[1]):
        v = cols[:, c]
        b = v > u
        u = np.where(b, v, u)
        idx = np.where(b, c, idx)
    return u, idx


def link_communities(links, gamma, lam, pairwise=False, chunk=None):
    """Everything get_lc_stats / gml compute, as arrays.  pairwise=True takes the link sums with np.sum instead (the
    order-dependence check of the band recheck)."""
    n, K = gamma.shape
    links = np.asarray(links, np.int64).reshape(-1, 2)
    E = len(links)
    chunk = chunk or max(1, (1 << 24) // K)                   # links per [chunk][K] block
    s = seq_sum(gamma)                                        # estimate_all, :700-716
    pi = gamma / s[:, None]
    beta = lam[:, 0] / (lam[:, 0] + lam[:, 1])                # estimate_beta (mmsbgen.hh:213-222)
    _, group = first_strict_max(pi)                           # most_likely_group
    inv = 1.0 / K
    v = np.zeros(n)
    for c in range(K):
        d = pi[:, c] - inv
        v = v + d * d
    deg = np.bincount(links.reshape(-1), minlength=n).astype(np.int64)
    bridg = (1 - np.sqrt(v * float(K) / float(K - 1))) * deg.astype(np.float64)
    colour = np.zeros(E, np.int64)
    ratio = np.zeros(E)
    for a in range(0, E, chunk):                              # inner_prod_max (matrix.hh:460-476) per link
        p, q = links[a:a + chunk, 0], links[a:a + chunk, 1]
        x = (pi[p] * pi[q]) * beta[None, :]
        u, idx = first_strict_max(x)
        tot = np.sum(x, axis=1) if pairwise else seq_sum(x)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio[a:a + chunk] = u / tot
        colour[a:a + chunk] = idx
    join = ~(ratio < 0.5)                                     # lc_current_draw_helper: `max < 0.5` leaves the link out
    gml = ~(ratio < 0.9)                                      # gml: `max < 0.9` is not an edge
    degc = np.zeros((n, K), np.int64)
    jl, jc = links[join], colour[join]
    np.add.at(degc, (jl[:, 0], jc), 1)
    np.add.at(degc, (jl[:, 1], jc), 1)
    nodes = (degc > 0).sum(axis=0)
    degsum = degc.sum(axis=0)
    cmax = degc.max(axis=0)
    argmax = np.where(nodes > 0, np.argmax(degc, axis=0), 0)  # the first (smallest seq id) of the largest
    return dict(pi=pi, beta=beta, group=group, bridgeness=bridg, deg=deg, colour=colour, ratio=ratio, join=join, gml=gml,
                deg_c=degc, memberships=(degc > 0).sum(axis=1), influence=degc[np.arange(n), group],
                comm_nodes=nodes, comm_degsum=degsum, comm_max=cmax, comm_argmax=argmax, unlikely=int((~join).sum()))


def _f5(x):
    """printf's "%.5f" on x86-64 glibc: 0.0 / 0 is the negative default NaN"""
    if np.isnan(x):
        return "-nan" if np.signbit(x) else "nan"
    return "%.5f" % x


def _avg(degsum, nodes):
    return float(degsum) / nodes if nodes else -np.nan


def texts(r, links, seq2id):
    """{file name: text} of the four stats files and network.gml"""
    n, K = r["deg_c"].shape
    ids = np.asarray(seq2id, np.int64)
    avg = [_avg(r["comm_degsum"][k], r["comm_nodes"][k]) for k in range(K)]
    cs = "".join("%d\t%s\t%s\t%d\t%d\n" % (k, _f5(avg[k]), _f5(float(r["comm_max"][k])), r["comm_argmax"][k],
                                              ids[r["comm_argmax"][k]]) for k in range(K))
    br, inf, mem, nodes = [], [], [], []
    for i in range(n):
        g = r["group"][i]
        br.append("%d\t%d\t%s\t%d\t%d\t%d\t%s\t%s\t%d\n" % (i, ids[i], _f5(r["bridgeness"][i]), r["deg_c"][i, g], r["deg"][i],
                                                           r["comm_nodes"][g], _f5(avg[g]), _f5(float(r["comm_max"][g])), g))
        inf.append("%d\t%d\t" % (i, ids[i]) + "".join("%d\t" % c for c in r["deg_c"][i]) + "\n")
        mem.append("%d\t%d\t%d\n" % (i, ids[i], r["memberships"][i]))
        nodes.append("\tnode\n\t[\n\t\tid %d\n\t\textid %d\n\t\tgroup %d\n\t\tbridgeness %s\n\t\tinfluence %d\n\t\tdegree %d\n\t]\n"
                     % (i, ids[i], g, _f5(r["bridgeness"][i]), r["deg_c"][i, g], r["deg"][i]))
    links = np.asarray(links, np.int64).reshape(-1, 2)
    order = np.lexsort((links[:, 1], links[:, 0]))
    edges = ["\tedge\n\t[\n\t\tsource %d\n\t\ttarget %d\n\t\tcolor %d\n\t]\n" % (links[x, 0], links[x, 1], r["colour"][x])
             for x in order if r["gml"][x]]
    return {"community_stats.txt": cs, "node_bridgeness.txt": "".join(br), "node_influence.txt": "".join(inf),
            "number_of_memberships.txt": "".join(mem),
            "network.gml": "graph\n[\n\tdirected 0\n" + "".join(nodes) + "".join(edges) + "]\n"}


def main(argv):
    if len(argv) < 6:
        print(__doc__)
        return 2
    path, n, k, mdir, out = argv[1], int(argv[2]), int(argv[3]), argv[4], argv[5]
    links, seq2id = read_graph(path, n)
    gamma, ids, lam = load_model(mdir, len(seq2id), k)
    if not np.array_equal(ids, seq2id):
        raise ValueError("gamma.txt's id column disagrees with the reader's numbering")
    r = link_communities(links, gamma, lam)
    os.makedirs(out, exist_ok=True)
    for name, t in texts(r, links, seq2id).items():
        if name == "network.gml" and "--lcstats" in argv:
            continue
        with open(os.path.join(out, name), "w") as f:
            f.write(t)
    print("links %d, unlikely %d, gml edges %d" % (len(links), r["unlikely"], int(r["gml"].sum())))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
