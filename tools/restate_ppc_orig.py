"""An INDEPENDENT numpy restatement of the K x K kind of the svils_ppc_* entry points (svils_ppc_set_params_orig,
svils_ppc_get_blocks) and of `svinet -ppc-orig` -- TEST INFRASTRUCTURE.  Written from DESIGN.md section 4p (the
definition of the draw), not from svils_ppc.hip.  The random numbers, the host sampler, `moments` and the formats are
those of tools/restate_ppc.py, imported; everything that knows the model is restated here, the plain way:

  * the pair draw as a loop over pairs, g and h (`pair_sum`, `draw_loops`); `draw` is the same arithmetic with the loop
    over pairs turned into whole-array operations -- the loops over g and h stay, so the ONE running sum is rounded in
    the same places;
  * blocks by np.argmax over the K^2 terms in row-major order (the first maximum), triangles by A @ A on a dense 0/1
    matrix, blogpe by math.fsum;
  * the texts of every file `svinet -ppc-orig` writes (`ppc_orig_texts`); the -ppc-hops files are restate_hops.py's.
"""
import math

import numpy as np

from restate_ppc import all_pairs, dirichlet_rows, fx, moments, pair_uniform, pair_uniforms, row_of, scalars, seq_sum


def terms(pi, B, P, Q):
    """x [m][K K] of the pairs (P, Q), P < Q: x_gh = (pi_P[g] pi_Q[h]) B[g][h] at column g K + h"""
    K = pi.shape[1]
    return ((pi[P][:, :, None] * pi[Q][:, None, :]) * B[None, :, :]).reshape(len(P), K * K)


def pair_sum(pi_p, pi_q, B):
    """s of one pair p < q: one running sum over g ascending and, within g, h ascending"""
    s = 0.0
    K = len(pi_p)
    for g in range(K):
        for h in range(K):
            s += (float(pi_p[g]) * float(pi_q[h])) * float(B[g][h])
    return s


def draw_loops(pi, B, seed, r):
    """the definition, as loops: the links [E][2] of replicate r in (p, q) order"""
    n = pi.shape[0]
    out = []
    for p in range(n):
        for q in range(p + 1, n):
            if pair_uniform(seed, r, p, q) < pair_sum(pi[p], pi[q], B):
                out.append((p, q))
    return np.array(out, np.int64).reshape(-1, 2)


def pair_sums(pi, B, P, Q):
    """pair_sum of every pair (P, Q): the loops over g and h stay, one column of terms at a time"""
    K = pi.shape[1]
    s = np.zeros(len(P))
    for g in range(K):
        a = pi[P, g]
        for h in range(K):
            s = s + (a * pi[Q, h]) * B[g, h]
    return s


def draw(pi, B, seed, r):
    """draw_loops with the loop over pairs as array operations (row-major upper triangle = (p, q) order)"""
    P, Q = all_pairs(pi.shape[0])
    y = pair_uniforms(seed, r, P, Q) < pair_sums(pi, B, P, Q)
    return np.stack([P[y], Q[y]], axis=1)


def stats(links, pi, B):
    """the statistics of a link list (p < q, any order; results per link in (p, q) order) under (pi, B)"""
    n, K = pi.shape
    links = np.asarray(links, np.int64).reshape(-1, 2)
    links = links[np.lexsort((links[:, 1], links[:, 0]))]
    P, Q = links[:, 0], links[:, 1]
    A = np.zeros((n, n), np.int64)
    A[P, Q] = 1
    A[Q, P] = 1
    deg = A.sum(1)
    tri = ((A @ A) * A).sum(1) // 2
    T = int(tri.sum()) // 3
    wedges = int((deg * (deg - 1) // 2).sum())
    local = [float(tri[i]) / float(deg[i] * (deg[i] - 1) // 2) if deg[i] >= 2 else 0.0 for i in range(n)]
    x = terms(pi, B, P, Q)
    s = seq_sum(x)
    colour = np.argmax(x, axis=1) if len(P) else np.zeros(0, np.int64)     # the first maximum; 0 where every term is 0
    xmax = x[np.arange(len(P)), colour]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = xmax / s
    join = ~(ratio < 0.5)
    bsize = np.bincount(colour[join], minlength=K * K).astype(np.int64).reshape(K, K)
    blogpe = np.zeros((K, K))
    for t in range(K * K):
        v = xmax[join & (colour == t)]
        blogpe[t // K, t % K] = -math.inf if np.any(v == 0) else math.fsum(math.log(e) for e in v)
    joined = int(bsize.sum())
    off = joined - int(np.trace(bsize))
    return dict(links=links, ones=len(P), deg=deg, tri=tri, max_deg=int(deg.max()), argmax_deg=int(np.argmax(deg)), triangles=T,
                wedges=wedges, transitivity=3.0 * T / wedges if wedges else math.nan, clustering=math.fsum(local) / n,
                colour=colour, join=join, ratio=ratio, bsize=bsize, blogpe=blogpe,
                offdiag_share=float(off) / float(joined) if joined else math.nan)


def mean_pi(gam):
    """-ppc-mean: pi = gamma / sum (ascending k)"""
    gam = np.asarray(gam, np.float64)
    return gam / seq_sum(gam)[:, None]


def replicates(gam, B, draws, seed, mean):
    """[(pi, links)] of the replicates 0 .. draws - 1 of `svinet -ppc-orig`: pi_i ~ Dirichlet(gamma_i) from stream 1 of
    (seed, r) -- or the mean with -ppc-mean --, B as it is"""
    gam = np.asarray(gam, np.float64)
    B = np.asarray(B, np.float64)
    out = []
    for r in range(draws):
        pi = mean_pi(gam) if mean else dirichlet_rows(gam, seed, r)
        out.append((pi, draw(pi, B, seed, r)))
    return out


def ppc_orig_texts(links, gam, B, draws, seed, mean, save=0):
    """every file `svinet -ppc-orig` writes (without -ppc-hops), as {path relative to the working directory: text}"""
    gam = np.asarray(gam, np.float64)
    B = np.asarray(B, np.float64)
    n, K = gam.shape
    pim = mean_pi(gam)
    obs = stats(links, pim, B)
    oc = scalars(obs, n)
    oc["offdiag_share"] = obs["offdiag_share"]
    out = {"ppc/obs.txt": row_of(oc), "obs-ones.txt": fx(oc["density"]) + "\n", "obs-avg-deg.txt": fx(oc["avg_deg"]) + "\n",
           "obs-max-deg.txt": "%d\n" % oc["max_deg"]}
    reps, cols = [], []
    for r, (pi, l) in enumerate(replicates(gam, B, draws, seed, mean)):
        reps.append(stats(l, pi, B))
        cols.append(scalars(reps[-1], n))
        cols[-1]["offdiag_share"] = reps[-1]["offdiag_share"]
        if r < save:
            out["ppc/%d/network.dat" % r] = "".join("%d\t%d\n" % (p, q) for p, q in l)
    out["ppc/rep.txt"] = "".join(row_of(c) for c in cols)
    out["ppc/ppc-ones.txt"] = "".join(fx(c["density"]) + "\n" for c in cols)
    out["ppc/ppc-avg-deg.txt"] = "".join(fx(c["avg_deg"]) + "\n" for c in cols)
    out["ppc/ppc-max-deg.txt"] = "".join("%d\n" % c["max_deg"] for c in cols)
    bsz = bpe = ""
    for g in range(K):
        for h in range(K):
            m = moments([float(s["bsize"][g, h]) for s in reps], float(obs["bsize"][g, h]))
            bsz += "%d\t%d\t%d\t%s\t%s\t%s\n" % (g, h, obs["bsize"][g, h], fx(m[0]), fx(m[1]), fx(m[2]))
            m = moments([float(s["blogpe"][g, h]) for s in reps], float(obs["blogpe"][g, h]))
            bpe += "%d\t%d\t%s\t%s\t%s\t%s\n" % (g, h, fx(float(obs["blogpe"][g, h])), fx(m[0]), fx(m[1]), fx(m[2]))
    out.update({"ppc/block_size.txt": bsz, "ppc/block_logpe.txt": bpe})
    sm = ""
    for name in ("ones", "density", "avg_deg", "max_deg", "triangles", "transitivity", "clustering", "offdiag_share"):
        d = 8 if name == "density" else 5
        m = moments([float(c[name]) for c in cols], float(oc[name]))
        sm += "%s\t%s\t%s\t%s\t%s\n" % (name, fx(float(oc[name]), d), fx(m[0], d), fx(m[1], d), fx(m[3]))
    out["ppc/summary.txt"] = sm
    return out
