"""An INDEPENDENT numpy restatement of the svils_ppc_* entry points (posterior predictive replicates and the statistics
of a link list) -- TEST INFRASTRUCTURE.  Written from DESIGN.md section 4l (the definition of the draw), not from
svils_ppc.hip, with everything done the plain way:

  * Philox4x32-10 from the round function of Salmon et al. (SC'11), in Python integers or uint64 arrays;
  * the pair draw as a loop over pairs and j (`pair_sum`, `draw_loops`); `draw` is the same arithmetic with the loop over
    pairs turned into whole-array operations -- the loop over j stays, so every sum is rounded in the same places;
  * colours by np.argmax (the first maximum), triangles by A @ A on a dense 0/1 matrix, logpe by math.fsum;
  * the host sampler's stream (Marsaglia-Tsang Gamma variates over Philox streams 1 and 2) in Python floats, and the
    texts of every file `svinet -ppc` and `svinet -gen` write (`ppc_texts`, `gen_texts`).
"""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
STREAM_PAIR = 0


def philox4x32_10(ctr, key):
    """ctr = (c0, c1, c2, c3), key = (k0, k1): Python integers, or uint64 arrays holding 32-bit values -> four words"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def to_uniform(w0, w1):
    """((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53, in [0, 1)"""
    return ((w0 >> 5) * 67108864 + (w1 >> 6)) * (1.0 / 9007199254740992.0)


def pair_uniform(seed, r, p, q):
    w = philox4x32_10((p, q, STREAM_PAIR, 0), (seed, r))
    return to_uniform(w[0], w[1])


def pair_uniforms(seed, r, P, Q):
    P, Q = np.asarray(P, np.uint64), np.asarray(Q, np.uint64)
    z = np.zeros_like(P)
    w = philox4x32_10((P, Q, z, z), (int(seed), int(r)))
    return to_uniform(w[0], w[1]).astype(np.float64)


def pair_sum(pi_p, pi_q, beta):
    """s of one pair: x_j = (pi_p[j] pi_q[j]) beta_j summed in ascending j"""
    s = 0.0
    for j in range(len(beta)):
        s += (float(pi_p[j]) * float(pi_q[j])) * float(beta[j])
    return s


def draw_loops(pi, beta, seed, r):
    """the definition, as loops: the links [E][2] of replicate r in (p, q) order"""
    n = pi.shape[0]
    out = []
    for p in range(n):
        for q in range(p + 1, n):
            if pair_uniform(seed, r, p, q) < pair_sum(pi[p], pi[q], beta):
                out.append((p, q))
    return np.array(out, np.int64).reshape(-1, 2)


def all_pairs(n):
    P, Q = np.triu_indices(n, 1)
    return P.astype(np.int64), Q.astype(np.int64)


def terms(pi, beta, P, Q):
    """x [m][K] of the pairs (P, Q)"""
    return (pi[P] * pi[Q]) * beta[None, :]


def seq_sum(x):
    s = np.zeros(x.shape[0])
    for j in range(x.shape[1]):
        s = s + x[:, j]
    return s


def pair_sums(pi, beta, P, Q):
    return seq_sum(terms(pi, beta, P, Q))


def draw(pi, beta, seed, r):
    """draw_loops with the loop over pairs as array operations (row-major upper triangle = (p, q) order)"""
    P, Q = all_pairs(pi.shape[0])
    y = pair_uniforms(seed, r, P, Q) < pair_sums(pi, beta, P, Q)
    return np.stack([P[y], Q[y]], axis=1)


def stats(links, pi, beta):
    """the statistics of a link list (p < q, any order; results per link in (p, q) order) under (pi, beta)"""
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
    x = terms(pi, beta, P, Q)
    s = seq_sum(x)
    colour = np.argmax(x, axis=1) if len(P) else np.zeros(0, np.int64)     # the first maximum; 0 where every term is 0
    xmax = x[np.arange(len(P)), colour]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = xmax / s
    join = ~(ratio < 0.5)
    size = np.bincount(colour[join], minlength=K).astype(np.int64)
    logpe = np.zeros(K)
    for k in range(K):
        v = xmax[join & (colour == k)]
        logpe[k] = -math.inf if np.any(v == 0) else math.fsum(math.log(t) for t in v)
    return dict(links=links, ones=len(P), deg=deg, tri=tri, max_deg=int(deg.max()), argmax_deg=int(np.argmax(deg)), triangles=T,
                wedges=wedges, transitivity=3.0 * T / wedges if wedges else math.nan, clustering=math.fsum(local) / n,
                colour=colour, join=join, ratio=ratio, size=size, logpe=logpe)


def mean_params(gam, lam):
    """-ppc-mean, the reference's estimate_all: pi = gamma / sum (ascending k), beta = l0 / (l0 + l1)"""
    gam = np.asarray(gam, np.float64)
    lam = np.asarray(lam, np.float64).reshape(-1, 2)
    return gam / seq_sum(gam)[:, None], lam[:, 0] / (lam[:, 0] + lam[:, 1])


# ---- the host sampler: Gamma variates by Marsaglia-Tsang over Philox streams 1 (pi) and 2 (beta) of the key (seed, r) ----

STREAM_PI, STREAM_BETA = 1, 2
BLOCK_BOOST = 0xFFFFFFFF


def _uniform_pair(seed, r, a, b, stream, block):
    w = philox4x32_10((a, b, stream, block), (seed, r))
    return to_uniform(w[0], w[1]), to_uniform(w[2], w[3])


def gamma_variate(shape, seed, r, a, b, stream):
    """Gamma(shape, 1) for the variate (a, b) of `stream`.  Attempt t = 0, 1, ... reads blocks 2 t (u1, u2: the normal
    z = sqrt(-2 log(1 - u1)) cos(2 pi u2)) and 2 t + 1 (u3: the acceptance test against log(1 - u3)); a shape below 1 is
    drawn at shape + 1 and scaled by (1 - ub)^(1 / shape), ub the first uniform of block 0xffffffff"""
    a1 = shape + 1.0 if shape < 1.0 else shape
    d = a1 - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    t = 0
    while True:
        u1, u2 = _uniform_pair(seed, r, a, b, stream, 2 * t)
        u3, _ = _uniform_pair(seed, r, a, b, stream, 2 * t + 1)
        t += 1
        z = math.sqrt(-2.0 * math.log(1.0 - u1)) * math.cos(2.0 * math.pi * u2)
        v = 1.0 + c * z
        if v <= 0.0:
            continue
        v = v * v * v
        if math.log(1.0 - u3) < 0.5 * z * z + d - d * v + d * math.log(v):
            break
    g = d * v
    if shape < 1.0:
        ub, _ = _uniform_pair(seed, r, a, b, stream, BLOCK_BOOST)
        g *= math.pow(1.0 - ub, 1.0 / shape)
    return g


def dirichlet_rows(gam, seed, r):
    """pi_i ~ Dirichlet(gam_i): variate (i, j) of stream 1, the row divided by its sum in ascending j (1 / K where it is 0)"""
    gam = np.asarray(gam, np.float64)
    n, K = gam.shape
    pi = np.zeros((n, K))
    for i in range(n):
        g = [gamma_variate(float(gam[i, j]), seed, r, i, j, STREAM_PI) for j in range(K)]
        s = 0.0
        for v in g:
            s += v
        pi[i] = [v / s for v in g] if s > 0 else [1.0 / K] * K
    return pi


def beta_draws(lam, seed, r):
    """beta_k ~ Beta(lam_k0, lam_k1) = g0 / (g0 + g1): variates (k, 0) and (k, 1) of stream 2"""
    lam = np.asarray(lam, np.float64).reshape(-1, 2)
    out = np.zeros(lam.shape[0])
    for k in range(lam.shape[0]):
        g0 = gamma_variate(float(lam[k, 0]), seed, r, k, 0, STREAM_BETA)
        g1 = gamma_variate(float(lam[k, 1]), seed, r, k, 1, STREAM_BETA)
        out[k] = g0 / (g0 + g1)
    return out


# ---- the files of `svinet -ppc` and `svinet -gen` ----

def fx(x, digits=5):
    return "nan" if math.isnan(x) else "%.*f" % (digits, x)


def moments(x, obs):
    """(mean, sample deviation, z, two-sided p) of the replicate values x against obs, sums in replicate order"""
    R = len(x)
    s = 0.0
    for v in x:
        s += v
    mean = s / R
    q = 0.0
    for v in x:
        q += (v - mean) * (v - mean)
    sd = math.sqrt(q / (R - 1)) if R > 1 else 0.0
    z = (obs - mean) / sd if sd > 0 else math.nan
    ge, le = sum(1 for v in x if v >= obs), sum(1 for v in x if v <= obs)
    return mean, sd, z, min(1.0, 2.0 * min(ge, le) / R)


def scalars(s, n):
    return dict(ones=s["ones"], density=s["ones"] / (n * (n - 1) / 2.0), avg_deg=(2 * s["ones"]) / float(n), max_deg=s["max_deg"],
                triangles=s["triangles"], transitivity=s["transitivity"], clustering=s["clustering"])


def row_of(c):
    return "%d\t%s\t%s\t%d\t%d\t%s\t%s\n" % (c["ones"], fx(c["density"], 8), fx(c["avg_deg"]), c["max_deg"], c["triangles"],
                                                fx(c["transitivity"]), fx(c["clustering"]))


def ppc_texts(links, gam, lam, draws, seed, mean, save=0):
    """every file `svinet -ppc` writes, as {path relative to the working directory: text}"""
    gam = np.asarray(gam, np.float64)
    n, K = gam.shape
    pim, betam = mean_params(gam, lam)
    obs = stats(links, pim, betam)
    oc = scalars(obs, n)
    out = {"ppc/obs.txt": row_of(oc), "obs-ones.txt": fx(oc["density"]) + "\n", "obs-avg-deg.txt": fx(oc["avg_deg"]) + "\n",
           "obs-max-deg.txt": "%d\n" % oc["max_deg"]}
    reps, cols = [], []
    for r in range(draws):
        pi, beta = (pim, betam) if mean else (dirichlet_rows(gam, seed, r), beta_draws(lam, seed, r))
        l = draw(pi, beta, seed, r)
        reps.append(stats(l, pi, beta))
        cols.append(scalars(reps[-1], n))
        if r < save:
            out["ppc/%d/network.dat" % r] = "".join("%d\t%d\n" % (p, q) for p, q in l)
    out["ppc/rep.txt"] = "".join(row_of(c) for c in cols)
    out["ppc/ppc-ones.txt"] = "".join(fx(c["density"]) + "\n" for c in cols)
    out["ppc/ppc-avg-deg.txt"] = "".join(fx(c["avg_deg"]) + "\n" for c in cols)
    out["ppc/ppc-max-deg.txt"] = "".join("%d\n" % c["max_deg"] for c in cols)
    lsz = lpe = zsz = zpe = ""
    for k in range(K):
        m = moments([float(s["size"][k]) for s in reps], float(obs["size"][k]))
        lsz += "%d\t%d\t%s\t%s\t%s\n" % (k, obs["size"][k], fx(m[0]), fx(m[1]), fx(m[2]))
        zsz += "%d\t%s\n" % (k, fx(m[2]))
        m = moments([float(s["logpe"][k]) for s in reps], float(obs["logpe"][k]))
        lpe += "%d\t%s\t%s\t%s\t%s\n" % (k, fx(float(obs["logpe"][k])), fx(m[0]), fx(m[1]), fx(m[2]))
        zpe += "%d\t%s\n" % (k, fx(m[2]))
    out.update({"ppc/lc_size.txt": lsz, "ppc/lc_logpe.txt": lpe, "ppc/lc_zscores_size.txt": zsz, "ppc/lc_zscores_pe.txt": zpe})
    sm = ""
    for name in ("ones", "density", "avg_deg", "max_deg", "triangles", "transitivity", "clustering"):
        d = 8 if name == "density" else 5
        m = moments([float(c[name]) for c in cols], float(oc[name]))
        sm += "%s\t%s\t%s\t%s\t%s\n" % (name, fx(float(oc[name]), d), fx(m[0], d), fx(m[1], d), fx(m[3]))
    out["ppc/summary.txt"] = sm
    return out


def gen_texts(n, K, seed):
    """the files of `svinet -gen`: pi ~ Dirichlet(0.05), beta ~ Beta(4700.59, 0.77), replicate 0"""
    pi = dirichlet_rows(np.full((n, K), 0.05), seed, 0)
    beta = beta_draws(np.tile([4700.59, 0.77], (K, 1)), seed, 0)
    l = draw(pi, beta, seed, 0)
    return {"gen/network_gen.dat": "".join("%d\t%d\n" % (p, q) for p, q in l),
            "gen/pi-gen.txt": "".join("%d\t%d\t%s\n" % (i, i, "\t".join(fx(v) for v in pi[i])) for i in range(n)),
            "gen/beta-gen.txt": "".join("%d\t%s\n" % (k, fx(beta[k])) for k in range(K))}
