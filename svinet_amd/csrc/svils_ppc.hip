// svils_ppc.hip -- -ppc / -gen on the device: networks drawn from a model and the statistics of a link list, the
// reference's MMSBGen::gen (src/mmsbgen.cc:43-71) and MMSBGen::ppc (draw_and_save, :662-697; lc_current_draw_helper,
// :425-470; edge_likelihood, :605-630).  The draw is the definition of DESIGN.md section 4l, not GSL's stream.
//
// The network lives as a symmetric bit matrix bits [n][nw] (nw = ceil(n / 64) words of 64 columns): a row is the sorted
// neighbour set of its node, so the link list in (p, q) order and the CSR with sorted rows both come out of it in order,
// without a sort.  A draw fills a second matrix; it becomes the current one only when its links fit the list.
//
//   k_draw_tiles  one block per 64 x 64 tile of the upper triangle: score_tile (svils_pairtiles.h) with aq = pi beta and
//                 cand = pi, one Philox4x32-10 uniform per pair p < q, y = (u < s).  A pair whose tile sum lies within
//                 2 K DBL_EPSILON s of u is decided again by its own thread with s summed in ascending j.  The tile's 64
//                 row masks go to (tp, tq), their transpose to (tq, tp); a diagonal tile writes the union
//   k_set_bits    an observed list into a zeroed matrix (both orientations, integer atomics)
//   k_row_count   one wavefront per row: deg and the upper degree (the bits above the diagonal), and their total, the links
//                 of a matrix;  k_scan: the exclusive scans of the two (rowptr, uoff)
//   k_fill        one wavefront per row: its bits in ascending order into the CSR row and, above the diagonal, the list
//   k_link_stats  one wavefront per link: x_j over the lanes, the first strict maximum by an exact wave reduction, s by
//                 a fixed tree, the join decision rechecked in ascending j within 2 K eps of 0.5 (by lane 0), and the
//                 common neighbours of p and q by the search of svils_nbr.hip (the shorter sorted row against the
//                 longer).  size_k and the triangle counts are integer atomics; -log x_max goes into 32-bit-wide integer
//                 bins per community (three adds per link), which hold the sum exactly in any order
// The same handle serves the K x K blockmodel of svils_orig (svils_ppc_set_params_orig): a model kind
// is a policy struct (Assortative, Blockmodel) that k_draw_tiles and k_link_stats are instantiated with -- the terms of a
// pair, the definition's sequential sum and the band of the recheck; k_ppc_aq makes the query operand pi B.
// The O(n) and O(K) closings -- wedges, the largest degree, the mean local clustering, the bins to a double -- run on
// the host in index order.
//
// The hop plot and the components of the current list (svils_ppc_hops): all-sources BFS, bit-parallel
// over sources.  Sources go in passes of 64 W consecutive ids (W words of 64 bits per node); a pass holds visited and two
// frontier tables [n][W].
//   k_hop_seed    a pass's tables: bit s - s0 of row s for the sources s of the pass, nothing else
//   k_hop_level   one launch, one level, pull form over the sorted CSR: 16 lanes own a node and split its neighbours, each
//                 reads whole rows of the frontier table (16-byte loads) and ORs them; fresh = acc & ~visited goes to the
//                 next frontier.  A node that every source of the pass has reached already gathers nothing.  popcount(fresh) is reduced over the wavefront into one integer atomicAdd on the level's
//                 counter; the OR of fresh over the block goes by integer atomicOr into the level's source mask, which
//                 the NEXT launch reads (block 0: ecc[s] = the last level whose mask holds s).  A launch whose
//                 predecessor counted nothing returns at once
//   k_hop_close   a pass's counters into D, and comp[v] = the first source of the first pass that reached v
// The host queues the levels in chunks and reads one counter per chunk; the summary (integers, and two doubles) is the host's.
#include "svils_tool.h"
#include "svils_pairtiles.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t NBIN = 36;            // bins of 32 bits from 2^-1088 up: -log x_max < 2^10 ends in bin 34
constexpr int BIN_BIAS = 1088;
constexpr double DBL_EPS = 2.220446049250313e-16;

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t *o0, uint32_t *o1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  *o0 = c0;
  *o1 = c1;
}

__device__ __forceinline__ double pair_uniform(uint32_t seed, uint32_t r, uint32_t p, uint32_t q) {
  uint32_t w0, w1;
  philox4x32_10(p, q, 0u, 0u, seed, r, &w0, &w1);
  return (double)(((uint64_t)(w0 >> 5) << 26) | (uint64_t)(w1 >> 6)) * 0x1p-53;
}

// A model kind is a policy passed by value to the draw and to the statistics: the terms x_t of a pair (a = pi_p, b = pi_q,
// p < q) and the definition's s, ONE running sum over them in ascending t.  The tile sum and the fixed trees are held to
// it within band(K) relative: a pair or a ratio that close to its threshold is decided again with sum().
//
// Assortative (section 4l): x_j = (pi_p[j] pi_q[j]) beta_j, K terms
struct Assortative {
  const double *__restrict__ beta;
  static double band(uint32_t K) { return 2.0 * (double)K * DBL_EPS; }
  __device__ __forceinline__ uint32_t terms(uint32_t K) const { return K; }
  __device__ __forceinline__ double term(const double *__restrict__ a, const double *__restrict__ b, uint32_t, uint32_t t) const {
    return (a[t] * b[t]) * beta[t];
  }
  __device__ inline double sum(const double *__restrict__ a, const double *__restrict__ b, uint32_t K) const {
    double s = 0;
    for (uint32_t j = 0; j < K; ++j) s += (a[j] * b[j]) * beta[j];
    return s;
  }
};

// K x K (section 4p): x_gh = (pi_p[g] pi_q[h]) B[g][h], K^2 terms in row-major t = g K + h; the smaller id indexes the rows
// of B.  The definition's sum has at most K^2 + 1 roundings per term, the tile sum K + k16 + 1 (k_ppc_aq, then the MFMA
// chain), k16 <= K + 15: they differ by less than (K^2 + 2 K + 18) DBL_EPSILON / 2 of s, half the band
struct Blockmodel {
  const double *__restrict__ B;
  static double band(uint32_t K) { return ((double)K * (double)K + 2.0 * (double)K + 18.0) * DBL_EPS; }
  __device__ __forceinline__ uint32_t terms(uint32_t K) const { return K * K; }
  __device__ __forceinline__ double term(const double *__restrict__ a, const double *__restrict__ b, uint32_t K, uint32_t t) const {
    const uint32_t g = t / K;
    return (a[g] * b[t - g * K]) * B[t];
  }
  __device__ inline double sum(const double *__restrict__ a, const double *__restrict__ b, uint32_t K) const {
    double s = 0;
    for (uint32_t g = 0; g < K; ++g)
      for (uint32_t h = 0; h < K; ++h) s += (a[g] * b[h]) * B[g * K + h];
    return s;
  }
};

// the query operand of the K x K kind: aq[i][h] = sum_g pi_i[g] B[g][h], g ascending by fma (as k_orig_aq), zero past
// column K and past row n.  For a diagonal B row i is pi_i[h] B[h][h] rounded once: the assortative operand, bit for bit
__global__ __launch_bounds__(256) void k_ppc_aq(uint32_t rows, uint32_t n, uint32_t K, uint32_t ld, uint32_t k16, const double *__restrict__ pi,
                                                const double *__restrict__ B, double *__restrict__ aq) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (uint64_t)rows * k16) return;
  const uint32_t i = (uint32_t)(e / k16), h = (uint32_t)(e % k16);
  double s = 0.0;
  if (i < n && h < K) {
    const double *row = pi + (size_t)i * ld;
    for (uint32_t g = 0; g < K; ++g) s = fma(row[g], B[(size_t)g * K + h], s);
  }
  aq[e] = s;
}

// tile t of the upper triangle of nt x nt tiles, row by row: (tp, tq) with tp <= tq
__device__ inline void tile_of(uint32_t t, uint32_t nt, uint32_t *tp, uint32_t *tq) {
  const double m = 2.0 * nt + 1.0;
  int64_t r = (int64_t)((m - sqrt(m * m - 8.0 * (double)t)) * 0.5);
  r = r < 0 ? 0 : (r > (int64_t)nt - 1 ? (int64_t)nt - 1 : r);
  auto off = [nt](int64_t x) { return x * (int64_t)nt - x * (x - 1) / 2; };   // tiles before row x
  while (r + 1 < (int64_t)nt && off(r + 1) <= (int64_t)t) ++r;
  while (r > 0 && off(r) > (int64_t)t) --r;
  *tp = (uint32_t)r;
  *tq = (uint32_t)(r + ((int64_t)t - off(r)));
}

template <class M>
__global__ __launch_bounds__(256) void k_draw_tiles(uint32_t t0, uint32_t t1, uint32_t n, uint32_t K, uint32_t ld, uint32_t k16,
                                                    uint32_t nt, const double *__restrict__ pi, const double *__restrict__ aq,
                                                    const M model, uint32_t seed, uint32_t rep, double band,
                                                    unsigned long long *__restrict__ bits, unsigned long long *__restrict__ nrecheck) {
  __shared__ double S[PQ][PC + 1];
  __shared__ unsigned long long RM[64];
  const uint32_t tile = t0 + blockIdx.x;
  if (tile >= t1) return;
  uint32_t tp, tq;
  tile_of(tile, nt, &tp, &tq);
  const uint32_t t = threadIdx.x, w = t >> 6, l = t & 63, g = l >> 4, r16 = l & 15;
  uint32_t cand[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) cand[j] = PC * tq + 16 * j + r16 < n ? PC * tq + 16 * j + r16 : NONE;
  score_tile<false>(S, aq + (size_t)(PQ * tp + 16 * w + r16) * k16, cand, K, ld, k16, pi, nullptr, w, g, r16);
  __syncthreads();
  const uint32_t row = t >> 2, sub = t & 3, p = PQ * tp + row;
  unsigned long long mask = 0;
  if (p < n) {
    for (uint32_t i = 0; i < PC / 4; ++i) {
      const uint32_t c = sub + 4 * i, q = PC * tq + c;
      if (q >= n || q <= p) continue;
      double s = S[row][c];
      const double u = pair_uniform(seed, rep, p, q);
      if (fabs(s - u) <= band * s) {
        s = model.sum(pi + (size_t)p * ld, pi + (size_t)q * ld, K);
        atomicAdd(nrecheck, 1ull);
      }
      if (u < s) mask |= 1ull << c;
    }
  }
  mask |= __shfl_xor(mask, 1);
  mask |= __shfl_xor(mask, 2);
  if (sub == 0) RM[row] = mask;
  __syncthreads();
  if (t >= 128) return;
  const uint32_t c = t & 63;
  unsigned long long col = 0;
  if (t >= 64 || tp == tq)
    for (uint32_t i = 0; i < 64; ++i) col |= ((RM[i] >> c) & 1ull) << i;
  if (tp == tq) {
    if (t < 64 && PQ * tp + c < n) bits[(size_t)(PQ * tp + c) * nt + tp] = RM[c] | col;
  } else if (t < 64) {
    if (PQ * tp + c < n) bits[(size_t)(PQ * tp + c) * nt + tq] = RM[c];
  } else {
    if (PC * tq + c < n) bits[(size_t)(PC * tq + c) * nt + tp] = col;
  }
}

__global__ __launch_bounds__(256) void k_set_bits(uint64_t E, uint32_t nw, const uint32_t *__restrict__ links, unsigned long long *__restrict__ bits) {
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= E) return;
  const uint32_t p = links[2 * x], q = links[2 * x + 1];
  atomicOr(&bits[(size_t)p * nw + (q >> 6)], 1ull << (q & 63));
  atomicOr(&bits[(size_t)q * nw + (p >> 6)], 1ull << (p & 63));
}

// the bits of word w of row i that lie above the diagonal
__device__ __forceinline__ unsigned long long upper_of(unsigned long long v, uint32_t w, uint32_t i) {
  if (w > (i >> 6)) return v;
  if (w < (i >> 6) || (i & 63) == 63) return 0;
  return v & (~0ull << ((i & 63) + 1));
}

// one row per wavefront: deg / up (null: not written), total += the bits above the diagonal
__global__ __launch_bounds__(256) void k_row_count(uint32_t n, uint32_t nw, const unsigned long long *__restrict__ bits,
                                                   uint32_t *__restrict__ deg, uint32_t *__restrict__ up, unsigned long long *__restrict__ total) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  uint32_t d = 0, u = 0;
  for (uint32_t w = lane; w < nw; w += 64) {
    const unsigned long long v = bits[(size_t)i * nw + w];
    d += (uint32_t)__popcll(v);
    u += (uint32_t)__popcll(upper_of(v, w, i));
  }
  for (int o = 32; o > 0; o >>= 1) {
    d += (uint32_t)__shfl_xor((int)d, o, 64);
    u += (uint32_t)__shfl_xor((int)u, o, 64);
  }
  if (lane != 0) return;
  if (deg) deg[i] = d;
  if (up) up[i] = u;
  if (total && u) atomicAdd(total, (unsigned long long)u);
}

// one block: rowptr [n + 1] / uoff [n + 1] = the exclusive scans of deg / up
__global__ __launch_bounds__(1024) void k_scan(uint32_t n, const uint32_t *__restrict__ deg, const uint32_t *__restrict__ up,
                                               uint64_t *__restrict__ rowptr, uint64_t *__restrict__ uoff) {
  __shared__ unsigned long long pa[1024], pb[1024];
  const uint32_t t = threadIdx.x, per = (n + 1023) / 1024;
  const uint32_t b0 = min(n, t * per), b1 = min(n, b0 + per);
  unsigned long long sa = 0, sb = 0;
  for (uint32_t i = b0; i < b1; ++i) { sa += deg[i]; sb += up[i]; }
  pa[t] = sa;
  pb[t] = sb;
  __syncthreads();
  for (uint32_t o = 1; o < 1024; o <<= 1) {
    const unsigned long long va = t >= o ? pa[t - o] : 0, vb = t >= o ? pb[t - o] : 0;
    __syncthreads();
    pa[t] += va;
    pb[t] += vb;
    __syncthreads();
  }
  unsigned long long oa = pa[t] - sa, ob = pb[t] - sb;
  for (uint32_t i = b0; i < b1; ++i) {
    rowptr[i] = oa;
    uoff[i] = ob;
    oa += deg[i];
    ob += up[i];
  }
  if (t == 1023) { rowptr[n] = pa[1023]; uoff[n] = pb[1023]; }
}

// one row per wavefront: the set bits in ascending order -> scol[rowptr[i] ..], and those above the diagonal -> links
__global__ __launch_bounds__(256) void k_fill(uint32_t n, uint32_t nw, const unsigned long long *__restrict__ bits,
                                              const uint64_t *__restrict__ rowptr, const uint64_t *__restrict__ uoff,
                                              const uint32_t *__restrict__ deg, const uint32_t *__restrict__ up,
                                              uint32_t *__restrict__ scol, uint32_t *__restrict__ links) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const uint64_t rb = rowptr[i], ub = uoff[i];
  const uint32_t low = deg[i] - up[i];   // the neighbours below i come first
  uint32_t base = 0;
  for (uint32_t w0 = 0; w0 < nw; w0 += 64) {
    const uint32_t w = w0 + lane;
    unsigned long long v = w < nw ? bits[(size_t)i * nw + w] : 0;
    const uint32_t c = (uint32_t)__popcll(v);
    uint32_t inc = c;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)inc, o, 64);
      if ((int)lane >= o) inc += y;
    }
    uint32_t pos = base + inc - c;
    while (v) {
      const uint32_t q = 64 * w + (uint32_t)__builtin_ctzll(v);
      v &= v - 1;
      scol[rb + pos] = q;
      if (q > i) {
        links[2 * (ub + pos - low)] = i;
        links[2 * (ub + pos - low) + 1] = q;
      }
      ++pos;
    }
    base += (uint32_t)__shfl((int)inc, 63, 64);
  }
}

// the common neighbours of p and q, by a whole wavefront: the shorter sorted row, 64 entries at a time, searched for in the
// longer one.  Every lane returns the count
__device__ __forceinline__ uint32_t common_neighbours(const uint64_t *__restrict__ rowptr, const uint32_t *__restrict__ scol, uint32_t p,
                                                      uint32_t q, uint32_t lane) {
  uint64_t ab = rowptr[p], ae = rowptr[p + 1], bb = rowptr[q], be = rowptr[q + 1];
  if (ae - ab > be - bb) {
    uint64_t s = ab; ab = bb; bb = s;
    s = ae; ae = be; be = s;
  }
  uint32_t common = 0;
  for (uint64_t base = ab; base < ae; base += 64) {
    const bool hit = base + lane < ae && in_row(scol, bb, be, scol[base + lane]);
    common += (uint32_t)__popcll(__ballot(hit));
  }
  return common;
}

// -log m = mant 2^e >= 0 (0 < m <= 1) into the NBIN bins of `row`: bin b holds units of 2^(32 b - BIN_BIAS)
__device__ __forceinline__ void add_neg_log(unsigned long long *__restrict__ row, double m) {
  const double v = -log(m);
  if (!(v > 0)) return;
  int ex;
  const double fr = frexp(v, &ex);                              // v = fr 2^ex, fr in [0.5, 1)
  const unsigned long long mant = (unsigned long long)ldexp(fr, 53);   // 53 bits, exact
  const int e = ex - 53 + BIN_BIAS;                             // v = mant 2^(ex - 53); v >= 2^-54, so e > 0
  if (e < 0 || ((uint32_t)e >> 5) + 2 >= NBIN) return;         // no -log of a double in (0, 1) lies out there
  const uint32_t bin = (uint32_t)e >> 5, sh = (uint32_t)e & 31;
  row += bin;
  const unsigned long long rest = mant >> (32 - sh);            // (mant << sh) >> 32, mant << sh being up to 84 bits wide
  const unsigned long long p0 = (mant << sh) & 0xffffffffull, p1 = rest & 0xffffffffull, p2 = rest >> 32;
  if (p0) atomicAdd(row, p0);
  if (p1) atomicAdd(row + 1, p1);
  if (p2) atomicAdd(row + 2, p2);
}

// one link per wavefront, four per block.  The terms of the link go over the lanes in ascending t (lane, lane + 64, ...),
// so a lane's first strict maximum is the first in t among its own; size, bins and ninf have one entry (row) per term
// index: K communities (Assortative) or K^2 blocks (Blockmodel, section 4p)
template <class M>
__global__ __launch_bounds__(256) void k_link_stats(uint64_t E, uint32_t K, uint32_t ld, const uint32_t *__restrict__ links,
                                                    const double *__restrict__ pi, const M model,
                                                    const uint64_t *__restrict__ rowptr, const uint32_t *__restrict__ scol, double band,
                                                    uint32_t *__restrict__ colour, uint8_t *__restrict__ joined, uint32_t *__restrict__ t2,
                                                    unsigned long long *__restrict__ tri3, unsigned long long *__restrict__ size,
                                                    unsigned long long *__restrict__ bins, uint32_t *__restrict__ ninf) {
  const uint64_t x = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (x >= E) return;   // whole wavefronts leave together
  const uint32_t p = links[2 * x], q = links[2 * x + 1];
  const uint32_t common = common_neighbours(rowptr, scol, p, q, lane);
  const double *a = pi + (size_t)p * ld, *b = pi + (size_t)q * ld;
  double s = 0, u = 0;
  uint32_t idx = NONE;
  for (uint32_t t = lane, T = model.terms(K); t < T; t += 64) {
    const double v = model.term(a, b, K, t);
    s += v;
    if (v > u) { u = v; idx = t; }
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  double m = u;
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  uint32_t wi = (u == m) ? idx : NONE;   // the lowest index holding the maximum: the first strict maximum
  for (int o = 32; o > 0; o >>= 1) wi = min(wi, (uint32_t)__shfl_xor((int)wi, o, 64));
  if (lane != 0) return;
  if (wi == NONE) wi = 0;   // all terms 0: idx stays 0, the ratio is 0 / 0
  double ratio = m / s;
  if (fabs(ratio - 0.5) <= band * ratio) ratio = m / model.sum(a, b, K);
  const bool join = !(ratio < 0.5);
  colour[x] = wi;
  joined[x] = join ? 1 : 0;
  if (common) {
    atomicAdd(&t2[p], common);
    atomicAdd(&t2[q], common);
    atomicAdd(tri3, (unsigned long long)common);
  }
  if (!join) return;
  atomicAdd(&size[wi], 1ull);
  if (!(m > 0)) {
    atomicAdd(&ninf[wi], 1u);
    return;
  }
  add_neg_log(bins + (size_t)wi * NBIN, m);
}

// ---- hop plot and components (section 4o) ----

constexpr uint32_t HOP_WORDS = 8, HOP_CHUNK = 8;   // the defaults of svils_ppc_set_hop_batch

// the tables of the pass of sources s0 .. s0 + nsrc: row s holds bit s - s0; cnt[0] = the pairs at distance 0
__global__ __launch_bounds__(256) void k_hop_seed(uint32_t n, uint32_t W, uint32_t s0, uint32_t nsrc, unsigned long long *__restrict__ vis,
                                                  unsigned long long *__restrict__ front, unsigned long long *__restrict__ cnt) {
  const uint32_t x = blockIdx.x * 256 + threadIdx.x;
  if (x == 0) cnt[0] = nsrc;
  if (x >= n * W) return;
  const uint32_t v = x / W, w = x - v * W, b = v - s0;   // b wraps below s0: then it is >= nsrc
  const unsigned long long word = (v >= s0 && b < nsrc && (b >> 6) == w) ? 1ull << (b & 63) : 0ull;
  vis[x] = word;
  front[x] = word;
}

// level `level` >= 1 of a pass: 16 lanes per node, 16 nodes per block.  cnt [n + 2]: pairs found per level; mask [2][8]: the
// sources that found a node at level l, in slot l & 1 -- written here for `level`, read (and cleared for level + 1) for level - 1
template <int W>
__global__ __launch_bounds__(256) void k_hop_level(uint32_t n, uint32_t level, uint32_t s0, uint32_t nsrc, const uint64_t *__restrict__ rowptr,
                                                   const uint32_t *__restrict__ scol, const unsigned long long *__restrict__ front,
                                                   unsigned long long *__restrict__ next, unsigned long long *__restrict__ vis,
                                                   unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ mask,
                                                   uint32_t *__restrict__ ecc) {
  if (cnt[level - 1] == 0) return;   // written by the launch before: the pass has ended
  __shared__ unsigned long long sm[HOP_WORDS];
  const uint32_t t = threadIdx.x, lane = t & 63, j = t & 15, v = blockIdx.x * 16 + (t >> 4);
  unsigned long long *mprev = mask + HOP_WORDS * ((level - 1) & 1), *mcur = mask + HOP_WORDS * (level & 1);
  if (t < HOP_WORDS) sm[t] = 0;
  if (blockIdx.x == 0) {
    for (uint32_t b = t; b < 64 * W; b += 256)
      if (((mprev[b >> 6] >> (b & 63)) & 1ull) && s0 + b < n) ecc[s0 + b] = level - 1;
    __syncthreads();
    if (t < W) mprev[t] = 0;   // the slot of level + 1; nobody else touches it in this launch
  }
  __syncthreads();
  // lane j of the group owns word j of the node: a node every source of the pass has reached gathers nothing
  const bool owner = v < n && j < (uint32_t)W;
  const size_t slot = (size_t)v * W + j;
  const unsigned long long old = owner ? vis[slot] : ~0ull;
  const uint32_t real = nsrc > 64 * j ? min(64u, nsrc - 64 * j) : 0u;   // the sources of the pass in word j
  const bool open = owner && real && (~old & (~0ull >> (64 - real)));
  const bool gather = ((__ballot(open) >> (lane & 48)) & 0xffffull) != 0;
  unsigned long long acc[W];
#pragma unroll
  for (int w = 0; w < W; ++w) acc[w] = 0;
  if (gather) {
    const uint64_t e = rowptr[v + 1];
    for (uint64_t x = rowptr[v] + j; x < e; x += 16) {
      const unsigned long long *row = front + (size_t)scol[x] * W;
      if constexpr (W % 2 == 0) {   // rows are 16-byte aligned
#pragma unroll
        for (int w = 0; w < W; w += 2) {
          const ulonglong2 p = *reinterpret_cast<const ulonglong2 *>(row + w);
          acc[w] |= p.x;
          acc[w + 1] |= p.y;
        }
      } else {
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] |= row[w];
      }
    }
  }
#pragma unroll
  for (int w = 0; w < W; ++w)
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) acc[w] |= __shfl_xor(acc[w], o, 64);
  unsigned long long fresh = 0;
  if (owner) {
    unsigned long long a = 0;
#pragma unroll
    for (int w = 0; w < W; ++w)
      if (j == (uint32_t)w) a = acc[w];
    fresh = a & ~old;
    if (fresh) vis[slot] = old | fresh;
    next[slot] = fresh;
  }
  uint32_t c = (uint32_t)__popcll(fresh);
  for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o, 64);
  if (lane == 0 && c) atomicAdd(&cnt[level], (unsigned long long)c);
  unsigned long long m = fresh;   // word j of the wavefront's four nodes
  m |= __shfl_xor(m, 16, 64);
  m |= __shfl_xor(m, 32, 64);
  if (lane < (uint32_t)W && m) atomicOr(&sm[lane], m);
  __syncthreads();
  if (t < (uint32_t)W && sm[t]) atomicOr(&mcur[t], sm[t]);
}

// the end of a pass: its counters into D [n + 1], and the label of every node this pass reached first
__global__ __launch_bounds__(256) void k_hop_close(uint32_t n, uint32_t W, uint32_t s0, const unsigned long long *__restrict__ vis,
                                                   const unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ D,
                                                   uint32_t *__restrict__ comp) {
  const uint32_t x = blockIdx.x * 256 + threadIdx.x;
  if (x > n) return;
  D[x] += cnt[x];
  if (x == n || comp[x] != NONE) return;
  for (uint32_t w = 0; w < W; ++w) {
    const unsigned long long word = vis[(size_t)x * W + w];
    if (word) {
      comp[x] = s0 + 64 * w + (uint32_t)__builtin_ctzll(word);
      return;
    }
  }
}

using HopLevel = void (*)(uint32_t, uint32_t, uint32_t, uint32_t, const uint64_t *, const uint32_t *, const unsigned long long *, unsigned long long *,
                          unsigned long long *, unsigned long long *, unsigned long long *, uint32_t *);
constexpr HopLevel kHopLevel[HOP_WORDS] = {k_hop_level<1>, k_hop_level<2>, k_hop_level<3>, k_hop_level<4>,
                                           k_hop_level<5>, k_hop_level<6>, k_hop_level<7>, k_hop_level<8>};

// the 90th percentile of the hop plot, linearly interpolated (SNAP's CalcEffDiam) over the cumulative counts C: these
// operations in this order, nothing contracted (the pragma above)
__attribute__((noinline)) double effective_diameter(const std::vector<uint64_t> &C) {
  const double t = 0.9 * (double)C.back();
  size_t hs = 0;
  while ((double)C[hs] < t) ++hs;
  if (hs == 0) return 0.0;
  const double below = (double)C[hs - 1], step = (double)(C[hs] - C[hs - 1]);
  const double part = (t - below) / step;
  return (double)(hs - 1) + part;
}

}  // namespace

// events ev[6]: draw, list / CSR build, statistics (a bracket each); ev[6], ev[7] (made by the first svils_ppc_hops): the hop passes
struct svils_ppc : ToolHandle {
  uint32_t n = 0, k = 0, ld = 0, k16 = 0, nt = 0, tile_batch = 0;
  uint64_t cap = 0, E = 0;
  unsigned long long *bits = nullptr, *bits_new = nullptr, *counters = nullptr;   // counters: [0] links of a matrix, [1] rechecked pairs, [2] 3 T
  double *pi = nullptr, *aq = nullptr, *beta = nullptr;
  uint32_t *links = nullptr, *scol = nullptr, *colour = nullptr, *deg = nullptr, *up = nullptr, *t2 = nullptr, *ninf = nullptr;
  uint8_t *joined = nullptr;
  uint64_t *rowptr = nullptr, *uoff = nullptr;
  unsigned long long *size = nullptr, *bins = nullptr;
  // the K x K kind (svils_ppc_set_params_orig; made by its first call): B [k][k], and one counter, one row of bins and one
  // count of zero maxima per block
  enum Kind { NO_MODEL, ASSORTATIVE, BLOCKMODEL } kind = NO_MODEL;
  double *B = nullptr;
  unsigned long long *bsize = nullptr, *bbins = nullptr;
  uint32_t *bninf = nullptr;
  bool have_list = false, done = false, timed[3] = {false, false, false};
  uint64_t last_count = 0, last_recheck = 0;
  // the statistics' closings (host)
  std::vector<uint32_t> hdeg, htri;
  uint64_t maxdeg = 0, argmax = 0, triangles = 0, wedges = 0;
  double transitivity = 0, clustering = 0;
  // the hop plot (svils_ppc_hops): tables [n][W], cnt [n + 2] and mask [2][8] in hopc, D [n + 1]; made by the first call
  uint32_t hop_words = HOP_WORDS, hop_chunk = HOP_CHUNK;
  unsigned long long *hvis = nullptr, *hfa = nullptr, *hfb = nullptr, *hopc = nullptr, *hopd = nullptr;
  uint32_t *hecc = nullptr, *hcomp = nullptr;
  bool hops_done = false, hops_timed = false;
  uint64_t hop_launches = 0, hop_counts[6] = {0, 0, 0, 0, 0, 0};
  double hop_values[2] = {0, 0};
  std::vector<uint64_t> hopD;
  std::vector<uint32_t> ecc, comp;
};

namespace {

// the list in (p, q) order and the CSR with sorted rows out of h->bits, which holds E links
int build_lists(svils_ppc *h, uint64_t E) {
  const uint32_t n = h->n;
  hipStream_t st = h->st;
  HIPCHK(hipEventRecord(h->ev[2], st));
  hipLaunchKernelGGL(k_row_count, dim3(blocks(n, 4)), dim3(256), 0, st, n, h->nt, h->bits, h->deg, h->up, (unsigned long long *)nullptr);
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, n, h->deg, h->up, h->rowptr, h->uoff);
  if (E)
    hipLaunchKernelGGL(k_fill, dim3(blocks(n, 4)), dim3(256), 0, st, n, h->nt, h->bits, h->rowptr, h->uoff, h->deg, h->up, h->scol, h->links);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev[3], st));
  HIPCHK(hipStreamSynchronize(st));
  h->E = E;
  h->have_list = h->timed[1] = true;
  h->done = h->hops_done = false;
  return 0;
}

int check_done(svils_ppc *h, const char *name) {
  if (int rc = check(h, name)) return rc;
  if (!h->done) return fail(SVILS_ERR_ARG, "%s: svils_ppc_stats has not run on the current list and parameters", name);
  return 0;
}

// the conditions on pi [n][k] of both kinds, and hp = pi padded to the handle's even leading dimension (16-byte rows)
int padded_pi(const svils_ppc *h, const char *name, const double *pi, std::vector<double> &hp) {
  const uint32_t n = h->n, K = h->k, ld = h->ld;
  hp.assign((size_t)n * ld, 0.0);
  for (uint32_t i = 0; i < n; ++i) {
    double s = 0;
    for (uint32_t j = 0; j < K; ++j) {
      const double v = pi[(size_t)i * K + j];
      if (!(v >= 0.0) || !std::isfinite(v)) return fail(SVILS_ERR_ARG, "%s: pi[%u][%u] = %g is not a finite number >= 0", name, i, j, v);
      s += v;
      hp[(size_t)i * ld + j] = v;
    }
    if (!(std::fabs(s - 1.0) <= 1e-9)) return fail(SVILS_ERR_ARG, "%s: row %u of pi sums to %.17g, not 1 within 1e-9", name, i, s);
  }
  return 0;
}

// the joined links and the sum of log x_max of `cells` communities or blocks (either pointer may be null)
int read_cells(size_t cells, const unsigned long long *dsize, const unsigned long long *dbins, const uint32_t *dninf, uint64_t *size,
               double *logpe) {
  if (size) HIPCHK(hipMemcpy(size, dsize, cells * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (!logpe) return 0;
  std::vector<unsigned long long> bins(cells * NBIN);
  std::vector<uint32_t> ninf(cells);
  HIPCHK(hipMemcpy(bins.data(), dbins, bins.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ninf.data(), dninf, cells * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (size_t k = 0; k < cells; ++k) {
    // the bins hold the sum exactly; from the top down, every term is a 64-bit integer times a power of two
    long double s = 0;
    for (int b = (int)NBIN - 1; b >= 0; --b)
      if (bins[k * NBIN + b]) s += std::ldexp((long double)bins[k * NBIN + b], 32 * b - BIN_BIAS);
    logpe[k] = ninf[k] ? -HUGE_VAL : (s > 0 ? -(double)s : 0.0);
  }
  return 0;
}

int check_hops(svils_ppc *h, const char *name) {
  if (int rc = check(h, name)) return rc;
  if (!h->hops_done) return fail(SVILS_ERR_ARG, "%s: svils_ppc_hops has not run on the current list", name);
  return 0;
}

}  // namespace

extern "C" {

int svils_ppc_create(int device, uint32_t n, uint32_t k, uint64_t max_links, svils_ppc **out) {
  if (!out) return fail(SVILS_ERR_ARG, "svils_ppc_create: null argument");
  *out = nullptr;
  if (n > SVILS_PPC_MAX_N || k > SVILS_PPC_MAX_K)
    return fail(SVILS_ERR_UNSUPPORTED, "svils_ppc_create: n = %u, k = %u (at most SVILS_PPC_MAX_N = %d nodes and SVILS_PPC_MAX_K = %d communities)",
                n, k, SVILS_PPC_MAX_N, SVILS_PPC_MAX_K);
  if (int rc = open_device(device, n < 2 || k < 1 ? "svils_ppc_create: need n >= 2 and k >= 1" : nullptr)) return rc;
  svils_ppc *h = new (std::nothrow) svils_ppc();
  if (!h) return fail(SVILS_ERR_NOMEM, "out of host memory");
  h->n = n;
  h->k = k;
  h->ld = (k + 1u) & ~1u;
  h->k16 = (k + 15u) & ~15u;
  h->nt = (n + 63) / 64;
  h->cap = std::min<uint64_t>(max_links, (uint64_t)n * (n - 1) / 2);
  const auto scope = ToolHandle::HANDLE;
  const size_t words = (size_t)n * h->nt;
  int rc = h->open(device, 6);
  if (!rc) rc = h->dalloc(scope, &h->bits, words);
  if (!rc) rc = h->dalloc(scope, &h->bits_new, words);
  if (!rc) rc = h->dalloc(scope, &h->counters, 3);
  if (!rc) rc = h->dalloc(scope, &h->pi, (size_t)n * h->ld);
  if (!rc) rc = h->dalloc(scope, &h->aq, (size_t)h->nt * 64 * h->k16);
  if (!rc) rc = h->dalloc(scope, &h->beta, (size_t)k);
  if (!rc) rc = h->dalloc(scope, &h->links, 2 * (size_t)h->cap);
  if (!rc) rc = h->dalloc(scope, &h->scol, 2 * (size_t)h->cap);
  if (!rc) rc = h->dalloc(scope, &h->colour, (size_t)h->cap);
  if (!rc) rc = h->dalloc(scope, &h->joined, (size_t)h->cap);
  if (!rc) rc = h->dalloc(scope, &h->deg, (size_t)n);
  if (!rc) rc = h->dalloc(scope, &h->up, (size_t)n);
  if (!rc) rc = h->dalloc(scope, &h->t2, (size_t)n);
  if (!rc) rc = h->dalloc(scope, &h->ninf, (size_t)k);
  if (!rc) rc = h->dalloc(scope, &h->rowptr, (size_t)n + 1);
  if (!rc) rc = h->dalloc(scope, &h->uoff, (size_t)n + 1);
  if (!rc) rc = h->dalloc(scope, &h->size, (size_t)k);
  if (!rc) rc = h->dalloc(scope, &h->bins, (size_t)k * NBIN);
  if (rc) {
    svils_ppc_destroy(h);
    return rc;
  }
  *out = h;
  return 0;
}

int svils_ppc_destroy(svils_ppc *h) {
  delete h;   // ~ToolHandle: waits for the stream, frees the buffers
  return 0;
}

int svils_ppc_set_tile_batch(svils_ppc *h, uint32_t tiles_per_launch) {
  if (int rc = check(h, "svils_ppc_set_tile_batch")) return rc;
  h->tile_batch = tiles_per_launch;
  return 0;
}

int svils_ppc_set_params(svils_ppc *h, const double *pi, const double *beta) {
  if (int rc = check(h, "svils_ppc_set_params")) return rc;
  if (!pi || !beta) return fail(SVILS_ERR_ARG, "svils_ppc_set_params: null argument");
  const uint32_t n = h->n, K = h->k, k16 = h->k16;
  for (uint32_t j = 0; j < K; ++j)
    if (!(beta[j] >= 0.0 && beta[j] <= 1.0)) return fail(SVILS_ERR_ARG, "svils_ppc_set_params: beta[%u] = %g is not in [0, 1]", j, beta[j]);
  // pi padded to an even leading dimension (16-byte rows), and the query operand pi beta padded to whole tiles
  std::vector<double> hp, ha((size_t)h->nt * 64 * k16, 0.0);
  if (int rc = padded_pi(h, "svils_ppc_set_params", pi, hp)) return rc;
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = 0; j < K; ++j) ha[(size_t)i * k16 + j] = pi[(size_t)i * K + j] * beta[j];
  HIPCHK(hipStreamSynchronize(h->st));
  HIPCHK(hipMemcpy(h->pi, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->aq, ha.data(), ha.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->beta, beta, (size_t)K * sizeof(double), hipMemcpyHostToDevice));
  h->kind = svils_ppc::ASSORTATIVE;
  h->done = false;
  return 0;
}

int svils_ppc_set_params_orig(svils_ppc *h, const double *pi, const double *B) {
  if (!h) return no_device_or_null("svils_ppc_set_params_orig");
  if (h->k < 2 || h->k > SVILS_ORIG_MAX_K)
    return fail(SVILS_ERR_UNSUPPORTED, "svils_ppc_set_params_orig: k = %u (the K x K kind holds 2 <= k <= SVILS_ORIG_MAX_K = %d)", h->k,
                SVILS_ORIG_MAX_K);
  if (int rc = check(h, "svils_ppc_set_params_orig")) return rc;
  if (!pi || !B) return fail(SVILS_ERR_ARG, "svils_ppc_set_params_orig: null argument");
  const uint32_t n = h->n, K = h->k;
  const size_t KK = (size_t)K * K;
  for (size_t t = 0; t < KK; ++t)
    if (!(B[t] >= 0.0 && B[t] <= 1.0))
      return fail(SVILS_ERR_ARG, "svils_ppc_set_params_orig: B[%u][%u] = %g is not in [0, 1]", (uint32_t)(t / K), (uint32_t)(t % K), B[t]);
  std::vector<double> hp;
  if (int rc = padded_pi(h, "svils_ppc_set_params_orig", pi, hp)) return rc;
  const auto scope = ToolHandle::HANDLE;
  if (int rc = h->reserve(scope, &h->B, KK)) return rc;
  if (int rc = h->reserve(scope, &h->bsize, KK)) return rc;
  if (int rc = h->reserve(scope, &h->bbins, KK * NBIN)) return rc;
  if (int rc = h->reserve(scope, &h->bninf, KK)) return rc;
  hipStream_t st = h->st;
  HIPCHK(hipStreamSynchronize(st));
  h->kind = svils_ppc::NO_MODEL;   // until the operand is whole
  h->done = false;
  HIPCHK(hipMemcpy(h->pi, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->B, B, KK * sizeof(double), hipMemcpyHostToDevice));
  const uint32_t rows = h->nt * 64;
  hipLaunchKernelGGL(k_ppc_aq, dim3(blocks((uint64_t)rows * h->k16, 256)), dim3(256), 0, st, rows, n, K, h->ld, h->k16, h->pi, h->B, h->aq);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  h->kind = svils_ppc::BLOCKMODEL;
  return 0;
}

int svils_ppc_draw(svils_ppc *h, uint32_t seed, uint32_t r) {
  if (int rc = check(h, "svils_ppc_draw")) return rc;
  if (h->kind == svils_ppc::NO_MODEL) return fail(SVILS_ERR_ARG, "svils_ppc_draw: set the parameters first");
  const uint32_t n = h->n, K = h->k, nt = h->nt;
  hipStream_t st = h->st;
  const uint32_t tiles = (uint32_t)((uint64_t)nt * (nt + 1) / 2), per = h->tile_batch ? h->tile_batch : tiles;
  const bool block = h->kind == svils_ppc::BLOCKMODEL;
  const double band = block ? Blockmodel::band(K) : Assortative::band(K);
  HIPCHK(hipEventRecord(h->ev[0], st));
  HIPCHK(hipMemsetAsync(h->counters, 0, 2 * sizeof(unsigned long long), st));
  for (uint32_t t0 = 0; t0 < tiles; t0 += per) {
    const uint32_t t1 = std::min<uint64_t>(tiles, (uint64_t)t0 + per);
    if (block)
      hipLaunchKernelGGL(k_draw_tiles<Blockmodel>, dim3(t1 - t0), dim3(256), 0, st, t0, t1, n, K, h->ld, h->k16, nt, h->pi, h->aq, Blockmodel{h->B},
                         seed, r, band, h->bits_new, h->counters + 1);
    else
      hipLaunchKernelGGL(k_draw_tiles<Assortative>, dim3(t1 - t0), dim3(256), 0, st, t0, t1, n, K, h->ld, h->k16, nt, h->pi, h->aq,
                         Assortative{h->beta}, seed, r, band, h->bits_new, h->counters + 1);
    if (t1 == tiles) break;
  }
  hipLaunchKernelGGL(k_row_count, dim3(blocks(n, 4)), dim3(256), 0, st, n, nt, h->bits_new, (uint32_t *)nullptr, (uint32_t *)nullptr, h->counters);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev[1], st));
  unsigned long long c[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(c, h->counters, sizeof c, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  h->timed[0] = true;
  h->last_count = c[0];
  h->last_recheck = c[1];
  if (c[0] > h->cap)
    return fail(SVILS_ERR_NOMEM, "svils_ppc_draw: the replicate has %llu links, the list has room for %llu", c[0], (unsigned long long)h->cap);
  std::swap(h->bits, h->bits_new);   // two values change places: each buffer stays owned once
  return build_lists(h, c[0]);
}

int svils_ppc_set_links(svils_ppc *h, const uint32_t *links, uint64_t nlinks) {
  if (int rc = check(h, "svils_ppc_set_links")) return rc;
  if (nlinks && !links) return fail(SVILS_ERR_ARG, "svils_ppc_set_links: null argument");
  const uint32_t n = h->n;
  std::vector<uint64_t> key(nlinks);
  for (uint64_t x = 0; x < nlinks; ++x) {
    const uint32_t p = links[2 * x], q = links[2 * x + 1];
    if (p >= q || q >= n)
      return fail(SVILS_ERR_ARG, "svils_ppc_set_links: link %llu (%u, %u) is not p < q < n = %u", (unsigned long long)x, p, q, n);
    key[x] = ((uint64_t)p << 32) | q;
  }
  std::sort(key.begin(), key.end());
  for (uint64_t x = 1; x < nlinks; ++x)
    if (key[x] == key[x - 1])
      return fail(SVILS_ERR_ARG, "svils_ppc_set_links: link (%u, %u) is given twice", (uint32_t)(key[x] >> 32), (uint32_t)key[x]);
  if (nlinks > h->cap)
    return fail(SVILS_ERR_NOMEM, "svils_ppc_set_links: %llu links, the list has room for %llu", (unsigned long long)nlinks, (unsigned long long)h->cap);
  hipStream_t st = h->st;
  HIPCHK(hipStreamSynchronize(st));
  h->have_list = h->done = h->hops_done = false;
  HIPCHK(hipMemsetAsync(h->bits, 0, (size_t)n * h->nt * sizeof(unsigned long long), st));
  if (nlinks) {   // the caller's list waits in scol until k_fill overwrites it with the CSR (2 cap words: room for it)
    HIPCHK(hipMemcpyAsync(h->scol, links, 2 * nlinks * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_set_bits, dim3(blocks(nlinks, 256)), dim3(256), 0, st, nlinks, h->nt, h->scol, h->bits);
    HIPCHK(hipGetLastError());
  }
  return build_lists(h, nlinks);
}

int svils_ppc_stats(svils_ppc *h) {
  if (int rc = check(h, "svils_ppc_stats")) return rc;
  if (h->kind == svils_ppc::NO_MODEL || !h->have_list) return fail(SVILS_ERR_ARG, "svils_ppc_stats: set the parameters and a list (draw / set_links) first");
  const uint32_t n = h->n, K = h->k;
  const uint64_t E = h->E;
  hipStream_t st = h->st;
  HIPCHK(hipEventRecord(h->ev[4], st));
  HIPCHK(hipMemsetAsync(h->t2, 0, (size_t)n * sizeof(uint32_t), st));
  const bool block = h->kind == svils_ppc::BLOCKMODEL;
  const size_t cells = block ? (size_t)K * K : (size_t)K;   // blocks, or communities
  unsigned long long *size = block ? h->bsize : h->size, *bins = block ? h->bbins : h->bins;
  uint32_t *ninf = block ? h->bninf : h->ninf;
  HIPCHK(hipMemsetAsync(ninf, 0, cells * sizeof(uint32_t), st));
  HIPCHK(hipMemsetAsync(size, 0, cells * sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(bins, 0, cells * NBIN * sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(h->counters + 2, 0, sizeof(unsigned long long), st));
  if (E) {
    if (block)
      hipLaunchKernelGGL(k_link_stats<Blockmodel>, dim3(blocks(E, 4)), dim3(256), 0, st, E, K, h->ld, h->links, h->pi, Blockmodel{h->B}, h->rowptr,
                         h->scol, Blockmodel::band(K), h->colour, h->joined, h->t2, h->counters + 2, size, bins, ninf);
    else
      hipLaunchKernelGGL(k_link_stats<Assortative>, dim3(blocks(E, 4)), dim3(256), 0, st, E, K, h->ld, h->links, h->pi, Assortative{h->beta},
                         h->rowptr, h->scol, Assortative::band(K), h->colour, h->joined, h->t2, h->counters + 2, size, bins, ninf);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(h->ev[5], st));
  h->hdeg.assign(n, 0);
  h->htri.assign(n, 0);
  unsigned long long t3 = 0;
  HIPCHK(hipMemcpyAsync(h->hdeg.data(), h->deg, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(h->htri.data(), h->t2, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&t3, h->counters + 2, sizeof t3, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  // the closings, in node order: every triangle through i was counted at two of i's links, every triangle at its three
  h->maxdeg = h->argmax = h->wedges = 0;
  double cl = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t d = h->hdeg[i], w = d * (d - (d ? 1 : 0)) / 2;
    h->htri[i] /= 2;
    h->wedges += w;
    if (d > h->maxdeg) { h->maxdeg = d; h->argmax = i; }
    if (d >= 2) cl += (double)h->htri[i] / (double)w;
  }
  h->triangles = t3 / 3;
  h->transitivity = 3.0 * (double)h->triangles / (double)h->wedges;   // 0 / 0 = NaN without a wedge
  h->clustering = cl / (double)n;
  h->done = h->timed[2] = true;
  return 0;
}

int svils_ppc_get_draw_counts(svils_ppc *h, uint64_t counts[2]) {
  if (int rc = check(h, "svils_ppc_get_draw_counts")) return rc;
  if (!counts) return fail(SVILS_ERR_ARG, "svils_ppc_get_draw_counts: null argument");
  counts[0] = h->last_count;
  counts[1] = h->last_recheck;
  return 0;
}

int svils_ppc_get_links(svils_ppc *h, uint64_t *count, uint32_t *links, uint32_t *colour, uint8_t *joined) {
  if (int rc = check(h, "svils_ppc_get_links")) return rc;
  if (!h->have_list) return fail(SVILS_ERR_ARG, "svils_ppc_get_links: no list yet (svils_ppc_draw / svils_ppc_set_links)");
  if ((colour || joined) && !h->done) return fail(SVILS_ERR_ARG, "svils_ppc_get_links: colours need svils_ppc_stats on the current list");
  if (count) *count = h->E;
  if (!h->E) return 0;
  if (links) HIPCHK(hipMemcpy(links, h->links, 2 * h->E * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (colour) HIPCHK(hipMemcpy(colour, h->colour, h->E * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (joined) HIPCHK(hipMemcpy(joined, h->joined, h->E, hipMemcpyDeviceToHost));
  return 0;
}

int svils_ppc_get_nodes(svils_ppc *h, uint32_t *deg, uint32_t *tri) {
  if (int rc = check_done(h, "svils_ppc_get_nodes")) return rc;
  if (deg) memcpy(deg, h->hdeg.data(), (size_t)h->n * sizeof(uint32_t));
  if (tri) memcpy(tri, h->htri.data(), (size_t)h->n * sizeof(uint32_t));
  return 0;
}

int svils_ppc_get_summary(svils_ppc *h, uint64_t counts[5], double values[2]) {
  if (int rc = check_done(h, "svils_ppc_get_summary")) return rc;
  if (counts) {
    counts[0] = h->E;
    counts[1] = h->maxdeg;
    counts[2] = h->argmax;
    counts[3] = h->triangles;
    counts[4] = h->wedges;
  }
  if (values) {
    values[0] = h->transitivity;
    values[1] = h->clustering;
  }
  return 0;
}

int svils_ppc_get_communities(svils_ppc *h, uint64_t *size, double *logpe) {
  if (int rc = check_done(h, "svils_ppc_get_communities")) return rc;
  if (h->kind != svils_ppc::ASSORTATIVE)
    return fail(SVILS_ERR_ARG, "svils_ppc_get_communities: the current parameters are K x K (svils_ppc_get_blocks answers for them)");
  return read_cells(h->k, h->size, h->bins, h->ninf, size, logpe);
}

int svils_ppc_get_blocks(svils_ppc *h, uint64_t *bsize, double *blogpe) {
  if (int rc = check_done(h, "svils_ppc_get_blocks")) return rc;
  if (h->kind != svils_ppc::BLOCKMODEL)
    return fail(SVILS_ERR_ARG, "svils_ppc_get_blocks: the current parameters are not K x K (svils_ppc_get_communities answers for them)");
  return read_cells((size_t)h->k * h->k, h->bsize, h->bbins, h->bninf, bsize, blogpe);
}

int svils_ppc_get_timing(svils_ppc *h, double ms[3]) {
  if (int rc = check(h, "svils_ppc_get_timing")) return rc;
  if (!ms) return fail(SVILS_ERR_ARG, "svils_ppc_get_timing: null argument");
  HIPCHK(hipStreamSynchronize(h->st));
  for (int p = 0; p < 3; ++p) ms[p] = h->elapsed_ms(2 * p, 2 * p + 1, h->timed[p]);
  return 0;
}

int svils_ppc_set_hop_batch(svils_ppc *h, uint32_t words, uint32_t levels_per_chunk) {
  if (int rc = check(h, "svils_ppc_set_hop_batch")) return rc;
  if (words > HOP_WORDS) return fail(SVILS_ERR_ARG, "svils_ppc_set_hop_batch: words = %u is not in 1 .. %u (0: the default)", words, HOP_WORDS);
  h->hop_words = words ? words : HOP_WORDS;
  h->hop_chunk = levels_per_chunk ? levels_per_chunk : HOP_CHUNK;
  return 0;
}

int svils_ppc_hops(svils_ppc *h) {
  if (int rc = check(h, "svils_ppc_hops")) return rc;
  if (!h->have_list) return fail(SVILS_ERR_ARG, "svils_ppc_hops: no list yet (svils_ppc_draw / svils_ppc_set_links)");
  const uint32_t n = h->n, W = h->hop_words, per = 64 * W;
  const size_t table = (size_t)n * W, ncnt = (size_t)n + 2;
  const auto scope = ToolHandle::HANDLE;
  hipStream_t st = h->st;
  if (int rc = h->need_events(8)) return rc;
  if (int rc = h->reserve(scope, &h->hvis, table)) return rc;
  if (int rc = h->reserve(scope, &h->hfa, table)) return rc;
  if (int rc = h->reserve(scope, &h->hfb, table)) return rc;
  if (int rc = h->reserve(scope, &h->hopc, ncnt + 2 * HOP_WORDS)) return rc;
  if (int rc = h->reserve(scope, &h->hopd, (size_t)n + 1)) return rc;
  if (int rc = h->reserve(scope, &h->hecc, (size_t)n)) return rc;
  if (int rc = h->reserve(scope, &h->hcomp, (size_t)n)) return rc;
  h->hops_done = false;
  unsigned long long *cnt = h->hopc, *mask = h->hopc + ncnt;
  uint64_t launches = 0;
  HIPCHK(hipEventRecord(h->ev[6], st));
  HIPCHK(hipMemsetAsync(h->hopd, 0, ((size_t)n + 1) * sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(h->hecc, 0, (size_t)n * sizeof(uint32_t), st));
  HIPCHK(hipMemsetAsync(h->hcomp, 0xff, (size_t)n * sizeof(uint32_t), st));   // NONE
  for (uint32_t s0 = 0; s0 < n; s0 += per) {   // passes in ascending source order: the labels depend on it
    const uint32_t nsrc = std::min(per, n - s0);
    HIPCHK(hipMemsetAsync(h->hopc, 0, (ncnt + 2 * HOP_WORDS) * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_hop_seed, dim3(blocks(table, 256)), dim3(256), 0, st, n, W, s0, nsrc, h->hvis, h->hfa, cnt);
    ++launches;
    unsigned long long *cur = h->hfa, *nxt = h->hfb;
    // levels 1 .. n: no distance exceeds n - 1, so level n is empty whatever the graph
    for (uint32_t level = 1; level <= n;) {
      const uint32_t m = std::min(h->hop_chunk, n - level + 1);
      for (uint32_t i = 0; i < m; ++i, ++level) {
        hipLaunchKernelGGL(kHopLevel[W - 1], dim3(blocks(n, 16)), dim3(256), 0, st, n, level, s0, nsrc, h->rowptr, h->scol, cur, nxt, h->hvis, cnt, mask,
                           h->hecc);
        std::swap(cur, nxt);
      }
      launches += m;
      HIPCHK(hipGetLastError());
      unsigned long long last = 0;   // the chunk's last level: empty, and so is every later one
      HIPCHK(hipMemcpyAsync(&last, cnt + (level - 1), sizeof last, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (!last) break;
    }
    hipLaunchKernelGGL(k_hop_close, dim3(blocks((uint64_t)n + 1, 256)), dim3(256), 0, st, n, W, s0, h->hvis, cnt, h->hopd, h->hcomp);
    ++launches;
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev[7], st));
  std::vector<uint64_t> D((size_t)n + 1);
  std::vector<uint32_t> deg(n);
  h->ecc.assign(n, 0);
  h->comp.assign(n, 0);
  HIPCHK(hipMemcpyAsync(D.data(), h->hopd, D.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(h->ecc.data(), h->hecc, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(h->comp.data(), h->hcomp, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(deg.data(), h->deg, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  h->hop_launches = launches;
  h->hops_timed = true;
  // the summary, in index order
  uint32_t levels = 1;
  for (uint32_t l = 1; l < n; ++l)
    if (D[l]) levels = l + 1;
  D.resize(levels);
  std::vector<uint64_t> cum(levels), size(n, 0);
  uint64_t run = 0, far = 0, components = 0, largest = 0, isolated = 0;
  for (uint32_t l = 0; l < levels; ++l) {
    run += D[l];
    cum[l] = run;
    far += (uint64_t)l * D[l];
  }
  for (uint32_t v = 0; v < n; ++v) {
    if (h->comp[v] >= n) return fail(SVILS_ERR_DEVICE, "svils_ppc_hops: node %u has no component", v);
    components += h->comp[v] == v;
    largest = std::max(largest, ++size[h->comp[v]]);
    isolated += deg[v] == 0;
  }
  const uint64_t reachable = run - n;
  h->hop_counts[0] = reachable;
  h->hop_counts[1] = levels - 1;
  h->hop_counts[2] = components;
  h->hop_counts[3] = largest;
  h->hop_counts[4] = isolated;
  h->hop_counts[5] = levels;
  h->hop_values[0] = effective_diameter(cum);
  h->hop_values[1] = reachable ? (double)far / (double)reachable : (double)NAN;
  h->hopD.swap(D);
  h->hops_done = true;
  return 0;
}

int svils_ppc_get_hops(svils_ppc *h, uint32_t *levels, uint64_t *D, uint32_t cap) {
  if (int rc = check_hops(h, "svils_ppc_get_hops")) return rc;
  if (levels) *levels = (uint32_t)h->hopD.size();
  if (D) memcpy(D, h->hopD.data(), std::min<size_t>(h->hopD.size(), cap) * sizeof(uint64_t));
  return 0;
}

int svils_ppc_get_hop_nodes(svils_ppc *h, uint32_t *ecc, uint32_t *comp) {
  if (int rc = check_hops(h, "svils_ppc_get_hop_nodes")) return rc;
  if (ecc) memcpy(ecc, h->ecc.data(), (size_t)h->n * sizeof(uint32_t));
  if (comp) memcpy(comp, h->comp.data(), (size_t)h->n * sizeof(uint32_t));
  return 0;
}

int svils_ppc_get_hop_summary(svils_ppc *h, uint64_t counts[6], double values[2]) {
  if (int rc = check_hops(h, "svils_ppc_get_hop_summary")) return rc;
  if (counts) memcpy(counts, h->hop_counts, sizeof h->hop_counts);
  if (values) memcpy(values, h->hop_values, sizeof h->hop_values);
  return 0;
}

int svils_ppc_get_hop_timing(svils_ppc *h, double ms[2]) {
  if (int rc = check(h, "svils_ppc_get_hop_timing")) return rc;
  if (!ms) return fail(SVILS_ERR_ARG, "svils_ppc_get_hop_timing: null argument");
  HIPCHK(hipStreamSynchronize(h->st));
  ms[0] = h->hops_timed ? h->elapsed_ms(6, 7, true) : -1.0;
  ms[1] = h->hops_timed ? (double)h->hop_launches : -1.0;
  return 0;
}

}  // extern "C"
