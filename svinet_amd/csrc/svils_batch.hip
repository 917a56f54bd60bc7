// svils_batch.hip -- -batch-gpu: the reference's MMSBInfer::batch_infer (src/mmsbinfer.cc:833-930) on the device, coordinate
// ascent over ALL n (n - 1) / 2 pairs.  One sweep is
//
//   k_batch_dir_exp    set_dir_exp (src/mmsbinfer.hh:563-580): one wavefront per node, Elogpi = psi(gamma) - psi(row sum)
//   k_batch_beta       the same for lambda [k][2]
//   k_batch_fill       gamma_next = alpha, lambda_next = eta (:887-888)
//   k_batch_pairs<W,V> the pair pass (:846-880).  The pair triangle is cut into tiles of
//                      TA rows x 64 columns (TA = 4 A, A rows per wavefront: tile_rows()), one workgroup of 4 wavefronts
//                      per tile; a group of W lanes holds one pair, V values per lane (k = v W + lw).  A wavefront walks the
//                      64 columns in chunks of G = 64 / W -- group g owns column c G + g of the chunk and keeps its phi2 sum
//                      in registers -- and inside a chunk its A rows, one row per step: all G groups of a step share the row,
//                      their phi1 are summed by a fixed butterfly and added to the row's accumulator in LDS (touched by this
//                      wavefront alone).  A step loops until all its groups have left the fixed point; a group that has
//                      left keeps its vectors.  Out come per-tile partials: TA row sums, 4 x 64 column sums (one set per
//                      wavefront), 4 lambda partials -- plain stores, every address written by exactly one lane
//   k_batch_reduce_*   gamma_next / lambda_next += the partials of the tiles, in ascending tile order (rows first, then columns)
//   k_batch_pair_ll    edge_likelihood (src/mmsbinfer.hh:634-668) of a list of (p, q, y), one wavefront per pair
//
// No floating-point atomics: every sum has one owner and a fixed order, so a sweep is bitwise reproducible.  The tiles of
// a sweep go through the partial buffers in batches of at most BATCH_TILES.
//
// There is ONE fixed point in this file: pair_fixed_point<W,V> (PhiComp, src/mmsbinfer.hh:104-203), called by the pair pass,
// by the step kernels and by the star chain below, with count_pairs for their counters -- sweeps and steps mixed on one
// handle run the same arithmetic by construction.  And one launch table: launch_for_width maps the handle's lane width to
// the <W, VARIANT_V> instantiation of whichever kernel the caller names.
//
// -rnode / -rpair: the sampled-pair steps of MMSBInfer::infer (src/mmsbinfer.cc:459-740) on the same handle (DESIGN.md
// section 4g), one fixed chain of launches per step, queued without a host round trip:
//
//   k_batch_step_node<W,V>  node step: group j holds pair (a, j), blends gamma_j and writes Elogpi_j itself; phi_a and the
//                           lambda terms leave as per-wavefront partials
//   k_batch_step_phi<W,V>   pair step: group e holds the e-th listed pair; phi to the step's buffer, lambda partials
//   k_batch_step_rows<W,V>  pair step: group i adds node i's phi vectors in list order, blends gamma_i, writes Elogpi_i
//   k_batch_step_tail       block k: the partials of community k in a fixed order; gamma_a[k] (node steps), lambda[k], Elogbeta[k]
//
// -infset: the informative-set steps of FastAMM::infer (src/fastamm.cc:549-672) on the same handle:
//
//   k_batch_star_chain<W,V> a chain of star steps in one workgroup of one launch, a barrier between steps
//
// -snode: the stratified random node steps of FastAMM2::infer (src/fastamm2.cc:535-702) on the same handle (DESIGN.md section
// 4m).  Every row of gamma moves at every step; the rows a step does not name are not written -- their decay is one factor
// per row, kept on the host and applied when the row is next read:
//
//   k_batch_strat_pairs<W,V> group e holds pair (a, j_e): catches both rows up, forms their Elogpi in registers, writes the
//                            blended gamma_j and no Elogpi; phi_a and the lambda terms leave as per-wavefront partials
//   k_batch_strat_tail       block k: the partials in a fixed order; gamma_a[k] caught up and blended, lambda[k], Elogbeta[k]
//   k_batch_catch_up         every row at its true value, before any other entry point touches gamma
//
// -logl: approx_log_likelihood (src/mmsbinfer.cc:1948-2060) of the current state on the same handle:
//
//   k_batch_elbo<W,V>       the tiles of k_batch_pairs; a pair's term from the registers its group holds, one double per
//                           (tile, wavefront)
//   k_batch_elbo_nodes      one wavefront per node: the node's term
//   k_batch_elbo_reduce     one block: the lambda terms, and the three sums in a fixed order
#include <cassert>

#include "svils_csr.h"
#include "svils_devutil.h"
#include "svils_elbo.h"
#include "svils_steplists.h"
#include "svils_tool.h"
#include "svils_waveutil.h"

namespace {

constexpr uint32_t TILE_COLS = 64;
constexpr uint32_t BATCH_TILES = 2048;              // tiles per launch of the pair kernel
constexpr size_t BATCH_BYTES = (size_t)256 << 20;   // ... and at most this much of partial sums

// rows of a tile one wavefront owns: its row accumulators are A x (W V) doubles of LDS, 32 KiB per workgroup at most
constexpr int rows_per_wave(int wv) { return wv <= 64 ? 16 : wv == 128 ? 8 : 4; }

// the instantiation table: V = 4 everywhere, W the smallest power of two with 4 W >= k
inline uint32_t variant_w(uint32_t k) {
  uint32_t w = 1;
  while (4 * w < k) w <<= 1;
  return w;
}
constexpr uint32_t VARIANT_V = 4;

// one wavefront per node: lanes stride k, the row sum by a fixed butterfly
__global__ __launch_bounds__(256) void k_batch_dir_exp(uint32_t n, uint32_t K, const double *__restrict__ gamma,
                                                       const double *__restrict__ gtab, double *__restrict__ elogpi) {
  __shared__ double2 logtab[128];
  load_logtab(logtab, gtab);
  __syncthreads();
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;   // whole wavefronts leave together
  const double *g = gamma + (size_t)i * K;
  double s = 0.0;
  for (uint32_t k = lane; k < K; k += 64) s += g[k];
  const double ps = digamma(wave_sum_f64(s), logtab);
  for (uint32_t k = lane; k < K; k += 64) elogpi[(size_t)i * K + k] = digamma(g[k], logtab) - ps;
}

__global__ __launch_bounds__(256) void k_batch_beta(uint32_t K, const double *__restrict__ lam, const double *__restrict__ gtab,
                                                    double *__restrict__ elogbeta) {
  __shared__ double2 logtab[128];
  load_logtab(logtab, gtab);
  __syncthreads();
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const double ps = digamma(lam[2 * k] + lam[2 * k + 1], logtab);
  elogbeta[2 * k] = digamma(lam[2 * k], logtab) - ps;
  elogbeta[2 * k + 1] = digamma(lam[2 * k + 1], logtab) - ps;
}

__global__ __launch_bounds__(256) void k_batch_fill(uint64_t nk, uint32_t K, double alpha, double eta0, double eta1,
                                                    double *__restrict__ gnext, double *__restrict__ lnext) {
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (x < nk) gnext[x] = alpha;
  if (x < K) { lnext[2 * x] = eta0; lnext[2 * x + 1] = eta1; }
}

// ---- the pair fixed point: PhiComp (src/mmsbinfer.hh:104-203), the ONE copy every kernel below runs -------------------
// the start vector: 1 / K on the lanes that hold a community
__device__ __forceinline__ double phi_start(bool kval, uint32_t K) { return kval ? 1.0 / (double)K : 0.0; }

// The fixed point of the one pair a group of W lanes holds: Jacobi order (both updates from the previous round's vectors),
// the exit test after every odd round, at most MAX_ROUNDS rounds; a pair whose normaliser is not > 0 leaves with what it
// has and adds one to `under` (the reference asserts there).  p1 / p2 come in as phi_start -- the caller seeds them in the
// loop that loads elp, which is what keeps k_batch_pairs at its registers (profiles/r19a_batch_refactor.md) -- and go out
// as the pair's phi; `under` is only ever added to, in every lane of the group.  Called by whole wavefronts; a group with
// valid = false runs along without a round.
template <int W, int V>
__device__ __forceinline__ void pair_fixed_point(const double (&elp)[V], const double (&elq)[V], const double (&ef)[V], double le,
                                                 const bool (&kval)[V], uint32_t K, bool valid, double (&p1)[V], double (&p2)[V],
                                                 uint32_t &rounds, uint32_t &under) {
  const double dK = (double)K;
  double o1[V], o2[V];
#pragma unroll
  for (int v = 0; v < V; ++v) o1[v] = o2[v] = 0.0;
  bool live = valid;
  rounds = 0;
  for (uint32_t i = 0; i < MAX_ROUNDS; ++i) {
    if (!__ballot(live)) break;
    if ((i & 1) == 0) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        o1[v] = live ? p1[v] : o1[v];
        o2[v] = live ? p2[v] : o2[v];
      }
    }
    double e[2 * V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      e[v] = (elp[v] + ef[v] * p2[v]) + (1.0 - p2[v]) * le;
      e[V + v] = (elq[v] + ef[v] * p1[v]) + (1.0 - p1[v]) * le;
    }
    exp_neg_n<2 * V>(e);
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      e[v] = kval[v] ? e[v] : 0.0;
      e[V + v] = kval[v] ? e[V + v] : 0.0;
      s1 += e[v];
      s2 += e[V + v];
    }
    s1 = group_sum<W>(s1);
    s2 = group_sum<W>(s2);
    const bool ok = s1 > 0.0 && s2 > 0.0;
    if (live && !ok) {
      ++under;
      live = false;
    }
    const double r1 = fast_rcp(ok ? s1 : 1.0), r2 = fast_rcp(ok ? s2 : 1.0);
    double m1 = 0.0, m2 = 0.0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      e[v] *= r1;
      e[V + v] *= r2;
      m1 += fabs(e[v] - o1[v]);
      m2 += fabs(e[V + v] - o2[v]);
      p1[v] = live ? e[v] : p1[v];
      p2[v] = live ? e[V + v] : p2[v];
    }
    rounds += live;
    if (i & 1) {
      m1 = group_sum<W>(m1);
      m2 = group_sum<W>(m2);
      if (m1 / dK < MEAN_CHANGE_THRESH && m2 / dK < MEAN_CHANGE_THRESH) live = false;
    }
  }
}

// the counters of a wavefront's groups (lane lw == 0 of a group carries its pair's) into the handle's five
__device__ inline void count_pairs(unsigned long long *ctr, uint32_t lane, uint32_t npairs, uint32_t rtot, uint32_t rmax, uint32_t under) {
  npairs = wave_sum_u32(npairs);
  rtot = wave_sum_u32(rtot);
  under = wave_sum_u32(under);
  rmax = wave_max_u32(rmax);
  if (lane == 0) {
    if (npairs) atomicAdd(&ctr[0], (unsigned long long)npairs);
    if (rtot) atomicAdd(&ctr[1], (unsigned long long)rtot);
    if (rmax) atomicMax(&ctr[2], (unsigned long long)rmax);
    if (under) { atomicAdd(&ctr[3], (unsigned long long)under); atomicAdd(&ctr[4], (unsigned long long)under); }
  }
}

struct PairArgs {
  uint32_t n, K, nw, t0;            // nw: words per row of the bit matrices; t0: first tile of this launch
  const uint32_t *tiles;            // [T][2] (row block, column block)
  const uint32_t *adj, *skip;       // [n][nw] bit q of row p: y(p, q) / the pair is left out
  const double *elogpi, *elogbeta;  // [n][K], [K][2]
  double logeps;
  double *pa, *pb, *pl;             // partials of the launch: [tile][TA][K], [tile][4][64][K], [tile][4][K][2]
  unsigned long long *ctr;          // pairs, rounds, most rounds of a pair, underflows of the sweep, underflows since set_state
};

template <int W, int V>
__global__ __launch_bounds__(256) void k_batch_pairs(PairArgs x) {
  constexpr int G = 64 / W, WV = W * V, A = rows_per_wave(WV);
  __shared__ double accA[4][A][WV];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane / W, lw = lane % W;
  const uint32_t bt = blockIdx.x, K = x.K, n = x.n;
  const uint32_t rb = x.tiles[2 * (size_t)(x.t0 + bt)], cb = x.tiles[2 * (size_t)(x.t0 + bt) + 1];
  const uint32_t row0 = rb * (4 * A) + wave * A, col0 = cb * TILE_COLS;
  bool kval[V];
  double ef0[V], ef1[V];   // elogf for y = 0 / y = 1
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const uint32_t k = v * W + lw;
    kval[v] = k < K;
    ef1[v] = kval[v] ? x.elogbeta[2 * k] : 0.0;
    ef0[v] = kval[v] ? x.elogbeta[2 * k + 1] : 0.0;
  }
  for (uint32_t i = lane; i < (uint32_t)(A * WV); i += 64) (&accA[wave][0][0])[i] = 0.0;
  double l0[V], l1[V];
#pragma unroll
  for (int v = 0; v < V; ++v) l0[v] = l1[v] = 0.0;
  uint32_t npairs = 0, rtot = 0, rmax = 0, under = 0;

  for (uint32_t c = 0; c < (uint32_t)W; ++c) {   // 64 / G chunks of G columns
    const uint32_t b = col0 + c * G + g;
    const bool bval = b < n;
    double elq[V], accB[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      elq[v] = bval && kval[v] ? x.elogpi[(size_t)b * K + v * W + lw] : 0.0;
      accB[v] = 0.0;
    }
    for (uint32_t ai = 0; ai < (uint32_t)A; ++ai) {
      const uint32_t a = row0 + ai;
      if (a >= n) break;   // the same in every lane
      bool valid = bval && a < b;
      bool y = false;
      if (valid) {
        const size_t wd = (size_t)a * x.nw + (b >> 5);
        const uint32_t bit = 1u << (b & 31);
        valid = (x.skip[wd] & bit) == 0;
        y = (x.adj[wd] & bit) != 0;
      }
      if (!__ballot(valid)) continue;   // the same in every lane
      double elp[V], ef[V], p1[V], p2[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        elp[v] = kval[v] ? x.elogpi[(size_t)a * K + v * W + lw] : 0.0;
        ef[v] = y ? ef1[v] : ef0[v];
        p1[v] = p2[v] = phi_start(kval[v], K);
      }
      uint32_t rounds;
      pair_fixed_point<W, V>(elp, elq, ef, y ? x.logeps : 0.0, kval, K, valid, p1, p2, rounds, under);
      if (valid && lw == 0) {
        ++npairs;
        rtot += rounds;
        rmax = max(rmax, rounds);
      }
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const double q1 = valid ? p1[v] : 0.0, q2 = valid ? p2[v] : 0.0;
        accB[v] += q2;
        const double pp = q1 * q2;
        l0[v] += y ? pp : 0.0;
        l1[v] += y ? 0.0 : pp;
        const double rs = cross_group_sum<W>(q1);
        if (g == 0) accA[wave][ai][v * W + lw] += rs;
      }
    }
    // the chunk's column sums (zero for a column past n or without a pair here)
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (kval[v]) x.pb[(((size_t)bt * 4 + wave) * TILE_COLS + c * G + g) * K + v * W + lw] = accB[v];
  }
  for (uint32_t i = lane; i < (uint32_t)(A * WV); i += 64) {
    const uint32_t ai = i / WV, k = i % WV;
    if (k < K) x.pa[((size_t)bt * (4 * A) + wave * A + ai) * K + k] = accA[wave][ai][k];
  }
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const double t0 = cross_group_sum<W>(l0[v]), t1 = cross_group_sum<W>(l1[v]);
    if (g == 0 && kval[v]) {
      double *o = x.pl + (((size_t)bt * 4 + wave) * K + v * W + lw) * 2;
      o[0] = t0;
      o[1] = t1;
    }
  }
  count_pairs(x.ctr, lane, npairs, rtot, rmax, lw == 0 ? under : 0);
}

struct ReduceArgs {
  uint32_t n, K, TA, t0, t1;        // the launch's tiles [t0, t1)
  uint32_t rb_lo, rb_hi;            // their row blocks, inclusive
  uint32_t nrb;
  const uint32_t *rowoff, *jfirst;  // [nrb + 1] first tile of a row block, [nrb] its first column block
  const double *pa, *pb;
  double *gnext;
};

// one thread per (node, k): the node's row partials in ascending tile order, then its column partials in ascending tile
// order (the four wavefronts of a tile in order)
__global__ __launch_bounds__(256) void k_batch_reduce_gamma(ReduceArgs x) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (uint64_t)x.n * x.K) return;
  const uint32_t i = (uint32_t)(idx / x.K), k = (uint32_t)(idx % x.K), K = x.K, TA = x.TA;
  double s = x.gnext[idx];
  const uint32_t rb = i / TA;
  if (rb < x.nrb) {
    const uint32_t lo = max(x.t0, x.rowoff[rb]), hi = min(x.t1, x.rowoff[rb + 1]);
    for (uint32_t t = lo; t < hi; ++t) s += x.pa[((size_t)(t - x.t0) * TA + i % TA) * K + k];
  }
  const uint32_t cb = i / TILE_COLS;
  for (uint32_t r = x.rb_lo; r <= x.rb_hi && r < x.nrb; ++r) {
    if (x.jfirst[r] > cb) break;   // jfirst never decreases
    const uint32_t t = x.rowoff[r] + (cb - x.jfirst[r]);
    if (t < x.t0 || t >= x.t1 || t >= x.rowoff[r + 1]) continue;
    for (uint32_t w = 0; w < 4; ++w) s += x.pb[(((size_t)(t - x.t0) * 4 + w) * TILE_COLS + i % TILE_COLS) * K + k];
  }
  x.gnext[idx] = s;
}

// block k: lambda_next[k][j] += the sum of the launch's nent = 4 x tiles partials -- every thread its entries in ascending
// order, then a fixed tree over the threads
__global__ __launch_bounds__(256) void k_batch_reduce_lambda(uint32_t K, uint32_t nent, const double *__restrict__ pl,
                                                             double *__restrict__ lnext) {
  __shared__ double red[2][256];
  const uint32_t k = blockIdx.x, t = threadIdx.x;
  double s0 = 0.0, s1 = 0.0;
  for (uint32_t e = t; e < nent; e += 256) {
    s0 += pl[((size_t)e * K + k) * 2];
    s1 += pl[((size_t)e * K + k) * 2 + 1];
  }
  red[0][t] = s0;
  red[1][t] = s1;
  __syncthreads();
  for (uint32_t o = 128; o > 0; o >>= 1) {
    if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; }
    __syncthreads();
  }
  if (t == 0) { lnext[2 * k] += red[0][0]; lnext[2 * k + 1] += red[1][0]; }
}

// one wavefront per pair; the y = 0 sum is the reference's k x k loop (lanes over zp, zq in order)
__global__ __launch_bounds__(256) void k_batch_pair_ll(uint64_t m, uint32_t K, double eps, const uint32_t *__restrict__ pairs,
                                                       const uint8_t *__restrict__ y, const double *__restrict__ gamma,
                                                       const double *__restrict__ lam, double *__restrict__ out) {
  const uint64_t x = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (x >= m) return;   // whole wavefronts leave together
  const double *gp = gamma + (size_t)pairs[2 * x] * K, *gq = gamma + (size_t)pairs[2 * x + 1] * K;
  double sp = 0.0, sq = 0.0;
  for (uint32_t k = 0; k < K; ++k) { sp += gp[k]; sq += gq[k]; }
  double s = 0.0;
  if (y[x]) {
    for (uint32_t z = lane; z < K; z += 64) s += (gp[z] / sp) * (gq[z] / sq) * (lam[2 * z] / (lam[2 * z] + lam[2 * z + 1]));
  } else {
    for (uint32_t zp = lane; zp < K; zp += 64) {
      const double pp = gp[zp] / sp, beta = lam[2 * zp] / (lam[2 * zp] + lam[2 * zp + 1]);
      for (uint32_t zq = 0; zq < K; ++zq) s += pp * (gq[zq] / sq) * (1.0 - (zp == zq ? beta : eps));
    }
  }
  s = wave_sum_f64(s);
  if (lane == 0) out[x] = log(s < 1e-30 ? 1e-30 : s);
}

// ---- the variational lower bound (svils_batch_elbo) -------------------------------------------
// approx_log_likelihood (src/mmsbinfer.cc:1948-2060): s = G + P + N.  The pair part runs the tiles of a sweep and keeps a
// scalar where the sweep keeps gamma and lambda partials.

// (xlogx and the node term: svils_elbo.h, shared with svils_orig_elbo)

struct ElboArgs {
  uint32_t n, K, nw, t0;            // as PairArgs
  const uint32_t *tiles;
  const uint32_t *adj, *skip;
  const double *elogpi, *elogbeta;
  double logeps;
  double *part;                     // [tile of the pass][4]: one double per (tile, wavefront), indexed by the pass's tile
  unsigned long long *ctr;          // the pass's own five: pairs, rounds, most rounds, underflows (twice)
};

// The tile and group layout of k_batch_pairs<W,V>.  A group that has left the fixed point forms its pair's term from the
// registers it holds; a lane adds its share of every step of its wavefront, one butterfly at the end.
template <int W, int V>
__global__ __launch_bounds__(256) void k_batch_elbo(ElboArgs x) {
  constexpr int G = 64 / W, WV = W * V, A = rows_per_wave(WV);
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane / W, lw = lane % W;
  const uint32_t bt = blockIdx.x, K = x.K, n = x.n;
  const uint32_t rb = x.tiles[2 * (size_t)(x.t0 + bt)], cb = x.tiles[2 * (size_t)(x.t0 + bt) + 1];
  const uint32_t row0 = rb * (4 * A) + wave * A, col0 = cb * TILE_COLS;
  bool kval[V];
  double ef0[V], ef1[V];   // elogf for y = 0 / y = 1
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const uint32_t k = v * W + lw;
    kval[v] = k < K;
    ef1[v] = kval[v] ? x.elogbeta[2 * k] : 0.0;
    ef0[v] = kval[v] ? x.elogbeta[2 * k + 1] : 0.0;
  }
  double acc = 0.0;
  uint32_t npairs = 0, rtot = 0, rmax = 0, under = 0;

  for (uint32_t c = 0; c < (uint32_t)W; ++c) {   // 64 / G chunks of G columns
    const uint32_t b = col0 + c * G + g;
    const bool bval = b < n;
    double elq[V];
#pragma unroll
    for (int v = 0; v < V; ++v) elq[v] = bval && kval[v] ? x.elogpi[(size_t)b * K + v * W + lw] : 0.0;
    for (uint32_t ai = 0; ai < (uint32_t)A; ++ai) {
      const uint32_t a = row0 + ai;
      if (a >= n) break;   // the same in every lane
      bool valid = bval && a < b;
      bool y = false;
      if (valid) {
        const size_t wd = (size_t)a * x.nw + (b >> 5);
        const uint32_t bit = 1u << (b & 31);
        valid = (x.skip[wd] & bit) == 0;
        y = (x.adj[wd] & bit) != 0;
      }
      if (!__ballot(valid)) continue;   // the same in every lane
      double elp[V], ef[V], p1[V], p2[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        elp[v] = kval[v] ? x.elogpi[(size_t)a * K + v * W + lw] : 0.0;
        ef[v] = y ? ef1[v] : ef0[v];
        p1[v] = p2[v] = phi_start(kval[v], K);
      }
      uint32_t rounds;
      const double le = y ? x.logeps : 0.0;
      pair_fixed_point<W, V>(elp, elq, ef, le, kval, K, valid, p1, p2, rounds, under);
      if (valid && lw == 0) {
        ++npairs;
        rtot += rounds;
        rmax = max(rmax, rounds);
      }
      // sum_k phi1 phi2 elogf + phi1 Elogpi_p + phi2 Elogpi_q - phi1 log phi1 - phi2 log phi2, this lane's k; the g != h sum
      // of a link is S1 S2 - sum_k phi1 phi2 (lane 0 of the group carries S1 S2)
      double t = 0.0, s1 = 0.0, s2 = 0.0, spp = 0.0;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const double q1 = p1[v], q2 = p2[v], pp = q1 * q2;
        t += pp * ef[v] + q1 * elp[v] + q2 * elq[v] - xlogx(q1) - xlogx(q2);
        s1 += q1;
        s2 += q2;
        spp += pp;
      }
      s1 = group_sum<W>(s1);
      s2 = group_sum<W>(s2);
      t += le * ((lw == 0 ? s1 * s2 : 0.0) - spp);
      acc += valid ? t : 0.0;
    }
  }
  acc = wave_sum_f64(acc);
  if (lane == 0) x.part[(size_t)(x.t0 + bt) * 4 + wave] = acc;
  count_pairs(x.ctr, lane, npairs, rtot, rmax, lw == 0 ? under : 0);
}

// one wavefront per node, as k_batch_dir_exp: the node's term of N
__global__ __launch_bounds__(256) void k_batch_elbo_nodes(uint32_t n, uint32_t K, double alpha, const double *__restrict__ gamma,
                                                          const double *__restrict__ elogpi, double *__restrict__ out) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;   // whole wavefronts leave together
  const double t = elbo_node_term(gamma + (size_t)i * K, elogpi + (size_t)i * K, K, alpha, lane);
  if (lane == 0) out[i] = t;
}

// One block.  P: the (tile, wavefront) partials of the whole pass; N: the node terms; G: the terms of the communities,
// formed here.  Each sum: every thread its entries in ascending order, then a fixed tree over the threads -- the order
// depends on the counts alone, never on how the tiles were cut into launches.  out: total, G, P, N
__global__ __launch_bounds__(256) void k_batch_elbo_reduce(uint64_t nent, const double *__restrict__ part, uint32_t n,
                                                           const double *__restrict__ node, uint32_t K, const double *__restrict__ lam,
                                                           const double *__restrict__ elogbeta, double eta0, double eta1,
                                                           double *__restrict__ out) {
  __shared__ double red[3][256];
  const uint32_t t = threadIdx.x;
  double sp = 0.0, sn = 0.0, sg = 0.0;
  for (uint64_t e = t; e < nent; e += 256) sp += part[e];
  for (uint32_t i = t; i < n; i += 256) sn += node[i];
  for (uint32_t k = t; k < K; k += 256) {
    const double l0 = lam[2 * k], l1 = lam[2 * k + 1], e0 = elogbeta[2 * k], e1 = elogbeta[2 * k + 1];
    sg += (lgamma(eta0 + eta1) - lgamma(eta0) - lgamma(eta1)) + ((eta0 - 1.0) * e0 + (eta1 - 1.0) * e1) -
          (lgamma(l0 + l1) - lgamma(l0) - lgamma(l1)) - ((l0 - 1.0) * e0 + (l1 - 1.0) * e1);
  }
  red[0][t] = sg;
  red[1][t] = sp;
  red[2][t] = sn;
  __syncthreads();
  for (uint32_t o = 128; o > 0; o >>= 1) {
    if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; red[2][t] += red[2][t + o]; }
    __syncthreads();
  }
  if (t == 0) {
    out[0] = red[0][0] + red[1][0] + red[2][0];
    out[1] = red[0][0];
    out[2] = red[1][0];
    out[3] = red[2][0];
  }
}

// ---- sampled-pair steps (svils_batch_step_node / svils_batch_step_pairs) ----------------------

// Elogpi of the row a group holds in registers (0 on the lanes past K): psi(g) - psi(row sum), the sum by group_sum
template <int W, int V>
__device__ __forceinline__ void row_elogpi(const double (&g)[V], const bool (&kval)[V], bool row_ok, const double2 *logtab,
                                           double (&el)[V]) {
  double s = 0.0;
#pragma unroll
  for (int v = 0; v < V; ++v) s += g[v];
  s = group_sum<W>(s);
  const double ps = digamma(row_ok ? s : 1.0, logtab);
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const bool ok = row_ok && kval[v];
    const double d = digamma(ok ? g[v] : 1.0, logtab) - ps;
    el[v] = ok ? d : 0.0;
  }
}

// a group's new row: gamma = (1 - rho) gamma + rho (alpha + scale t), then Elogpi of it.  Only groups with row < n store.
// The arithmetic of row_elogpi, written out: each Elogpi is stored as it is formed.  Through row_elogpi the four stay live
// together, and k_batch_step_rows goes from 50 to 74 VGPRs, a step down in occupancy (profiles/r25a_batch_steps.md)
template <int W, int V>
__device__ __forceinline__ void blend_row(bool row_ok, size_t row, uint32_t K, uint32_t lw, const bool (&kval)[V], const double (&t)[V],
                                          double rho, double alpha, double scale, double *__restrict__ gamma, double *__restrict__ elogpi,
                                          const double2 *logtab) {
  double gn[V], s = 0.0;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const bool ok = row_ok && kval[v];
    const double g = ok ? gamma[row * K + v * W + lw] : 0.0;
    gn[v] = ok ? (1.0 - rho) * g + rho * (alpha + scale * t[v]) : 0.0;
    s += gn[v];
  }
  s = group_sum<W>(s);
  const double ps = digamma(row_ok ? s : 1.0, logtab);
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const bool ok = row_ok && kval[v];
    const double el = digamma(ok ? gn[v] : 1.0, logtab) - ps;
    if (ok) {
      gamma[row * K + v * W + lw] = gn[v];
      elogpi[row * K + v * W + lw] = el;
    }
  }
}

// What wavefront wv hands to the tail for community k, from inside the caller's loop over its V values: its groups'
// phi_a (WITH_A: to part_a [wavefront][K]) and lambda terms (to pl [wavefront][K][2], y = 1 first), each summed over the
// groups in cross_group_sum's fixed order.  A group without a pair comes with zeros.  One value at a time, so that the
// caller's other stores of that value stay in the same loop: as a loop of its own behind them it cost k_batch_step_phi 1 %
// and k_batch_strat_pairs 1.5-3 % (profiles/r25a_batch_steps.md)
template <int W, bool WITH_A>
__device__ __forceinline__ void wave_partial(double pa, double pj, bool y, bool kval, uint32_t g, uint32_t k, uint32_t wv, uint32_t K,
                                             double *part_a, double *pl) {
  const double pp = pa * pj;
  double sa = 0.0;
  if constexpr (WITH_A) sa = cross_group_sum<W>(pa);
  const double t0 = cross_group_sum<W>(y ? pp : 0.0), t1 = cross_group_sum<W>(y ? 0.0 : pp);
  if (g == 0 && kval) {
    if constexpr (WITH_A) part_a[(size_t)wv * K + k] = sa;
    pl[((size_t)wv * K + k) * 2] = t0;
    pl[((size_t)wv * K + k) * 2 + 1] = t1;
  }
}

// a stored row value at its true value (strat steps, below): f == 1 exactly (a row that is not behind) keeps its bits
__device__ __forceinline__ double caught_up(double g, double alpha, double f) { return f == 1.0 ? g : alpha + (g - alpha) * f; }

// ---- the graph of the step kernels: one policy per form of the handle (svils_batch_create / svils_batch_create_sparse),
// in the style of BitRows / CsrRows (svils_pairtiles.h).  star(a, j): the pair of a node step, looked up from a's side -- is
// it left out, and its y; link(p, q), p < q: y of a listed pair

// dense form: bit q of row p (p < q) of two [n][nw] bit matrices, one word read each
struct DenseGraph {
  const uint32_t *adj, *skip;
  uint32_t nw;
  __device__ __forceinline__ void star(uint32_t a, uint32_t j, bool &skipped, bool &y) const {
    const uint32_t p = min(a, j), q = max(a, j);
    const size_t wd = (size_t)p * nw + (q >> 5);
    const uint32_t bit = 1u << (q & 31);
    skipped = (skip[wd] & bit) != 0;
    y = (adj[wd] & bit) != 0;
  }
  __device__ __forceinline__ bool link(uint32_t p, uint32_t q) const { return (adj[(size_t)p * nw + (q >> 5)] & (1u << (q & 31))) != 0; }
};

// sparse form: the links and the skip pairs as two symmetric CSRs with ascending rows and 64-bit row offsets.  A lookup is
// a lower-bound search without a branch in its loop: at most ceil(log2(row length)) probes, none in an empty row.  A node
// step searches the rows of a: ONE row per list, read by every group of the grid and resident in L2, a hub's included
struct SparseGraph {
  const uint64_t *lrow, *srow;      // [n + 1]
  const uint32_t *lcol, *scol;
  // q among col[b .. e), ascending and without repeats: what lies right of the window is > q, so q is there iff it ends the search
  static __device__ __forceinline__ bool has(const uint32_t *__restrict__ col, uint64_t b, uint64_t e, uint32_t q) {
    uint64_t len = e - b;
    while (len > 1) {
      const uint64_t half = len >> 1;
      b += col[b + half - 1] < q ? half : 0;
      len -= half;
    }
    return len != 0 && col[b] == q;
  }
  __device__ __forceinline__ void star(uint32_t a, uint32_t j, bool &skipped, bool &y) const {
    skipped = has(scol, srow[a], srow[a + 1], j);
    y = has(lcol, lrow[a], lrow[a + 1], j);
  }
  __device__ __forceinline__ bool link(uint32_t p, uint32_t q) const { return has(lcol, lrow[p], lrow[p + 1], q); }
};

struct StepArgs {
  uint32_t n, K;
  double *gamma, *elogpi;           // [n][K]: the kernel that owns a row writes both
  const double *elogbeta;
  double logeps, alpha, scale, rho;
  double *part_a, *pl;              // per-wavefront partials: [wavefront][K] (node steps), [wavefront][K][2]
  unsigned long long *ctr;
  const double *gtab;
  // node steps
  uint32_t a;
  // pair steps
  uint32_t m;                       // pairs of the step
  const uint32_t *pairs;            // [m][2]
  const uint32_t *noff, *ent;       // [n + 1] offsets into ent; ent[x] = 2 e + side, every node's in list order
  double *phi;                      // [m][2][K]
};

// Node step, first launch: group j holds the pair (a, j).  Row a and Elogpi_a are only read; row j belongs to its group,
// which blends it and writes Elogpi_j (a skipped pair: with phi = 0).  phi_a and the lambda terms leave per wavefront.
template <int W, int V, class Graph>
__global__ __launch_bounds__(256) void k_batch_step_node(StepArgs x, Graph gr) {
  constexpr int G = 64 / W;
  __shared__ double2 logtab[128];
  load_logtab(logtab, x.gtab);
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane / W, lw = lane % W;
  const uint32_t K = x.K, n = x.n, a = x.a;
  const uint32_t wv = blockIdx.x * 4 + wave, j = wv * G + g;
  const bool row_ok = j < n && j != a;
  bool valid = row_ok, y = false;
  if (row_ok) {
    bool skipped;
    gr.star(a, j, skipped, y);
    valid = !skipped;
  }
  bool kval[V];
  double ela[V], elj[V], ef[V], pa[V], pj[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const uint32_t k = v * W + lw;
    kval[v] = k < K;
    ela[v] = kval[v] ? x.elogpi[(size_t)a * K + k] : 0.0;
    elj[v] = kval[v] && row_ok ? x.elogpi[(size_t)j * K + k] : 0.0;
    ef[v] = kval[v] ? x.elogbeta[2 * k + (y ? 0 : 1)] : 0.0;
    pa[v] = pj[v] = phi_start(kval[v], K);
  }
  uint32_t rounds, under = 0;
  pair_fixed_point<W, V>(ela, elj, ef, y ? x.logeps : 0.0, kval, K, valid, pa, pj, rounds, under);
#pragma unroll
  for (int v = 0; v < V; ++v) {
    pa[v] = valid ? pa[v] : 0.0;
    pj[v] = valid ? pj[v] : 0.0;
  }
  blend_row<W, V>(row_ok, j, K, lw, kval, pj, x.rho, x.alpha, x.scale, x.gamma, x.elogpi, logtab);
#pragma unroll
  for (int v = 0; v < V; ++v) wave_partial<W, true>(pa[v], pj[v], y, kval[v], g, v * W + lw, wv, K, x.part_a, x.pl);
  const bool cnt = valid && lw == 0;
  count_pairs(x.ctr, lane, cnt, cnt ? rounds : 0, cnt ? rounds : 0, cnt ? under : 0);
}

// Pair step, first launch: group e holds the e-th listed pair; phi goes to the step's buffer, the lambda terms leave per wavefront
template <int W, int V, class Graph>
__global__ __launch_bounds__(256) void k_batch_step_phi(StepArgs x, Graph gr) {
  constexpr int G = 64 / W;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane / W, lw = lane % W;
  const uint32_t K = x.K, wv = blockIdx.x * 4 + wave, e = wv * G + g;
  const bool valid = e < x.m;
  uint32_t p = 0, q = 0;
  bool y = false;
  if (valid) {
    p = x.pairs[2 * (size_t)e];
    q = x.pairs[2 * (size_t)e + 1];
    y = gr.link(p, q);
  }
  bool kval[V];
  double elp[V], elq[V], ef[V], p1[V], p2[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const uint32_t k = v * W + lw;
    kval[v] = k < K;
    elp[v] = kval[v] && valid ? x.elogpi[(size_t)p * K + k] : 0.0;
    elq[v] = kval[v] && valid ? x.elogpi[(size_t)q * K + k] : 0.0;
    ef[v] = kval[v] ? x.elogbeta[2 * k + (y ? 0 : 1)] : 0.0;
    p1[v] = p2[v] = phi_start(kval[v], K);
  }
  uint32_t rounds, under = 0;
  pair_fixed_point<W, V>(elp, elq, ef, y ? x.logeps : 0.0, kval, K, valid, p1, p2, rounds, under);
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const uint32_t k = v * W + lw;
    const double q1 = valid ? p1[v] : 0.0, q2 = valid ? p2[v] : 0.0;
    if (valid && kval[v]) {
      x.phi[(2 * (size_t)e) * K + k] = q1;
      x.phi[(2 * (size_t)e + 1) * K + k] = q2;
    }
    wave_partial<W, false>(q1, q2, y, kval[v], g, k, wv, K, nullptr, x.pl);
  }
  const bool cnt = valid && lw == 0;
  count_pairs(x.ctr, lane, cnt, cnt ? rounds : 0, cnt ? rounds : 0, cnt ? under : 0);
}

// Pair step, second launch: group i owns node i -- its phi vectors of the step added in list order, then the blend and Elogpi_i
template <int W, int V>
__global__ __launch_bounds__(256) void k_batch_step_rows(StepArgs x) {
  constexpr int G = 64 / W;
  __shared__ double2 logtab[128];
  load_logtab(logtab, x.gtab);
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane / W, lw = lane % W;
  const uint32_t K = x.K, i = (blockIdx.x * 4 + wave) * G + g;
  const bool row_ok = i < x.n;
  bool kval[V];
  double t[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    kval[v] = (uint32_t)(v * W) + lw < K;
    t[v] = 0.0;
  }
  if (row_ok)
    for (uint32_t o = x.noff[i]; o < x.noff[i + 1]; ++o) {
      const double *ph = x.phi + (size_t)x.ent[o] * K;
#pragma unroll
      for (int v = 0; v < V; ++v) t[v] += kval[v] ? ph[v * W + lw] : 0.0;
    }
  blend_row<W, V>(row_ok, i, K, lw, kval, t, x.rho, x.alpha, x.scale, x.gamma, x.elogpi, logtab);
}

// Last launch of a step, block k: the nwv per-wavefront partials of community k -- every thread its entries in ascending
// order, then a fixed tree over the threads.  Node steps (part_a non-null) blend gamma[a][k] here; rho_l >= 0 blends
// lambda[k] and renews Elogbeta[k], rho_l < 0 leaves both alone.
__global__ __launch_bounds__(256) void k_batch_step_tail(uint32_t K, uint32_t nwv, const double *__restrict__ part_a,
                                                         const double *__restrict__ pl, double *__restrict__ gamma_a, double alpha,
                                                         double eta0, double eta1, double scale, double rho_g, double rho_l,
                                                         double *__restrict__ lam, double *__restrict__ elogbeta,
                                                         const double *__restrict__ gtab) {
  __shared__ double red[3][256];
  const uint32_t k = blockIdx.x, t = threadIdx.x;
  double sa = 0.0, s0 = 0.0, s1 = 0.0;
  for (uint32_t w = t; w < nwv; w += 256) {
    if (part_a) sa += part_a[(size_t)w * K + k];
    s0 += pl[((size_t)w * K + k) * 2];
    s1 += pl[((size_t)w * K + k) * 2 + 1];
  }
  red[0][t] = sa;
  red[1][t] = s0;
  red[2][t] = s1;
  __syncthreads();
  for (uint32_t o = 128; o > 0; o >>= 1) {
    if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; red[2][t] += red[2][t + o]; }
    __syncthreads();
  }
  if (t != 0) return;
  if (part_a) gamma_a[k] = (1.0 - rho_g) * gamma_a[k] + rho_g * (alpha + scale * red[0][0]);
  if (rho_l >= 0.0) {
    const double2 *tab = reinterpret_cast<const double2 *>(gtab);
    const double l0 = (1.0 - rho_l) * lam[2 * k] + rho_l * (eta0 + scale * red[1][0]);
    const double l1 = (1.0 - rho_l) * lam[2 * k + 1] + rho_l * (eta1 + scale * red[2][0]);
    lam[2 * k] = l0;
    lam[2 * k + 1] = l1;
    const double ps = digamma(l0 + l1, tab);
    elogbeta[2 * k] = digamma(l0, tab) - ps;
    elogbeta[2 * k + 1] = digamma(l1, tab) - ps;
  }
}

// ---- stratified random node steps (svils_batch_step_strat) -------------------------------------
// FastAMM2::infer (src/fastamm2.cc:565-640): a step is a star, but EVERY row of gamma moves -- the rows of the star towards
// alpha + scale phi, all others a step rho towards alpha.  The others are not written: gamma_i - alpha of an untouched row
// is multiplied by (1 - rho_s) at every step, so the host keeps the running c = sum log1p(-rho_s) and per row the c of its
// last write, and a row is caught up (caught_up, above) with the one factor f = exp(c - c_i) when it is next read.

struct StratArgs {
  uint32_t K, m, a;                 // entries of the step, its start node
  double *gamma;                    // [n][K]: group e writes row partner[e]; row a is only read
  const double *elogbeta;
  const uint32_t *partner;          // [m]
  const uint8_t *y;                 // [m]
  const double *fj;                 // [m]: what catches row partner[e] up
  double fa;                        // ... and row a
  double logeps, alpha, scale, rho;
  double *part_a, *pl;              // per-wavefront partials, as StepArgs
  unsigned long long *ctr;
  const double *gtab;
};

// First launch of a step: group e holds the pair (a, partner[e]).  Both rows are caught up and their Elogpi formed in
// registers -- the Elogpi buffer is neither read nor written.  Row j belongs to its group (a partner is listed once),
// which writes the blended row; row a is only read.  phi_a and the lambda terms leave per wavefront.
template <int W, int V>
__global__ __launch_bounds__(256) void k_batch_strat_pairs(StratArgs x) {
  constexpr int G = 64 / W;
  __shared__ double2 logtab[128];
  load_logtab(logtab, x.gtab);
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane / W, lw = lane % W;
  const uint32_t K = x.K, a = x.a, wv = blockIdx.x * 4 + wave, e = wv * G + g;
  const bool valid = e < x.m;
  const uint32_t j = valid ? x.partner[e] : 0;
  const bool y = valid && x.y[e] != 0;
  const double f = valid ? x.fj[e] : 1.0;
  bool kval[V];
  double ga[V], gj[V], ef[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const uint32_t k = v * W + lw;
    kval[v] = k < K;
    ga[v] = kval[v] ? caught_up(x.gamma[(size_t)a * K + k], x.alpha, x.fa) : 0.0;
    gj[v] = kval[v] && valid ? caught_up(x.gamma[(size_t)j * K + k], x.alpha, f) : 0.0;
    ef[v] = kval[v] ? x.elogbeta[2 * k + (y ? 0 : 1)] : 0.0;
  }
  double ela[V], elj[V], pa[V], pj[V];
  row_elogpi<W, V>(ga, kval, true, logtab, ela);
  row_elogpi<W, V>(gj, kval, valid, logtab, elj);
#pragma unroll
  for (int v = 0; v < V; ++v) pa[v] = pj[v] = phi_start(kval[v], K);
  uint32_t rounds, under = 0;
  pair_fixed_point<W, V>(ela, elj, ef, y ? x.logeps : 0.0, kval, K, valid, pa, pj, rounds, under);
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const uint32_t k = v * W + lw;
    pa[v] = valid ? pa[v] : 0.0;
    pj[v] = valid ? pj[v] : 0.0;
    if (valid && kval[v]) x.gamma[(size_t)j * K + k] = (1.0 - x.rho) * gj[v] + x.rho * (x.alpha + x.scale * pj[v]);
    wave_partial<W, true>(pa[v], pj[v], y, kval[v], g, k, wv, K, x.part_a, x.pl);
  }
  const bool cnt = valid && lw == 0;
  count_pairs(x.ctr, lane, cnt, cnt ? rounds : 0, cnt ? rounds : 0, cnt ? under : 0);
}

// Last launch of a step, block k: the fixed-order sums of k_batch_step_tail over the nwv wavefronts of the first launch
// (nwv = 0, a step without entries: zero sums); gamma[a][k] caught up, then blended; lambda[k] and Elogbeta[k] as there.
// A kernel of its own: k_batch_step_tail keeps its text, and with it the bits of the steps that run it
__global__ __launch_bounds__(256) void k_batch_strat_tail(uint32_t K, uint32_t nwv, const double *__restrict__ part_a,
                                                          const double *__restrict__ pl, double *__restrict__ gamma_a, double alpha,
                                                          double fa, double eta0, double eta1, double scale, double rho_g,
                                                          double rho_l, double *__restrict__ lam, double *__restrict__ elogbeta,
                                                          const double *__restrict__ gtab) {
  __shared__ double red[3][256];
  const uint32_t k = blockIdx.x, t = threadIdx.x;
  double sa = 0.0, s0 = 0.0, s1 = 0.0;
  for (uint32_t w = t; w < nwv; w += 256) {
    sa += part_a[(size_t)w * K + k];
    s0 += pl[((size_t)w * K + k) * 2];
    s1 += pl[((size_t)w * K + k) * 2 + 1];
  }
  red[0][t] = sa;
  red[1][t] = s0;
  red[2][t] = s1;
  __syncthreads();
  for (uint32_t o = 128; o > 0; o >>= 1) {
    if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; red[2][t] += red[2][t + o]; }
    __syncthreads();
  }
  if (t != 0) return;
  gamma_a[k] = (1.0 - rho_g) * caught_up(gamma_a[k], alpha, fa) + rho_g * (alpha + scale * red[0][0]);
  if (rho_l >= 0.0) {
    const double2 *tab = reinterpret_cast<const double2 *>(gtab);
    const double l0 = (1.0 - rho_l) * lam[2 * k] + rho_l * (eta0 + scale * red[1][0]);
    const double l1 = (1.0 - rho_l) * lam[2 * k + 1] + rho_l * (eta1 + scale * red[2][0]);
    lam[2 * k] = l0;
    lam[2 * k + 1] = l1;
    const double ps = digamma(l0 + l1, tab);
    elogbeta[2 * k] = digamma(l0, tab) - ps;
    elogbeta[2 * k + 1] = digamma(l1, tab) - ps;
  }
}

// every row at its true value: one thread per cell, one factor per row; a row with f == 1 exactly is not rewritten
__global__ __launch_bounds__(256) void k_batch_catch_up(uint64_t nk, uint32_t K, double alpha, const double *__restrict__ fac,
                                                        double *__restrict__ gamma) {
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= nk) return;
  const double f = fac[x / K];
  if (f != 1.0) gamma[x] = alpha + (gamma[x] - alpha) * f;
}

// ---- informative-set steps (svils_batch_step_star) ---------------------------------------------
// FastAMM::infer (src/fastamm.cc:565-616) with opt_process / opt_process_noninf (:915-1126): a step is a star -- a start
// node a and the listed partners j -- and moves only the rows it names, each with its own step size.  A chain of steps
// runs in ONE workgroup of ONE launch: step t + 1 reads rows step t wrote, and between them stands a __syncthreads(),
// not a launch.  Passes of STAR_WAVES x 64 / W entries run over a step's list; group e of a pass holds pair (a, j_e),
// blends gamma_j and writes Elogpi_j itself (a partner is listed once per step: one owner per row); phi_a and the lambda
// terms stay in the group's registers across the passes, leave per wavefront to LDS and are added there in ascending
// wavefront order by thread k.  The kernel waits on nothing but its own barriers.  gamma / Elogpi / lambda / Elogbeta are
// read and written here: plain pointers, plain loads.
constexpr int STAR_THREADS = 512, STAR_WAVES = STAR_THREADS / 64;
constexpr uint32_t STAR_CHAIN = 64;   // steps per launch unless svils_batch_set_star_chain says otherwise
constexpr uint32_t STAR_CHAIN_MAX = SVILS_BATCH_STAR_CHAIN_MAX;   // ... and the most it may say

struct StarArgs {
  uint32_t K, s0, s1;                         // the launch runs steps [s0, s1) of the call
  double *gamma, *elogpi, *lam, *elogbeta;
  const double *gtab;
  double logeps, alpha, eta0, eta1;
  const uint32_t *off, *start, *partner;      // [nsteps + 1], [nsteps], [total]
  const uint8_t *y;                           // [total]
  const double *rho_partner, *rho_start, *scale, *rho_lambda;   // [total], [nsteps] x 3
  unsigned long long *ctr;
};

template <int W, int V>
__global__ __launch_bounds__(STAR_THREADS) void k_batch_star_chain(StarArgs x) {
  constexpr int G = 64 / W, WV = W * V;
  constexpr uint32_t P = STAR_WAVES * G;      // entries per pass
  __shared__ double2 logtab[128];
  __shared__ double part[STAR_WAVES][3][WV];  // per wavefront: phi_a, the y = 1 and the y = 0 lambda terms
  __shared__ double rowa[WV];                 // the new gamma_a
  load_logtab(logtab, x.gtab);
  __syncthreads();
  const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63, g = lane / W, lw = lane % W, K = x.K;
  bool kval[V];
#pragma unroll
  for (int v = 0; v < V; ++v) kval[v] = (uint32_t)(v * W) + lw < K;
  uint32_t npairs = 0, rtot = 0, rmax = 0, nunder = 0;
  for (uint32_t s = x.s0; s < x.s1; ++s) {
    const uint32_t a = x.start[s], e0 = x.off[s], e1 = x.off[s + 1];
    const double scale = x.scale[s];
    double ela[V], ef0[V], ef1[V], acc[V], l0[V], l1[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const uint32_t k = v * W + lw;
      ela[v] = kval[v] ? x.elogpi[(size_t)a * K + k] : 0.0;
      ef1[v] = kval[v] ? x.elogbeta[2 * k] : 0.0;
      ef0[v] = kval[v] ? x.elogbeta[2 * k + 1] : 0.0;
      acc[v] = l0[v] = l1[v] = 0.0;
    }
    for (uint32_t base = e0; base < e1; base += P) {   // the same trip count in every wavefront
      const uint32_t e = base + wave * G + g;
      const bool valid = e < e1;
      const uint32_t j = valid ? x.partner[e] : 0;
      const bool y = valid && x.y[e] != 0;
      const double rho = valid ? x.rho_partner[e] : 1.0;
      double elj[V], ef[V], pa[V], pj[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        elj[v] = kval[v] && valid ? x.elogpi[(size_t)j * K + v * W + lw] : 0.0;
        ef[v] = y ? ef1[v] : ef0[v];
        pa[v] = pj[v] = phi_start(kval[v], K);
      }
      uint32_t rounds;
      pair_fixed_point<W, V>(ela, elj, ef, y ? x.logeps : 0.0, kval, K, valid, pa, pj, rounds, nunder);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        pa[v] = valid ? pa[v] : 0.0;
        pj[v] = valid ? pj[v] : 0.0;
      }
      blend_row<W, V>(valid, j, K, lw, kval, pj, rho, x.alpha, scale, x.gamma, x.elogpi, logtab);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const double pp = pa[v] * pj[v];
        acc[v] += pa[v];
        l0[v] += y ? pp : 0.0;
        l1[v] += y ? 0.0 : pp;
      }
      const bool cnt = valid && lw == 0;
      npairs += cnt;
      rtot += cnt ? rounds : 0;
      rmax = max(rmax, cnt ? rounds : 0);
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const double sa = cross_group_sum<W>(acc[v]), t0 = cross_group_sum<W>(l0[v]), t1 = cross_group_sum<W>(l1[v]);
      if (g == 0) {
        part[wave][0][v * W + lw] = sa;
        part[wave][1][v * W + lw] = t0;
        part[wave][2][v * W + lw] = t1;
      }
    }
    __syncthreads();
    if (t < K) {   // thread k: the wavefronts' partials of community k in ascending order; gamma_a[k], lambda[k], Elogbeta[k]
      double sa = 0.0, s0 = 0.0, s1 = 0.0;
      for (int w = 0; w < STAR_WAVES; ++w) {
        sa += part[w][0][t];
        s0 += part[w][1][t];
        s1 += part[w][2][t];
      }
      const double rho_a = x.rho_start[s], rho_l = x.rho_lambda[s];
      const double ga = (1.0 - rho_a) * x.gamma[(size_t)a * K + t] + rho_a * (x.alpha + scale * sa);
      x.gamma[(size_t)a * K + t] = ga;
      rowa[t] = ga;
      if (rho_l >= 0.0) {
        const double n0 = (1.0 - rho_l) * x.lam[2 * t] + rho_l * (x.eta0 + scale * s0);
        const double n1 = (1.0 - rho_l) * x.lam[2 * t + 1] + rho_l * (x.eta1 + scale * s1);
        x.lam[2 * t] = n0;
        x.lam[2 * t + 1] = n1;
        const double ps = digamma(n0 + n1, logtab);
        x.elogbeta[2 * t] = digamma(n0, logtab) - ps;
        x.elogbeta[2 * t + 1] = digamma(n1, logtab) - ps;
      }
    }
    __syncthreads();
    if (wave == 0) {   // Elogpi_a as k_batch_dir_exp forms it
      double rs = 0.0;
      for (uint32_t k = lane; k < K; k += 64) rs += rowa[k];
      const double ps = digamma(wave_sum_f64(rs), logtab);
      for (uint32_t k = lane; k < K; k += 64) x.elogpi[(size_t)a * K + k] = digamma(rowa[k], logtab) - ps;
    }
    __syncthreads();   // the next step reads what this one wrote
  }
  count_pairs(x.ctr, lane, npairs, rtot, rmax, lw == 0 ? nunder : 0);
}

}  // namespace

// events: ev[0] sweep begin, ev[1] Elogpi / Elogbeta done, then per launch of the pair kernel ev[2 + 2 b] (pairs done) and
// ev[3 + 2 b] (reduced)
struct svils_batch : ToolHandle {
  uint32_t n = 0, k = 0, w = 0, ta = 0, nw = 0;
  bool sparse = false;                                            // svils_batch_create_sparse: no n x n structure anywhere
  HostCsr h_links, h_skips;                                       // sparse form (svils_csr.h): what h_adj / h_skip are to the dense form
  double alpha = 0, eta0 = 0, eta1 = 0, epsilon = 0;
  // HANDLE scope
  double *gamma = nullptr, *gnext = nullptr, *elogpi = nullptr;   // [n][k]
  double *lam = nullptr, *lnext = nullptr, *elogbeta = nullptr;   // [k][2]
  double *gtab = nullptr;                                         // [128][2] log_tab's table
  unsigned long long *ctr = nullptr;                              // [5]
  // GRAPH scope
  uint32_t *adj = nullptr, *skip = nullptr;                       // [n][nw] (dense form)
  uint64_t *lrow = nullptr, *srow = nullptr;                      // sparse form: the links and the skip pairs as symmetric
  uint32_t *lcol = nullptr, *scol = nullptr;                      // CSRs, [n + 1] offsets and ascending rows
  uint32_t *tiles = nullptr, *rowoff = nullptr, *jfirst = nullptr;
  double *pa = nullptr, *pb = nullptr, *pl = nullptr;
  uint32_t *ll_pairs = nullptr;                                   // svils_batch_pair_loglik: grown on demand
  uint8_t *ll_y = nullptr;
  double *ll_out = nullptr;
  uint32_t ntiles = 0, nrb = 0, batch = 0;                        // batch: tiles per launch
  std::vector<uint32_t> h_tiles;
  bool have_graph = false, have_state = false;
  // the last timed call: a sweep (ev[0] .. and the launches' events), a step call (ev[0] .. ev[1] bracket it), svils_batch_elbo
  // (ev_elbo; the sweep's events are as they were)
  enum class Timed { NONE, SWEEP, STEPS, ELBO } timed = Timed::NONE;
  uint32_t nlaunch = 0;                                           // launches of the last sweep
  // sampled-pair steps.  HANDLE scope, grown on demand: the per-wavefront partials, one step's phi, a call's lists
  bool elog_fresh = false;                                        // Elogpi / Elogbeta are those of gamma / lambda
  std::vector<uint32_t> h_skip;                                   // the skip bits, to refuse a listed skipped pair
  std::vector<uint32_t> h_adj;                                    // the link bits, to refuse a star entry whose y disagrees: fetched by the first star call
  uint32_t star_chain = STAR_CHAIN;                               // steps per launch of k_batch_star_chain
  double *st_part = nullptr, *st_pl = nullptr, *st_phi = nullptr;
  uint32_t *st_lists = nullptr;                                   // a call's pairs [total][2], entries [2 total], offsets [nsteps][n + 1]
  uint32_t *pin = nullptr;                                        // pinned staging of st_lists; ev_copy: its last copy has left it
  size_t cap_pin = 0;
  hipEvent_t ev_copy = nullptr;
  bool copy_pending = false;
  // stratified random node steps (svils_batch_step_strat): the decay of the rows no step wrote, kept on the host.  A
  // row's true value is alpha + (gamma_i - alpha) exp(lag_c - row_c[i])
  double lag_c = 0.0;                                             // sum of log1p(-rho_s) over the strat steps, in step order
  std::vector<double> row_c;                                      // [n] what lag_c was when the row was last written
  bool behind = false;                                            // a strat step ran since every row was last at its true value
  bool elogbeta_fresh = false;                                    // Elogbeta is that of lambda (the strat steps keep it, not Elogpi)
  std::vector<double> h_fac;                                      // [n] the factors of a catch-up, alive until its copy is done
  double *d_fac = nullptr;                                        // HANDLE scope
  // the lower bound (svils_batch_elbo): buffers, counters and events of its own -- nothing a sweep or a step reads
  uint32_t elbo_tiles = BATCH_TILES;                              // tiles per launch of k_batch_elbo
  double *el_part = nullptr;                                      // GRAPH scope: [ntiles][4]
  double *el_node = nullptr, *el_out = nullptr;                   // HANDLE scope: [n], [4]
  unsigned long long *el_ctr = nullptr;                           // HANDLE scope: [5]
  hipEvent_t ev_elbo[2] = {nullptr, nullptr};                     // the bracket of the last pass
};

namespace {

void free_graph(svils_batch *h) {
  h->release(ToolHandle::GRAPH);
  h->have_graph = false;
  std::vector<uint32_t>().swap(h->h_skip);   // the host copies of the graph's bits go with it
  std::vector<uint32_t>().swap(h->h_adj);
  h->h_links.clear();
  h->h_skips.clear();
}

// the host's answer to "is (p, q), p < q, in the skip set" / "is it a link", in either form
bool host_skipped(const svils_batch *h, uint32_t p, uint32_t q) {
  return h->sparse ? h->h_skips.has(p, q) : (h->h_skip[(size_t)p * h->nw + (q >> 5)] & (1u << (q & 31))) != 0;
}
bool host_link(const svils_batch *h, uint32_t p, uint32_t q) {
  return h->sparse ? h->h_links.has(p, q) : (h->h_adj[(size_t)p * h->nw + (q >> 5)] & (1u << (q & 31))) != 0;
}

// the all-pairs passes walk the tiles of the bit matrices
int dense_only(const svils_batch *h, const char *name) {
  if (h->sparse)
    return fail(SVILS_ERR_UNSUPPORTED, "%s: the all-pairs passes need the dense form (svils_batch_create), this handle is in sparse form", name);
  return 0;
}

DenseGraph dense_graph(const svils_batch *h) { return DenseGraph{h->adj, h->skip, h->nw}; }
SparseGraph sparse_graph(const svils_batch *h) { return SparseGraph{h->lrow, h->srow, h->lcol, h->scol}; }

// *p = count elements, as ToolHandle::reserve (for a pointer the scope does not hold yet: a plain allocation); where the
// device has no room, the message the allocation left is replaced by one that names the buffer
template <class T>
int reserve_named(svils_batch *h, ToolHandle::Scope s, T **p, size_t count, const char *name, const char *what) {
  const int rc = h->reserve(s, p, count);
  if (rc == SVILS_ERR_NOMEM) return fail(SVILS_ERR_NOMEM, "%s: out of device memory for %s (%zu bytes)", name, what, count * sizeof(T));
  return rc;
}

// The launch table, the one place that maps the handle's lane width to an instantiation: launch(Width<W>()) for W = h->w.
// The caller's generic lambda names the kernel <decltype(w)::value, VARIANT_V>, its grid and its block.
template <int W>
struct Width {
  static constexpr int value = W;
};
template <class Launch>
int launch_for_width(const svils_batch *h, const char *name, Launch &&launch) {
  switch (h->w) {
    case 1: launch(Width<1>()); break;
    case 2: launch(Width<2>()); break;
    case 4: launch(Width<4>()); break;
    case 8: launch(Width<8>()); break;
    case 16: launch(Width<16>()); break;
    case 32: launch(Width<32>()); break;
    case 64: launch(Width<64>()); break;
    default: return fail(SVILS_ERR_UNSUPPORTED, "%s: no kernel for W = %u", name, h->w);   // a missing kernel is an error
  }
  return 0;
}

// waits for the stream; the sticky underflow counter becomes an error
int settle(svils_batch *h, const char *name) {
  unsigned long long c = 0;
  HIPCHK(hipMemcpyAsync(&c, h->ctr + 4, sizeof c, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  if (c)
    return fail(SVILS_ERR_UNSUPPORTED, "%s: phi normaliser underflow in %llu pair(s) since the state was set (the reference asserts s > 0 there)",
                name, c);
  return 0;
}

// Every row of gamma at its true value: what every entry point other than svils_batch_step_strat runs before it reads
// or writes gamma.  Nothing to do unless a strat step ran since the last one; the bookkeeping starts again from zero
int catch_up(svils_batch *h) {
  if (!h->behind) return 0;
  const uint32_t n = h->n, K = h->k;
  HIPCHK(hipStreamSynchronize(h->st));   // h_fac may still be on its way from the previous catch-up
  h->h_fac.resize(n);
  for (uint32_t i = 0; i < n; ++i) h->h_fac[i] = std::exp(h->lag_c - h->row_c[i]);   // exp(0) is 1 exactly
  if (int rc = h->reserve(ToolHandle::HANDLE, &h->d_fac, (size_t)n)) return rc;
  HIPCHK(hipMemcpyAsync(h->d_fac, h->h_fac.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->st));
  const uint64_t nk = (uint64_t)n * K;
  hipLaunchKernelGGL(k_batch_catch_up, dim3(blocks(nk, 256)), dim3(256), 0, h->st, nk, K, h->alpha, h->d_fac, h->gamma);
  HIPCHK(hipGetLastError());
  h->lag_c = 0.0;
  std::fill(h->row_c.begin(), h->row_c.end(), 0.0);
  h->behind = false;
  return 0;
}

int one_sweep(svils_batch *h) {
  const uint32_t n = h->n, K = h->k;
  const uint64_t nk = (uint64_t)n * K;
  HIPCHK(hipEventRecord(h->ev[0], h->st));
  hipLaunchKernelGGL(k_batch_dir_exp, dim3(blocks(n, 4)), dim3(256), 0, h->st, n, K, h->gamma, h->gtab, h->elogpi);
  hipLaunchKernelGGL(k_batch_beta, dim3(blocks(K, 256)), dim3(256), 0, h->st, K, h->lam, h->gtab, h->elogbeta);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev[1], h->st));
  hipLaunchKernelGGL(k_batch_fill, dim3(blocks(std::max<uint64_t>(nk, K), 256)), dim3(256), 0, h->st, nk, K, h->alpha, h->eta0,
                     h->eta1, h->gnext, h->lnext);
  HIPCHK(hipMemsetAsync(h->ctr, 0, 4 * sizeof(unsigned long long), h->st));
  uint32_t b = 0;
  for (uint32_t t0 = 0; t0 < h->ntiles; t0 += h->batch, ++b) {
    const uint32_t t1 = std::min(h->ntiles, t0 + h->batch), nt = t1 - t0;
    PairArgs a{n, K, h->nw, t0, h->tiles, h->adj, h->skip, h->elogpi, h->elogbeta, std::log(h->epsilon), h->pa, h->pb, h->pl, h->ctr};
    if (int rc = launch_for_width(h, "svils_batch_sweep", [&](auto w) {
          hipLaunchKernelGGL((k_batch_pairs<decltype(w)::value, (int)VARIANT_V>), dim3(nt), dim3(256), 0, h->st, a);
        }))
      return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev[2 + 2 * b], h->st));
    ReduceArgs r{n, K, h->ta, t0, t1, h->h_tiles[2 * (size_t)t0], h->h_tiles[2 * (size_t)(t1 - 1)], h->nrb, h->rowoff, h->jfirst,
                 h->pa, h->pb, h->gnext};
    hipLaunchKernelGGL(k_batch_reduce_gamma, dim3(blocks(nk, 256)), dim3(256), 0, h->st, r);
    hipLaunchKernelGGL(k_batch_reduce_lambda, dim3(K), dim3(256), 0, h->st, K, 4 * nt, h->pl, h->lnext);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev[3 + 2 * b], h->st));
  }
  h->nlaunch = b;
  std::swap(h->gamma, h->gnext);   // gamma = gamma_next (:883-886); later launches take the new pointers
  std::swap(h->lam, h->lnext);
  h->timed = svils_batch::Timed::SWEEP;
  h->elog_fresh = h->elogbeta_fresh = false;
  return 0;
}

// ---- sampled-pair steps: host side ----
// what both step entry points check of their handle and step sizes
int check_steps(svils_batch *h, const char *name, uint32_t nsteps, const double *rho_gamma, const double *rho_lambda) {
  if (!h->have_graph || !h->have_state) return fail(SVILS_ERR_ARG, "%s: set the graph and the state first", name);
  for (uint32_t s = 0; s < nsteps; ++s) {
    if (!(rho_gamma[s] > 0.0 && rho_gamma[s] <= 1.0)) return fail(SVILS_ERR_ARG, "%s: rho_gamma[%u] is not in (0, 1]", name, s);
    if (!(rho_lambda[s] <= 1.0)) return fail(SVILS_ERR_ARG, "%s: rho_lambda[%u] is not <= 1 (negative: lambda is left alone)", name, s);
  }
  return 0;
}

// Elogpi / Elogbeta of the current state if a sweep or set_state came in between; the counters of the call start at zero
int renew_expectations(svils_batch *h) {
  if (h->elog_fresh) return 0;
  hipLaunchKernelGGL(k_batch_dir_exp, dim3(blocks(h->n, 4)), dim3(256), 0, h->st, h->n, h->k, h->gamma, h->gtab, h->elogpi);
  hipLaunchKernelGGL(k_batch_beta, dim3(blocks(h->k, 256)), dim3(256), 0, h->st, h->k, h->lam, h->gtab, h->elogbeta);
  HIPCHK(hipGetLastError());
  h->elog_fresh = h->elogbeta_fresh = true;
  return 0;
}

int begin_steps(svils_batch *h) {
  if (int rc = renew_expectations(h)) return rc;
  HIPCHK(hipMemsetAsync(h->ctr, 0, 4 * sizeof(unsigned long long), h->st));
  HIPCHK(hipEventRecord(h->ev[0], h->st));
  return 0;
}

int end_steps(svils_batch *h) {
  HIPCHK(hipEventRecord(h->ev[1], h->st));
  h->timed = svils_batch::Timed::STEPS;
  return 0;
}

// What the star entry points (svils_batch_step_star, _step_strat) check of their entries: the partner a node other than
// the start, listed once in its step (seen[j] = s + 1: one owner per row), the pair outside the skip set, y the graph's
// link bit, and rho_partner, where the steps have one per entry, in (0, 1].  The link bits come back from the device once
// per graph, for handles that take such steps
int check_star_entries(svils_batch *h, const char *name, uint32_t nsteps, const uint32_t *start, const uint64_t *off,
                       const uint32_t *partner, const uint8_t *y, const double *rho_partner) {
  const uint32_t n = h->n;
  if (off[nsteps] && !h->sparse && h->h_adj.empty()) {
    std::vector<uint32_t> bits((size_t)n * h->nw);
    HIPCHK(hipStreamSynchronize(h->st));
    HIPCHK(hipMemcpy(bits.data(), h->adj, bits.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    h->h_adj.swap(bits);
  }
  std::vector<uint32_t> seen(n, 0);
  for (uint32_t s = 0; s < nsteps; ++s)
    for (uint64_t e = off[s]; e < off[s + 1]; ++e) {
      const uint32_t a = start[s], j = partner[e];
      const unsigned long long x = e - off[s];
      if (j >= n || j == a) return fail(SVILS_ERR_ARG, "%s: entry %llu of step %u pairs node %u with %u (n = %u)", name, x, s, a, j, n);
      if (seen[j] == s + 1) return fail(SVILS_ERR_ARG, "%s: entry %llu of step %u lists partner %u twice", name, x, s, j);
      seen[j] = s + 1;
      const uint32_t p = std::min(a, j), q = std::max(a, j);
      if (host_skipped(h, p, q)) return fail(SVILS_ERR_ARG, "%s: entry %llu of step %u (%u, %u) is in the skip set", name, x, s, p, q);
      if (host_link(h, p, q) != (y[e] != 0))
        return fail(SVILS_ERR_ARG, "%s: entry %llu of step %u (%u, %u) has y = %u, the graph says otherwise", name, x, s, p, q, (unsigned)y[e]);
      if (rho_partner && !(rho_partner[e] > 0.0 && rho_partner[e] <= 1.0))
        return fail(SVILS_ERR_ARG, "%s: rho_partner of entry %llu of step %u is not in (0, 1]", name, x, s);
    }
  return 0;
}

// A call's lists on their way to the device: typed segments, back to back in the pinned staging area and, after ONE async
// copy, at the same offsets in st_lists, so that the call need not wait for it.  A call declares its segments with add(),
// open()s the pinned area (its host arrays are copied in; a segment without one is the caller's to fill through pinned()),
// send()s it and takes the device pointers.
// THE ALIGNMENT RULE: doubles are declared first, then 32-bit words, then bytes.  Both areas start aligned for a double
// and offsets are kept in 32-bit words, so every segment then starts at a multiple of its element size; bytes, which come
// last, are rounded up to whole words.  add() asserts the order; the library is built without NDEBUG (build.py), so the
// assert is there in the product build too.
class Staging {
 public:
  template <class T>
  struct Seg {
    size_t at;   // in 32-bit words
  };
  explicit Staging(svils_batch *h) : h_(h) {}
  template <class T>
  Seg<T> add(const T *src, size_t count) {
    assert(sizeof(T) <= elem_);
    elem_ = sizeof(T);
    segs_.push_back({src, count * sizeof(T), nwords_});
    nwords_ += (count * sizeof(T) + 3) / 4;
    return {segs_.back().at};
  }
  // the pinned area: free again once the previous call's copy has left it
  int open() {
    svils_batch *h = h_;
    if (h->copy_pending) {
      HIPCHK(hipEventSynchronize(h->ev_copy));
      h->copy_pending = false;
    }
    if (!h->ev_copy) HIPCHK(hipEventCreateWithFlags(&h->ev_copy, hipEventDisableTiming));
    if (nwords_ > h->cap_pin) {
      if (h->pin) (void)hipHostFree(h->pin);
      h->pin = nullptr;
      h->cap_pin = 0;
      HIPCHK(hipHostMalloc((void **)&h->pin, nwords_ * sizeof(uint32_t), hipHostMallocDefault));
      h->cap_pin = nwords_;
    }
    for (const Segment &s : segs_)
      if (s.src && s.bytes) std::memcpy(h->pin + s.at, s.src, s.bytes);
    return 0;
  }
  // ordered behind the steps of earlier calls, which read the device copy, by the stream
  int send() {
    svils_batch *h = h_;
    if (int rc = h->reserve(ToolHandle::HANDLE, &h->st_lists, nwords_)) return rc;
    HIPCHK(hipMemcpyAsync(h->st_lists, h->pin, nwords_ * sizeof(uint32_t), hipMemcpyHostToDevice, h->st));
    HIPCHK(hipEventRecord(h->ev_copy, h->st));
    h->copy_pending = true;
    return 0;
  }
  template <class T>
  T *pinned(Seg<T> s) const { return reinterpret_cast<T *>(h_->pin + s.at); }
  template <class T>
  const T *device(Seg<T> s) const { return reinterpret_cast<const T *>(h_->st_lists + s.at); }

 private:
  struct Segment {
    const void *src;
    size_t bytes, at;
  };
  svils_batch *h_;
  std::vector<Segment> segs_;
  size_t nwords_ = 0, elem_ = sizeof(double);
};

// svils_batch_set_graph of a sparse-form handle: the two CSRs, on the host for the checks of the step calls and on the
// device for the step kernels.  No tile list, no tile partials, no bit copies: nothing here is n x n
int set_graph_sparse(svils_batch *h, const uint32_t *links, uint64_t nlinks, const uint32_t *skip, uint64_t nskip) {
  HostCsr lk, sk;
  if (int rc = build_csr("svils_batch_set_graph", h->n, links, nlinks, "link", lk)) return rc;
  if (int rc = build_csr("svils_batch_set_graph", h->n, skip, nskip, "skipped pair", sk)) return rc;
  HIPCHK(hipStreamSynchronize(h->st));
  free_graph(h);
  const auto scope = ToolHandle::GRAPH;
  int rc = h->upload(scope, &h->lrow, lk.row);
  if (!rc) rc = h->upload(scope, &h->lcol, lk.col);   // an empty list: a null pointer no search reads
  if (!rc) rc = h->upload(scope, &h->srow, sk.row);
  if (!rc) rc = h->upload(scope, &h->scol, sk.col);
  if (!rc && hipStreamSynchronize(h->st) != hipSuccess) rc = fail(SVILS_ERR_DEVICE, "svils_batch_set_graph: upload failed");
  if (rc) {
    free_graph(h);
    return rc;
  }
  h->h_links.row.swap(lk.row);
  h->h_links.col.swap(lk.col);
  h->h_skips.row.swap(sk.row);
  h->h_skips.col.swap(sk.col);
  std::vector<uint32_t>().swap(h->h_tiles);
  h->ntiles = h->nrb = h->batch = 0;
  h->have_graph = true;
  h->timed = svils_batch::Timed::NONE;
  return 0;
}

StepArgs step_args(svils_batch *h, double scale, double rho) {
  StepArgs x{};
  x.n = h->n;
  x.K = h->k;
  x.gamma = h->gamma;
  x.elogpi = h->elogpi;
  x.elogbeta = h->elogbeta;
  x.logeps = std::log(h->epsilon);
  x.alpha = h->alpha;
  x.scale = scale;
  x.rho = rho;
  x.part_a = h->st_part;
  x.pl = h->st_pl;
  x.ctr = h->ctr;
  x.gtab = h->gtab;
  return x;
}

}  // namespace

extern "C" {

int svils_batch_variant(uint32_t k, uint32_t *w, uint32_t *v) {
  if (!w || !v) return fail(SVILS_ERR_ARG, "svils_batch_variant: null argument");
  if (k < 2) return fail(SVILS_ERR_ARG, "svils_batch_variant: need k >= 2");
  if (k > SVILS_BATCH_MAX_K) return fail(SVILS_ERR_UNSUPPORTED, "svils_batch_variant: k = %u exceeds SVILS_BATCH_MAX_K = %d", k, SVILS_BATCH_MAX_K);
  *w = variant_w(k);
  *v = VARIANT_V;
  return 0;
}

// both forms of the handle: the dense form (sparse = false) keeps the n cap of its bit matrices, the sparse form has none
static int create_batch(const char *name, bool sparse, int device, uint32_t n, uint32_t k, double alpha, double eta0, double eta1,
                        double epsilon, svils_batch **out) {
  if (!out) return fail(SVILS_ERR_ARG, "%s: null argument", name);
  *out = nullptr;
  if (n < 2 || k < 2 || !(alpha > 0) || !(eta0 > 0) || !(eta1 > 0) || !(epsilon > 0) || !(epsilon < 1))
    return fail(SVILS_ERR_ARG, "%s: need n >= 2, k >= 2, alpha, eta0, eta1 > 0 and 0 < epsilon < 1", name);
  if (k > SVILS_BATCH_MAX_K) return fail(SVILS_ERR_UNSUPPORTED, "%s: k = %u exceeds SVILS_BATCH_MAX_K = %d", name, k, SVILS_BATCH_MAX_K);
  if (!sparse && n > SVILS_BATCH_MAX_N) return fail(SVILS_ERR_UNSUPPORTED, "%s: n = %u exceeds SVILS_BATCH_MAX_N = %d", name, n, SVILS_BATCH_MAX_N);
  if (int rc = open_device(device)) return rc;
  svils_batch *h = new (std::nothrow) svils_batch();
  if (!h) return fail(SVILS_ERR_NOMEM, "out of host memory");
  h->n = n;
  h->k = k;
  h->w = variant_w(k);
  h->ta = 4 * (uint32_t)rows_per_wave((int)(h->w * VARIANT_V));
  h->sparse = sparse;
  h->nw = sparse ? 0 : (n + 31) / 32;
  h->alpha = alpha;
  h->eta0 = eta0;
  h->eta1 = eta1;
  h->epsilon = epsilon;
  h->row_c.assign(n, 0.0);
  const auto scope = ToolHandle::HANDLE;
  const size_t nk = (size_t)n * k;
  int rc = h->open(device, 2);
  if (!rc) rc = reserve_named(h, scope, &h->gamma, nk, name, "gamma");
  if (!rc) rc = reserve_named(h, scope, &h->gnext, nk, name, "gamma_next");
  if (!rc) rc = reserve_named(h, scope, &h->elogpi, nk, name, "Elogpi");
  if (!rc) rc = reserve_named(h, scope, &h->lam, 2 * (size_t)k, name, "lambda");
  if (!rc) rc = reserve_named(h, scope, &h->lnext, 2 * (size_t)k, name, "lambda_next");
  if (!rc) rc = reserve_named(h, scope, &h->elogbeta, 2 * (size_t)k, name, "Elogbeta");
  if (!rc) rc = reserve_named(h, scope, &h->ctr, (size_t)5, name, "the counters");
  if (!rc) rc = h->upload(scope, &h->gtab, log_table());
  if (!rc && hipMemsetAsync(h->ctr, 0, 5 * sizeof(unsigned long long), h->st) != hipSuccess) rc = fail(SVILS_ERR_DEVICE, "%s: memset failed", name);
  if (!rc && hipStreamSynchronize(h->st) != hipSuccess) rc = fail(SVILS_ERR_DEVICE, "%s: upload failed", name);
  if (rc) {
    svils_batch_destroy(h);
    return rc;
  }
  *out = h;
  return 0;
}

int svils_batch_create(int device, uint32_t n, uint32_t k, double alpha, double eta0, double eta1, double epsilon, svils_batch **out) {
  return create_batch("svils_batch_create", false, device, n, k, alpha, eta0, eta1, epsilon, out);
}

int svils_batch_create_sparse(int device, uint32_t n, uint32_t k, double alpha, double eta0, double eta1, double epsilon,
                              svils_batch **out) {
  return create_batch("svils_batch_create_sparse", true, device, n, k, alpha, eta0, eta1, epsilon, out);
}

int svils_batch_destroy(svils_batch *h) {
  if (h && h->st) {   // the steps' staging area and its event are not in a scope
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->st);
    if (h->pin) (void)hipHostFree(h->pin);
    if (h->ev_copy) (void)hipEventDestroy(h->ev_copy);
    for (hipEvent_t e : h->ev_elbo)
      if (e) (void)hipEventDestroy(e);
  }
  delete h;   // ~ToolHandle: waits for the stream, frees both scopes
  return 0;
}

int svils_batch_set_graph(svils_batch *h, const uint32_t *links, uint64_t nlinks, const uint32_t *skip, uint64_t nskip) {
  if (int rc = check(h, "svils_batch_set_graph")) return rc;
  if ((nlinks && !links) || (nskip && !skip)) return fail(SVILS_ERR_ARG, "svils_batch_set_graph: null argument");
  if (h->sparse) return set_graph_sparse(h, links, nlinks, skip, nskip);
  const uint32_t n = h->n, nw = h->nw;
  std::vector<uint32_t> adj((size_t)n * nw, 0), skp((size_t)n * nw, 0);
  for (int which = 0; which < 2; ++which) {
    const uint32_t *list = which ? skip : links;
    const uint64_t cnt = which ? nskip : nlinks;
    std::vector<uint32_t> &bits = which ? skp : adj;
    for (uint64_t x = 0; x < cnt; ++x) {
      const uint32_t p = list[2 * x], q = list[2 * x + 1];
      if (p >= q || q >= n)
        return fail(SVILS_ERR_ARG, "svils_batch_set_graph: %s %llu (%u, %u) is not a pair p < q < n = %u", which ? "skipped pair" : "link",
                    (unsigned long long)x, p, q, n);
      uint32_t &wd = bits[(size_t)p * nw + (q >> 5)];
      if (wd & (1u << (q & 31)))
        return fail(SVILS_ERR_ARG, "svils_batch_set_graph: %s %llu (%u, %u) is repeated", which ? "skipped pair" : "link", (unsigned long long)x, p, q);
      wd |= 1u << (q & 31);
    }
  }
  // the tiles in (row block, column block) order: row block r holds rows [r TA, r TA + TA), its first column block is the one of
  // its first row's first partner
  const uint32_t TA = h->ta, ncb = (n + TILE_COLS - 1) / TILE_COLS, nrb = (n + TA - 1) / TA;
  std::vector<uint32_t> tiles, rowoff(nrb + 1, 0), jfirst(nrb, 0);
  for (uint32_t r = 0; r < nrb; ++r) {
    jfirst[r] = (r * TA + 1) / TILE_COLS;
    rowoff[r] = (uint32_t)(tiles.size() / 2);
    for (uint32_t c = jfirst[r]; c < ncb; ++c) { tiles.push_back(r); tiles.push_back(c); }
  }
  rowoff[nrb] = (uint32_t)(tiles.size() / 2);
  const uint32_t ntiles = rowoff[nrb];
  const size_t per_tile = ((size_t)TA + 4 * TILE_COLS) * h->k * sizeof(double);
  const uint32_t batch = (uint32_t)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(BATCH_TILES, ntiles), BATCH_BYTES / per_tile));
  const uint32_t nlaunch = (ntiles + batch - 1) / batch;
  HIPCHK(hipStreamSynchronize(h->st));
  free_graph(h);
  if (int rc = h->need_events(2 + 2 * (size_t)nlaunch)) return rc;
  const auto scope = ToolHandle::GRAPH;
  int rc = 0;
  if (!rc) rc = h->upload(scope, &h->adj, adj);
  if (!rc) rc = h->upload(scope, &h->skip, skp);
  if (!rc) rc = h->upload(scope, &h->tiles, tiles);
  if (!rc) rc = h->upload(scope, &h->rowoff, rowoff);
  if (!rc) rc = h->upload(scope, &h->jfirst, jfirst);
  if (!rc) rc = h->dalloc(scope, &h->pa, (size_t)batch * TA * h->k);
  if (!rc) rc = h->dalloc(scope, &h->pb, (size_t)batch * 4 * TILE_COLS * h->k);
  if (!rc) rc = h->dalloc(scope, &h->pl, (size_t)batch * 4 * h->k * 2);
  if (!rc && hipStreamSynchronize(h->st) != hipSuccess) rc = fail(SVILS_ERR_DEVICE, "svils_batch_set_graph: upload failed");
  if (rc) {
    free_graph(h);
    return rc;
  }
  h->h_tiles.swap(tiles);
  h->h_skip.swap(skp);
  h->ntiles = ntiles;
  h->nrb = nrb;
  h->batch = batch;
  h->have_graph = true;
  h->timed = svils_batch::Timed::NONE;
  return 0;
}

int svils_batch_set_state(svils_batch *h, const double *gamma, const double *lambda) {
  if (int rc = check(h, "svils_batch_set_state")) return rc;
  if (!gamma || !lambda) return fail(SVILS_ERR_ARG, "svils_batch_set_state: null argument");
  const size_t nk = (size_t)h->n * h->k;
  for (size_t x = 0; x < nk; ++x)
    if (!(gamma[x] > 0)) return fail(SVILS_ERR_ARG, "svils_batch_set_state: gamma[%zu] is not > 0", x);
  for (size_t x = 0; x < 2 * (size_t)h->k; ++x)
    if (!(lambda[x] > 0)) return fail(SVILS_ERR_ARG, "svils_batch_set_state: lambda[%zu] is not > 0", x);
  HIPCHK(hipStreamSynchronize(h->st));
  HIPCHK(hipMemcpy(h->gamma, gamma, nk * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->lam, lambda, 2 * (size_t)h->k * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(h->ctr, 0, 5 * sizeof(unsigned long long)));
  h->have_state = true;
  h->elog_fresh = h->elogbeta_fresh = false;
  h->lag_c = 0.0;   // the rows are as given: nothing is behind
  std::fill(h->row_c.begin(), h->row_c.end(), 0.0);
  h->behind = false;
  return 0;
}

int svils_batch_get_state(svils_batch *h, double *gamma, double *lambda) {
  if (int rc = check(h, "svils_batch_get_state")) return rc;
  if (!h->have_state) return fail(SVILS_ERR_ARG, "svils_batch_get_state: no state");
  if (int rc = catch_up(h)) return rc;
  if (int rc = settle(h, "svils_batch_get_state")) return rc;
  if (gamma) HIPCHK(hipMemcpy(gamma, h->gamma, (size_t)h->n * h->k * sizeof(double), hipMemcpyDeviceToHost));
  if (lambda) HIPCHK(hipMemcpy(lambda, h->lam, 2 * (size_t)h->k * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int svils_batch_sweep(svils_batch *h, uint32_t nsweeps) {
  if (int rc = check(h, "svils_batch_sweep")) return rc;
  if (int rc = dense_only(h, "svils_batch_sweep")) return rc;
  if (!h->have_graph || !h->have_state) return fail(SVILS_ERR_ARG, "svils_batch_sweep: set the graph and the state first");
  if (int rc = catch_up(h)) return rc;
  for (uint32_t s = 0; s < nsweeps; ++s)
    if (int rc = one_sweep(h)) return rc;
  return 0;
}

int svils_batch_step_node(svils_batch *h, uint32_t nsteps, const uint32_t *nodes, double scale, const double *rho_gamma,
                          const double *rho_lambda) {
  const char *name = "svils_batch_step_node";
  if (int rc = check(h, name)) return rc;
  if (nsteps && (!nodes || !rho_gamma || !rho_lambda)) return fail(SVILS_ERR_ARG, "%s: null argument", name);
  if (!(scale > 0.0) || !std::isfinite(scale)) return fail(SVILS_ERR_ARG, "%s: scale is not a positive number", name);
  if (int rc = check_steps(h, name, nsteps, rho_gamma, rho_lambda)) return rc;
  for (uint32_t s = 0; s < nsteps; ++s)
    if (nodes[s] >= h->n) return fail(SVILS_ERR_ARG, "%s: nodes[%u] = %u is not < n = %u", name, s, nodes[s], h->n);
  if (!nsteps) return 0;
  if (int rc = catch_up(h)) return rc;
  const uint32_t n = h->n, K = h->k, G = 64 / h->w, nb = blocks(n, 4 * G), nwv = 4 * nb;
  // the per-wavefront partials grow with n ([ceil(n / G)][K] and twice that): allocated by the first node step, not at creation
  if (int rc = reserve_named(h, ToolHandle::HANDLE, &h->st_part, (size_t)nwv * K, name, "the node steps' phi partials")) return rc;
  if (int rc = reserve_named(h, ToolHandle::HANDLE, &h->st_pl, (size_t)nwv * K * 2, name, "the node steps' lambda partials")) return rc;
  if (int rc = begin_steps(h)) return rc;
  for (uint32_t s = 0; s < nsteps; ++s) {
    StepArgs x = step_args(h, scale, rho_gamma[s]);
    x.a = nodes[s];
    const auto launch = [&](auto gr) {
      return launch_for_width(h, name, [&](auto w) {
        hipLaunchKernelGGL((k_batch_step_node<decltype(w)::value, (int)VARIANT_V, decltype(gr)>), dim3(nb), dim3(256), 0, h->st, x, gr);
      });
    };
    if (int rc = h->sparse ? launch(sparse_graph(h)) : launch(dense_graph(h)))
      return rc;
    double *ga = h->gamma + (size_t)x.a * K;
    hipLaunchKernelGGL(k_batch_step_tail, dim3(K), dim3(256), 0, h->st, K, nwv, h->st_part, h->st_pl, ga, h->alpha, h->eta0, h->eta1,
                       scale, rho_gamma[s], rho_lambda[s], h->lam, h->elogbeta, h->gtab);
    hipLaunchKernelGGL(k_batch_dir_exp, dim3(1), dim3(256), 0, h->st, 1u, K, ga, h->gtab, h->elogpi + (size_t)x.a * K);
    HIPCHK(hipGetLastError());
  }
  return end_steps(h);
}

int svils_batch_step_pairs(svils_batch *h, uint32_t nsteps, const uint64_t *off, const uint32_t *pairs, const double *scale,
                           const double *rho_gamma, const double *rho_lambda) {
  const char *name = "svils_batch_step_pairs";
  if (int rc = check(h, name)) return rc;
  if (nsteps && (!off || !scale || !rho_gamma || !rho_lambda)) return fail(SVILS_ERR_ARG, "%s: null argument", name);
  if (!nsteps) return 0;
  if (int rc = check_steps(h, name, nsteps, rho_gamma, rho_lambda)) return rc;
  uint64_t total, most;
  if (int rc = check_step_lists(name, "pairs", h->n, nsteps, off, scale, nullptr, nullptr, pairs != nullptr, &total, &most)) return rc;
  const uint32_t n = h->n, K = h->k, G = 64 / h->w;
  // checked before anything is enqueued
  for (uint32_t s = 0; s < nsteps; ++s)
    for (uint64_t e = off[s]; e < off[s + 1]; ++e) {
      const uint32_t p = pairs[2 * e], q = pairs[2 * e + 1];
      if (p >= q || q >= n)
        return fail(SVILS_ERR_ARG, "%s: pair %llu of step %u (%u, %u) is not a pair p < q < n = %u", name, (unsigned long long)(e - off[s]), s, p, q, n);
      if (host_skipped(h, p, q))
        return fail(SVILS_ERR_ARG, "%s: pair %llu of step %u (%u, %u) is in the skip set", name, (unsigned long long)(e - off[s]), s, p, q);
    }
  if (int rc = catch_up(h)) return rc;
  // the call's lists: pairs [total][2], entries [2 total], offsets [nsteps][n + 1] -- the last two written where they are staged
  Staging lists(h);
  const auto s_pairs = lists.add(pairs, 2 * (size_t)total);
  const auto s_ent = lists.add<uint32_t>(nullptr, 2 * (size_t)total), s_noff = lists.add<uint32_t>(nullptr, (size_t)nsteps * (n + 1));
  if (int rc = lists.open()) return rc;
  uint32_t *const pin_ent = lists.pinned(s_ent), *const pin_noff = lists.pinned(s_noff);
  std::memset(pin_noff, 0, (size_t)nsteps * (n + 1) * sizeof(uint32_t));
  // every node's (pair, side) entries of a step in list order: a counting sort per step
  for (uint32_t s = 0; s < nsteps; ++s) {
    uint32_t *no = pin_noff + (size_t)s * (n + 1);
    const uint32_t *pr = pairs + 2 * off[s];
    const uint32_t m = (uint32_t)(off[s + 1] - off[s]);
    for (uint32_t e = 0; e < m; ++e) {
      ++no[pr[2 * e] + 1];
      ++no[pr[2 * e + 1] + 1];
    }
    for (uint32_t i = 0; i < n; ++i) no[i + 1] += no[i];
    std::vector<uint32_t> at(no, no + n);
    uint32_t *en = pin_ent + 2 * off[s];
    for (uint32_t e = 0; e < m; ++e) {
      en[at[pr[2 * e]]++] = 2 * e;
      en[at[pr[2 * e + 1]]++] = 2 * e + 1;
    }
  }
  const uint32_t nwv_most = 4 * blocks(std::max<uint64_t>(most, 1), 4 * G);
  if (int rc = h->reserve(ToolHandle::HANDLE, &h->st_pl, (size_t)nwv_most * K * 2)) return rc;
  if (int rc = h->reserve(ToolHandle::HANDLE, &h->st_phi, 2 * (size_t)most * K)) return rc;
  if (int rc = lists.send()) return rc;
  if (int rc = begin_steps(h)) return rc;
  for (uint32_t s = 0; s < nsteps; ++s) {
    const uint32_t m = (uint32_t)(off[s + 1] - off[s]);
    StepArgs x = step_args(h, scale[s], rho_gamma[s]);
    x.m = m;
    x.pairs = lists.device(s_pairs) + 2 * off[s];
    x.ent = lists.device(s_ent) + 2 * off[s];
    x.noff = lists.device(s_noff) + (size_t)s * (n + 1);
    x.phi = h->st_phi;
    const uint32_t nb = blocks(m, 4 * G);
    const auto launch = [&](auto gr) {
      return launch_for_width(h, name, [&](auto w) {
        constexpr int W = decltype(w)::value, V = (int)VARIANT_V;
        if (m) hipLaunchKernelGGL((k_batch_step_phi<W, V, decltype(gr)>), dim3(nb), dim3(256), 0, h->st, x, gr);
        hipLaunchKernelGGL((k_batch_step_rows<W, V>), dim3(blocks(n, 4 * G)), dim3(256), 0, h->st, x);
      });
    };
    if (int rc = h->sparse ? launch(sparse_graph(h)) : launch(dense_graph(h)))
      return rc;
    if (rho_lambda[s] >= 0.0)
      hipLaunchKernelGGL(k_batch_step_tail, dim3(K), dim3(256), 0, h->st, K, 4 * nb, (const double *)nullptr, h->st_pl, (double *)nullptr,
                         h->alpha, h->eta0, h->eta1, scale[s], rho_gamma[s], rho_lambda[s], h->lam, h->elogbeta, h->gtab);
    HIPCHK(hipGetLastError());
  }
  return end_steps(h);
}

int svils_batch_set_star_chain(svils_batch *h, uint32_t max_steps) {
  if (int rc = check(h, "svils_batch_set_star_chain")) return rc;
  if (max_steps > STAR_CHAIN_MAX)   // a longer chain is a longer kernel on a shared machine
    return fail(SVILS_ERR_ARG, "svils_batch_set_star_chain: %u steps per launch exceed the most, %u", max_steps, STAR_CHAIN_MAX);
  h->star_chain = max_steps ? max_steps : STAR_CHAIN;
  return 0;
}

int svils_batch_get_expectations(svils_batch *h, double *elogpi, double *elogbeta) {
  const char *name = "svils_batch_get_expectations";
  if (int rc = check(h, name)) return rc;
  if (!h->have_state) return fail(SVILS_ERR_ARG, "%s: no state", name);
  if (int rc = catch_up(h)) return rc;
  if (int rc = renew_expectations(h)) return rc;   // what the next step call would do first
  if (int rc = settle(h, name)) return rc;
  if (elogpi) HIPCHK(hipMemcpy(elogpi, h->elogpi, (size_t)h->n * h->k * sizeof(double), hipMemcpyDeviceToHost));
  if (elogbeta) HIPCHK(hipMemcpy(elogbeta, h->elogbeta, 2 * (size_t)h->k * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int svils_batch_step_star(svils_batch *h, uint32_t nsteps, const uint32_t *start, const uint64_t *off, const uint32_t *partner,
                          const uint8_t *y, const double *rho_partner, const double *rho_start, const double *scale,
                          const double *rho_lambda) {
  const char *name = "svils_batch_step_star";
  if (int rc = check(h, name)) return rc;
  if (nsteps && (!start || !off || !rho_start || !scale || !rho_lambda)) return fail(SVILS_ERR_ARG, "%s: null argument", name);
  if (!nsteps) return 0;
  if (int rc = check_steps(h, name, nsteps, rho_start, rho_lambda)) return rc;
  uint64_t total, most;
  if (int rc = check_step_lists(name, "entries", h->n, nsteps, off, scale, start, nullptr, partner && y && rho_partner, &total, &most)) return rc;
  if (int rc = check_star_entries(h, name, nsteps, start, off, partner, y, rho_partner)) return rc;
  if (int rc = catch_up(h)) return rc;
  // the call's lists; off travels as uint32
  Staging lists(h);
  const auto s_rp = lists.add(rho_partner, total), s_rs = lists.add(rho_start, nsteps), s_sc = lists.add(scale, nsteps),
             s_rl = lists.add(rho_lambda, nsteps);
  const auto s_off = lists.add<uint32_t>(nullptr, (size_t)nsteps + 1), s_start = lists.add(start, nsteps), s_partner = lists.add(partner, total);
  const auto s_y = lists.add(y, total);
  if (int rc = lists.open()) return rc;
  for (uint32_t s = 0; s <= nsteps; ++s) lists.pinned(s_off)[s] = (uint32_t)off[s];
  if (int rc = lists.send()) return rc;
  if (int rc = begin_steps(h)) return rc;
  StarArgs x{};
  x.K = h->k;
  x.gamma = h->gamma;
  x.elogpi = h->elogpi;
  x.lam = h->lam;
  x.elogbeta = h->elogbeta;
  x.gtab = h->gtab;
  x.logeps = std::log(h->epsilon);
  x.alpha = h->alpha;
  x.eta0 = h->eta0;
  x.eta1 = h->eta1;
  x.rho_partner = lists.device(s_rp);
  x.rho_start = lists.device(s_rs);
  x.scale = lists.device(s_sc);
  x.rho_lambda = lists.device(s_rl);
  x.off = lists.device(s_off);
  x.start = lists.device(s_start);
  x.partner = lists.device(s_partner);
  x.y = lists.device(s_y);
  x.ctr = h->ctr;
  // a chain is cut into launches of at most star_chain steps: no kernel runs long, and a step does the same wherever the cut falls
  for (uint32_t s0 = 0; s0 < nsteps; s0 += h->star_chain) {
    x.s0 = s0;
    x.s1 = (uint32_t)std::min<uint64_t>(nsteps, (uint64_t)s0 + h->star_chain);
    if (int rc = launch_for_width(h, name, [&](auto w) {
          hipLaunchKernelGGL((k_batch_star_chain<decltype(w)::value, (int)VARIANT_V>), dim3(1), dim3(STAR_THREADS), 0, h->st, x);
        }))
      return rc;
    HIPCHK(hipGetLastError());
  }
  return end_steps(h);
}

int svils_batch_step_strat(svils_batch *h, uint32_t nsteps, const uint32_t *start, const uint64_t *off, const uint32_t *partner,
                           const uint8_t *y, const double *rho_gamma, const double *scale, const double *rho_lambda) {
  const char *name = "svils_batch_step_strat";
  if (int rc = check(h, name)) return rc;
  if (nsteps && (!start || !off || !rho_gamma || !scale || !rho_lambda)) return fail(SVILS_ERR_ARG, "%s: null argument", name);
  if (!nsteps) return 0;
  if (int rc = check_steps(h, name, nsteps, rho_gamma, rho_lambda)) return rc;
  uint64_t total, most;
  if (int rc = check_step_lists(name, "entries", h->n, nsteps, off, scale, start, rho_gamma, partner && y, &total, &most)) return rc;
  if (int rc = check_star_entries(h, name, nsteps, start, off, partner, y, nullptr)) return rc;
  // The call is accepted.  What catches up every row it reads, on COPIES of the handle's bookkeeping, which replace it
  // below: c takes one log1p(-rho) per step, in step order, and a step's factors come from row_c as it stood before the step
  const uint32_t K = h->k, G = 64 / h->w;
  std::vector<double> row_c(h->row_c), fj((size_t)total), fa(nsteps);
  double c = h->lag_c;
  for (uint32_t s = 0; s < nsteps; ++s) {
    fa[s] = std::exp(c - row_c[start[s]]);
    for (uint64_t e = off[s]; e < off[s + 1]; ++e) fj[e] = std::exp(c - row_c[partner[e]]);
    c += std::log1p(-rho_gamma[s]);
    row_c[start[s]] = c;
    for (uint64_t e = off[s]; e < off[s + 1]; ++e) row_c[partner[e]] = c;
  }
  // the call's lists; a call without entries sends nothing
  Staging lists(h);
  const auto s_fj = lists.add(fj.data(), total);
  const auto s_partner = lists.add(partner, total);
  const auto s_y = lists.add(y, total);
  const uint32_t nwv_most = 4 * blocks(most, 4 * G);
  if (int rc = lists.open()) return rc;
  if (int rc = h->reserve(ToolHandle::HANDLE, &h->st_part, (size_t)nwv_most * K)) return rc;
  if (int rc = h->reserve(ToolHandle::HANDLE, &h->st_pl, (size_t)nwv_most * K * 2)) return rc;
  if (total)
    if (int rc = lists.send()) return rc;
  if (!h->elogbeta_fresh) {   // Elogbeta of the current lambda; Elogpi is formed per row in the step's registers
    hipLaunchKernelGGL(k_batch_beta, dim3(blocks(K, 256)), dim3(256), 0, h->st, K, h->lam, h->gtab, h->elogbeta);
    HIPCHK(hipGetLastError());
    h->elogbeta_fresh = true;
  }
  HIPCHK(hipMemsetAsync(h->ctr, 0, 4 * sizeof(unsigned long long), h->st));
  HIPCHK(hipEventRecord(h->ev[0], h->st));
  // from here on rows are written with the call's factors: the bookkeeping is the call's
  h->row_c.swap(row_c);
  h->lag_c = c;
  h->behind = true;
  h->elog_fresh = false;      // nothing here maintains Elogpi
  StratArgs x{};
  x.K = K;
  x.gamma = h->gamma;
  x.elogbeta = h->elogbeta;
  x.logeps = std::log(h->epsilon);
  x.alpha = h->alpha;
  x.part_a = h->st_part;
  x.pl = h->st_pl;
  x.ctr = h->ctr;
  x.gtab = h->gtab;
  for (uint32_t s = 0; s < nsteps; ++s) {
    const uint32_t m = (uint32_t)(off[s + 1] - off[s]), nb = blocks(m, 4 * G);
    x.m = m;
    x.a = start[s];
    x.partner = lists.device(s_partner) + off[s];
    x.y = lists.device(s_y) + off[s];
    x.fj = lists.device(s_fj) + off[s];
    x.fa = fa[s];
    x.scale = scale[s];
    x.rho = rho_gamma[s];
    if (m)
      if (int rc = launch_for_width(h, name, [&](auto w) {
            hipLaunchKernelGGL((k_batch_strat_pairs<decltype(w)::value, (int)VARIANT_V>), dim3(nb), dim3(256), 0, h->st, x);
          }))
        return rc;
    hipLaunchKernelGGL(k_batch_strat_tail, dim3(K), dim3(256), 0, h->st, K, 4 * nb, h->st_part, h->st_pl,
                       h->gamma + (size_t)x.a * K, h->alpha, x.fa, h->eta0, h->eta1, x.scale, x.rho, rho_lambda[s], h->lam, h->elogbeta,
                       h->gtab);
    HIPCHK(hipGetLastError());
  }
  return end_steps(h);
}

int svils_batch_get_lag(svils_batch *h, uint64_t *rows_behind) {
  if (int rc = check(h, "svils_batch_get_lag")) return rc;
  if (!rows_behind) return fail(SVILS_ERR_ARG, "svils_batch_get_lag: null argument");
  uint64_t c = 0;
  for (double rc : h->row_c) c += rc != h->lag_c;
  *rows_behind = c;
  return 0;
}

int svils_batch_pair_loglik(svils_batch *h, const uint32_t *pairs, const uint8_t *y, uint64_t m, double *out) {
  if (int rc = check(h, "svils_batch_pair_loglik")) return rc;
  if (m && (!pairs || !y || !out)) return fail(SVILS_ERR_ARG, "svils_batch_pair_loglik: null argument");
  if (!h->have_state) return fail(SVILS_ERR_ARG, "svils_batch_pair_loglik: no state");
  for (uint64_t x = 0; x < m; ++x)
    if (pairs[2 * x] >= h->n || pairs[2 * x + 1] >= h->n)
      return fail(SVILS_ERR_ARG, "svils_batch_pair_loglik: pair %llu names a node >= n = %u", (unsigned long long)x, h->n);
  if (int rc = catch_up(h)) return rc;
  if (int rc = settle(h, "svils_batch_pair_loglik")) return rc;
  if (!m) return 0;
  const auto scope = ToolHandle::GRAPH;   // the lists are the held-out sets of a graph
  if (int rc = h->reserve(scope, &h->ll_pairs, 2 * (size_t)m)) return rc;
  if (int rc = h->reserve(scope, &h->ll_y, (size_t)m)) return rc;
  if (int rc = h->reserve(scope, &h->ll_out, (size_t)m)) return rc;
  HIPCHK(hipMemcpyAsync(h->ll_pairs, pairs, 2 * m * sizeof(uint32_t), hipMemcpyHostToDevice, h->st));
  HIPCHK(hipMemcpyAsync(h->ll_y, y, m, hipMemcpyHostToDevice, h->st));
  hipLaunchKernelGGL(k_batch_pair_ll, dim3(blocks(m, 4)), dim3(256), 0, h->st, m, h->k, h->epsilon, h->ll_pairs, h->ll_y, h->gamma,
                     h->lam, h->ll_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, h->ll_out, m * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  return 0;
}

int svils_batch_set_elbo_tiles(svils_batch *h, uint32_t tiles_per_launch) {
  if (int rc = check(h, "svils_batch_set_elbo_tiles")) return rc;
  if (int rc = dense_only(h, "svils_batch_set_elbo_tiles")) return rc;
  if (tiles_per_launch > BATCH_TILES)
    return fail(SVILS_ERR_ARG, "svils_batch_set_elbo_tiles: %u tiles per launch exceed the most, %u", tiles_per_launch, BATCH_TILES);
  h->elbo_tiles = tiles_per_launch ? tiles_per_launch : BATCH_TILES;
  return 0;
}

int svils_batch_elbo(svils_batch *h, double parts[4], uint64_t *pairs_done, uint64_t *rounds_total) {
  const char *name = "svils_batch_elbo";
  if (int rc = check(h, name)) return rc;
  if (int rc = dense_only(h, name)) return rc;
  if (!parts) return fail(SVILS_ERR_ARG, "%s: null argument", name);
  if (!h->have_graph || !h->have_state) return fail(SVILS_ERR_ARG, "%s: set the graph and the state first", name);
  if (int rc = catch_up(h)) return rc;
  if (int rc = settle(h, name)) return rc;
  const uint32_t n = h->n, K = h->k;
  if (int rc = h->reserve(ToolHandle::GRAPH, &h->el_part, 4 * (size_t)h->ntiles)) return rc;
  if (int rc = h->reserve(ToolHandle::HANDLE, &h->el_node, (size_t)n)) return rc;
  if (int rc = h->reserve(ToolHandle::HANDLE, &h->el_out, (size_t)4)) return rc;
  if (int rc = h->reserve(ToolHandle::HANDLE, &h->el_ctr, (size_t)5)) return rc;
  for (hipEvent_t &e : h->ev_elbo)
    if (!e) HIPCHK(hipEventCreate(&e));
  if (int rc = renew_expectations(h)) return rc;   // those svils_batch_get_expectations would return
  HIPCHK(hipMemsetAsync(h->el_ctr, 0, 5 * sizeof(unsigned long long), h->st));
  HIPCHK(hipEventRecord(h->ev_elbo[0], h->st));
  hipLaunchKernelGGL(k_batch_elbo_nodes, dim3(blocks(n, 4)), dim3(256), 0, h->st, n, K, h->alpha, h->gamma, h->elogpi, h->el_node);
  HIPCHK(hipGetLastError());
  for (uint32_t t0 = 0; t0 < h->ntiles; t0 += h->elbo_tiles) {
    const uint32_t nt = std::min(h->ntiles - t0, h->elbo_tiles);
    ElboArgs a{n, K, h->nw, t0, h->tiles, h->adj, h->skip, h->elogpi, h->elogbeta, std::log(h->epsilon), h->el_part, h->el_ctr};
    if (int rc = launch_for_width(h, name, [&](auto w) {
          hipLaunchKernelGGL((k_batch_elbo<decltype(w)::value, (int)VARIANT_V>), dim3(nt), dim3(256), 0, h->st, a);
        }))
      return rc;
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_batch_elbo_reduce, dim3(1), dim3(256), 0, h->st, (uint64_t)4 * h->ntiles, h->el_part, n, h->el_node, K, h->lam,
                     h->elogbeta, h->eta0, h->eta1, h->el_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev_elbo[1], h->st));
  h->timed = svils_batch::Timed::ELBO;
  unsigned long long c[5] = {};
  double out[4] = {};
  HIPCHK(hipMemcpyAsync(c, h->el_ctr, sizeof c, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipMemcpyAsync(out, h->el_out, sizeof out, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  if (c[3])
    return fail(SVILS_ERR_UNSUPPORTED, "%s: phi normaliser underflow in %llu pair(s) of the pass (the reference asserts s > 0 there)", name,
                c[3]);
  for (int i = 0; i < 4; ++i) parts[i] = out[i];
  if (pairs_done) *pairs_done = c[0];
  if (rounds_total) *rounds_total = c[1];
  return 0;
}

int svils_batch_get_stats(svils_batch *h, uint64_t *pairs_done, uint64_t *rounds_total, uint32_t *rounds_max, uint64_t *underflow_pairs) {
  if (int rc = check(h, "svils_batch_get_stats")) return rc;
  unsigned long long c[5] = {};
  HIPCHK(hipMemcpyAsync(c, h->ctr, sizeof c, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  if (pairs_done) *pairs_done = c[0];
  if (rounds_total) *rounds_total = c[1];
  if (rounds_max) *rounds_max = (uint32_t)c[2];
  if (underflow_pairs) *underflow_pairs = c[4];
  return 0;
}

int svils_batch_get_timing(svils_batch *h, double ms[3]) {
  if (int rc = check(h, "svils_batch_get_timing")) return rc;
  if (!ms) return fail(SVILS_ERR_ARG, "svils_batch_get_timing: null argument");
  HIPCHK(hipStreamSynchronize(h->st));
  using Timed = svils_batch::Timed;
  if (h->timed == Timed::ELBO) {   // its own bracket
    float t = 0;
    ms[0] = hipEventElapsedTime(&t, h->ev_elbo[0], h->ev_elbo[1]) == hipSuccess ? (double)t : -1.0;
    ms[1] = ms[2] = -1.0;
    return 0;
  }
  ms[0] = h->elapsed_ms(0, 1, h->timed != Timed::NONE);
  const bool swept = h->timed == Timed::SWEEP;
  ms[1] = h->launches_ms(1, h->nlaunch, swept);   // (the first launch's bracket includes the fill)
  ms[2] = h->launches_ms(2, h->nlaunch, swept);
  return 0;
}

}  // extern "C"
