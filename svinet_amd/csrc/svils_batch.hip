// svils_batch.hip -- -batch-gpu: the reference's MMSBInfer::batch_infer (src/mmsbinfer.cc:833-930) on the device, coordinate
// ascent over ALL n (n - 1) / 2 pairs.  One sweep is
//
//   k_batch_dir_exp    set_dir_exp (src/mmsbinfer.hh:563-580): one wavefront per node, Elogpi = psi(gamma) - psi(row sum)
//   k_batch_beta       the same for lambda [k][2]
//   k_batch_fill       gamma_next = alpha, lambda_next = eta (:887-888)
//   k_batch_pairs<W,V> the pair pass (:846-880, PhiComp src/mmsbinfer.hh:104-203).  The pair triangle is cut into tiles of
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
#include "svils_devutil.h"
#include "svils_tool.h"

namespace {

constexpr uint32_t TILE_COLS = 64;
constexpr uint32_t BATCH_TILES = 2048;              // tiles per launch of the pair kernel
constexpr size_t BATCH_BYTES = (size_t)256 << 20;   // ... and at most this much of partial sums
constexpr uint32_t MAX_ROUNDS = 50;                 // src/env.hh:415
constexpr double MEAN_CHANGE_THRESH = 0.00001;      // src/env.hh:337

// rows of a tile one wavefront owns: its row accumulators are A x (W V) doubles of LDS, 32 KiB per workgroup at most
constexpr int rows_per_wave(int wv) { return wv <= 64 ? 16 : wv == 128 ? 8 : 4; }

// the instantiation table: V = 4 everywhere, W the smallest power of two with 4 W >= k
inline uint32_t variant_w(uint32_t k) {
  uint32_t w = 1;
  while (4 * w < k) w <<= 1;
  return w;
}
constexpr uint32_t VARIANT_V = 4;

__device__ inline uint32_t wave_sum_u32(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ inline uint32_t wave_max_u32(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ inline double wave_sum_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

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
  const double invK = 1.0 / (double)K, dK = (double)K;

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
      double elp[V], ef[V], p1[V], p2[V], o1[V], o2[V];
      const double le = y ? x.logeps : 0.0;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        elp[v] = kval[v] ? x.elogpi[(size_t)a * K + v * W + lw] : 0.0;
        ef[v] = y ? ef1[v] : ef0[v];
        p1[v] = p2[v] = kval[v] ? invK : 0.0;
        o1[v] = o2[v] = 0.0;
      }
      bool live = valid;
      uint32_t rounds = 0;
      for (uint32_t i = 0; i < MAX_ROUNDS; ++i) {
        if (!__ballot(live)) break;
        if ((i & 1) == 0) {
#pragma unroll
          for (int v = 0; v < V; ++v) {
            o1[v] = live ? p1[v] : o1[v];
            o2[v] = live ? p2[v] : o2[v];
          }
        }
        // both updates from the previous round's vectors: e[0..V) the new phi1 (from phi2), e[V..2V) the new phi2
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
        if (live && !ok) {   // the reference asserts here; the pair leaves with what it has
          under += lw == 0;
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
  npairs = wave_sum_u32(npairs);
  rtot = wave_sum_u32(rtot);
  under = wave_sum_u32(under);
  rmax = wave_max_u32(rmax);
  if (lane == 0) {
    if (npairs) atomicAdd(&x.ctr[0], (unsigned long long)npairs);
    if (rtot) atomicAdd(&x.ctr[1], (unsigned long long)rtot);
    if (rmax) atomicMax(&x.ctr[2], (unsigned long long)rmax);
    if (under) { atomicAdd(&x.ctr[3], (unsigned long long)under); atomicAdd(&x.ctr[4], (unsigned long long)under); }
  }
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

}  // namespace

// events: ev[0] sweep begin, ev[1] Elogpi / Elogbeta done, then per launch of the pair kernel ev[2 + 2 b] (pairs done) and
// ev[3 + 2 b] (reduced)
struct svils_batch : ToolHandle {
  uint32_t n = 0, k = 0, w = 0, ta = 0, nw = 0;
  double alpha = 0, eta0 = 0, eta1 = 0, epsilon = 0;
  // HANDLE scope
  double *gamma = nullptr, *gnext = nullptr, *elogpi = nullptr;   // [n][k]
  double *lam = nullptr, *lnext = nullptr, *elogbeta = nullptr;   // [k][2]
  double *gtab = nullptr;                                         // [128][2] log_tab's table
  unsigned long long *ctr = nullptr;                              // [5]
  // GRAPH scope
  uint32_t *adj = nullptr, *skip = nullptr;                       // [n][nw]
  uint32_t *tiles = nullptr, *rowoff = nullptr, *jfirst = nullptr;
  double *pa = nullptr, *pb = nullptr, *pl = nullptr;
  uint32_t *ll_pairs = nullptr;                                   // svils_batch_pair_loglik: grown on demand
  uint8_t *ll_y = nullptr;
  double *ll_out = nullptr;
  uint64_t ll_cap = 0;
  uint32_t ntiles = 0, nrb = 0, batch = 0;                        // batch: tiles per launch
  std::vector<uint32_t> h_tiles;
  bool have_graph = false, have_state = false, timed = false;
  uint32_t nlaunch = 0;                                           // launches of the last sweep
};

namespace {

void free_graph(svils_batch *h) {
  h->release(ToolHandle::GRAPH);
  h->have_graph = false;
  h->ll_cap = 0;
}

template <int W>
void launch_pairs(svils_batch *h, uint32_t nt, const PairArgs &a) {
  hipLaunchKernelGGL((k_batch_pairs<W, (int)VARIANT_V>), dim3(nt), dim3(256), 0, h->st, a);
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
    switch (h->w) {
      case 1: launch_pairs<1>(h, nt, a); break;
      case 2: launch_pairs<2>(h, nt, a); break;
      case 4: launch_pairs<4>(h, nt, a); break;
      case 8: launch_pairs<8>(h, nt, a); break;
      case 16: launch_pairs<16>(h, nt, a); break;
      case 32: launch_pairs<32>(h, nt, a); break;
      case 64: launch_pairs<64>(h, nt, a); break;
      default: return fail(SVILS_ERR_UNSUPPORTED, "svils_batch_sweep: no pair kernel for W = %u", h->w);   // a missing kernel is an error
    }
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
  h->timed = true;
  return 0;
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

int svils_batch_create(int device, uint32_t n, uint32_t k, double alpha, double eta0, double eta1, double epsilon, svils_batch **out) {
  if (!out) return fail(SVILS_ERR_ARG, "svils_batch_create: null argument");
  *out = nullptr;
  if (n < 2 || k < 2 || !(alpha > 0) || !(eta0 > 0) || !(eta1 > 0) || !(epsilon > 0) || !(epsilon < 1))
    return fail(SVILS_ERR_ARG, "svils_batch_create: need n >= 2, k >= 2, alpha, eta0, eta1 > 0 and 0 < epsilon < 1");
  if (k > SVILS_BATCH_MAX_K) return fail(SVILS_ERR_UNSUPPORTED, "svils_batch_create: k = %u exceeds SVILS_BATCH_MAX_K = %d", k, SVILS_BATCH_MAX_K);
  if (n > SVILS_BATCH_MAX_N) return fail(SVILS_ERR_UNSUPPORTED, "svils_batch_create: n = %u exceeds SVILS_BATCH_MAX_N = %d", n, SVILS_BATCH_MAX_N);
  if (int rc = open_device(device)) return rc;
  svils_batch *h = new (std::nothrow) svils_batch();
  if (!h) return fail(SVILS_ERR_NOMEM, "out of host memory");
  h->n = n;
  h->k = k;
  h->w = variant_w(k);
  h->ta = 4 * (uint32_t)rows_per_wave((int)(h->w * VARIANT_V));
  h->nw = (n + 31) / 32;
  h->alpha = alpha;
  h->eta0 = eta0;
  h->eta1 = eta1;
  h->epsilon = epsilon;
  const auto scope = ToolHandle::HANDLE;
  const size_t nk = (size_t)n * k;
  std::vector<double> tab(256);   // {1 / c_i, ln c_i} at the centres of 128 equal sub-intervals of [1, 2) (log_tab)
  for (int i = 0; i < 128; ++i) {
    const double c = 1.0 + (i + 0.5) / 128.0;
    tab[2 * i] = 1.0 / c;
    tab[2 * i + 1] = std::log(c);
  }
  int rc = h->open(device, 2);
  if (!rc) rc = h->dalloc(scope, &h->gamma, nk);
  if (!rc) rc = h->dalloc(scope, &h->gnext, nk);
  if (!rc) rc = h->dalloc(scope, &h->elogpi, nk);
  if (!rc) rc = h->dalloc(scope, &h->lam, 2 * (size_t)k);
  if (!rc) rc = h->dalloc(scope, &h->lnext, 2 * (size_t)k);
  if (!rc) rc = h->dalloc(scope, &h->elogbeta, 2 * (size_t)k);
  if (!rc) rc = h->dalloc(scope, &h->ctr, 5);
  if (!rc) rc = h->upload(scope, &h->gtab, tab);
  if (!rc && hipMemsetAsync(h->ctr, 0, 5 * sizeof(unsigned long long), h->st) != hipSuccess) rc = fail(SVILS_ERR_DEVICE, "svils_batch_create: memset failed");
  if (!rc && hipStreamSynchronize(h->st) != hipSuccess) rc = fail(SVILS_ERR_DEVICE, "svils_batch_create: upload failed");
  if (rc) {
    svils_batch_destroy(h);
    return rc;
  }
  *out = h;
  return 0;
}

int svils_batch_destroy(svils_batch *h) {
  delete h;   // ~ToolHandle: waits for the stream, frees both scopes
  return 0;
}

int svils_batch_set_graph(svils_batch *h, const uint32_t *links, uint64_t nlinks, const uint32_t *skip, uint64_t nskip) {
  if (int rc = check(h, "svils_batch_set_graph")) return rc;
  if ((nlinks && !links) || (nskip && !skip)) return fail(SVILS_ERR_ARG, "svils_batch_set_graph: null argument");
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
  while (h->ev.size() < 2 + 2 * (size_t)nlaunch) {
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreate(&e));
    h->ev.push_back(e);
  }
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
  h->ntiles = ntiles;
  h->nrb = nrb;
  h->batch = batch;
  h->have_graph = true;
  h->timed = false;
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
  return 0;
}

int svils_batch_get_state(svils_batch *h, double *gamma, double *lambda) {
  if (int rc = check(h, "svils_batch_get_state")) return rc;
  if (!h->have_state) return fail(SVILS_ERR_ARG, "svils_batch_get_state: no state");
  if (int rc = settle(h, "svils_batch_get_state")) return rc;
  if (gamma) HIPCHK(hipMemcpy(gamma, h->gamma, (size_t)h->n * h->k * sizeof(double), hipMemcpyDeviceToHost));
  if (lambda) HIPCHK(hipMemcpy(lambda, h->lam, 2 * (size_t)h->k * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int svils_batch_sweep(svils_batch *h, uint32_t nsweeps) {
  if (int rc = check(h, "svils_batch_sweep")) return rc;
  if (!h->have_graph || !h->have_state) return fail(SVILS_ERR_ARG, "svils_batch_sweep: set the graph and the state first");
  for (uint32_t s = 0; s < nsweeps; ++s)
    if (int rc = one_sweep(h)) return rc;
  return 0;
}

int svils_batch_pair_loglik(svils_batch *h, const uint32_t *pairs, const uint8_t *y, uint64_t m, double *out) {
  if (int rc = check(h, "svils_batch_pair_loglik")) return rc;
  if (m && (!pairs || !y || !out)) return fail(SVILS_ERR_ARG, "svils_batch_pair_loglik: null argument");
  if (!h->have_state) return fail(SVILS_ERR_ARG, "svils_batch_pair_loglik: no state");
  for (uint64_t x = 0; x < m; ++x)
    if (pairs[2 * x] >= h->n || pairs[2 * x + 1] >= h->n)
      return fail(SVILS_ERR_ARG, "svils_batch_pair_loglik: pair %llu names a node >= n = %u", (unsigned long long)x, h->n);
  if (int rc = settle(h, "svils_batch_pair_loglik")) return rc;
  if (!m) return 0;
  if (m > h->ll_cap) {   // GRAPH scope (the lists are the held-out sets of a graph); the stream is idle after settle()
    if (h->ll_pairs) (void)hipFree(h->ll_pairs);
    if (h->ll_y) (void)hipFree(h->ll_y);
    if (h->ll_out) (void)hipFree(h->ll_out);
    h->ll_pairs = nullptr;
    h->ll_y = nullptr;
    h->ll_out = nullptr;
    h->ll_cap = 0;
    const auto scope = ToolHandle::GRAPH;
    int rc = h->dalloc(scope, &h->ll_pairs, 2 * (size_t)m);
    if (!rc) rc = h->dalloc(scope, &h->ll_y, (size_t)m);
    if (!rc) rc = h->dalloc(scope, &h->ll_out, (size_t)m);
    if (rc) return rc;
    h->ll_cap = m;
  }
  HIPCHK(hipMemcpyAsync(h->ll_pairs, pairs, 2 * m * sizeof(uint32_t), hipMemcpyHostToDevice, h->st));
  HIPCHK(hipMemcpyAsync(h->ll_y, y, m, hipMemcpyHostToDevice, h->st));
  hipLaunchKernelGGL(k_batch_pair_ll, dim3(blocks(m, 4)), dim3(256), 0, h->st, m, h->k, h->epsilon, h->ll_pairs, h->ll_y, h->gamma,
                     h->lam, h->ll_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, h->ll_out, m * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
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
  ms[0] = h->elapsed_ms(0, 1, h->timed);
  ms[1] = ms[2] = h->timed ? 0.0 : -1.0;
  for (uint32_t b = 0; h->timed && b < h->nlaunch; ++b) {
    ms[1] += h->elapsed_ms(1 + 2 * b, 2 + 2 * b, true);   // (the first launch's bracket includes the fill)
    ms[2] += h->elapsed_ms(2 + 2 * b, 3 + 2 * b, true);
  }
  return 0;
}

}  // extern "C"
