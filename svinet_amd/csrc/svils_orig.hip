// svils_orig.hip -- -orig: the reference's MMSBInferOrig::batch_infer (src/mmsbinferorig.cc:212-294, fixed point PhiComp2,
// src/mmsbinferorig.hh:110-220) on the device: the mixed-membership blockmodel with a full K x K matrix of block rates,
// coordinate ascent over every ORDERED pair (p, q), p != q.  One sweep is
//
//   k_orig_dir_exp      set_dir_exp (:601-622): one wavefront per node, Elogpi = psi(max(gamma, 1e-30)) - psi(row sum)
//   k_orig_tables       L0 = log(1 - beta), L1 = log(beta), transposed and zero-padded to KP = 16 ceil(K / 16)
//   k_orig_fill         gamma_next = alpha, num = tot = 0; latches the degenerate flag of the sweep before
//   per launch of at most `rows` p rows (svils.h: the bound):
//     k_orig_pairs<KP,LREG>  the pair pass.  A wavefront owns a tile of 16 pairs (p, q0 .. q0 + 15), one pair per MFMA
//                         column.  With v_mfma_f64_16x16x4_f64 (A: lane l = row l & 15, k-slot l >> 4; B: k-slot l >> 4, column
//                         l & 15; C/D: register r of lane l = row (l >> 4) + 4 r, column l & 15) and k-slot g of step s
//                         standing for h = 4 s + g, lane (g, c) holds phi[h] of pair c for all h = g (mod 4) BOTH as the B
//                         operand and as the result (row block b, register r <-> step s = 4 b + r): a round's output is the
//                         next round's operand, no relayout.  U = L0 ((1 - y) o Phi) + L1 (y o Phi): a pair's column is zero
//                         in the product that is not its own, so every pair gets exactly L_y phi, and a product no pair of
//                         the tile needs is skipped (wave-uniform).  The accumulators start at Elogpi; the softmax sum goes
//                         over the four lane groups by a fixed butterfly.  A pair that has met the exit rule is frozen; the
//                         tile ends when all its pairs have.  Out go phi1, phi2 [slot][KP] (zero for a pair that is not
//                         visited) and y [slot], slot = (p - p0) n + q
//     k_orig_gamma_rows   gamma_next[p] += sum_q phi1(p, q): one workgroup per row, a fixed order
//     k_orig_gamma_cols   gamma_next[q] += sum_p phi2(p, q): one thread per (q, k), p ascending
//     k_orig_acc<KP>      num += (y o Phi1)^T Phi2, tot += Phi1^T Phi2 over the slots of the launch: a GEMM whose k dimension is
//                         the pair; every wavefront takes a contiguous run of slots and leaves its 2 KP^2 partial sums
//     k_orig_acc_reduce   num / tot += the partials, in ascending wavefront order
//   k_orig_final        gamma = gamma_next, beta = num / tot; a beta outside (0, 1) is counted and raises the flag
//
// No floating-point atomics: every sum has one owner and a fixed order, so a sweep is bitwise reproducible.  Once the flag is
// up the pair pass, the reductions and k_orig_final of every later sweep return at once: the state stays as it is.
#include "svils_devutil.h"
#include "svils_orig.h"
#include "svils_waveutil.h"

using namespace svils_impl;

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr uint32_t TILES_PER_BLOCK = 16;            // four per wavefront
constexpr size_t PHI_BYTES = (size_t)256 << 20;     // phi1 and phi2 of one launch
constexpr uint32_t ACC_WAVES = 256;                 // wavefronts (and partial sums) of k_orig_acc

inline uint32_t padded_k(uint32_t k) { return (k + 15) / 16 * 16; }

// the sum over the four lane groups of a pair (lanes c, c + 16, c + 32, c + 48): the same bits in all four
__device__ inline double groups_sum(double v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

__global__ __launch_bounds__(256) void k_orig_dir_exp(uint32_t n, uint32_t K, const double *__restrict__ gamma,
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
  for (uint32_t k = lane; k < K; k += 64) elogpi[(size_t)i * K + k] = digamma(fmax(g[k], 1e-30), logtab) - ps;
}

// tabs[which][h][ld]: entry (h, g) = log f[g][h], f = 1 - beta (which 0) or beta (which 1); zero past K
// (eps: 0 for the sweep's L tables; 1e-10 for the T tables of the lower bound, svils_orig_elbo.hip)
__global__ __launch_bounds__(256) void k_orig_tables(uint32_t K, uint32_t KP, uint32_t ld, const double *__restrict__ beta,
                                                     double eps, double *__restrict__ tabs) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= KP * ld) return;
  const uint32_t h = e / ld, g = e % ld;
  double l0 = 0.0, l1 = 0.0;
  if (h < K && g < K) {
    const double b = beta[(size_t)g * K + h];
    l0 = log((1.0 - b) + eps);
    l1 = log(b + eps);
  }
  tabs[e] = l0;
  tabs[(size_t)KP * ld + e] = l1;
}

__global__ __launch_bounds__(256) void k_orig_fill(uint64_t nk, uint32_t nnt, double alpha, double *__restrict__ gnext,
                                                   double *__restrict__ nt, u64 *__restrict__ ctr) {
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (x < nk) gnext[x] = alpha;
  if (x < nnt) nt[x] = 0.0;
  if (x == 0) ctr[CTR_FLAG] = ctr[CTR_PENDING];   // no launch reads the flag between k_orig_final and here
}

template <int KP, bool LREG>
__global__ __launch_bounds__(256) void k_orig_pairs(PairArgs x) {
  constexpr int R = KP / 16, S = KP / 4, LD = tab_ld(KP);
  __shared__ double lt[LREG ? 1 : 2 * KP * LD];
  __shared__ double olds[LREG ? 1 : 4 * 2 * S * 64];   // the saved vectors of the larger instantiations: [wavefront][side][s][lane]
  if (x.ctr[CTR_FLAG]) return;   // the same answer in every lane of the launch
  const uint32_t t = threadIdx.x, w = t >> 6, l = t & 63, g = l >> 4, c = l & 15;
  const uint32_t K = x.K, n = x.n;
  double a0r[LREG ? R * S : 1], a1r[LREG ? R * S : 1];
  if (LREG) {
#pragma unroll
    for (int b = 0; b < R; ++b)
#pragma unroll
      for (int s = 0; s < S; ++s) {
        a0r[LREG ? b * S + s : 0] = x.tabs[(4 * s + g) * LD + 16 * b + c];
        a1r[LREG ? b * S + s : 0] = x.tabs[KP * LD + (4 * s + g) * LD + 16 * b + c];
      }
  } else {
    for (uint32_t i = t; i < 2 * KP * LD; i += 256) lt[LREG ? 0 : i] = x.tabs[i];
    __syncthreads();
  }
  const uint32_t ntiles = x.rows * x.tpr, tb = blockIdx.x * TILES_PER_BLOCK;
  const uint32_t te = min(ntiles, tb + TILES_PER_BLOCK);
  const double unif = 1.0 / (double)K, dk = (double)K;
  u64 c_pairs = 0, c_rounds = 0, c_norm = 0;
  uint32_t c_max = 0;
  for (uint32_t ti = tb + w; ti < te; ti += 4) {   // wave-uniform
    const uint32_t pr = ti / x.tpr, p = x.p0 + pr, q = (ti % x.tpr) * TILE_PAIRS + c;
    bool valid = q < n && q != p;
    bool y = false;
    if (valid) {
      const size_t wd = (size_t)p * x.nw + (q >> 5);
      if ((x.skip[wd] >> (q & 31)) & 1u) valid = false;
      y = (x.adj[wd] >> (q & 31)) & 1u;
    }
    const double *ep = x.elogpi + (size_t)p * K, *eq = x.elogpi + (size_t)(q < n ? q : 0) * K;
    const bool any1 = __any(valid && y), any0 = __any(valid && !y);
    double phi1[S], phi2[S], old1[LREG ? S : 1], old2[LREG ? S : 1];
    double *const o1 = olds + (LREG ? 0 : (w * 2 * S) * 64 + l), *const o2 = o1 + (LREG ? 0 : S * 64);
#pragma unroll
    for (int s = 0; s < S; ++s) phi1[s] = phi2[s] = (uint32_t)(4 * s) + g < K ? unif : 0.0;
    bool done = !valid, bad = false;
    uint32_t rounds = 0;
    for (uint32_t i = 0; i < MAX_ROUNDS; ++i) {
      if (!__any(!done)) break;
      if ((i & 1u) == 0) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
          if (LREG) { old1[LREG ? s : 0] = phi1[s]; old2[LREG ? s : 0] = phi2[s]; }
          else { o1[s * 64] = phi1[s]; o2[s * 64] = phi2[s]; }   // read back by the same lane alone
        }
      }
      d4 acc1[R], acc2[R];
#pragma unroll
      for (int b = 0; b < R; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t h = 16 * b + 4 * r + g;
          acc1[b][r] = h < K ? ep[h] : 0.0;
          acc2[b][r] = h < K ? eq[h] : 0.0;
        }
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const double z1 = y ? 0.0 : phi1[s], z2 = y ? 0.0 : phi2[s], y1 = y ? phi1[s] : 0.0, y2 = y ? phi2[s] : 0.0;
#pragma unroll
        for (int b = 0; b < R; ++b) {
          const double a0 = LREG ? a0r[LREG ? b * S + s : 0] : lt[LREG ? 0 : (4 * s + g) * LD + 16 * b + c];
          const double a1 = LREG ? a1r[LREG ? b * S + s : 0] : lt[LREG ? 0 : KP * LD + (4 * s + g) * LD + 16 * b + c];
          if (any0) {
            acc1[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, z2, acc1[b], 0, 0, 0);
            acc2[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, z1, acc2[b], 0, 0, 0);
          }
          if (any1) {
            acc1[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, y2, acc1[b], 0, 0, 0);
            acc2[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, y1, acc2[b], 0, 0, 0);
          }
        }
      }
      double s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int b = 0; b < R; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool in = (uint32_t)(16 * b + 4 * r) + g < K;
          const double e1 = in ? exp_neg(acc1[b][r]) : 0.0, e2 = in ? exp_neg(acc2[b][r]) : 0.0;
          acc1[b][r] = e1;
          acc2[b][r] = e2;
          s1 += e1;
          s2 += e2;
        }
      s1 = groups_sum(s1);
      s2 = groups_sum(s2);
      const double i1 = 1.0 / s1, i2 = 1.0 / s2;
      double d1 = 0.0, d2 = 0.0;
#pragma unroll
      for (int b = 0; b < R; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          acc1[b][r] *= i1;
          acc2[b][r] *= i2;
          d1 += fabs(acc1[b][r] - (LREG ? old1[LREG ? 4 * b + r : 0] : o1[(4 * b + r) * 64]));
          d2 += fabs(acc2[b][r] - (LREG ? old2[LREG ? 4 * b + r : 0] : o2[(4 * b + r) * 64]));
        }
      d1 = groups_sum(d1);
      d2 = groups_sum(d2);
      if (!done) {
#pragma unroll
        for (int b = 0; b < R; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r) { phi1[4 * b + r] = acc1[b][r]; phi2[4 * b + r] = acc2[b][r]; }
        if (!(s1 > 0.0) || !(s2 > 0.0)) bad = true;
        rounds = i + 1;
        if ((i & 1u) && d1 / dk < MEAN_CHANGE_THRESH && d2 / dk < MEAN_CHANGE_THRESH) done = true;
      }
    }
    if (q < n) {
      const size_t slot = (size_t)pr * n + q;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        x.phi1[slot * KP + 4 * s + g] = valid ? phi1[s] : 0.0;
        x.phi2[slot * KP + 4 * s + g] = valid ? phi2[s] : 0.0;
      }
      if (g == 0) x.yv[slot] = valid && y ? 1 : 0;
    }
    if (g == 0 && valid) {
      c_pairs += 1;
      c_rounds += rounds;
      c_norm += bad ? 1 : 0;
      c_max = max(c_max, rounds);
    }
  }
  c_pairs = wave_sum_u64(c_pairs);
  c_rounds = wave_sum_u64(c_rounds);
  c_norm = wave_sum_u64(c_norm);
  c_max = wave_max_u32(c_max);
  if (l == 0 && c_pairs) {   // integer atomics: the counters do not depend on the order
    atomicAdd(x.ctr + CTR_PAIRS, c_pairs);
    atomicAdd(x.ctr + CTR_ROUNDS, c_rounds);
    if (c_norm) atomicAdd(x.ctr + CTR_NORM, c_norm);
    atomicMax(x.ctr + CTR_MAXR, (u64)c_max);
  }
}

// one workgroup per row of the launch: thread (j, k) adds the slots q = j, j + 4, ... of community k, then the four j in order
__global__ __launch_bounds__(256) void k_orig_gamma_rows(uint32_t n, uint32_t K, uint32_t KP, uint32_t p0,
                                                         const double *__restrict__ phi1, double *__restrict__ gnext,
                                                         const u64 *__restrict__ ctr) {
  __shared__ double sm[4][64];
  if (ctr[CTR_FLAG]) return;
  const uint32_t pr = blockIdx.x, k = threadIdx.x & 63, j = threadIdx.x >> 6;
  double s = 0.0;
  if (k < K)
    for (uint32_t q = j; q < n; q += 4) s += phi1[((size_t)pr * n + q) * KP + k];
  sm[j][k] = s;
  __syncthreads();
  if (j == 0 && k < K) gnext[(size_t)(p0 + pr) * K + k] += ((sm[0][k] + sm[1][k]) + sm[2][k]) + sm[3][k];
}

__global__ __launch_bounds__(256) void k_orig_gamma_cols(uint32_t n, uint32_t K, uint32_t KP, uint32_t rows,
                                                         const double *__restrict__ phi2, double *__restrict__ gnext,
                                                         const u64 *__restrict__ ctr) {
  if (ctr[CTR_FLAG]) return;
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (uint64_t)n * K) return;
  const uint32_t q = (uint32_t)(e / K), k = (uint32_t)(e % K);
  double s = 0.0;
  for (uint32_t pr = 0; pr < rows; ++pr) s += phi2[((size_t)pr * n + q) * KP + k];
  gnext[e] += s;
}

// part[wave][which][block bi R + bj][register r][lane]: which 0 = num, 1 = tot, in the C/D layout of the MFMA
template <int KP>
__global__ __launch_bounds__(256) void k_orig_acc(uint64_t nslots, const double *__restrict__ phi1, const double *__restrict__ phi2,
                                                  const uint8_t *__restrict__ yv, double *__restrict__ part,
                                                  const u64 *__restrict__ ctr) {
  constexpr int R = KP / 16;
  if (ctr[CTR_FLAG]) return;
  const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63, g = l >> 4, c = l & 15;
  const uint64_t per = (((nslots + ACC_WAVES - 1) / ACC_WAVES) + 3) & ~(uint64_t)3;
  const uint64_t s0 = min(nslots, (uint64_t)wave * per), s1 = min(nslots, s0 + per);
  d4 num[R][R], tot[R][R];
#pragma unroll
  for (int bi = 0; bi < R; ++bi)
#pragma unroll
    for (int bj = 0; bj < R; ++bj) num[bi][bj] = tot[bi][bj] = d4{0.0, 0.0, 0.0, 0.0};
  for (uint64_t sl = s0; sl < s1; sl += 4) {   // wave-uniform
    const uint64_t me = sl + g;
    const bool in = me < s1;
    const bool yy = in && yv[me];
    double a[R], ay[R], b[R];
#pragma unroll
    for (int bb = 0; bb < R; ++bb) {
      a[bb] = in ? phi1[me * KP + 16 * bb + c] : 0.0;
      b[bb] = in ? phi2[me * KP + 16 * bb + c] : 0.0;
      ay[bb] = yy ? a[bb] : 0.0;
    }
#pragma unroll
    for (int bi = 0; bi < R; ++bi)
#pragma unroll
      for (int bj = 0; bj < R; ++bj) {
        tot[bi][bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[bi], b[bj], tot[bi][bj], 0, 0, 0);
        num[bi][bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(ay[bi], b[bj], num[bi][bj], 0, 0, 0);
      }
  }
  double *o = part + (size_t)wave * 2 * R * R * 256;
#pragma unroll
  for (int bi = 0; bi < R; ++bi)
#pragma unroll
    for (int bj = 0; bj < R; ++bj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        o[(size_t)(bi * R + bj) * 256 + r * 64 + l] = num[bi][bj][r];
        o[(size_t)(R * R + bi * R + bj) * 256 + r * 64 + l] = tot[bi][bj][r];
      }
}

__global__ __launch_bounds__(256) void k_orig_acc_reduce(uint32_t nnt, const double *__restrict__ part, double *__restrict__ nt,
                                                         const u64 *__restrict__ ctr) {
  if (ctr[CTR_FLAG]) return;
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nnt) return;
  double s = 0.0;
  for (uint32_t wv = 0; wv < ACC_WAVES; ++wv) s += part[(size_t)wv * nnt + e];
  nt[e] += s;
}

__global__ __launch_bounds__(256) void k_orig_final(uint64_t nk, uint32_t K, uint32_t KP, const double *__restrict__ gnext,
                                                    const double *__restrict__ nt, double *__restrict__ gamma,
                                                    double *__restrict__ beta, u64 *__restrict__ ctr) {
  if (ctr[CTR_FLAG]) return;
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < nk) gamma[e] = gnext[e];
  if (e < (uint64_t)K * K) {
    const uint32_t R = KP / 16, gi = (uint32_t)(e / K), hj = (uint32_t)(e % K);
    const uint32_t rr = gi % 16, lane = (rr % 4) * 16 + hj % 16;
    const size_t idx = (size_t)((gi / 16) * R + hj / 16) * 256 + (rr / 4) * 64 + lane;
    const double b = nt[idx] / nt[(size_t)R * R * 256 + idx];
    beta[e] = b;
    if (!(b > 0.0 && b < 1.0)) {   // the block saw only links or only non-links (or a normaliser failed)
      atomicAdd(ctr + CTR_BETA, (u64)1);
      ctr[CTR_PENDING] = 1;
    }
  }
}

// edge_likelihood (:563-587): one wavefront per pair, lanes stride the K^2 terms, a fixed butterfly
__global__ __launch_bounds__(256) void k_orig_pair_ll(uint64_t m, uint32_t K, const uint32_t *__restrict__ pairs,
                                                      const uint8_t *__restrict__ y, const double *__restrict__ gamma,
                                                      const double *__restrict__ beta, double *__restrict__ out) {
  const uint64_t x = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (x >= m) return;
  const double *gp = gamma + (size_t)pairs[2 * x] * K, *gq = gamma + (size_t)pairs[2 * x + 1] * K;
  double sp = 0.0, sq = 0.0;
  for (uint32_t k = lane; k < K; k += 64) { sp += gp[k]; sq += gq[k]; }
  sp = wave_sum_f64(sp);
  sq = wave_sum_f64(sq);
  const bool yy = y[x] != 0;
  double s = 0.0;
  for (uint32_t e = lane; e < K * K; e += 64) {
    const uint32_t g = e / K, h = e % K;
    const double b = beta[e];
    s += (gp[g] / sp) * (gq[h] / sq) * (yy ? b : 1.0 - b);
  }
  s = wave_sum_f64(s);
  if (lane == 0) out[x] = log(s);
}

}  // namespace

namespace {

void free_graph(svils_orig *h) {
  h->release(ToolHandle::GRAPH);
  h->have_graph = false;   // (the lists of svils_orig_pair_loglik go with the graph)
}

template <int KP, bool LREG>
void launch_pairs(svils_orig *h, uint32_t nblocks, const PairArgs &a) {
  hipLaunchKernelGGL((k_orig_pairs<KP, LREG>), dim3(nblocks), dim3(256), 0, h->st, a);
}
template <int KP>
void launch_acc(svils_orig *h, uint64_t nslots) {
  hipLaunchKernelGGL((k_orig_acc<KP>), dim3(ACC_WAVES / 4), dim3(256), 0, h->st, nslots, h->phi1, h->phi2, h->yv, h->part, h->ctr);
}

int one_sweep(svils_orig *h) {
  const uint32_t n = h->n, K = h->k, KP = h->kp;
  const uint64_t nk = (uint64_t)n * K;
  const uint32_t nnt = 2 * KP * KP;
  HIPCHK(hipEventRecord(h->ev[0], h->st));
  if (int rc = orig_launch_prologue(h, h->elogpi, h->tabs, 0.0)) return rc;
  HIPCHK(hipEventRecord(h->ev[1], h->st));
  hipLaunchKernelGGL(k_orig_fill, dim3(blocks(std::max<uint64_t>(nk, nnt), 256)), dim3(256), 0, h->st, nk, nnt, h->alpha, h->gnext,
                     h->nt, h->ctr);
  uint32_t b = 0;
  for (uint32_t p0 = 0; p0 < n; p0 += h->rows, ++b) {
    const uint32_t rows = std::min(h->rows, n - p0), tpr = (n + TILE_PAIRS - 1) / TILE_PAIRS;
    PairArgs a{n, K, h->nw, p0, rows, tpr, h->adj, h->skip, h->elogpi, h->tabs, h->phi1, h->phi2, h->yv, h->ctr};
    if (int rc = orig_launch_pairs(h, "svils_orig_sweep", a)) return rc;
    HIPCHK(hipEventRecord(h->ev[2 + 2 * b], h->st));
    hipLaunchKernelGGL(k_orig_gamma_rows, dim3(rows), dim3(256), 0, h->st, n, K, KP, p0, h->phi1, h->gnext, h->ctr);
    hipLaunchKernelGGL(k_orig_gamma_cols, dim3(blocks(nk, 256)), dim3(256), 0, h->st, n, K, KP, rows, h->phi2, h->gnext, h->ctr);
    const uint64_t nslots = (uint64_t)rows * n;
    switch (KP) {
      case 16: launch_acc<16>(h, nslots); break;
      case 32: launch_acc<32>(h, nslots); break;
      case 48: launch_acc<48>(h, nslots); break;
      default: launch_acc<64>(h, nslots); break;
    }
    hipLaunchKernelGGL(k_orig_acc_reduce, dim3(blocks(nnt, 256)), dim3(256), 0, h->st, nnt, h->part, h->nt, h->ctr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev[3 + 2 * b], h->st));
  }
  hipLaunchKernelGGL(k_orig_final, dim3(blocks(std::max<uint64_t>(nk, (uint64_t)K * K), 256)), dim3(256), 0, h->st, nk, K, KP, h->gnext,
                     h->nt, h->gamma, h->beta, h->ctr);
  HIPCHK(hipGetLastError());
  h->nlaunch = b;
  h->timed = true;
  return 0;
}

}  // namespace

namespace svils_impl {

int orig_launch_prologue(svils_orig *h, double *elogpi, double *tabs, double eps) {
  const uint32_t n = h->n, K = h->k, KP = h->kp;
  if (elogpi) hipLaunchKernelGGL(k_orig_dir_exp, dim3(blocks(n, 4)), dim3(256), 0, h->st, n, K, h->gamma, h->gtab, elogpi);
  hipLaunchKernelGGL(k_orig_tables, dim3(blocks((uint64_t)KP * h->ld, 256)), dim3(256), 0, h->st, K, KP, h->ld, h->beta, eps, tabs);
  HIPCHK(hipGetLastError());
  return 0;
}

int orig_launch_pairs(svils_orig *h, const char *name, const PairArgs &a) {
  const uint32_t nblocks = blocks((uint64_t)a.rows * a.tpr, TILES_PER_BLOCK);
  switch (h->kp) {
    case 16: launch_pairs<16, true>(h, nblocks, a); break;
    case 32: launch_pairs<32, true>(h, nblocks, a); break;
    case 48: launch_pairs<48, false>(h, nblocks, a); break;
    case 64: launch_pairs<64, false>(h, nblocks, a); break;
    default: return fail(SVILS_ERR_UNSUPPORTED, "%s: no pair kernel for padded K = %u", name, h->kp);   // a missing kernel is an error
  }
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace svils_impl

extern "C" {

int svils_orig_variant(uint32_t k, uint32_t *kp, uint32_t *pairs_per_wave, uint32_t *tables_in_lds) {
  if (!kp || !pairs_per_wave || !tables_in_lds) return fail(SVILS_ERR_ARG, "svils_orig_variant: null argument");
  if (k < 2) return fail(SVILS_ERR_ARG, "svils_orig_variant: need k >= 2");
  if (k > SVILS_ORIG_MAX_K) return fail(SVILS_ERR_UNSUPPORTED, "svils_orig_variant: k = %u exceeds SVILS_ORIG_MAX_K = %d", k, SVILS_ORIG_MAX_K);
  *kp = padded_k(k);
  *pairs_per_wave = TILE_PAIRS;
  *tables_in_lds = padded_k(k) > 32 ? 1 : 0;
  return 0;
}

int svils_orig_create(int device, uint32_t n, uint32_t k, double alpha, svils_orig **out) {
  if (!out) return fail(SVILS_ERR_ARG, "svils_orig_create: null argument");
  *out = nullptr;
  if (n < 2 || k < 2 || !(alpha > 0)) return fail(SVILS_ERR_ARG, "svils_orig_create: need n >= 2, k >= 2 and alpha > 0");
  if (k > SVILS_ORIG_MAX_K) return fail(SVILS_ERR_UNSUPPORTED, "svils_orig_create: k = %u exceeds SVILS_ORIG_MAX_K = %d", k, SVILS_ORIG_MAX_K);
  if (n > SVILS_ORIG_MAX_N) return fail(SVILS_ERR_UNSUPPORTED, "svils_orig_create: n = %u exceeds SVILS_ORIG_MAX_N = %d", n, SVILS_ORIG_MAX_N);
  if (int rc = open_device(device)) return rc;
  svils_orig *h = new (std::nothrow) svils_orig();
  if (!h) return fail(SVILS_ERR_NOMEM, "out of host memory");
  h->n = n;
  h->k = k;
  h->kp = padded_k(k);
  h->ld = (uint32_t)tab_ld((int)h->kp);
  h->nw = (n + 31) / 32;
  h->alpha = alpha;
  const auto scope = ToolHandle::HANDLE;
  const size_t nk = (size_t)n * k, nnt = 2 * (size_t)h->kp * h->kp;
  int rc = h->open(device, 2);
  if (!rc) rc = h->dalloc(scope, &h->gamma, nk);
  if (!rc) rc = h->dalloc(scope, &h->gnext, nk);
  if (!rc) rc = h->dalloc(scope, &h->elogpi, nk);
  if (!rc) rc = h->dalloc(scope, &h->beta, (size_t)k * k);
  if (!rc) rc = h->dalloc(scope, &h->tabs, 2 * (size_t)h->kp * h->ld);
  if (!rc) rc = h->dalloc(scope, &h->nt, nnt);
  if (!rc) rc = h->dalloc(scope, &h->part, (size_t)ACC_WAVES * nnt);
  if (!rc) rc = h->dalloc(scope, &h->ctr, (size_t)CTR_COUNT);
  if (!rc) rc = h->upload(scope, &h->gtab, log_table());
  if (!rc && hipMemsetAsync(h->ctr, 0, CTR_COUNT * sizeof(u64), h->st) != hipSuccess) rc = fail(SVILS_ERR_DEVICE, "svils_orig_create: memset failed");
  if (!rc && hipStreamSynchronize(h->st) != hipSuccess) rc = fail(SVILS_ERR_DEVICE, "svils_orig_create: upload failed");
  if (rc) {
    svils_orig_destroy(h);
    return rc;
  }
  *out = h;
  return 0;
}

int svils_orig_destroy(svils_orig *h) {
  if (h && h->st) {   // the batch buffers of the link queries are not in a scope
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->st);
    free_queries(h);
    free_elbo(h);
  }
  delete h;   // ~ToolHandle: waits for the stream, frees both scopes
  return 0;
}

int svils_orig_set_graph(svils_orig *h, const uint32_t *links, uint64_t nlinks, const uint32_t *skip, uint64_t nskip) {
  if (int rc = check(h, "svils_orig_set_graph")) return rc;
  if ((nlinks && !links) || (nskip && !skip)) return fail(SVILS_ERR_ARG, "svils_orig_set_graph: null argument");
  const uint32_t n = h->n, nw = h->nw;
  std::vector<uint32_t> adj((size_t)n * nw, 0), skp((size_t)n * nw, 0);
  for (uint64_t x = 0; x < nlinks; ++x) {
    const uint32_t p = links[2 * x], q = links[2 * x + 1];
    if (p >= q || q >= n)
      return fail(SVILS_ERR_ARG, "svils_orig_set_graph: link %llu (%u, %u) is not a pair p < q < n = %u", (unsigned long long)x, p, q, n);
    uint32_t &wd = adj[(size_t)p * nw + (q >> 5)];
    if (wd & (1u << (q & 31))) return fail(SVILS_ERR_ARG, "svils_orig_set_graph: link %llu (%u, %u) is repeated", (unsigned long long)x, p, q);
    wd |= 1u << (q & 31);
    adj[(size_t)q * nw + (p >> 5)] |= 1u << (p & 31);   // y(q, p) = y(p, q)
  }
  for (uint64_t x = 0; x < nskip; ++x) {
    const uint32_t p = skip[2 * x], q = skip[2 * x + 1];
    if (p == q || p >= n || q >= n)
      return fail(SVILS_ERR_ARG, "svils_orig_set_graph: skipped pair %llu (%u, %u) is not an ordered pair of two nodes < n = %u",
                  (unsigned long long)x, p, q, n);
    uint32_t &wd = skp[(size_t)p * nw + (q >> 5)];
    if (wd & (1u << (q & 31)))
      return fail(SVILS_ERR_ARG, "svils_orig_set_graph: skipped pair %llu (%u, %u) is repeated", (unsigned long long)x, p, q);
    wd |= 1u << (q & 31);
  }
  const size_t cap = PHI_BYTES / (2 * (size_t)h->kp * sizeof(double));   // slots of one launch
  uint32_t rows = (uint32_t)std::max<size_t>(1, std::min<size_t>(n, cap / n));
  if (h->rows_req) rows = std::min(rows, h->rows_req);
  const uint32_t nlaunch = (n + rows - 1) / rows;
  HIPCHK(hipStreamSynchronize(h->st));
  free_graph(h);
  if (int rc = h->need_events(2 + 2 * (size_t)nlaunch)) return rc;
  const auto scope = ToolHandle::GRAPH;
  const size_t nslots = (size_t)rows * n;
  int rc = 0;
  if (!rc) rc = h->upload(scope, &h->adj, adj);
  if (!rc) rc = h->upload(scope, &h->skip, skp);
  if (!rc) rc = h->dalloc(scope, &h->phi1, nslots * h->kp);
  if (!rc) rc = h->dalloc(scope, &h->phi2, nslots * h->kp);
  if (!rc) rc = h->dalloc(scope, &h->yv, nslots);
  if (!rc && hipStreamSynchronize(h->st) != hipSuccess) rc = fail(SVILS_ERR_DEVICE, "svils_orig_set_graph: upload failed");
  if (rc) {
    free_graph(h);
    return rc;
  }
  h->rows = rows;
  h->have_graph = true;
  h->timed = false;
  return 0;
}

int svils_orig_set_launch_rows(svils_orig *h, uint32_t rows) {
  if (int rc = check(h, "svils_orig_set_launch_rows")) return rc;
  h->rows_req = rows;
  return 0;
}

int svils_orig_set_state(svils_orig *h, const double *gamma, const double *beta) {
  if (int rc = check(h, "svils_orig_set_state")) return rc;
  if (!gamma || !beta) return fail(SVILS_ERR_ARG, "svils_orig_set_state: null argument");
  const size_t nk = (size_t)h->n * h->k, kk = (size_t)h->k * h->k;
  for (size_t x = 0; x < nk; ++x)
    if (!(gamma[x] >= 0) || !std::isfinite(gamma[x])) return fail(SVILS_ERR_ARG, "svils_orig_set_state: gamma[%zu] is negative or not finite", x);
  for (size_t x = 0; x < kk; ++x)
    if (!(beta[x] > 0 && beta[x] < 1)) return fail(SVILS_ERR_ARG, "svils_orig_set_state: beta[%zu] is not inside (0, 1)", x);
  HIPCHK(hipStreamSynchronize(h->st));
  HIPCHK(hipMemcpy(h->gamma, gamma, nk * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->beta, beta, kk * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(h->ctr, 0, CTR_COUNT * sizeof(u64)));
  h->have_state = true;
  ++h->state_gen;
  return 0;
}

int svils_orig_get_state(svils_orig *h, double *gamma, double *beta) {
  if (int rc = check(h, "svils_orig_get_state")) return rc;
  if (!h->have_state) return fail(SVILS_ERR_ARG, "svils_orig_get_state: no state");
  HIPCHK(hipStreamSynchronize(h->st));   // the state is copied out even where the flag is up: it is what the last applied sweep left
  if (gamma) HIPCHK(hipMemcpy(gamma, h->gamma, (size_t)h->n * h->k * sizeof(double), hipMemcpyDeviceToHost));
  if (beta) HIPCHK(hipMemcpy(beta, h->beta, (size_t)h->k * h->k * sizeof(double), hipMemcpyDeviceToHost));
  return settle(h, "svils_orig_get_state");
}

int svils_orig_sweep(svils_orig *h, uint32_t nsweeps) {
  if (int rc = check(h, "svils_orig_sweep")) return rc;
  if (!h->have_graph || !h->have_state) return fail(SVILS_ERR_ARG, "svils_orig_sweep: set the graph and the state first");
  HIPCHK(hipMemsetAsync(h->ctr, 0, 4 * sizeof(u64), h->st));   // pairs, rounds, most rounds, normalisers: of this call
  ++h->state_gen;   // before the first launch: a sweep call that fails half way has changed the state too
  for (uint32_t s = 0; s < nsweeps; ++s)
    if (int rc = one_sweep(h)) return rc;
  return 0;
}

int svils_orig_pair_loglik(svils_orig *h, const uint32_t *pairs, const uint8_t *y, uint64_t m, double *out) {
  if (int rc = check(h, "svils_orig_pair_loglik")) return rc;
  if (!h->have_state) return fail(SVILS_ERR_ARG, "svils_orig_pair_loglik: no state");
  if (m && (!pairs || !y || !out)) return fail(SVILS_ERR_ARG, "svils_orig_pair_loglik: null argument");
  for (uint64_t x = 0; x < m; ++x)
    if (pairs[2 * x] == pairs[2 * x + 1] || pairs[2 * x] >= h->n || pairs[2 * x + 1] >= h->n)
      return fail(SVILS_ERR_ARG, "svils_orig_pair_loglik: pair %llu (%u, %u) is not a pair of two nodes < n = %u", (unsigned long long)x,
                  pairs[2 * x], pairs[2 * x + 1], h->n);
  if (int rc = settle(h, "svils_orig_pair_loglik")) return rc;
  if (!m) return 0;
  const auto scope = ToolHandle::GRAPH;   // the lists are the held-out sets of a graph
  if (int rc = h->reserve(scope, &h->ll_pairs, 2 * (size_t)m)) return rc;
  if (int rc = h->reserve(scope, &h->ll_y, (size_t)m)) return rc;
  if (int rc = h->reserve(scope, &h->ll_out, (size_t)m)) return rc;
  HIPCHK(hipMemcpyAsync(h->ll_pairs, pairs, 2 * m * sizeof(uint32_t), hipMemcpyHostToDevice, h->st));
  HIPCHK(hipMemcpyAsync(h->ll_y, y, m, hipMemcpyHostToDevice, h->st));
  hipLaunchKernelGGL(k_orig_pair_ll, dim3(blocks(m, 4)), dim3(256), 0, h->st, m, h->k, h->ll_pairs, h->ll_y, h->gamma, h->beta, h->ll_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, h->ll_out, m * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  return 0;
}

int svils_orig_get_stats(svils_orig *h, uint64_t *pairs_done, uint64_t *rounds_total, uint32_t *rounds_max, uint64_t *bad_normalisers,
                         uint64_t *bad_betas) {
  if (int rc = check(h, "svils_orig_get_stats")) return rc;
  u64 c[CTR_COUNT] = {0};
  HIPCHK(hipMemcpyAsync(c, h->ctr, sizeof c, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  if (pairs_done) *pairs_done = c[CTR_PAIRS];
  if (rounds_total) *rounds_total = c[CTR_ROUNDS];
  if (rounds_max) *rounds_max = (uint32_t)c[CTR_MAXR];
  if (bad_normalisers) *bad_normalisers = c[CTR_NORM];
  if (bad_betas) *bad_betas = c[CTR_BETA];
  return 0;
}

int svils_orig_get_timing(svils_orig *h, double ms[3]) {
  if (int rc = check(h, "svils_orig_get_timing")) return rc;
  if (!ms) return fail(SVILS_ERR_ARG, "svils_orig_get_timing: null argument");
  HIPCHK(hipStreamSynchronize(h->st));
  ms[0] = h->elapsed_ms(0, 1, h->timed);
  ms[1] = h->launches_ms(1, h->nlaunch, h->timed);
  ms[2] = h->launches_ms(2, h->nlaunch, h->timed);
  return 0;
}

}  // extern "C"
