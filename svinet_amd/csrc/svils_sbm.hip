// svils_sbm.hip -- -single: the reference's SBM::batch_infer (src/sbm.cc:457-543, src/sbm.hh), the single-membership
// stochastic blockmodel, on the device.  include/svils.h has the written definition of an iteration; DESIGN.md section 4r
// the algebra.  The reference walks all n^2 pairs in both steps.  Here, with S_k = sum_i phi_ik, D1_k = Elogbeta[k][0] -
// Elogbeta[K][0] and D0_k = Elogbeta[k][1] - Elogbeta[K][1], node p's update is
//
//   a_k = Elogpi_k + D1_k L_k(p) + D0_k Z_k(p)      (+ a term without k, which the softmax cancels)
//   L_k(p) = A_k - B1_k,   Z_k(p) = S_k - phi_pk - A_k - B0_k
//   A = sum of phi_q over all link neighbours of p, B1 / B0 = the same over p's skipped partners that are links / non-links
//
// and in the M-step the sum of phi_ik phi_jk over the trained non-links is (S_k^2 - sum_i phi_ik^2) / 2 minus the sum over
// all links minus the sum over the skipped non-links.  A pass costs O((links + skips) K).
//
//   k_sbm_colsum        per block of nodes, S_k and sum phi^2 in a fixed order; runs before every pass, so S carries no
//                       rounding from pass to pass.  The block partials are folded (ascending block) where they are read
//   k_sbm_chain<B,V>    the Gauss-Seidel pass over nodes [p0, p1): ONE workgroup of B wavefronts per launch; its only waits
//                       are its own barriers.  Blocks of B consecutive nodes: wavefront w first sums the rows of node b0 + w's
//                       partners outside [b0, b0 + w) -- rows that are final for its purpose, so the B gathers overlap their
//                       memory latency -- then B short serial turns follow: turn w adds the rows of its in-block earlier
//                       partners from the LDS copy of the block's new rows, takes S from LDS, does the softmax across its
//                       lanes, writes the row to LDS and to phi, moves S by new - old and adds |old - new| to msum, in node
//                       order.  B = 1 is the plain chain.  A row's sums are two chains of additions, over the partners
//                       below p and over those above it, each in ascending order: where a block starts changes which
//                       additions the gather makes and which the turn, never their order -- so the bits depend neither on B
//                       nor on how a pass is cut into launches.  S and msum travel between launches in `carry`.  At the
//                       end of a pass the kernel records msum, counts the pass and raises `done` if msum < 0.01; launches
//                       behind a raised flag return at once
//   k_sbm_links         phi_i o phi_j over the link list, and over the skip list split by y: every wavefront takes a contiguous
//                       run and leaves its partial sums
//   k_sbm_mstep         one block: folds the partials in ascending order; gamma, lambda, Elogpi, Elogbeta
//   k_sbm_elog          Elogpi, Elogbeta of a state that arrives from the host
//   k_sbm_pair_ll       edge_likelihood2 (src/sbm.hh:284-308): one wavefront per pair
//   k_sbm_elbo_rows     svils_sbmelbo (-single-logl): sum phi (Elogpi - log phi) per piece of the rows,
//                       rows packed into a wavefront as k_sbm_links packs pairs
//   k_sbm_elbo_fold     one block: the pair part of the bound from the colsum and link partials as the M-step folds them,
//                       and the sum of the row partials, in ascending order
//
// No floating-point atomics; all sums fp64 in a fixed order.
#include "svils_csr.h"
#include "svils_devutil.h"
#include "svils_tool.h"
#include "svils_waveutil.h"

using namespace svils_impl;

namespace {

typedef unsigned long long u64;
enum { CTL_DONE, CTL_PASSES, CTL_TOTAL, CTL_COUNT };

constexpr int CHAIN_B = 8;                    // wavefronts of the chain's workgroup = nodes whose gathers overlap
constexpr uint32_t CHAIN_NODES = 2048;        // nodes per launch unless svils_sbm_set_launch_nodes says otherwise
constexpr uint32_t COLSUM_BLOCKS = 256;       // at most; a block takes at least 64 nodes
constexpr uint32_t LINK_WAVES = 1024;         // wavefronts (and partial sums) of k_sbm_links
constexpr double ESTEP_THRESH = 0.01;         // src/sbm.cc:481
constexpr int MAX_V = SVILS_SBM_MAX_K / 64;

__device__ inline double wave_max_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// sum over the colsum blocks, ascending: which 0 = S_k, 1 = sum_i phi_ik^2
__device__ inline double fold_colsum(const double *cpart, uint32_t nb, uint32_t K, uint32_t which, uint32_t k) {
  double s = 0.0;
  for (uint32_t b = 0; b < nb; ++b) s += cpart[((size_t)b * 2 + which) * K + k];
  return s;
}

// cpart[block][2][K].  Thread (r, k) takes the rows i0 + r, i0 + r + R, .. of the block's nodes, R = 256 / K; thread k then
// adds the R partials in ascending r
__global__ __launch_bounds__(256) void k_sbm_colsum(uint32_t n, uint32_t K, uint32_t per, const double *phi, double *cpart,
                                                    const u64 *ctl, int guard) {
  __shared__ double sm[2][256];
  if (guard && ctl[CTL_DONE]) return;
  const uint32_t t = threadIdx.x, R = 256 / K, r = t / K, k = t % K;
  const uint32_t i0 = blockIdx.x * per, i1 = min(n, i0 + per);
  double s = 0.0, q = 0.0;
  if (r < R)
    for (uint32_t i = i0 + r; i < i1; i += R) {
      const double v = phi[(size_t)i * K + k];
      s += v;
      q = fma(v, v, q);
    }
  sm[0][t] = s;
  sm[1][t] = q;
  __syncthreads();
  if (t < K) {
    double ts = 0.0, tq = 0.0;
    for (uint32_t j = 0; j < R; ++j) {
      ts += sm[0][j * K + t];
      tq += sm[1][j * K + t];
    }
    cpart[((size_t)blockIdx.x * 2) * K + t] = ts;
    cpart[((size_t)blockIdx.x * 2 + 1) * K + t] = tq;
  }
}

struct ChainArgs {
  uint32_t n, K, p0, p1, nb;                  // the launch takes nodes [p0, p1); nb: colsum blocks
  double *phi;                                // [n][K] read and written here: a plain pointer, plain loads
  const double *elogpi, *elogbeta, *cpart;
  double *carry, *msums;                      // [K + 1]: S, msum; [SVILS_SBM_MAX_PASSES]
  u64 *ctl;
  const uint64_t *lrow, *srow;                // [n + 1]
  const uint32_t *lcol, *scol;
  const uint8_t *sy;                          // y of every skip entry
};

// acc += the rows col[a .. b) of phi, one entry after the other (four loads in flight)
template <int V>
__device__ inline void add_rows(const double *phi, const uint32_t *col, uint64_t a, uint64_t b, uint32_t K, uint32_t lane,
                                double (&acc)[V]) {
  uint64_t e = a;
  for (; e + 4 <= b; e += 4) {
    const uint32_t q0 = col[e], q1 = col[e + 1], q2 = col[e + 2], q3 = col[e + 3];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const uint32_t k = lane + 64 * v;
      if (k < K) {
        const double r0 = phi[(size_t)q0 * K + k], r1 = phi[(size_t)q1 * K + k], r2 = phi[(size_t)q2 * K + k],
                     r3 = phi[(size_t)q3 * K + k];
        acc[v] = (((acc[v] + r0) + r1) + r2) + r3;
      }
    }
  }
  for (; e < b; ++e) {
    const uint32_t q = col[e];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const uint32_t k = lane + 64 * v;
      if (k < K) acc[v] += phi[(size_t)q * K + k];
    }
  }
}

// the same over skip entries: a link partner's row goes to a1, a non-link partner's to a0 (the other takes + 0.0)
template <int V>
__device__ inline void add_rows_y(const double *phi, const uint32_t *col, const uint8_t *sy, uint64_t a, uint64_t b, uint32_t K,
                                  uint32_t lane, double (&a1)[V], double (&a0)[V]) {
  for (uint64_t e = a; e < b; ++e) {
    const uint32_t q = col[e];
    const bool y = sy[e] != 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const uint32_t k = lane + 64 * v;
      if (k < K) {
        const double r = phi[(size_t)q * K + k];
        a1[v] += y ? r : 0.0;
        a0[v] += y ? 0.0 : r;
      }
    }
  }
}

// entries of the ascending row col[e0 .. e1) below b0 and below p (the whole wavefront calls it)
__device__ inline void split_row(const uint32_t *col, uint64_t e0, uint64_t e1, uint32_t b0, uint32_t p, uint32_t lane, uint64_t &mid0,
                                 uint64_t &mid1) {
  uint32_t c0 = 0, c1 = 0;
  for (uint64_t e = e0 + lane; e < e1; e += 64) {
    const uint32_t q = col[e];
    c0 += q < b0;
    c1 += q < p;
  }
  mid0 = e0 + wave_sum_u32(c0);
  mid1 = e0 + wave_sum_u32(c1);
}

template <int B, int V>
__global__ __launch_bounds__(64 * B) void k_sbm_chain(ChainArgs x) {
  __shared__ double sS[64 * V];               // the current column sums
  __shared__ double rows[B][64 * V];          // the new rows of the block at hand
  __shared__ double s_msum;
  if (x.ctl[CTL_DONE]) return;                // the same answer in every thread of the launch
  const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63, K = x.K;
  for (uint32_t k = t; k < K; k += 64 * B) sS[k] = x.p0 == 0 ? fold_colsum(x.cpart, x.nb, K, 0, k) : x.carry[k];
  if (t == 0) s_msum = x.p0 == 0 ? 0.0 : x.carry[K];
  double ep[V], d1[V], d0[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const uint32_t k = lane + 64 * v;
    ep[v] = d1[v] = d0[v] = 0.0;
    if (k < K) {
      ep[v] = x.elogpi[k];
      d1[v] = x.elogbeta[2 * k] - x.elogbeta[2 * K];
      d0[v] = x.elogbeta[2 * k + 1] - x.elogbeta[2 * K + 1];
    }
  }
  __syncthreads();
  for (uint32_t b0 = x.p0; b0 < x.p1; b0 += B) {   // the same trip count in every wavefront
    const uint32_t p = b0 + w;
    const bool active = p < x.p1;
    double alo[V], ahi[V], l1lo[V], l1hi[V], l0lo[V], l0hi[V], old[V];
#pragma unroll
    for (int v = 0; v < V; ++v) alo[v] = ahi[v] = l1lo[v] = l1hi[v] = l0lo[v] = l0hi[v] = old[v] = 0.0;
    uint64_t lm0 = 0, lm1 = 0, sm0 = 0, sm1 = 0;
    if (active) {                                   // the gather: partners outside [b0, p)
      const uint64_t le0 = x.lrow[p], le1 = x.lrow[p + 1], se0 = x.srow[p], se1 = x.srow[p + 1];
      split_row(x.lcol, le0, le1, b0, p, lane, lm0, lm1);
      split_row(x.scol, se0, se1, b0, p, lane, sm0, sm1);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const uint32_t k = lane + 64 * v;
        if (k < K) old[v] = x.phi[(size_t)p * K + k];
      }
      add_rows<V>(x.phi, x.lcol, le0, lm0, K, lane, alo);
      add_rows<V>(x.phi, x.lcol, lm1, le1, K, lane, ahi);
      add_rows_y<V>(x.phi, x.scol, x.sy, se0, sm0, K, lane, l1lo, l0lo);
      add_rows_y<V>(x.phi, x.scol, x.sy, sm1, se1, K, lane, l1hi, l0hi);
    }
    for (uint32_t u = 0; u < (uint32_t)B; ++u) {    // the turns: one wavefront at a time, a barrier after each
      if (w == u && active) {
        for (uint64_t e = lm0; e < lm1; ++e) {      // in-block earlier partners: their new rows are in LDS
          const double *r = rows[x.lcol[e] - b0];
#pragma unroll
          for (int v = 0; v < V; ++v) alo[v] += r[lane + 64 * v];
        }
        for (uint64_t e = sm0; e < sm1; ++e) {
          const double *r = rows[x.scol[e] - b0];
          const bool y = x.sy[e] != 0;
#pragma unroll
          for (int v = 0; v < V; ++v) {
            l1lo[v] += y ? r[lane + 64 * v] : 0.0;
            l0lo[v] += y ? 0.0 : r[lane + 64 * v];
          }
        }
        double a[V], m = NEG_INF;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const uint32_t k = lane + 64 * v;
          const double A = alo[v] + ahi[v];
          const double L = A - (l1lo[v] + l1hi[v]);
          const double Z = ((sS[k] - old[v]) - A) - (l0lo[v] + l0hi[v]);
          a[v] = k < K ? fma(d0[v], Z, fma(d1[v], L, ep[v])) : NEG_INF;
          m = fmax(m, a[v]);
        }
        m = wave_max_f64(m);
        double s = 0.0;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          a[v] = lane + 64 * v < K ? exp_neg(a[v] - m) : 0.0;
          s += a[v];
        }
        s = wave_sum_f64(s);
        double diff = 0.0;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const uint32_t k = lane + 64 * v;
          const double nw = a[v] / s;
          rows[u][k] = nw;                          // (0 past column K: no turn reads it for a column it owns)
          if (k < K) {
            x.phi[(size_t)p * K + k] = nw;
            sS[k] = (sS[k] + nw) - old[v];
            diff += fabs(old[v] - nw);
          }
        }
        diff = wave_sum_f64(diff);
        if (lane == 0) s_msum += diff;
      }
      __syncthreads();
    }
  }
  for (uint32_t k = t; k < K; k += 64 * B) x.carry[k] = sS[k];
  if (t == 0) {
    if (x.p1 == x.n) {                              // the pass ends here
      const u64 pass = x.ctl[CTL_PASSES];
      if (pass < SVILS_SBM_MAX_PASSES) x.msums[pass] = s_msum;
      x.ctl[CTL_PASSES] = pass + 1;
      x.ctl[CTL_TOTAL] += 1;
      if (s_msum < ESTEP_THRESH) x.ctl[CTL_DONE] = 1;
    } else {
      x.carry[K] = s_msum;
    }
  }
}

// lpart[wave][3][K]: the sums of phi_i o phi_j over the wavefront's run of the link list (0) and of the skip list, links (1)
// and non-links (2).  W lanes hold a row (W the power of two >= min(K, 64)); the 64 / W lane groups take every (64 / W)th pair
// of the run and are added by a fixed butterfly
__global__ __launch_bounds__(256) void k_sbm_links(uint32_t K, uint32_t W, uint64_t nl, uint64_t ns, const uint32_t *__restrict__ edges,
                                                   const uint32_t *__restrict__ spairs, const uint8_t *__restrict__ sy,
                                                   const double *__restrict__ phi, double *__restrict__ lpart) {
  const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane / W, lw = lane % W, G = 64 / W;
  const uint64_t perl = (nl + LINK_WAVES - 1) / LINK_WAVES, pers = (ns + LINK_WAVES - 1) / LINK_WAVES;
  const uint64_t l0 = min(nl, wave * perl), l1 = min(nl, l0 + perl), s0 = min(ns, wave * pers), s1 = min(ns, s0 + pers);
  double X[MAX_V], Y1[MAX_V], Y0[MAX_V];
#pragma unroll
  for (int v = 0; v < MAX_V; ++v) X[v] = Y1[v] = Y0[v] = 0.0;
  for (uint64_t e = l0 + g; e < l1; e += G) {
    const uint32_t i = edges[2 * e], j = edges[2 * e + 1];
#pragma unroll
    for (int v = 0; v < MAX_V; ++v) {
      const uint32_t k = lw + 64 * v;
      if (k < K) X[v] = fma(phi[(size_t)i * K + k], phi[(size_t)j * K + k], X[v]);
    }
  }
  for (uint64_t e = s0 + g; e < s1; e += G) {
    const uint32_t i = spairs[2 * e], j = spairs[2 * e + 1];
    const bool y = sy[e] != 0;
#pragma unroll
    for (int v = 0; v < MAX_V; ++v) {
      const uint32_t k = lw + 64 * v;
      if (k < K) {
        const double pp = phi[(size_t)i * K + k] * phi[(size_t)j * K + k];
        Y1[v] += y ? pp : 0.0;
        Y0[v] += y ? 0.0 : pp;
      }
    }
  }
#pragma unroll
  for (int v = 0; v < MAX_V; ++v) {
    for (uint32_t o = W; o < 64; o <<= 1) {
      X[v] += __shfl_xor(X[v], o, 64);
      Y1[v] += __shfl_xor(Y1[v], o, 64);
      Y0[v] += __shfl_xor(Y0[v], o, 64);
    }
    const uint32_t k = lw + 64 * v;
    if (g == 0 && k < K) {
      lpart[((size_t)wave * 3 + 0) * K + k] = X[v];
      lpart[((size_t)wave * 3 + 1) * K + k] = Y1[v];
      lpart[((size_t)wave * 3 + 2) * K + k] = Y0[v];
    }
  }
}

// Elogpi [K] and Elogbeta [K + 1][2] of gamma and lambda; the whole block calls it (behind a barrier where the block wrote them)
__device__ inline void write_elog(uint32_t K, const double *gamma, const double *lam, double *elogpi, double *elogbeta,
                                  const double2 *logtab, double *s_sg) {
  const uint32_t t = threadIdx.x;
  if (t == 0) {
    double sg = 0.0;
    for (uint32_t k = 0; k < K; ++k) sg += gamma[k];
    *s_sg = digamma(sg, logtab);
  }
  __syncthreads();
  if (t < K) elogpi[t] = digamma(gamma[t], logtab) - *s_sg;
  for (uint32_t k = t; k <= K; k += blockDim.x) {
    const double ps = digamma(lam[2 * k] + lam[2 * k + 1], logtab);
    elogbeta[2 * k] = digamma(lam[2 * k], logtab) - ps;
    elogbeta[2 * k + 1] = digamma(lam[2 * k + 1], logtab) - ps;
  }
}

struct MstepArgs {
  uint32_t K, nb;
  double alpha, n1, n0;                       // n1, n0: the trained links and non-links, exact integers
  const double *eta, *cpart, *lpart, *gtab;
  double *gamma, *lam, *elogpi, *elogbeta;
};

__global__ __launch_bounds__(256) void k_sbm_mstep(MstepArgs x) {
  __shared__ double2 logtab[128];
  __shared__ double sa[256], sb[256], s_sg;
  load_logtab(logtab, x.gtab);
  const uint32_t t = threadIdx.x, K = x.K;
  if (t < K) {
    const double S = fold_colsum(x.cpart, x.nb, K, 0, t), Q = fold_colsum(x.cpart, x.nb, K, 1, t);
    double X = 0.0, Y1 = 0.0, Y0 = 0.0;
    for (uint32_t wv = 0; wv < LINK_WAVES; ++wv) {
      X += x.lpart[((size_t)wv * 3 + 0) * K + t];
      Y1 += x.lpart[((size_t)wv * 3 + 1) * K + t];
      Y0 += x.lpart[((size_t)wv * 3 + 2) * K + t];
    }
    const double a = X - Y1;                                    // over the trained links
    const double b = (0.5 * fma(S, S, -Q) - X) - Y0;            // over the trained non-links
    x.gamma[t] = x.alpha + S;
    x.lam[2 * t] = x.eta[2 * t] + a;
    x.lam[2 * t + 1] = x.eta[2 * t + 1] + b;
    sa[t] = a;
    sb[t] = b;
  }
  __syncthreads();
  if (t == 0) {                                                 // row K: sum_k (1 - phi_ik phi_jk) over the pairs (src/sbm.cc:512-515)
    double ta = 0.0, tb = 0.0;
    for (uint32_t k = 0; k < K; ++k) {
      ta += sa[k];
      tb += sb[k];
    }
    x.lam[2 * K] = x.eta[2 * K] + ((double)K * x.n1 - ta);
    x.lam[2 * K + 1] = x.eta[2 * K + 1] + ((double)K * x.n0 - tb);
  }
  __syncthreads();
  write_elog(K, x.gamma, x.lam, x.elogpi, x.elogbeta, logtab, &s_sg);
}

__global__ __launch_bounds__(256) void k_sbm_elog(uint32_t K, const double *gamma, const double *lam, const double *gtab, double *elogpi,
                                                  double *elogbeta) {
  __shared__ double2 logtab[128];
  __shared__ double s_sg;
  load_logtab(logtab, gtab);
  __syncthreads();
  write_elog(K, gamma, lam, elogpi, elogbeta, logtab, &s_sg);
}

__global__ __launch_bounds__(256) void k_sbm_pair_ll(uint64_t m, uint32_t K, const uint32_t *__restrict__ pairs,
                                                     const uint8_t *__restrict__ y, const double *__restrict__ phi,
                                                     const double *__restrict__ lam, double *__restrict__ out) {
  const uint64_t x = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (x >= m) return;   // whole wavefronts leave together
  const double *pp = phi + (size_t)pairs[2 * x] * K, *pq = phi + (size_t)pairs[2 * x + 1] * K;
  const bool yy = y[x] != 0;
  double s = 0.0, sum = 0.0;
  for (uint32_t k = lane; k < K; k += 64) {
    const double r = lam[2 * k] / (lam[2 * k] + lam[2 * k + 1]), v = pp[k] * pq[k];
    s += v * (yy ? r : 1.0 - r);
    sum += v;
  }
  s = wave_sum_f64(s);
  sum = wave_sum_f64(sum);
  const double rK = lam[2 * K] / (lam[2 * K] + lam[2 * K + 1]);
  s += (1.0 - sum) * (yy ? rK : 1.0 - rK);
  if (lane == 0) out[x] = log(s < 1e-30 ? 1e-30 : s);
}

// ---- svils_sbmelbo: the lower bound of the current state ------------------------------------------
// epart[piece] = sum over the piece's rows i and all k of phi_ik (Elogpi_k - log phi_ik), an exact 0 of phi adding 0.  One
// wavefront per piece of `per` consecutive rows; lanes as in k_sbm_links: W lanes hold a row, the 64 / W lane groups take
// every (64 / W)th row of the piece, a lane adds its entries in ascending row (and column), the lanes by the fixed butterfly
__global__ __launch_bounds__(256) void k_sbm_elbo_rows(uint32_t n, uint32_t K, uint32_t W, uint32_t per, uint32_t pieces,
                                                       const double *__restrict__ phi, const double *__restrict__ elogpi,
                                                       double *__restrict__ epart) {
  const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane / W, lw = lane % W, G = 64 / W;
  if (wave >= pieces) return;   // whole wavefronts leave together
  const uint32_t r0 = wave * per, r1 = min(n, r0 + per);
  double ep[MAX_V];
#pragma unroll
  for (int v = 0; v < MAX_V; ++v) ep[v] = lw + 64 * v < K ? elogpi[lw + 64 * v] : 0.0;
  double acc = 0.0;
  for (uint32_t i = r0 + g; i < r1; i += G) {
#pragma unroll
    for (int v = 0; v < MAX_V; ++v) {
      const uint32_t k = lw + 64 * v;
      if (k < K) {
        const double x = phi[(size_t)i * K + k];
        acc += x > 0.0 ? x * (ep[v] - log(x)) : 0.0;
      }
    }
  }
  acc = wave_sum_f64(acc);
  if (lane == 0) epart[wave] = acc;
}

struct ElboArgs {
  uint32_t K, nb, pieces;
  double n1, n0;
  const double *elogbeta, *cpart, *lpart, *epart;
  double *eout;                               // [2]: P, N
};

// one block: a_k and b_k from the partials exactly as k_sbm_mstep forms them, then P (thread 0) and N (thread 64), every
// sum in ascending order
__global__ __launch_bounds__(256) void k_sbm_elbo_fold(ElboArgs x) {
  __shared__ double sa[256], sb[256];
  const uint32_t t = threadIdx.x, K = x.K;
  if (t < K) {
    const double S = fold_colsum(x.cpart, x.nb, K, 0, t), Q = fold_colsum(x.cpart, x.nb, K, 1, t);
    double X = 0.0, Y1 = 0.0, Y0 = 0.0;
    for (uint32_t wv = 0; wv < LINK_WAVES; ++wv) {
      X += x.lpart[((size_t)wv * 3 + 0) * K + t];
      Y1 += x.lpart[((size_t)wv * 3 + 1) * K + t];
      Y0 += x.lpart[((size_t)wv * 3 + 2) * K + t];
    }
    const double a = X - Y1;                                    // over the trained links
    const double b = (0.5 * fma(S, S, -Q) - X) - Y0;            // over the trained non-links
    sa[t] = (x.elogbeta[2 * t] - x.elogbeta[2 * K]) * a;
    sb[t] = (x.elogbeta[2 * t + 1] - x.elogbeta[2 * K + 1]) * b;
  }
  __syncthreads();
  if (t == 0) {
    double pa = 0.0, pb = 0.0;
    for (uint32_t k = 0; k < K; ++k) {
      pa += sa[k];
      pb += sb[k];
    }
    x.eout[0] = ((pa + pb) + x.n1 * x.elogbeta[2 * K]) + x.n0 * x.elogbeta[2 * K + 1];
  }
  if (t == 64) {
    double s = 0.0;
    for (uint32_t p = 0; p < x.pieces; ++p) s += x.epart[p];
    x.eout[1] = s;
  }
}

}  // namespace

// events: ev[0] .. ev[1] the call; ev[2 + 2 b] .. ev[3 + 2 b] the chain launches of pass b of the last E-step; ev[22] .. ev[23]
// the M-step of the last iteration; ev[24] .. ev[25] the last svils_sbmelbo pass
struct svils_sbm : ToolHandle {
  uint32_t n = 0, k = 0;
  double alpha = 0;
  // HANDLE scope
  double *phi = nullptr;                                          // [n][k]
  double *gamma = nullptr, *elogpi = nullptr;                     // [k]
  double *lam = nullptr, *eta = nullptr, *elogbeta = nullptr;     // [k + 1][2]
  double *carry = nullptr, *msums = nullptr;                      // [k + 1], [SVILS_SBM_MAX_PASSES]
  double *cpart = nullptr, *lpart = nullptr;                      // [nb][2][k], [LINK_WAVES][3][k]
  double *gtab = nullptr;                                         // [128][2] log_tab's table
  double *epart = nullptr, *eout = nullptr;                       // svils_sbmelbo: [pieces] row partials; [2] P, N
  std::vector<double> eta_h;                                      // eta on the host (the G part of svils_sbmelbo)
  uint32_t eper = 0, epieces = 0;                                 // rows per piece of k_sbm_elbo_rows, pieces
  u64 *ctl = nullptr;                                             // [CTL_COUNT]
  // GRAPH scope
  uint64_t *lrow = nullptr, *srow = nullptr;                      // the links and the skipped pairs as symmetric CSRs
  uint32_t *lcol = nullptr, *scol = nullptr;
  uint8_t *sy = nullptr, *py = nullptr;                           // y of every skip entry of the CSR / of the pair list
  uint32_t *edges = nullptr, *spairs = nullptr;                   // [nlinks][2], [nskip][2]: the lists as given
  uint32_t *ll_pairs = nullptr;                                   // svils_sbm_pair_loglik: grown on demand
  uint8_t *ll_y = nullptr;
  double *ll_out = nullptr;
  uint64_t nlinks = 0, nskip = 0;
  double n1 = 0, n0 = 0;                                          // trained links / non-links
  uint32_t nb = 0, per = 0;                                       // colsum blocks, nodes per block
  uint32_t launch_nodes = 0;
  bool plain = false;
  bool have_graph = false, have_state = false, timed = false, timed_m = false, timed_e = false;
};

namespace {

constexpr int EV_PASS = 2, EV_MSTEP = 2 + 2 * SVILS_SBM_MAX_PASSES, EV_ELBO = EV_MSTEP + 2, EV_COUNT = EV_ELBO + 2;
constexpr uint32_t ELBO_PIECE_ROWS = SVILS_SBMELBO_PIECE_ROWS, ELBO_MAX_PIECES = 4096;   // the fold adds the pieces one by one

template <int B>
int launch_chain(svils_sbm *h, const ChainArgs &a) {
  switch ((h->k + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_sbm_chain<B, 1>), dim3(1), dim3(64 * B), 0, h->st, a); break;
    case 2: hipLaunchKernelGGL((k_sbm_chain<B, 2>), dim3(1), dim3(64 * B), 0, h->st, a); break;
    case 3: hipLaunchKernelGGL((k_sbm_chain<B, 3>), dim3(1), dim3(64 * B), 0, h->st, a); break;
    case 4: hipLaunchKernelGGL((k_sbm_chain<B, 4>), dim3(1), dim3(64 * B), 0, h->st, a); break;
    default: return fail(SVILS_ERR_UNSUPPORTED, "svils_sbm: no chain kernel for k = %u", h->k);   // a missing kernel is an error
  }
  return 0;
}

// the power of two >= min(k, 64) lanes that hold a row in k_sbm_links and k_sbm_elbo_rows
uint32_t row_lanes(uint32_t k) {
  uint32_t W = 2;
  while (W < 64 && W < k) W <<= 1;
  return W;
}

void launch_colsum(svils_sbm *h, int guard) {
  hipLaunchKernelGGL(k_sbm_colsum, dim3(h->nb), dim3(256), 0, h->st, h->n, h->k, h->per, h->phi, h->cpart, h->ctl, guard);
}

// one E-step of at most max_passes passes: every launch is queued; those behind the raised flag return at once
int queue_estep(svils_sbm *h, uint32_t max_passes) {
  HIPCHK(hipMemsetAsync(h->ctl, 0, 2 * sizeof(u64), h->st));   // done, passes
  HIPCHK(hipMemsetAsync(h->msums, 0, SVILS_SBM_MAX_PASSES * sizeof(double), h->st));
  const uint32_t cap = h->launch_nodes ? h->launch_nodes : CHAIN_NODES;
  for (uint32_t pass = 0; pass < SVILS_SBM_MAX_PASSES; ++pass) {
    if (pass < max_passes) launch_colsum(h, 1);
    HIPCHK(hipEventRecord(h->ev[EV_PASS + 2 * pass], h->st));
    for (uint32_t p0 = 0; pass < max_passes && p0 < h->n; p0 += std::min(cap, h->n - p0)) {
      const ChainArgs a{h->n, h->k, p0, p0 + std::min(cap, h->n - p0), h->nb, h->phi, h->elogpi, h->elogbeta, h->cpart, h->carry,
                        h->msums, h->ctl, h->lrow, h->srow, h->lcol, h->scol, h->sy};
      if (int rc = h->plain ? launch_chain<1>(h, a) : launch_chain<CHAIN_B>(h, a)) return rc;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev[EV_PASS + 2 * pass + 1], h->st));
  }
  return 0;
}

int queue_mstep(svils_sbm *h) {
  HIPCHK(hipEventRecord(h->ev[EV_MSTEP], h->st));
  launch_colsum(h, 0);
  const uint32_t W = row_lanes(h->k);
  hipLaunchKernelGGL(k_sbm_links, dim3(LINK_WAVES / 4), dim3(256), 0, h->st, h->k, W, (uint64_t)h->nlinks, (uint64_t)h->nskip, h->edges,
                     h->spairs, h->py, h->phi, h->lpart);
  const MstepArgs a{h->k, h->nb, h->alpha, h->n1, h->n0, h->eta, h->cpart, h->lpart, h->gtab, h->gamma, h->lam, h->elogpi, h->elogbeta};
  hipLaunchKernelGGL(k_sbm_mstep, dim3(1), dim3(256), 0, h->st, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev[EV_MSTEP + 1], h->st));
  return 0;
}

void free_graph(svils_sbm *h) {
  h->release(ToolHandle::GRAPH);
  h->have_graph = false;
}

int ready(svils_sbm *h, const char *name) {
  if (int rc = check(h, name)) return rc;
  if (!h->have_graph || !h->have_state) return fail(SVILS_ERR_ARG, "%s: set the graph and the state first", name);
  return 0;
}

}  // namespace

extern "C" {

int svils_sbm_variant(uint32_t k, uint32_t *cols_per_lane, uint32_t *block_nodes) {
  if (!cols_per_lane || !block_nodes) return fail(SVILS_ERR_ARG, "svils_sbm_variant: null argument");
  if (k < 2) return fail(SVILS_ERR_ARG, "svils_sbm_variant: need k >= 2");
  if (k > SVILS_SBM_MAX_K) return fail(SVILS_ERR_UNSUPPORTED, "svils_sbm_variant: k = %u exceeds SVILS_SBM_MAX_K = %d", k, SVILS_SBM_MAX_K);
  *cols_per_lane = (k + 63) / 64;
  *block_nodes = CHAIN_B;
  return 0;
}

int svils_sbm_create(int device, uint32_t n, uint32_t k, double alpha, const double *eta, svils_sbm **out) {
  if (!out) return fail(SVILS_ERR_ARG, "svils_sbm_create: null argument");
  *out = nullptr;
  if (!eta) return fail(SVILS_ERR_ARG, "svils_sbm_create: null argument");
  if (n < 2 || k < 2 || !(alpha > 0)) return fail(SVILS_ERR_ARG, "svils_sbm_create: need n >= 2, k >= 2 and alpha > 0");
  if (k > SVILS_SBM_MAX_K) return fail(SVILS_ERR_UNSUPPORTED, "svils_sbm_create: k = %u exceeds SVILS_SBM_MAX_K = %d", k, SVILS_SBM_MAX_K);
  for (uint32_t x = 0; x < 2 * (k + 1); ++x)
    if (!(eta[x] > 0) || !std::isfinite(eta[x])) return fail(SVILS_ERR_ARG, "svils_sbm_create: eta[%u] is not > 0", x);
  if (int rc = open_device(device)) return rc;
  svils_sbm *h = new (std::nothrow) svils_sbm();
  if (!h) return fail(SVILS_ERR_NOMEM, "out of host memory");
  h->n = n;
  h->k = k;
  h->alpha = alpha;
  h->nb = std::min(COLSUM_BLOCKS, (n + 63) / 64);
  h->per = (n + h->nb - 1) / h->nb;
  h->nb = (n + h->per - 1) / h->per;   // no empty block
  h->eper = std::max(ELBO_PIECE_ROWS, (n + ELBO_MAX_PIECES - 1) / ELBO_MAX_PIECES);
  h->epieces = (n + h->eper - 1) / h->eper;
  h->eta_h.assign(eta, eta + 2 * ((size_t)k + 1));
  const auto scope = ToolHandle::HANDLE;
  const size_t kk = 2 * ((size_t)k + 1);
  int rc = h->open(device, EV_COUNT);
  if (!rc) rc = h->dalloc(scope, &h->phi, (size_t)n * k);
  if (!rc) rc = h->dalloc(scope, &h->gamma, (size_t)k);
  if (!rc) rc = h->dalloc(scope, &h->elogpi, (size_t)k);
  if (!rc) rc = h->dalloc(scope, &h->lam, kk);
  if (!rc) rc = h->dalloc(scope, &h->elogbeta, kk);
  if (!rc) rc = h->upload(scope, &h->eta, std::vector<double>(eta, eta + kk));
  if (!rc) rc = h->dalloc(scope, &h->carry, (size_t)k + 1);
  if (!rc) rc = h->dalloc(scope, &h->msums, (size_t)SVILS_SBM_MAX_PASSES);
  if (!rc) rc = h->dalloc(scope, &h->cpart, (size_t)h->nb * 2 * k);
  if (!rc) rc = h->dalloc(scope, &h->lpart, (size_t)LINK_WAVES * 3 * k);
  if (!rc) rc = h->dalloc(scope, &h->ctl, (size_t)CTL_COUNT);
  if (!rc) rc = h->dalloc(scope, &h->epart, (size_t)h->epieces);
  if (!rc) rc = h->dalloc(scope, &h->eout, (size_t)2);
  if (!rc) rc = h->upload(scope, &h->gtab, log_table());
  if (!rc && (hipMemsetAsync(h->ctl, 0, CTL_COUNT * sizeof(u64), h->st) != hipSuccess ||
              hipMemsetAsync(h->msums, 0, SVILS_SBM_MAX_PASSES * sizeof(double), h->st) != hipSuccess))
    rc = fail(SVILS_ERR_DEVICE, "svils_sbm_create: memset failed");
  if (!rc && hipStreamSynchronize(h->st) != hipSuccess) rc = fail(SVILS_ERR_DEVICE, "svils_sbm_create: upload failed");
  if (rc) {
    svils_sbm_destroy(h);
    return rc;
  }
  *out = h;
  return 0;
}

int svils_sbm_destroy(svils_sbm *h) {
  delete h;   // ~ToolHandle: waits for the stream, frees both scopes
  return 0;
}

int svils_sbm_set_graph(svils_sbm *h, const uint32_t *links, uint64_t nlinks, const uint32_t *skip, uint64_t nskip) {
  if (int rc = check(h, "svils_sbm_set_graph")) return rc;
  if ((nlinks && !links) || (nskip && !skip)) return fail(SVILS_ERR_ARG, "svils_sbm_set_graph: null argument");
  HostCsr lk, sk;
  if (int rc = build_csr("svils_sbm_set_graph", h->n, links, nlinks, "link", lk)) return rc;
  if (int rc = build_csr("svils_sbm_set_graph", h->n, skip, nskip, "skipped pair", sk)) return rc;
  std::vector<uint8_t> sy(sk.col.size()), py((size_t)nskip);
  for (uint32_t p = 0; p < h->n; ++p)
    for (uint64_t e = sk.row[p]; e < sk.row[p + 1]; ++e) sy[e] = lk.has(p, sk.col[e]) ? 1 : 0;
  uint64_t s1 = 0;
  for (uint64_t x = 0; x < nskip; ++x) s1 += py[x] = lk.has(skip[2 * x], skip[2 * x + 1]) ? 1 : 0;
  HIPCHK(hipStreamSynchronize(h->st));
  free_graph(h);
  const auto scope = ToolHandle::GRAPH;
  int rc = h->upload(scope, &h->lrow, lk.row);
  if (!rc) rc = h->upload(scope, &h->lcol, lk.col);   // an empty list: a null pointer no kernel reads
  if (!rc) rc = h->upload(scope, &h->srow, sk.row);
  if (!rc) rc = h->upload(scope, &h->scol, sk.col);
  if (!rc) rc = h->upload(scope, &h->sy, sy);
  if (!rc) rc = h->upload(scope, &h->py, py);
  if (!rc) rc = h->upload(scope, &h->edges, std::vector<uint32_t>(links, links + 2 * nlinks));
  if (!rc) rc = h->upload(scope, &h->spairs, std::vector<uint32_t>(skip, skip + 2 * nskip));
  if (!rc && hipStreamSynchronize(h->st) != hipSuccess) rc = fail(SVILS_ERR_DEVICE, "svils_sbm_set_graph: upload failed");
  if (rc) {
    free_graph(h);
    return rc;
  }
  h->nlinks = nlinks;
  h->nskip = nskip;
  h->n1 = (double)(nlinks - s1);
  h->n0 = (double)((uint64_t)h->n * (h->n - 1) / 2 - nlinks - (nskip - s1));
  h->have_graph = true;
  h->timed = false;
  return 0;
}

int svils_sbm_set_launch_nodes(svils_sbm *h, uint32_t nodes) {
  if (int rc = check(h, "svils_sbm_set_launch_nodes")) return rc;
  h->launch_nodes = nodes;
  return 0;
}

int svils_sbm_set_plain_chain(svils_sbm *h, int plain) {
  if (int rc = check(h, "svils_sbm_set_plain_chain")) return rc;
  h->plain = plain != 0;
  return 0;
}

int svils_sbm_set_state(svils_sbm *h, const double *phi, const double *gamma, const double *lambda) {
  if (int rc = check(h, "svils_sbm_set_state")) return rc;
  if (!phi || !gamma || !lambda) return fail(SVILS_ERR_ARG, "svils_sbm_set_state: null argument");
  const uint32_t n = h->n, K = h->k;
  for (uint32_t i = 0; i < n; ++i) {
    double s = 0;
    for (uint32_t k = 0; k < K; ++k) {
      const double v = phi[(size_t)i * K + k];
      if (!(v >= 0) || !std::isfinite(v)) return fail(SVILS_ERR_ARG, "svils_sbm_set_state: phi[%u][%u] is negative or not finite", i, k);
      s += v;
    }
    if (!(fabs(s - 1.0) <= 1e-9)) return fail(SVILS_ERR_ARG, "svils_sbm_set_state: row %u of phi does not sum to 1 (%.17g)", i, s);
  }
  for (uint32_t k = 0; k < K; ++k)
    if (!(gamma[k] > 0) || !std::isfinite(gamma[k])) return fail(SVILS_ERR_ARG, "svils_sbm_set_state: gamma[%u] is not > 0", k);
  for (uint32_t x = 0; x < 2 * (K + 1); ++x)
    if (!(lambda[x] > 0) || !std::isfinite(lambda[x])) return fail(SVILS_ERR_ARG, "svils_sbm_set_state: lambda[%u][%u] is not > 0", x / 2, x % 2);
  HIPCHK(hipStreamSynchronize(h->st));
  HIPCHK(hipMemcpy(h->phi, phi, (size_t)n * K * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->gamma, gamma, K * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->lam, lambda, 2 * ((size_t)K + 1) * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_sbm_elog, dim3(1), dim3(256), 0, h->st, K, h->gamma, h->lam, h->gtab, h->elogpi, h->elogbeta);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->st));
  h->have_state = true;
  return 0;
}

int svils_sbm_get_state(svils_sbm *h, double *phi, double *gamma, double *lambda) {
  if (int rc = check(h, "svils_sbm_get_state")) return rc;
  if (!h->have_state) return fail(SVILS_ERR_ARG, "svils_sbm_get_state: no state");
  HIPCHK(hipStreamSynchronize(h->st));
  if (phi) HIPCHK(hipMemcpy(phi, h->phi, (size_t)h->n * h->k * sizeof(double), hipMemcpyDeviceToHost));
  if (gamma) HIPCHK(hipMemcpy(gamma, h->gamma, h->k * sizeof(double), hipMemcpyDeviceToHost));
  if (lambda) HIPCHK(hipMemcpy(lambda, h->lam, 2 * ((size_t)h->k + 1) * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int svils_sbm_estep(svils_sbm *h, uint32_t max_passes, uint32_t *passes, double *msum) {
  if (int rc = ready(h, "svils_sbm_estep")) return rc;
  if (max_passes < 1 || max_passes > SVILS_SBM_MAX_PASSES)
    return fail(SVILS_ERR_ARG, "svils_sbm_estep: max_passes = %u is not in 1 .. %d", max_passes, SVILS_SBM_MAX_PASSES);
  HIPCHK(hipMemsetAsync(h->ctl + CTL_TOTAL, 0, sizeof(u64), h->st));
  HIPCHK(hipEventRecord(h->ev[0], h->st));
  if (int rc = queue_estep(h, max_passes)) return rc;
  HIPCHK(hipEventRecord(h->ev[1], h->st));
  h->timed = true;
  h->timed_m = false;
  uint32_t np = 0;
  double ms[SVILS_SBM_MAX_PASSES];
  if (int rc = svils_sbm_get_stats(h, &np, nullptr, ms)) return rc;
  if (passes) *passes = np;
  if (msum) std::copy(ms, ms + max_passes, msum);
  return 0;
}

int svils_sbm_sweep(svils_sbm *h, uint32_t niter) {
  if (int rc = ready(h, "svils_sbm_sweep")) return rc;
  HIPCHK(hipMemsetAsync(h->ctl + CTL_TOTAL, 0, sizeof(u64), h->st));
  HIPCHK(hipEventRecord(h->ev[0], h->st));
  for (uint32_t it = 0; it < niter; ++it) {
    if (int rc = queue_estep(h, SVILS_SBM_MAX_PASSES)) return rc;
    if (int rc = queue_mstep(h)) return rc;
  }
  HIPCHK(hipEventRecord(h->ev[1], h->st));
  h->timed = h->timed_m = niter > 0;
  return 0;
}

int svils_sbm_pair_loglik(svils_sbm *h, const uint32_t *pairs, const uint8_t *y, uint64_t m, double *out) {
  if (int rc = check(h, "svils_sbm_pair_loglik")) return rc;
  if (!h->have_state) return fail(SVILS_ERR_ARG, "svils_sbm_pair_loglik: no state");
  if (m && (!pairs || !y || !out)) return fail(SVILS_ERR_ARG, "svils_sbm_pair_loglik: null argument");
  for (uint64_t x = 0; x < m; ++x)
    if (pairs[2 * x] == pairs[2 * x + 1] || pairs[2 * x] >= h->n || pairs[2 * x + 1] >= h->n)
      return fail(SVILS_ERR_ARG, "svils_sbm_pair_loglik: pair %llu (%u, %u) is not a pair of two nodes < n = %u", (unsigned long long)x,
                  pairs[2 * x], pairs[2 * x + 1], h->n);
  if (!m) return 0;
  const auto scope = ToolHandle::HANDLE;
  if (int rc = h->reserve(scope, &h->ll_pairs, 2 * (size_t)m)) return rc;
  if (int rc = h->reserve(scope, &h->ll_y, (size_t)m)) return rc;
  if (int rc = h->reserve(scope, &h->ll_out, (size_t)m)) return rc;
  HIPCHK(hipMemcpyAsync(h->ll_pairs, pairs, 2 * m * sizeof(uint32_t), hipMemcpyHostToDevice, h->st));
  HIPCHK(hipMemcpyAsync(h->ll_y, y, m, hipMemcpyHostToDevice, h->st));
  hipLaunchKernelGGL(k_sbm_pair_ll, dim3(blocks(m, 4)), dim3(256), 0, h->st, m, h->k, h->ll_pairs, h->ll_y, h->phi, h->lam, h->ll_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, h->ll_out, m * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  return 0;
}

int svils_sbm_get_stats(svils_sbm *h, uint32_t *passes_last, uint64_t *passes_call, double *msum) {
  if (int rc = check(h, "svils_sbm_get_stats")) return rc;
  u64 c[CTL_COUNT] = {0};
  double ms[SVILS_SBM_MAX_PASSES] = {0};
  HIPCHK(hipMemcpyAsync(c, h->ctl, sizeof c, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipMemcpyAsync(ms, h->msums, sizeof ms, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  if (passes_last) *passes_last = (uint32_t)c[CTL_PASSES];
  if (passes_call) *passes_call = c[CTL_TOTAL];
  if (msum) std::copy(ms, ms + SVILS_SBM_MAX_PASSES, msum);
  return 0;
}

int svils_sbm_get_timing(svils_sbm *h, double ms[3]) {
  if (int rc = check(h, "svils_sbm_get_timing")) return rc;
  if (!ms) return fail(SVILS_ERR_ARG, "svils_sbm_get_timing: null argument");
  HIPCHK(hipStreamSynchronize(h->st));
  ms[0] = h->elapsed_ms(0, 1, h->timed);
  ms[1] = h->launches_ms(EV_PASS, SVILS_SBM_MAX_PASSES, h->timed);
  ms[2] = h->elapsed_ms(EV_MSTEP, EV_MSTEP + 1, h->timed_m);
  return 0;
}

// The bound of the current state.  cpart and lpart are scratch here as in the M-step (every reader rewrites them first); the
// row partials, eout and the two events are this call's own; ctl, msums, carry and the state are only read
int svils_sbmelbo(svils_sbm *h, double out[4]) {
  if (!h) return fail(SVILS_ERR_ARG, "svils_sbmelbo: null handle");
  if (!out) return fail(SVILS_ERR_ARG, "svils_sbmelbo: null argument");
  if (int rc = ready(h, "svils_sbmelbo")) return rc;
  const uint32_t K = h->k, W = row_lanes(K);
  HIPCHK(hipEventRecord(h->ev[EV_ELBO], h->st));
  launch_colsum(h, 0);
  hipLaunchKernelGGL(k_sbm_links, dim3(LINK_WAVES / 4), dim3(256), 0, h->st, K, W, (uint64_t)h->nlinks, (uint64_t)h->nskip, h->edges,
                     h->spairs, h->py, h->phi, h->lpart);
  hipLaunchKernelGGL(k_sbm_elbo_rows, dim3(blocks(h->epieces, 4)), dim3(256), 0, h->st, h->n, K, W, h->eper, h->epieces, h->phi, h->elogpi,
                     h->epart);
  const ElboArgs a{K, h->nb, h->epieces, h->n1, h->n0, h->elogbeta, h->cpart, h->lpart, h->epart, h->eout};
  hipLaunchKernelGGL(k_sbm_elbo_fold, dim3(1), dim3(256), 0, h->st, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev[EV_ELBO + 1], h->st));
  h->timed_e = true;
  const size_t kk = 2 * ((size_t)K + 1);
  std::vector<double> gamma(K), elogpi(K), lam(kk), elogbeta(kk);
  double pn[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(pn, h->eout, sizeof pn, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipMemcpyAsync(gamma.data(), h->gamma, K * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipMemcpyAsync(elogpi.data(), h->elogpi, K * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipMemcpyAsync(lam.data(), h->lam, kk * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipMemcpyAsync(elogbeta.data(), h->elogbeta, kk * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  // G on the host: 4 (K + 1) + 2 K + 2 lnGamma (src/sbm.cc:1144-1164, :1193-1213)
  auto beta_term = [&](const double *p, uint32_t k) {
    return std::lgamma(p[2 * k] + p[2 * k + 1]) - std::lgamma(p[2 * k]) - std::lgamma(p[2 * k + 1]) +
           ((p[2 * k] - 1) * elogbeta[2 * k] + (p[2 * k + 1] - 1) * elogbeta[2 * k + 1]);
  };
  double G = 0.0;
  for (uint32_t k = 0; k <= K; ++k) G += beta_term(h->eta_h.data(), k) - beta_term(lam.data(), k);
  double se = 0.0, sg = 0.0, slg = 0.0, sge = 0.0;
  for (uint32_t k = 0; k < K; ++k) {
    se += elogpi[k];
    sg += gamma[k];
    slg += std::lgamma(gamma[k] < 1e-30 ? 1e-30 : gamma[k]);
    sge += (gamma[k] - 1) * elogpi[k];
  }
  G += std::lgamma(K * h->alpha) - K * std::lgamma(h->alpha) + (h->alpha - 1) * se;
  G -= std::lgamma(sg) - slg;
  G -= sge;
  out[1] = pn[0];
  out[2] = pn[1];
  out[3] = G;
  out[0] = (pn[0] + pn[1]) + G;
  return 0;
}

int svils_sbmelbo_get_timing(svils_sbm *h, double ms[1]) {
  if (!h) return fail(SVILS_ERR_ARG, "svils_sbmelbo_get_timing: null handle");
  if (!ms) return fail(SVILS_ERR_ARG, "svils_sbmelbo_get_timing: null argument");
  if (int rc = check(h, "svils_sbmelbo_get_timing")) return rc;
  HIPCHK(hipStreamSynchronize(h->st));
  ms[0] = h->elapsed_ms(EV_ELBO, EV_ELBO + 1, h->timed_e);
  return 0;
}

}  // extern "C"
