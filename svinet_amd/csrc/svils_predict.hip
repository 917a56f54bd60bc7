// svils_predict.hip -- link prediction from a fitted state: svils_link_prob (scores of given pairs) and svils_predict_links
// (the top-k candidate links of query nodes), svils_rank_links (where a given node stands among them).  The quantity is the reference's LinkSampling::link_prob
// (src/linksampling.hh:240-256): sum_z pi_pz pi_qz beta_z with pi_p = gamma_p / sum gamma_p (estimate_pi, :205-214) and
// beta_z = lambda_z0 / (lambda_z0 + lambda_z1) (estimate_bernoulli_rate, :217-225).
//
//   k_link_prob     one thread per pair, the reference's order of operations (row sums, pi = gamma / sum, sum of products)
//   k_rowinv        1 / sum_k gamma_pk of every node (a sequential sum per thread)
//   k_beta          beta_z
//   k_build_aq      the query rows of a batch: gamma_p / sum gamma_p * beta, zero-padded to a multiple of 16 columns
//   k_sort_rows     once per handle: every CSR row sorted ascending (the upper part of a row is in adjacency order)
//   score_tile      (device function) the one 64 x 64 score tile of the three tile kernels, from v_mfma_f64_16x16x4_f64
//   k_topk_tiles    grid (query tile of 64, candidate chunk): score tiles of the chunk's candidates, then every query's four
//                   selector threads keep a top-k heap each over their quarter of the chunk's candidates
//   k_topk_merge    one block per query: the 4 x chunks heaps sorted together (bitonic, in LDS), the first k kept
//   k_rank_thresh   svils_rank_links, one query row per directed pair (p, q): the score of (p, q) itself, from the tile
//                   whose 64 candidates are the q's of a query tile (the diagonal is kept)
//   k_rank_tiles    the grid and tiles of k_topk_tiles; in place of a heap every selector thread counts the candidates of its
//                   quarter that score above / equal to the row's threshold, and how many it saw (integer atomics per row)
//
// Host side: begin_tile_batch is the start of every batch of the two tile queries (chunks, query rows); the refusals, NONE,
// in_row and the way ranks go back to the caller are svils_pairs.h, shared with svils_nbr.hip.
//
// Read-only: everything here reads gamma, lambda and the CSR, and writes the scratch of svils_handle::pred only.
#include "svils_pairs.h"

namespace {

constexpr uint32_t PQ = 64;               // query rows per tile (four wavefronts of 16)
constexpr uint32_t PC = 64;               // candidates per tile (four 16-column MFMA blocks per wavefront)
constexpr uint32_t Q_BATCH = 8192;        // query nodes per internal batch (bounds the scratch, see include/svils.h)
constexpr uint32_t MERGE_MAX = 4096;      // entries one merge block sorts: 4 selectors x chunks x topk
constexpr uint64_t PAIR_BATCH = 1u << 20; // pairs per internal batch of svils_link_prob

typedef double d4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_link_prob(uint64_t np, uint32_t K, uint32_t ld, const double *__restrict__ gamma,
                                                   const double *__restrict__ lambda, const uint32_t *__restrict__ pairs,
                                                   double *__restrict__ prob) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  const double *gp = gamma + (size_t)pairs[2 * i] * ld, *gq = gamma + (size_t)pairs[2 * i + 1] * ld;
  double sp = .0, sq = .0;
  for (uint32_t k = 0; k < K; ++k) sp += gp[k];
  for (uint32_t k = 0; k < K; ++k) sq += gq[k];
  double s = .0;
  for (uint32_t z = 0; z < K; ++z) {
    const double u = lambda[2 * z] / (.0 + lambda[2 * z] + lambda[2 * z + 1]);
    s += (gp[z] / sp) * (gq[z] / sq) * u;
  }
  prob[i] = s;
}

__global__ __launch_bounds__(256) void k_rowinv(uint32_t n, uint32_t K, uint32_t ld, const double *__restrict__ gamma,
                                                double *__restrict__ inv) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const double *g = gamma + (size_t)p * ld;
  double s = .0;
  for (uint32_t k = 0; k < K; ++k) s += g[k];
  inv[p] = 1.0 / s;
}

__global__ __launch_bounds__(256) void k_beta(uint32_t K, const double *__restrict__ lambda, double *__restrict__ beta) {
  const uint32_t z = blockIdx.x * 256 + threadIdx.x;
  if (z < K) beta[z] = lambda[2 * z] / (.0 + lambda[2 * z] + lambda[2 * z + 1]);
}

// aq[i][k] for i < rows (a multiple of PQ), k < k16: rows past the batch (qnodes[i] == NONE) and columns past K are zero
__global__ __launch_bounds__(256) void k_build_aq(uint32_t rows, uint32_t K, uint32_t ld, uint32_t k16, const double *__restrict__ gamma,
                                                  const double *__restrict__ inv, const double *__restrict__ beta,
                                                  const uint32_t *__restrict__ qnodes, double *__restrict__ aq) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (uint64_t)rows * k16) return;
  const uint32_t i = (uint32_t)(e / k16), k = (uint32_t)(e % k16), p = qnodes[i];
  aq[e] = (p != NONE && k < K) ? gamma[(size_t)p * ld + k] * inv[p] * beta[k] : 0.0;
}

// one wavefront per row: every entry's rank in its row (ties by position, so a repeated neighbour keeps both slots)
__global__ __launch_bounds__(256) void k_sort_rows(uint32_t n, const uint64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                   uint32_t *__restrict__ scol) {
  const uint32_t x = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (x >= n) return;
  const uint64_t b = rowptr[x];
  const uint32_t d = (uint32_t)(rowptr[x + 1] - b);
  for (uint32_t i = lane; i < d; i += 64) {
    const uint32_t v = col[b + i];
    uint32_t r = 0;
    for (uint32_t j = 0; j < d; ++j) {
      const uint32_t u = col[b + j];
      r += (u < v || (u == v && j < i)) ? 1u : 0u;
    }
    scol[b + r] = v;
  }
}

// (as, ai) ranks below (bs, bi): lower score, or the same score and the higher id
__device__ inline bool worse(double as, uint32_t ai, double bs, uint32_t bi) { return as < bs || (as == bs && ai > bi); }

// row[col .. col + 3], zero at and past column K (row + col is 16-byte aligned: ld is even, col a multiple of 4)
__device__ inline void load4(const double *__restrict__ row, uint32_t col, uint32_t K, double *o) {
  if (col + 3 < K) {
    const double2 x = *(const double2 *)(row + col), y = *(const double2 *)(row + col + 2);
    o[0] = x.x; o[1] = x.y; o[2] = y.x; o[3] = y.y;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = col + e < K ? row[col + e] : 0.0;
  }
}

// The 64 x 64 score tile of the three tile kernels: 64 query rows (arow: this lane's row 16 w + (l & 15) of aq) against four
// candidate columns per lane -- cand[j] is the node behind column 16 j + (l & 15), NONE for a column past the end (its scores
// are zero).  Wavefront w computes the 16 x 64 scores of query rows 16 w .. 16 w + 15 as four 16 x 16 MFMA blocks, K in steps
// of 4.  Operand map of v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k-slot l >> 4] and B[k-slot l >> 4][col l & 15];
// the k column behind k-slot g in step s of a 16-column chunk is kc + 4 g + s (both operands use the same map, so every
// lane reads four consecutive doubles of its row per chunk).  C/D: register r of lane l is row (l >> 4) + 4 r, col l & 15.
// An element depends on its row of aq, its candidate and the k order only: (row, candidate) has the same bits wherever it
// sits in a tile and whichever kernel asks -- what svils_rank_links' "bitwise the score of svils_predict_links" rests on.
__device__ __forceinline__ void score_tile(double (*S)[PC + 1], const double *__restrict__ arow, const uint32_t *cand, uint32_t K,
                                           uint32_t ld, uint32_t k16, const double *__restrict__ gamma,
                                           const double *__restrict__ inv, uint32_t w, uint32_t g, uint32_t r16) {
  d4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
  for (uint32_t kc = 0; kc < k16; kc += 16) {
    const uint32_t col = kc + 4 * g;
    const double2 a01 = *(const double2 *)(arow + col), a23 = *(const double2 *)(arow + col + 2);
    const double a[4] = {a01.x, a01.y, a23.x, a23.y};
    double b[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (cand[j] != NONE) load4(gamma + (size_t)cand[j] * ld, col, K, b[j]);
      else b[j][0] = b[j][1] = b[j][2] = b[j][3] = 0.0;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[j][s], acc[j], 0, 0, 0);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double iq = cand[j] != NONE ? inv[cand[j]] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) S[16 * w + g + 4 * r][16 * j + r16] = acc[j][r] * iq;
  }
}

// Block (qt, c): query rows [64 qt, 64 qt + 64) of the batch against the candidates of chunk c of nch, a score_tile of 64
// candidates at a time.  Selection: thread t serves query row t >> 2 over the candidates t & 3, t & 3 + 4, ... of every tile
// (ascending ids) with a k-entry heap of its own in global scratch (slot i at stride 256: the block's heaps interleave),
// worst entry on top; a candidate is looked at further only if it beats that entry.  (Heaps in LDS for k <= 10 measured no
// faster: profiles/r09a_predict.md.)
__global__ __launch_bounds__(256) void k_topk_tiles(uint32_t n, uint32_t K, uint32_t ld, uint32_t k16, uint32_t topk, uint32_t nch,
                                                    const double *__restrict__ gamma, const double *__restrict__ inv,
                                                    const double *__restrict__ aq, const uint32_t *__restrict__ qnodes,
                                                    const uint64_t *__restrict__ rowptr, const uint32_t *__restrict__ scol,
                                                    double *__restrict__ hs, uint32_t *__restrict__ hi) {
  __shared__ double S[PQ][PC + 1];
  const uint32_t t = threadIdx.x, w = t >> 6, l = t & 63, g = l >> 4, r16 = l & 15;
  const uint32_t qt = blockIdx.x, c = blockIdx.y;
  uint32_t cb, ce;
  chunk_range(n, c, nch, &cb, &ce);
  const uint32_t qi = t >> 2, sub = t & 3;
  const uint32_t p = qnodes[qt * PQ + qi];
  uint64_t nb = 0, ne = 0;
  if (p != NONE) { nb = rowptr[p]; ne = rowptr[p + 1]; }
  const size_t hbase = ((size_t)qt * nch + c) * topk * 256 + t;
  double *hsc = hs + hbase;
  uint32_t *hid = hi + hbase;
  for (uint32_t i = 0; i < topk; ++i) { hsc[(size_t)i * 256] = -1.0; hid[(size_t)i * 256] = NONE; }
  double worst = -1.0;
  const double *arow = aq + (size_t)(qt * PQ + 16 * w + r16) * k16;
  for (uint32_t c0 = cb; c0 < ce; c0 += PC) {
    uint32_t cand[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cand[j] = c0 + 16 * j + r16 < ce ? c0 + 16 * j + r16 : NONE;
    score_tile(S, arow, cand, K, ld, k16, gamma, inv, w, g, r16);
    __syncthreads();
    if (p != NONE) {
      for (uint32_t i = 0; i < PC / 4; ++i) {
        const uint32_t cc = sub + 4 * i, q = c0 + cc;
        if (q >= ce) break;
        const double s = S[qi][cc];
        if (!(s > worst)) continue;
        if (q == p || in_row(scol, nb, ne, q)) continue;
        uint32_t pos = 0;
        for (;;) {
          uint32_t ch = 2 * pos + 1;
          if (ch >= topk) break;
          double cs = hsc[(size_t)ch * 256];
          uint32_t ci = hid[(size_t)ch * 256];
          if (ch + 1 < topk) {
            const double ds = hsc[(size_t)(ch + 1) * 256];
            const uint32_t di = hid[(size_t)(ch + 1) * 256];
            if (worse(ds, di, cs, ci)) { ++ch; cs = ds; ci = di; }
          }
          if (!worse(cs, ci, s, q)) break;
          hsc[(size_t)pos * 256] = cs;
          hid[(size_t)pos * 256] = ci;
          pos = ch;
        }
        hsc[(size_t)pos * 256] = s;
        hid[(size_t)pos * 256] = q;
        worst = hsc[0];
      }
    }
    __syncthreads();
  }
}

// query row i of the batch: its 4 x nch heaps (L entries, padded to lp = a power of two <= MERGE_MAX with the empty entry
// (-1, NONE)) sorted best first -- score descending, id ascending -- and the first topk written out
__global__ __launch_bounds__(256) void k_topk_merge(uint32_t topk, uint32_t nch, uint32_t lp, const double *__restrict__ hs,
                                                    const uint32_t *__restrict__ hi, double *__restrict__ oscore,
                                                    uint32_t *__restrict__ oid) {
  __shared__ double ks[MERGE_MAX];
  __shared__ uint32_t ki[MERGE_MAX];
  const uint32_t i = blockIdx.x, qt = i / PQ, qi = i % PQ;
  const uint32_t L = 4 * nch * topk;
  for (uint32_t e = threadIdx.x; e < lp; e += 256) {
    double s = -1.0;
    uint32_t id = NONE;
    if (e < L) {
      const uint32_t c = e / (4 * topk), rem = e % (4 * topk), sub = rem / topk, slot = rem % topk;
      const size_t idx = (((size_t)qt * nch + c) * topk + slot) * 256 + qi * 4 + sub;
      s = hs[idx];
      id = hi[idx];
    }
    ks[e] = s;
    ki[e] = id;
  }
  __syncthreads();
  for (uint32_t size = 2; size <= lp; size <<= 1)
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t x = threadIdx.x; x < lp / 2; x += 256) {
        const uint32_t a = 2 * x - (x & (stride - 1)), b = a + stride;
        const bool up = (a & size) == 0;   // this run ends best first
        const bool b_better = worse(ks[a], ki[a], ks[b], ki[b]);
        if (b_better == up) {
          const double ts = ks[a]; ks[a] = ks[b]; ks[b] = ts;
          const uint32_t ti = ki[a]; ki[a] = ki[b]; ki[b] = ti;
        }
      }
      __syncthreads();
    }
  for (uint32_t j = threadIdx.x; j < topk; j += 256) {
    oscore[(size_t)i * topk + j] = ks[j];
    oid[(size_t)i * topk + j] = ki[j];
  }
}

// Block qt: thr[i] = the score of (qnodes[i], qcand[i]) for the 64 rows i of query tile qt -- the diagonal of the tile whose
// candidate columns are the rows' own q's.
__global__ __launch_bounds__(256) void k_rank_thresh(uint32_t K, uint32_t ld, uint32_t k16, const double *__restrict__ gamma,
                                                     const double *__restrict__ inv, const double *__restrict__ aq,
                                                     const uint32_t *__restrict__ qcand, double *__restrict__ thr) {
  __shared__ double S[PQ][PC + 1];
  const uint32_t t = threadIdx.x, w = t >> 6, l = t & 63, g = l >> 4, r16 = l & 15, qt = blockIdx.x;
  uint32_t cand[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) cand[j] = qcand[qt * PQ + 16 * j + r16];
  score_tile(S, aq + (size_t)(qt * PQ + 16 * w + r16) * k16, cand, K, ld, k16, gamma, inv, w, g, r16);
  __syncthreads();
  if (t < PQ) thr[qt * PQ + t] = S[t][t];
}

// Block (qt, c) as in k_topk_tiles.  Thread t serves row t >> 2 over the candidates t & 3, t & 3 + 4, ... of every tile in
// ascending order; `np` walks the row's sorted training neighbours along with them (nv = the neighbour it stands on, NONE
// past the end), so p's neighbours, p and q are passed over without a search.  cnt[row][3] += above, tied, seen: the four
// threads of a row are summed by shuffles, the chunks by integer atomics (exact in any order).
__global__ __launch_bounds__(256) void k_rank_tiles(uint32_t n, uint32_t K, uint32_t ld, uint32_t k16, uint32_t nch,
                                                    const double *__restrict__ gamma, const double *__restrict__ inv,
                                                    const double *__restrict__ aq, const uint32_t *__restrict__ qnodes,
                                                    const uint32_t *__restrict__ qcand, const double *__restrict__ thr,
                                                    const uint64_t *__restrict__ rowptr, const uint32_t *__restrict__ scol,
                                                    uint32_t *__restrict__ cnt) {
  __shared__ double S[PQ][PC + 1];
  const uint32_t t = threadIdx.x, w = t >> 6, l = t & 63, g = l >> 4, r16 = l & 15;
  const uint32_t qt = blockIdx.x, c = blockIdx.y;
  uint32_t cb, ce;
  chunk_range(n, c, nch, &cb, &ce);
  const uint32_t qi = t >> 2, sub = t & 3, row = qt * PQ + qi;
  const uint32_t p = qnodes[row];
  uint32_t q = NONE, nv = NONE;
  uint64_t np = 0, ne = 0;
  double s = 0.0;
  if (p != NONE) {
    q = qcand[row];
    s = thr[row];
    uint64_t b = rowptr[p];
    ne = rowptr[p + 1];
    for (uint64_t e = ne; b < e;) {   // the first neighbour >= cb
      const uint64_t m = (b + e) >> 1;
      if (scol[m] < cb) b = m + 1; else e = m;
    }
    np = b;
    if (np < ne) nv = scol[np];
  }
  uint32_t above = 0, tied = 0, seen = 0;
  const double *arow = aq + (size_t)(qt * PQ + 16 * w + r16) * k16;
  for (uint32_t c0 = cb; c0 < ce; c0 += PC) {
    uint32_t cand[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cand[j] = c0 + 16 * j + r16 < ce ? c0 + 16 * j + r16 : NONE;
    score_tile(S, arow, cand, K, ld, k16, gamma, inv, w, g, r16);
    __syncthreads();
    if (p != NONE) {
      for (uint32_t i = 0; i < PC / 4; ++i) {
        const uint32_t cc = sub + 4 * i, x = c0 + cc;
        if (x >= ce) break;
        while (nv < x) nv = ++np < ne ? scol[np] : NONE;
        if (x == p || x == q || x == nv) continue;
        const double sc = S[qi][cc];
        above += sc > s ? 1u : 0u;
        tied += sc == s ? 1u : 0u;
        ++seen;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int m = 1; m <= 2; m <<= 1) {
    above += __shfl_xor(above, m);
    tied += __shfl_xor(tied, m);
    seen += __shfl_xor(seen, m);
  }
  if (p != NONE && sub == 0) {
    atomicAdd(cnt + 3 * (size_t)row, above);
    atomicAdd(cnt + 3 * (size_t)row + 1, tied);
    atomicAdd(cnt + 3 * (size_t)row + 2, seen);
  }
}

}  // namespace

// the sorted copy of the CSR (svils_handle::PredictScratch::scol), built on the handle's stream the first time it is asked for
int svils_impl::sorted_rows(svils_handle *h) {
  svils_handle::PredictScratch &s = h->pred;
  if (s.scol) return 0;
  if (int rc = dalloc(h, &s.scol, 2 * h->d.nlinks, false)) return rc;
  hipLaunchKernelGGL(k_sort_rows, dim3((h->geo.n + 3) / 4), dim3(256), 0, h->stream, h->geo.n, h->d.rowptr, h->d.col, s.scol);
  HIPCHK(hipGetLastError());
  return 0;
}

namespace {

// what every top-k or rank call needs besides its batches: the sorted rows (once), 1 / row sums and beta of the current state
int prepare(svils_handle *h) {
  const Geometry &g = h->geo;
  const DeviceState &d = h->d;
  svils_handle::PredictScratch &s = h->pred;
  if (int rc = sorted_rows(h)) return rc;
  if (!s.inv) {
    if (int rc = dalloc(h, &s.inv, g.n, false)) return rc;
    if (int rc = dalloc(h, &s.beta, g.K, false)) return rc;
  }
  hipLaunchKernelGGL(k_rowinv, dim3((g.n + 255) / 256), dim3(256), 0, h->stream, g.n, g.K, g.ld, d.gamma, s.inv);
  hipLaunchKernelGGL(k_beta, dim3((g.K + 255) / 256), dim3(256), 0, h->stream, g.K, d.lambda, s.beta);
  HIPCHK(hipGetLastError());
  return 0;
}

// The start of a batch for the tile kernels.  qh holds the batch's m query nodes and is padded here with NONE to rows = a
// multiple of PQ; the device gets them (pred.qnodes) and their rows of aq (k_build_aq).  nch = the candidate chunks of the
// grid: enough blocks for eight per CU, at most nch_max (the caller's own bound, if it has one) and at least 64 candidates
// per chunk.  No result depends on the cut: a top k is that of one total order, counts are sums over the chunks.
struct TileBatch {
  uint32_t nqt, rows, nch, k16;
};
int begin_tile_batch(svils_handle *h, std::vector<uint32_t> &qh, uint32_t nch_max, TileBatch *tb) {
  const Geometry &g = h->geo;
  svils_handle::PredictScratch &s = h->pred;
  tb->nqt = ((uint32_t)qh.size() + PQ - 1) / PQ;
  tb->rows = tb->nqt * PQ;
  tb->k16 = (g.K + 15u) & ~15u;
  tb->nch = std::max<uint32_t>(1, (8u * cu_count(h->cfg.device) + tb->nqt - 1) / tb->nqt);
  tb->nch = std::min(tb->nch, nch_max);
  tb->nch = std::min(tb->nch, std::max<uint32_t>(1, g.n / PC));
  const uint64_t ae = (uint64_t)tb->rows * tb->k16;
  if (int rc = reserve(h, s.qnodes, tb->rows)) return rc;
  if (int rc = reserve(h, s.aq, ae)) return rc;
  qh.resize(tb->rows, NONE);
  HIPCHK(hipMemcpyAsync(s.qnodes.p, qh.data(), tb->rows * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_build_aq, dim3((uint32_t)((ae + 255) / 256)), dim3(256), 0, h->stream, tb->rows, g.K, g.ld, tb->k16,
                     h->d.gamma, s.inv, s.beta, s.qnodes.p, s.aq.p);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int svils_link_prob(svils_handle *h, const uint32_t *pairs, uint64_t npairs, double *prob) {
  if (int rc = check_pair_handle(h, "svils_link_prob", true)) return rc;
  if (npairs && (!pairs || !prob)) return fail(SVILS_ERR_ARG, "svils_link_prob: null argument");
  if (int rc = check_pairs(h, "svils_link_prob", pairs, npairs)) return rc;
  if (!npairs) return 0;
  HIPCHK(hipSetDevice(h->cfg.device));
  const Geometry &g = h->geo;
  svils_handle::PredictScratch &s = h->pred;
  const uint64_t cap = std::min<uint64_t>(npairs, PAIR_BATCH);
  if (int rc = reserve(h, s.pairs, 2 * cap)) return rc;
  if (int rc = reserve(h, s.prob, cap)) return rc;
  for (uint64_t b = 0; b < npairs; b += PAIR_BATCH) {
    const uint64_t m = std::min<uint64_t>(PAIR_BATCH, npairs - b);
    HIPCHK(hipMemcpyAsync(s.pairs.p, pairs + 2 * b, 2 * m * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_link_prob, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, h->stream, m, g.K, g.ld, h->d.gamma,
                       h->d.lambda, s.pairs.p, s.prob.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(prob + b, s.prob.p, m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

int svils_predict_links(svils_handle *h, const uint32_t *nodes, uint32_t nnodes, uint32_t topk, uint32_t *ids, double *scores) {
  if (int rc = check_pair_handle(h, "svils_predict_links", true)) return rc;
  const Geometry &g = h->geo;
  if (topk == 0 || topk > SVILS_PREDICT_MAX_TOPK)
    return fail(SVILS_ERR_ARG, "svils_predict_links: topk = %u, need 1 .. %d", topk, SVILS_PREDICT_MAX_TOPK);
  if (!nodes && nnodes != 0 && nnodes != g.n)
    return fail(SVILS_ERR_ARG, "svils_predict_links: nodes = NULL means all %u nodes (nnodes = 0 or n, not %u)", g.n, nnodes);
  const uint32_t nq = nodes ? nnodes : g.n;
  if (nq && (!ids || !scores)) return fail(SVILS_ERR_ARG, "svils_predict_links: null argument");
  if (nodes)
    for (uint32_t i = 0; i < nq; ++i)
      if (nodes[i] >= g.n) return fail(SVILS_ERR_ARG, "svils_predict_links: node %u (entry %u) >= n = %u", nodes[i], i, g.n);
  if (!nq) return 0;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (int rc = prepare(h)) return rc;
  svils_handle::PredictScratch &s = h->pred;
  std::vector<uint32_t> qh;
  for (uint32_t b = 0; b < nq; b += Q_BATCH) {
    const uint32_t m = std::min(Q_BATCH, nq - b);
    qh.resize(m);
    for (uint32_t i = 0; i < m; ++i) qh[i] = nodes ? nodes[b + i] : b + i;
    TileBatch tb;   // at most MERGE_MAX / (4 topk) chunks: the merge sorts the 4 x nch x topk heap entries of a query in LDS
    if (int rc = begin_tile_batch(h, qh, std::max<uint32_t>(1, MERGE_MAX / (4 * topk)), &tb)) return rc;
    uint32_t L = 4 * tb.nch * topk, lp = 1;
    while (lp < L) lp <<= 1;
    const uint64_t oneed = (uint64_t)Q_BATCH * topk, hneed = (uint64_t)tb.nqt * tb.nch * topk * 256;
    if (int rc = reserve(h, s.ids, oneed)) return rc;
    if (int rc = reserve(h, s.scores, oneed)) return rc;
    if (int rc = reserve(h, s.hs, hneed)) return rc;
    if (int rc = reserve(h, s.hi, hneed)) return rc;
    hipLaunchKernelGGL(k_topk_tiles, dim3(tb.nqt, tb.nch), dim3(256), 0, h->stream, g.n, g.K, g.ld, tb.k16, topk, tb.nch,
                       h->d.gamma, s.inv, s.aq.p, s.qnodes.p, h->d.rowptr, s.scol, s.hs.p, s.hi.p);
    hipLaunchKernelGGL(k_topk_merge, dim3(m), dim3(256), 0, h->stream, topk, tb.nch, lp, s.hs.p, s.hi.p, s.scores.p, s.ids.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ids + (size_t)b * topk, s.ids.p, (size_t)m * topk * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(scores + (size_t)b * topk, s.scores.p, (size_t)m * topk * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

int svils_rank_links(svils_handle *h, const uint32_t *pairs, uint64_t npairs, uint32_t *above, uint32_t *tied, uint32_t *ncand,
                     double *score) {
  if (int rc = check_pair_handle(h, "svils_rank_links", true)) return rc;
  if (int rc = check_pairs(h, "svils_rank_links", pairs, npairs)) return rc;
  if (!npairs) return 0;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (int rc = prepare(h)) return rc;
  const Geometry &g = h->geo;
  svils_handle::PredictScratch &s = h->pred;
  std::vector<uint32_t> ph, qh;
  for (uint64_t b = 0; b < npairs; b += Q_BATCH) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(Q_BATCH, npairs - b);
    ph.resize(m);
    for (uint32_t i = 0; i < m; ++i) ph[i] = pairs[2 * (b + i)];
    TileBatch tb;   // no bound on the chunks: nothing is merged
    if (int rc = begin_tile_batch(h, ph, UINT32_MAX, &tb)) return rc;
    if (int rc = reserve(h, s.rq, tb.rows)) return rc;
    if (int rc = reserve(h, s.rthr, tb.rows)) return rc;
    if (int rc = reserve(h, s.rcnt, 3 * (uint64_t)tb.rows)) return rc;
    qh.assign(tb.rows, NONE);
    for (uint32_t i = 0; i < m; ++i) qh[i] = pairs[2 * (b + i) + 1];
    HIPCHK(hipMemcpyAsync(s.rq.p, qh.data(), tb.rows * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(s.rcnt.p, 0, 3 * (size_t)tb.rows * sizeof(uint32_t), h->stream));
    hipLaunchKernelGGL(k_rank_thresh, dim3(tb.nqt), dim3(256), 0, h->stream, g.K, g.ld, tb.k16, h->d.gamma, s.inv, s.aq.p, s.rq.p,
                       s.rthr.p);
    hipLaunchKernelGGL(k_rank_tiles, dim3(tb.nqt, tb.nch), dim3(256), 0, h->stream, g.n, g.K, g.ld, tb.k16, tb.nch, h->d.gamma,
                       s.inv, s.aq.p, s.qnodes.p, s.rq.p, s.rthr.p, h->d.rowptr, s.scol, s.rcnt.p);
    HIPCHK(hipGetLastError());
    if (int rc = fetch_ranks(h, s.rcnt.p, s.rthr.p, m, b, above, tied, ncand, score)) return rc;
  }
  return 0;
}

}  // extern "C"
