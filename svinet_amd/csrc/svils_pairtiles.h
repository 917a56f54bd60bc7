// svils_pairtiles.h -- the tile kernels of the top-k and rank queries, shared by the two model families that answer them:
// svils_predict.hip (svils_handle: svils_predict_links, svils_rank_links) and svils_orig_predict.hip (svils_orig:
// svils_orig_link_prob, svils_orig_predict_links, svils_orig_rank_links).  A family supplies two operands -- aq [rows][k16],
// the query rows, and a candidate matrix with one row per node -- and a candidate policy X, a small struct passed by value
// that says which nodes are NOT candidates of a query node (its training neighbours):
//
//   X::SCALED                     the candidate operand is gamma and a score is scaled by inv[candidate] (CsrRows), or
//                                 it is already normalised and nothing is scaled (BitRows, the bit matrix of svils_orig)
//   X::Row,  open(r, p), has(r, q)            membership test of k_topk_tiles: asked only of candidates that beat the heap
//   X::Walk, open(w, p, cb), advance(w, x), at(w, x)   membership test of k_rank_tiles: every candidate x, ascending from
//                                 cb, is announced with advance() and may then be asked about with at()
//
//   score_tile      (device function) the one 64 x 64 score tile of the three tile kernels, from v_mfma_f64_16x16x4_f64
//   k_topk_tiles    grid (query tile of 64, candidate chunk): score tiles of the chunk's candidates, then every query's four
//                   selector threads keep a top-k heap each over their quarter of the chunk's candidates
//   k_topk_merge    one block per query: the 4 x chunks heaps sorted together (bitonic, in LDS), the first k kept
//   k_rank_thresh   one query row per directed pair (p, q): the score of (p, q) itself, from the tile whose 64 candidates
//                   are the q's of a query tile (the diagonal is kept)
//   k_rank_tiles    the grid and tiles of k_topk_tiles; in place of a heap every selector thread counts the candidates of its
//                   quarter that score above / equal to the row's threshold, and how many it saw (integer atomics per row)
//
// Host side: plan_tile_batch is the geometry of every batch of the two tile queries (query rows, candidate chunks);
// launch_topk / launch_ranks enqueue the kernels of a batch.
#pragma once
#include "svils_pairs.h"

namespace svils_impl {

constexpr uint32_t PQ = 64;               // query rows per tile (four wavefronts of 16)
constexpr uint32_t PC = 64;               // candidates per tile (four 16-column MFMA blocks per wavefront)
constexpr uint32_t Q_BATCH = 8192;        // query nodes per internal batch (bounds the scratch, see include/svils.h)
constexpr uint32_t MERGE_MAX = 4096;      // entries one merge block sorts: 4 selectors x chunks x topk

typedef double tile_d4 __attribute__((ext_vector_type(4)));

// svils_handle: the training neighbours of p are row p of the CSR copy with sorted rows (svils_impl::sorted_rows)
struct CsrRows {
  static constexpr bool SCALED = true;
  const uint64_t *rowptr;
  const uint32_t *scol;
  struct Row {
    uint64_t nb = 0, ne = 0;
  };
  __device__ __forceinline__ void open(Row &r, uint32_t p) const {
    r.nb = rowptr[p];
    r.ne = rowptr[p + 1];
  }
  __device__ __forceinline__ bool has(const Row &r, uint32_t q) const { return in_row(scol, r.nb, r.ne, q); }
  // np walks the row along with the candidates (nv = the neighbour it stands on, NONE past the end), so p's neighbours are
  // passed over without a search
  struct Walk {
    uint64_t np = 0, ne = 0;
    uint32_t nv = NONE;
  };
  __device__ __forceinline__ void open(Walk &w, uint32_t p, uint32_t cb) const {
    uint64_t b = rowptr[p];
    w.ne = rowptr[p + 1];
    for (uint64_t e = w.ne; b < e;) {   // the first neighbour >= cb
      const uint64_t m = (b + e) >> 1;
      if (scol[m] < cb) b = m + 1; else e = m;
    }
    w.np = b;
    if (w.np < w.ne) w.nv = scol[w.np];
  }
  __device__ __forceinline__ void advance(Walk &w, uint32_t x) const {
    while (w.nv < x) w.nv = ++w.np < w.ne ? scol[w.np] : NONE;
  }
  __device__ __forceinline__ bool at(const Walk &w, uint32_t x) const { return x == w.nv; }
};

// svils_orig (and whichever family keeps its graph as bit matrices): bit c of row p of excl [n][nw] is set where c is a
// training neighbour of p.  Both tests are one word read; the walk has nothing to remember
struct BitRows {
  static constexpr bool SCALED = false;
  const uint32_t *excl;
  uint32_t nw;
  struct Row {
    const uint32_t *bits = nullptr;
  };
  typedef Row Walk;
  __device__ __forceinline__ void open(Row &r, uint32_t p) const { r.bits = excl + (size_t)p * nw; }
  __device__ __forceinline__ void open(Row &r, uint32_t p, uint32_t) const { open(r, p); }
  __device__ __forceinline__ bool has(const Row &r, uint32_t q) const { return (r.bits[q >> 5] >> (q & 31)) & 1u; }
  __device__ __forceinline__ void advance(Row &, uint32_t) const {}
  __device__ __forceinline__ bool at(const Row &r, uint32_t x) const { return has(r, x); }
};

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
// sits in a tile and whichever kernel asks -- what "bitwise the score of the top-k list" rests on in both families.
// SCALED: the score is the product times inv[candidate]; otherwise inv is not read.
template <bool SCALED>
__device__ __forceinline__ void score_tile(double (*S)[PC + 1], const double *__restrict__ arow, const uint32_t *cand, uint32_t K,
                                           uint32_t ld, uint32_t k16, const double *__restrict__ gamma,
                                           const double *__restrict__ inv, uint32_t w, uint32_t g, uint32_t r16) {
  tile_d4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = tile_d4{0.0, 0.0, 0.0, 0.0};
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
    if (SCALED) {
      const double iq = cand[j] != NONE ? inv[cand[j]] : 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) S[16 * w + g + 4 * r][16 * j + r16] = acc[j][r] * iq;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) S[16 * w + g + 4 * r][16 * j + r16] = acc[j][r];
    }
  }
}

// Block (qt, c): query rows [64 qt, 64 qt + 64) of the batch against the candidates of chunk c of nch, a score_tile of 64
// candidates at a time.  Selection: thread t serves query row t >> 2 over the candidates t & 3, t & 3 + 4, ... of every tile
// (ascending ids) with a k-entry heap of its own in global scratch (slot i at stride 256: the block's heaps interleave),
// worst entry on top; a candidate is looked at further only if it beats that entry.  (Heaps in LDS for k <= 10 measured no
// faster: profiles/r09a_predict.md.)
template <class X>
__global__ __launch_bounds__(256) void k_topk_tiles(uint32_t n, uint32_t K, uint32_t ld, uint32_t k16, uint32_t topk, uint32_t nch,
                                                    const double *__restrict__ gamma, const double *__restrict__ inv,
                                                    const double *__restrict__ aq, const uint32_t *__restrict__ qnodes,
                                                    const X x, double *__restrict__ hs, uint32_t *__restrict__ hi) {
  __shared__ double S[PQ][PC + 1];
  const uint32_t t = threadIdx.x, w = t >> 6, l = t & 63, g = l >> 4, r16 = l & 15;
  const uint32_t qt = blockIdx.x, c = blockIdx.y;
  uint32_t cb, ce;
  chunk_range(n, c, nch, &cb, &ce);
  const uint32_t qi = t >> 2, sub = t & 3;
  const uint32_t p = qnodes[qt * PQ + qi];
  typename X::Row row;
  if (p != NONE) x.open(row, p);
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
    score_tile<X::SCALED>(S, arow, cand, K, ld, k16, gamma, inv, w, g, r16);
    __syncthreads();
    if (p != NONE) {
      for (uint32_t i = 0; i < PC / 4; ++i) {
        const uint32_t cc = sub + 4 * i, q = c0 + cc;
        if (q >= ce) break;
        const double s = S[qi][cc];
        if (!(s > worst)) continue;
        if (q == p || x.has(row, q)) continue;
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
// (-1, NONE)) sorted best first -- score descending, id ascending -- and the first topk written out.  CAP: the entries the
// block has room for (MERGE_MAX)
template <uint32_t CAP>
__global__ __launch_bounds__(256) void k_topk_merge(uint32_t topk, uint32_t nch, uint32_t lp, const double *__restrict__ hs,
                                                    const uint32_t *__restrict__ hi, double *__restrict__ oscore,
                                                    uint32_t *__restrict__ oid) {
  __shared__ double ks[CAP];
  __shared__ uint32_t ki[CAP];
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
template <bool SCALED>
__global__ __launch_bounds__(256) void k_rank_thresh(uint32_t K, uint32_t ld, uint32_t k16, const double *__restrict__ gamma,
                                                     const double *__restrict__ inv, const double *__restrict__ aq,
                                                     const uint32_t *__restrict__ qcand, double *__restrict__ thr) {
  __shared__ double S[PQ][PC + 1];
  const uint32_t t = threadIdx.x, w = t >> 6, l = t & 63, g = l >> 4, r16 = l & 15, qt = blockIdx.x;
  uint32_t cand[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) cand[j] = qcand[qt * PQ + 16 * j + r16];
  score_tile<SCALED>(S, aq + (size_t)(qt * PQ + 16 * w + r16) * k16, cand, K, ld, k16, gamma, inv, w, g, r16);
  __syncthreads();
  if (t < PQ) thr[qt * PQ + t] = S[t][t];
}

// Block (qt, c) as in k_topk_tiles.  Thread t serves row t >> 2 over the candidates t & 3, t & 3 + 4, ... of every tile in
// ascending order, which is the order X::advance is called in; p, q and p's training neighbours are passed over.
// cnt[row][3] += above, tied, seen: the four threads of a row are summed by shuffles, the chunks by integer atomics (exact
// in any order).
template <class X>
__global__ __launch_bounds__(256) void k_rank_tiles(uint32_t n, uint32_t K, uint32_t ld, uint32_t k16, uint32_t nch,
                                                    const double *__restrict__ gamma, const double *__restrict__ inv,
                                                    const double *__restrict__ aq, const uint32_t *__restrict__ qnodes,
                                                    const uint32_t *__restrict__ qcand, const double *__restrict__ thr,
                                                    const X x, uint32_t *__restrict__ cnt) {
  __shared__ double S[PQ][PC + 1];
  const uint32_t t = threadIdx.x, w = t >> 6, l = t & 63, g = l >> 4, r16 = l & 15;
  const uint32_t qt = blockIdx.x, c = blockIdx.y;
  uint32_t cb, ce;
  chunk_range(n, c, nch, &cb, &ce);
  const uint32_t qi = t >> 2, sub = t & 3, row = qt * PQ + qi;
  const uint32_t p = qnodes[row];
  uint32_t q = NONE;
  typename X::Walk walk;
  double s = 0.0;
  if (p != NONE) {
    q = qcand[row];
    s = thr[row];
    x.open(walk, p, cb);
  }
  uint32_t above = 0, tied = 0, seen = 0;
  const double *arow = aq + (size_t)(qt * PQ + 16 * w + r16) * k16;
  for (uint32_t c0 = cb; c0 < ce; c0 += PC) {
    uint32_t cand[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cand[j] = c0 + 16 * j + r16 < ce ? c0 + 16 * j + r16 : NONE;
    score_tile<X::SCALED>(S, arow, cand, K, ld, k16, gamma, inv, w, g, r16);
    __syncthreads();
    if (p != NONE) {
      for (uint32_t i = 0; i < PC / 4; ++i) {
        const uint32_t cc = sub + 4 * i, v = c0 + cc;
        if (v >= ce) break;
        x.advance(walk, v);
        if (v == p || v == q || x.at(walk, v)) continue;
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

// The geometry of a batch of m query rows for the tile kernels: rows = m rounded up to PQ (the rows past the batch hold
// NONE), k16 = K rounded up to 16, and nch = the candidate chunks of the grid: enough blocks for eight per CU, at most
// nch_max (the caller's own bound, if it has one) and at least 64 candidates per chunk.  No result depends on the cut: a
// top k is that of one total order, counts are sums over the chunks.
struct TileBatch {
  uint32_t nqt, rows, nch, k16;
};
inline TileBatch plan_tile_batch(uint32_t m, uint32_t n, uint32_t K, uint32_t cus, uint32_t nch_max) {
  TileBatch tb;
  tb.nqt = (m + PQ - 1) / PQ;
  tb.rows = tb.nqt * PQ;
  tb.k16 = (K + 15u) & ~15u;
  tb.nch = std::max<uint32_t>(1, (8u * cus + tb.nqt - 1) / tb.nqt);
  tb.nch = std::min(tb.nch, nch_max);
  tb.nch = std::min(tb.nch, std::max<uint32_t>(1, n / PC));
  return tb;
}
// the bound on nch for svils_*_predict_links: the merge sorts the 4 x nch x topk heap entries of a query in LDS
inline uint32_t topk_chunk_bound(uint32_t topk) { return std::max<uint32_t>(1, MERGE_MAX / (4 * topk)); }
// entries of each of the two heap arrays of a batch
inline uint64_t heap_entries(const TileBatch &tb, uint32_t topk) { return (uint64_t)tb.nqt * tb.nch * topk * 256; }

// The operands of a batch on the device.  cand [n][ld] with K its columns in use (zero past K where ld > K), inv [n] where
// X::SCALED; aq [rows][k16]; qnodes [rows]
struct TileOperands {
  uint32_t n, K, ld;
  const double *cand, *inv, *aq;
  const uint32_t *qnodes;
};

// the top topk of the m query rows -> oscore / oid [m][topk]; hs / hi: heap_entries() each
template <class X>
inline void launch_topk(hipStream_t st, const TileBatch &tb, const TileOperands &o, const X &x, uint32_t m, uint32_t topk, double *hs,
                        uint32_t *hi, double *oscore, uint32_t *oid) {
  uint32_t L = 4 * tb.nch * topk, lp = 1;
  while (lp < L) lp <<= 1;
  hipLaunchKernelGGL((k_topk_tiles<X>), dim3(tb.nqt, tb.nch), dim3(256), 0, st, o.n, o.K, o.ld, tb.k16, topk, tb.nch, o.cand, o.inv,
                     o.aq, o.qnodes, x, hs, hi);
  hipLaunchKernelGGL(k_topk_merge<MERGE_MAX>, dim3(m), dim3(256), 0, st, topk, tb.nch, lp, hs, hi, oscore, oid);
}

// thr [rows] = the score of (qnodes[i], qcand[i])
template <class X>
inline void launch_thresh(hipStream_t st, const TileBatch &tb, const TileOperands &o, const uint32_t *qcand, double *thr) {
  hipLaunchKernelGGL((k_rank_thresh<X::SCALED>), dim3(tb.nqt), dim3(256), 0, st, o.K, o.ld, tb.k16, o.cand, o.inv, o.aq, qcand, thr);
}

// ... and cnt [rows][3] (zeroed by the caller) += the candidates c != qcand[i] above it, tied with it, seen
template <class X>
inline void launch_ranks(hipStream_t st, const TileBatch &tb, const TileOperands &o, const X &x, const uint32_t *qcand, double *thr,
                         uint32_t *cnt) {
  launch_thresh<X>(st, tb, o, qcand, thr);
  hipLaunchKernelGGL((k_rank_tiles<X>), dim3(tb.nqt, tb.nch), dim3(256), 0, st, o.n, o.K, o.ld, tb.k16, tb.nch, o.cand, o.inv, o.aq,
                     o.qnodes, qcand, thr, x, cnt);
}

}  // namespace svils_impl
