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
//   the tile kernels (score_tile, k_topk_tiles, k_topk_merge, k_rank_thresh, k_rank_tiles) are svils_pairtiles.h, shared
//   with svils_orig_predict.hip; here they run with the candidate policy CsrRows (the sorted CSR) and gamma as the operand
//
// Host side: begin_tile_batch is the start of every batch of the two tile queries (chunks, query rows); the refusals, NONE,
// in_row and the way ranks go back to the caller are svils_pairs.h, shared with svils_nbr.hip.
//
// Read-only: everything here reads gamma, lambda and the CSR, and writes the scratch of svils_handle::pred only.
#include "svils_pairtiles.h"

namespace {

constexpr uint64_t PAIR_BATCH = 1u << 20; // pairs per internal batch of svils_link_prob

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
// multiple of PQ; the device gets them (pred.qnodes) and their rows of aq (k_build_aq).  The geometry is plan_tile_batch's;
// *op are the operands of the batch's tile kernels.
int begin_tile_batch(svils_handle *h, std::vector<uint32_t> &qh, uint32_t nch_max, TileBatch *tb, TileOperands *op) {
  const Geometry &g = h->geo;
  svils_handle::PredictScratch &s = h->pred;
  *tb = plan_tile_batch((uint32_t)qh.size(), g.n, g.K, cu_count(h->cfg.device), nch_max);
  const uint64_t ae = (uint64_t)tb->rows * tb->k16;
  if (int rc = reserve(h, s.qnodes, tb->rows)) return rc;
  if (int rc = reserve(h, s.aq, ae)) return rc;
  qh.resize(tb->rows, NONE);
  HIPCHK(hipMemcpyAsync(s.qnodes.p, qh.data(), tb->rows * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_build_aq, dim3((uint32_t)((ae + 255) / 256)), dim3(256), 0, h->stream, tb->rows, g.K, g.ld, tb->k16,
                     h->d.gamma, s.inv, s.beta, s.qnodes.p, s.aq.p);
  HIPCHK(hipGetLastError());
  *op = TileOperands{g.n, g.K, g.ld, h->d.gamma, s.inv, s.aq.p, s.qnodes.p};
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
    TileBatch tb;
    TileOperands op;
    if (int rc = begin_tile_batch(h, qh, topk_chunk_bound(topk), &tb, &op)) return rc;
    const uint64_t oneed = (uint64_t)Q_BATCH * topk, hneed = heap_entries(tb, topk);
    if (int rc = reserve(h, s.ids, oneed)) return rc;
    if (int rc = reserve(h, s.scores, oneed)) return rc;
    if (int rc = reserve(h, s.hs, hneed)) return rc;
    if (int rc = reserve(h, s.hi, hneed)) return rc;
    launch_topk(h->stream, tb, op, CsrRows{h->d.rowptr, s.scol}, m, topk, s.hs.p, s.hi.p, s.scores.p, s.ids.p);
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
    TileOperands op;
    if (int rc = begin_tile_batch(h, ph, UINT32_MAX, &tb, &op)) return rc;
    if (int rc = reserve(h, s.rq, tb.rows)) return rc;
    if (int rc = reserve(h, s.rthr, tb.rows)) return rc;
    if (int rc = reserve(h, s.rcnt, 3 * (uint64_t)tb.rows)) return rc;
    qh.assign(tb.rows, NONE);
    for (uint32_t i = 0; i < m; ++i) qh[i] = pairs[2 * (b + i) + 1];
    HIPCHK(hipMemcpyAsync(s.rq.p, qh.data(), tb.rows * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(s.rcnt.p, 0, 3 * (size_t)tb.rows * sizeof(uint32_t), h->stream));
    launch_ranks(h->stream, tb, op, CsrRows{h->d.rowptr, s.scol}, s.rq.p, s.rthr.p, s.rcnt.p);
    HIPCHK(hipGetLastError());
    if (int rc = fetch_ranks(h->stream, s.rcnt.p, s.rthr.p, m, b, above, tied, ncand, score)) return rc;
  }
  return 0;
}

}  // extern "C"
