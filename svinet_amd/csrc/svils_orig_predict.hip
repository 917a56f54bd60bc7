// svils_orig_predict.hip -- link queries of a fitted -orig state: svils_orig_link_prob (scores of given ordered pairs),
// svils_orig_predict_links (the top-k candidate links of query nodes) and svils_orig_rank_links (where a given node stands
// among them).  The quantity is the argument of the reference's MMSBInferOrig::edge_likelihood(p, c, 1)
// (src/mmsbinferorig.cc:563-587): score(p, c) = sum_g sum_h pi_p[g] beta[g][h] pi_c[h], pi_x = gamma_x / sum_k gamma_xk.
// beta is not symmetric: score(p, c) != score(c, p), and every query is answered in the orientation it is asked in.
//
//   k_orig_pi      pi [n][kp], kp = 16 ceil(K / 16): gamma / row sum (a sequential sum, k ascending), zero past column K --
//                  the candidate operand of the tiles (gamma itself has ld = K, which may be odd: the tiles read double2s)
//   k_orig_excl    once per graph: excl = adj & ~(skip | skip^T), the bit matrix of the pairs that are NOT candidates -- a
//                  link is excluded unless it was left out of training in either orientation
//   k_orig_aq      the query rows of a batch: aq[i][h] = sum_g pi_p[g] beta[g][h], g ascending by fma, zero past the batch
//                  and past column K.  One function, one order: every bitwise statement of include/svils.h rests on it
//   the tile kernels are svils_pairtiles.h (shared with svils_predict.hip), with the candidate policy BitRows on excl,
//   operand pi, ld = kp and no row scaling.  All three calls get their scores from score_tile: svils_orig_link_prob is
//   k_rank_thresh alone.
//
// Read-only: gamma, beta, adj and skip are read; written are pi, excl and the batch buffers of svils_orig::qry.
#include "svils_orig.h"
#include "svils_pairtiles.h"

using namespace svils_impl;

namespace {

__global__ __launch_bounds__(256) void k_orig_pi(uint32_t n, uint32_t K, uint32_t kp, const double *__restrict__ gamma,
                                                 double *__restrict__ pi) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (uint64_t)n * kp) return;
  const uint32_t x = (uint32_t)(e / kp), k = (uint32_t)(e % kp);
  const double *g = gamma + (size_t)x * K;
  double s = 0.0;
  for (uint32_t j = 0; j < K; ++j) s += g[j];   // the same bits in every thread of the row
  pi[e] = k < K ? g[k] / s : 0.0;
}

// word w of row p: the links (p, c), c = 32 w + b, that no orientation of the skip list names
__global__ __launch_bounds__(256) void k_orig_excl(uint32_t n, uint32_t nw, const uint32_t *__restrict__ adj,
                                                   const uint32_t *__restrict__ skip, uint32_t *__restrict__ excl) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (uint64_t)n * nw) return;
  const uint32_t p = (uint32_t)(e / nw), w = (uint32_t)(e % nw);
  uint32_t out = 0;
  for (uint32_t m = adj[e] & ~skip[e]; m; m &= m - 1) {   // adj has no bit at or past column n
    const uint32_t b = (uint32_t)__ffs((int)m) - 1, c = 32 * w + b;
    if (!((skip[(size_t)c * nw + (p >> 5)] >> (p & 31)) & 1u)) out |= 1u << b;
  }
  excl[e] = out;
}

// aq[i][h] for i < rows (a multiple of PQ), h < kp
__global__ __launch_bounds__(256) void k_orig_aq(uint32_t rows, uint32_t K, uint32_t kp, const double *__restrict__ pi,
                                                 const double *__restrict__ beta, const uint32_t *__restrict__ qnodes,
                                                 double *__restrict__ aq) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (uint64_t)rows * kp) return;
  const uint32_t i = (uint32_t)(e / kp), h = (uint32_t)(e % kp), p = qnodes[i];
  double s = 0.0;
  if (p != NONE && h < K) {
    const double *row = pi + (size_t)p * kp;
    for (uint32_t g = 0; g < K; ++g) s = fma(row[g], beta[(size_t)g * K + h], s);
  }
  aq[e] = s;
}

template <class T>
int grow(DevBuf<T> &b, uint64_t need) {   // the stream is idle: every query call ends with a wait
  if (b.cap >= need) return 0;
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  HIPCHK(hipMalloc((void **)&b.p, need * sizeof(T)));
  b.cap = need;
  return 0;
}
template <class T>
void drop(DevBuf<T> &b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

// what every query needs before its batches: a handle with graph and state, no degenerate flag (waits for the sweeps), excl
// of the graph and pi of the current state
int prepare(svils_orig *h, const char *name) {
  if (!h->have_graph || !h->have_state) return fail(SVILS_ERR_ARG, "%s: set graph and state first", name);
  if (int rc = settle(h, name)) return rc;
  for (hipEvent_t &e : h->qry.ev)
    if (!e) HIPCHK(hipEventCreate(&e));
  h->qry.timed = false;
  HIPCHK(hipEventRecord(h->qry.ev[0], h->st));
  if (!h->excl) {
    if (int rc = h->dalloc(ToolHandle::GRAPH, &h->excl, (size_t)h->n * h->nw)) return rc;
    hipLaunchKernelGGL(k_orig_excl, dim3(blocks((uint64_t)h->n * h->nw, 256)), dim3(256), 0, h->st, h->n, h->nw, h->adj, h->skip, h->excl);
    HIPCHK(hipGetLastError());
  }
  if (!h->pi) {
    if (int rc = h->dalloc(ToolHandle::HANDLE, &h->pi, (size_t)h->n * h->kp)) return rc;
    h->pi_gen = 0;
  }
  if (h->pi_gen != h->state_gen) {
    hipLaunchKernelGGL(k_orig_pi, dim3(blocks((uint64_t)h->n * h->kp, 256)), dim3(256), 0, h->st, h->n, h->k, h->kp, h->gamma, h->pi);
    HIPCHK(hipGetLastError());
    h->pi_gen = h->state_gen;
  }
  return 0;
}

// the end of a query call's device work (the results of its last batch are copied out behind it)
int finish(svils_orig *h) {
  HIPCHK(hipEventRecord(h->qry.ev[1], h->st));
  h->qry.timed = true;
  return 0;
}

// The start of a batch: qh holds its m query nodes and is padded here with NONE to a multiple of PQ rows; the device gets
// them and their rows of aq
int begin_batch(svils_orig *h, std::vector<uint32_t> &qh, uint32_t nch_max, TileBatch *tb, TileOperands *op) {
  svils_orig::Query &s = h->qry;
  *tb = plan_tile_batch((uint32_t)qh.size(), h->n, h->k, cu_count(h->device), nch_max);
  const uint64_t ae = (uint64_t)tb->rows * h->kp;   // tb->k16 == h->kp
  if (int rc = grow(s.qnodes, tb->rows)) return rc;
  if (int rc = grow(s.aq, ae)) return rc;
  qh.resize(tb->rows, NONE);
  HIPCHK(hipMemcpyAsync(s.qnodes.p, qh.data(), tb->rows * sizeof(uint32_t), hipMemcpyHostToDevice, h->st));
  hipLaunchKernelGGL(k_orig_aq, dim3(blocks(ae, 256)), dim3(256), 0, h->st, tb->rows, h->k, h->kp, h->pi, h->beta, s.qnodes.p, s.aq.p);
  HIPCHK(hipGetLastError());
  *op = TileOperands{h->n, h->kp, h->kp, h->pi, nullptr, s.aq.p, s.qnodes.p};
  return 0;
}

// ... of a batch of m directed pairs: the p's are the query nodes, the q's go to qry.qcand
int begin_pair_batch(svils_orig *h, const uint32_t *pairs, uint32_t m, std::vector<uint32_t> &ph, std::vector<uint32_t> &qh,
                     TileBatch *tb, TileOperands *op) {
  svils_orig::Query &s = h->qry;
  ph.resize(m);
  for (uint32_t i = 0; i < m; ++i) ph[i] = pairs[2 * (size_t)i];
  if (int rc = begin_batch(h, ph, UINT32_MAX, tb, op)) return rc;   // no bound on the chunks: nothing is merged
  if (int rc = grow(s.qcand, tb->rows)) return rc;
  if (int rc = grow(s.thr, tb->rows)) return rc;
  qh.assign(tb->rows, NONE);
  for (uint32_t i = 0; i < m; ++i) qh[i] = pairs[2 * (size_t)i + 1];
  HIPCHK(hipMemcpyAsync(s.qcand.p, qh.data(), tb->rows * sizeof(uint32_t), hipMemcpyHostToDevice, h->st));
  return 0;
}

}  // namespace

void svils_impl::free_queries(svils_orig *h) {
  svils_orig::Query &s = h->qry;
  drop(s.qnodes); drop(s.qcand); drop(s.cnt); drop(s.ids); drop(s.hi);
  drop(s.aq); drop(s.thr); drop(s.scores); drop(s.hs);
  for (hipEvent_t &e : s.ev) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
}

extern "C" {

int svils_orig_link_prob(svils_orig *h, const uint32_t *pairs, uint64_t npairs, double *prob) {
  const char *name = "svils_orig_link_prob";
  if (int rc = check(h, name)) return rc;
  if (npairs && (!pairs || !prob)) return fail(SVILS_ERR_ARG, "%s: null argument", name);
  if (int rc = check_pairs(h->n, name, pairs, npairs)) return rc;
  if (int rc = prepare(h, name)) return rc;
  svils_orig::Query &s = h->qry;
  std::vector<uint32_t> ph, qh;
  for (uint64_t b = 0; b < npairs; b += Q_BATCH) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(Q_BATCH, npairs - b);
    TileBatch tb;
    TileOperands op;
    if (int rc = begin_pair_batch(h, pairs + 2 * b, m, ph, qh, &tb, &op)) return rc;
    launch_thresh<BitRows>(h->st, tb, op, s.qcand.p, s.thr.p);
    HIPCHK(hipGetLastError());
    if (b + m == npairs) finish(h);
    HIPCHK(hipMemcpyAsync(prob + b, s.thr.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
  }
  return 0;
}

int svils_orig_predict_links(svils_orig *h, const uint32_t *nodes, uint32_t nnodes, uint32_t topk, uint32_t *ids, double *scores) {
  const char *name = "svils_orig_predict_links";
  if (int rc = check(h, name)) return rc;
  const uint32_t n = h->n;
  if (topk == 0 || topk > SVILS_PREDICT_MAX_TOPK)
    return fail(SVILS_ERR_ARG, "%s: topk = %u, need 1 .. %d", name, topk, SVILS_PREDICT_MAX_TOPK);
  if (!nodes && nnodes != 0 && nnodes != n)
    return fail(SVILS_ERR_ARG, "%s: nodes = NULL means all %u nodes (nnodes = 0 or n, not %u)", name, n, nnodes);
  const uint32_t nq = nodes ? nnodes : n;
  if (nq && (!ids || !scores)) return fail(SVILS_ERR_ARG, "%s: null argument", name);
  if (nodes)
    for (uint32_t i = 0; i < nq; ++i)
      if (nodes[i] >= n) return fail(SVILS_ERR_ARG, "%s: node %u (entry %u) >= n = %u", name, nodes[i], i, n);
  if (int rc = prepare(h, name)) return rc;
  svils_orig::Query &s = h->qry;
  const BitRows x{h->excl, h->nw};
  std::vector<uint32_t> qh;
  for (uint32_t b = 0; b < nq; b += Q_BATCH) {
    const uint32_t m = std::min(Q_BATCH, nq - b);
    qh.resize(m);
    for (uint32_t i = 0; i < m; ++i) qh[i] = nodes ? nodes[b + i] : b + i;
    TileBatch tb;
    TileOperands op;
    if (int rc = begin_batch(h, qh, topk_chunk_bound(topk), &tb, &op)) return rc;
    const uint64_t oneed = (uint64_t)m * topk, hneed = heap_entries(tb, topk);
    if (int rc = grow(s.ids, oneed)) return rc;
    if (int rc = grow(s.scores, oneed)) return rc;
    if (int rc = grow(s.hs, hneed)) return rc;
    if (int rc = grow(s.hi, hneed)) return rc;
    launch_topk(h->st, tb, op, x, m, topk, s.hs.p, s.hi.p, s.scores.p, s.ids.p);
    HIPCHK(hipGetLastError());
    if (b + m == nq) finish(h);
    HIPCHK(hipMemcpyAsync(ids + (size_t)b * topk, s.ids.p, (size_t)m * topk * sizeof(uint32_t), hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipMemcpyAsync(scores + (size_t)b * topk, s.scores.p, (size_t)m * topk * sizeof(double), hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
  }
  return 0;
}

int svils_orig_rank_links(svils_orig *h, const uint32_t *pairs, uint64_t npairs, uint32_t *above, uint32_t *tied, uint32_t *ncand,
                          double *score) {
  const char *name = "svils_orig_rank_links";
  if (int rc = check(h, name)) return rc;
  if (int rc = check_pairs(h->n, name, pairs, npairs)) return rc;
  if (int rc = prepare(h, name)) return rc;
  svils_orig::Query &s = h->qry;
  const BitRows x{h->excl, h->nw};
  std::vector<uint32_t> ph, qh;
  for (uint64_t b = 0; b < npairs; b += Q_BATCH) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(Q_BATCH, npairs - b);
    TileBatch tb;
    TileOperands op;
    if (int rc = begin_pair_batch(h, pairs + 2 * b, m, ph, qh, &tb, &op)) return rc;
    if (int rc = grow(s.cnt, 3 * (uint64_t)tb.rows)) return rc;
    HIPCHK(hipMemsetAsync(s.cnt.p, 0, 3 * (size_t)tb.rows * sizeof(uint32_t), h->st));
    launch_ranks(h->st, tb, op, x, s.qcand.p, s.thr.p, s.cnt.p);
    HIPCHK(hipGetLastError());
    if (b + m == npairs) finish(h);
    if (int rc = fetch_ranks(h->st, s.cnt.p, s.thr.p, m, b, above, tied, ncand, score)) return rc;
  }
  return 0;
}

int svils_orig_get_query_timing(svils_orig *h, double *ms) {
  if (int rc = check(h, "svils_orig_get_query_timing")) return rc;
  if (!ms) return fail(SVILS_ERR_ARG, "svils_orig_get_query_timing: null argument");
  HIPCHK(hipStreamSynchronize(h->st));
  float t = 0;
  *ms = h->qry.timed && hipEventElapsedTime(&t, h->qry.ev[0], h->qry.ev[1]) == hipSuccess ? (double)t : -1.0;
  return 0;
}

}  // extern "C"
