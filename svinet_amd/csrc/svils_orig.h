// svils_orig.h -- the svils_orig handle (-orig, the full K x K blockmodel), shared by its two translation units:
//
//   svils_orig.hip           the sweeps, the state and the pair likelihoods
//   svils_orig_predict.hip   the link queries of a fitted state (svils_orig_link_prob / _predict_links / _rank_links)
#pragma once
#include "svils_tool.h"

namespace svils_impl {

typedef unsigned long long u64;
// the device counters of a handle (svils_orig::ctr)
enum { CTR_PAIRS, CTR_ROUNDS, CTR_MAXR, CTR_NORM, CTR_BETA, CTR_FLAG, CTR_PENDING, CTR_COUNT };

}  // namespace svils_impl

struct svils_orig : svils_impl::ToolHandle {
  typedef svils_impl::u64 u64;
  uint32_t n = 0, k = 0, kp = 0, ld = 0, nw = 0;
  double alpha = 0;
  // HANDLE scope
  double *gamma = nullptr, *gnext = nullptr, *elogpi = nullptr;   // [n][k]
  double *beta = nullptr;                                         // [k][k]
  double *tabs = nullptr;                                         // [2][kp][ld]
  double *nt = nullptr;                                           // [2][kp kp] num, tot in the C/D layout
  double *part = nullptr;                                         // [ACC_WAVES][2][kp kp]
  double *gtab = nullptr;                                         // [128][2] log_tab's table
  u64 *ctr = nullptr;                                             // [CTR_COUNT]
  double *pi = nullptr;                                           // [n][kp] the link queries' gamma / row sum, zero past column k: built on first use
  // GRAPH scope
  uint32_t *adj = nullptr, *skip = nullptr;                       // [n][nw]
  uint32_t *excl = nullptr;                                       // [n][nw] the link queries' adj & ~(skip | skip^T): built on first use
  double *phi1 = nullptr, *phi2 = nullptr;                        // [rows n][kp]
  uint8_t *yv = nullptr;                                          // [rows n]
  uint32_t *ll_pairs = nullptr;                                   // svils_orig_pair_loglik: grown on demand
  uint8_t *ll_y = nullptr;
  double *ll_out = nullptr;
  uint32_t rows = 0, nlaunch = 0;                                 // p rows per launch, launches per sweep
  uint32_t rows_req = 0;                                          // svils_orig_set_launch_rows: 0 = as many as the bound admits
  bool have_graph = false, have_state = false, timed = false;
  // The link queries (svils_orig_predict.hip).  state_gen counts the changes of the state (svils_orig_set_state, every
  // svils_orig_sweep call); pi is that of generation pi_gen and is rebuilt when the two differ.  The batch buffers are
  // outside the scopes: grown on demand, freed by svils_orig_destroy (free_queries)
  uint64_t state_gen = 1, pi_gen = 0;
  struct Query {
    svils_impl::DevBuf<uint32_t> qnodes, qcand, cnt, ids, hi;     // [rows], [rows], [rows][3], [batch][topk], heaps
    svils_impl::DevBuf<double> aq, thr, scores, hs;               // [rows][kp], [rows], [batch][topk], heaps
    hipEvent_t ev[2] = {nullptr, nullptr};                        // around the device work of the last query call
    bool timed = false;
  } qry;
};

namespace svils_impl {

// waits for the stream; a raised degenerate flag becomes an error
inline int settle(svils_orig *h, const char *name) {
  u64 c[CTR_COUNT] = {0};
  HIPCHK(hipMemcpyAsync(c, h->ctr, sizeof c, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  if (c[CTR_PENDING])
    return fail(SVILS_ERR_UNSUPPORTED,
                "%s: %llu block rate(s) left (0, 1) after a sweep (a block saw only links or only non-links; %llu pair(s) with a "
                "normaliser not > 0); later sweeps were not applied",
                name, c[CTR_BETA], c[CTR_NORM]);
  return 0;
}

// svils_orig_destroy: the batch buffers and the events of the link queries (svils_orig_predict.hip)
void free_queries(svils_orig *h);

}  // namespace svils_impl
