// svils_orig.h -- the svils_orig handle (-orig, the full K x K blockmodel), shared by its three translation units:
//
//   svils_orig.hip           the sweeps, the state and the pair likelihoods
//   svils_orig_predict.hip   the link queries of a fitted state (svils_orig_link_prob / _predict_links / _rank_links)
//   svils_orig_elbo.hip      the variational lower bound of the current state (svils_orig_elbo)
#pragma once
#include "svils_tool.h"

namespace svils_impl {

typedef unsigned long long u64;
// the device counters of a handle (svils_orig::ctr)
enum { CTR_PAIRS, CTR_ROUNDS, CTR_MAXR, CTR_NORM, CTR_BETA, CTR_FLAG, CTR_PENDING, CTR_COUNT };

constexpr uint32_t TILE_PAIRS = 16;                 // pairs per wavefront: the columns of one MFMA
// row stride of the transposed log tables: 16 (mod 32) doubles, so the four lane groups of an A operand read take two LDS passes
constexpr int tab_ld(int kp) { return kp % 32 == 0 ? kp + 16 : kp; }

// one launch of the pair kernel (svils_orig.hip: k_orig_pairs)
struct PairArgs {
  uint32_t n, K, nw, p0, rows, tpr;   // nw: words per row of the bit matrices; rows p0 .. p0 + rows; tpr = ceil(n / 16)
  const uint32_t *adj, *skip;         // [n][nw] bit q of row p: y(p, q) / the ordered pair (p, q) is left out
  const double *elogpi;               // [n][K]
  const double *tabs;                 // [2][KP][ld]
  double *phi1, *phi2;                // [rows n][KP]
  uint8_t *yv;                        // [rows n]
  u64 *ctr;
};

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
  // The lower bound (svils_orig_elbo.hip): scratch, counters and events of its own -- nothing a sweep or a query reads
  double *el_elogpi = nullptr;                                    // [n][k] Elogpi of the current gamma
  double *el_tabs = nullptr;                                      // [4][kp][ld]: L0, L1 (the fixed point's), T0, T1 (the bound's)
  double *el_part = nullptr;                                      // [n][4]: a row's tiles t = j (mod 4), one double each
  double *el_node = nullptr;                                      // [n]
  double *el_out = nullptr;                                       // [3] total, P, N
  u64 *el_ctr = nullptr;                                          // [CTR_COUNT] the pass's counter block
  std::vector<hipEvent_t> ev_elbo;                                // [2 + 2 launches]: start, (pairs, terms) per launch, end
  uint32_t el_nlaunch = 0;
  bool timed_elbo = false;
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

// What svils_orig_elbo.hip runs of a sweep (svils_orig.hip).  orig_launch_prologue: Elogpi of the handle's gamma into
// elogpi [n][k], and the log tables of its beta into tabs [2][kp][ld] -- T0 = log(1 - beta + eps), T1 = log(beta + eps).
// orig_launch_pairs: one launch of k_orig_pairs<KP, LREG> for the handle's padded K over the rows of a
int orig_launch_prologue(svils_orig *h, double *elogpi, double *tabs, double eps);
int orig_launch_pairs(svils_orig *h, const char *name, const PairArgs &a);
// svils_orig_destroy: the events of the lower bound (svils_orig_elbo.hip)
void free_elbo(svils_orig *h);

// svils_orig_destroy: the batch buffers and the events of the link queries (svils_orig_predict.hip)
void free_queries(svils_orig *h);

}  // namespace svils_impl
