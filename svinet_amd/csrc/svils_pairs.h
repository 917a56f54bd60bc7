// svils_pairs.h -- what the queries about node pairs share: svils_predict.hip (svils_link_prob, svils_predict_links,
// svils_rank_links), svils_nbr.hip (svils_nbr_score, svils_nbr_rank) and, through svils_pairtiles.h, svils_orig_predict.hip.  The refusals of include/svils.h in one order, the
// search in a sorted CSR row (svils_impl::sorted_rows), and the way a batch of ranks goes back to the caller.
#pragma once
#include "svils_handle.h"

namespace svils_impl {

constexpr uint32_t NONE = 0xffffffffu;   // no node: a query row past the batch, a tile column past the candidates

// q is in s[b, e), a sorted CSR row
__device__ inline bool in_row(const uint32_t *__restrict__ s, uint64_t b, uint64_t e, uint32_t q) {
  while (b < e) {
    const uint64_t m = (b + e) >> 1;
    const uint32_t v = s[m];
    if (v == q) return true;
    if (v < q) b = m + 1; else e = m;
  }
  return false;
}

// the handles an entry point `name` refuses: a whole-graph handle on one device with its graph set, and (need_state: the
// model's queries) a state and no mini-batch step open
inline int check_pair_handle(svils_handle *h, const char *name, bool need_state) {
  if (!h) return fail(SVILS_ERR_ARG, "%s: null handle", name);
  if (TILED(h)) return fail(SVILS_ERR_UNSUPPORTED, "%s: not available on a column-tiled handle (k > SVILS_MAX_K = %d)", name, SVILS_MAX_K);
  if (h->d.ksh) return fail(SVILS_ERR_UNSUPPORTED, "%s: not available on a K-sharded handle", name);
  if (h->geo.node_begin != 0 || h->geo.node_end != h->geo.n || h->blocks_set || h->comm)
    return fail(SVILS_ERR_UNSUPPORTED, "%s: not available on a node-block handle", name);
  if (!need_state) return h->have_graph ? 0 : fail(SVILS_ERR_ARG, "%s: set the graph first", name);
  if (!h->have_graph || !h->have_state) return fail(SVILS_ERR_ARG, "%s: set graph and state first", name);
  if (h->step_open) return fail(SVILS_ERR_ARG, "%s: a mini-batch step is open (close it with phase D)", name);
  return 0;
}

// ... and the pair lists it refuses: pairs[npairs][2], two different nodes < n each
inline int check_pairs(uint32_t n, const char *name, const uint32_t *pairs, uint64_t npairs) {
  if (npairs && !pairs) return fail(SVILS_ERR_ARG, "%s: null argument", name);
  for (uint64_t i = 0; i < npairs; ++i) {
    const uint32_t p = pairs[2 * i], q = pairs[2 * i + 1];
    if (p >= n || q >= n) return fail(SVILS_ERR_ARG, "%s: pair %llu = (%u, %u): node id >= n = %u", name, (unsigned long long)i, p, q, n);
    if (p == q) return fail(SVILS_ERR_ARG, "%s: pair %llu = (%u, %u): p == q", name, (unsigned long long)i, p, q);
  }
  return 0;
}

inline int check_pairs(const svils_handle *h, const char *name, const uint32_t *pairs, uint64_t npairs) {
  return check_pairs(h->geo.n, name, pairs, npairs);
}

// The end of a batch of m ranks: cnt[m][3] = above, tied, ncand and score[m] on the device go to entries b .. b + m - 1 of
// the caller's arrays, any of which may be null.  Waits for the stream.
inline int fetch_ranks(hipStream_t stream, const uint32_t *cnt, const double *dscore, uint32_t m, uint64_t b, uint32_t *above,
                       uint32_t *tied, uint32_t *ncand, double *score) {
  std::vector<uint32_t> ch(3 * (size_t)m);
  HIPCHK(hipMemcpyAsync(ch.data(), cnt, ch.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  if (score) HIPCHK(hipMemcpyAsync(score + b, dscore, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  for (uint32_t i = 0; i < m; ++i) {
    if (above) above[b + i] = ch[3 * (size_t)i];
    if (tied) tied[b + i] = ch[3 * (size_t)i + 1];
    if (ncand) ncand[b + i] = ch[3 * (size_t)i + 2];
  }
  return 0;
}

}  // namespace svils_impl
