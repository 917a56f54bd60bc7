// svils_nbr.hip -- neighbourhood scores of node pairs from the training graph alone: svils_nbr_score (the score of given
// pairs) and svils_nbr_rank (where q stands among p's candidates by that score).  No model: the baselines a fitted model's
// link ranks are read against.  score(p, q) = sum over the common training neighbours z of p and q, in ASCENDING z, of
// w[deg z]: common neighbours (w = 1), Adamic-Adar (w = 1 / log deg z; the reference's -adamic-adar,
// FastAMM::compute_adamic_adar_score, src/fastamm.cc:1486-1575) and resource allocation (w = 1 / deg z).  The weight tables
// are built on the host (build_weights) and only read here: equal scores are counted as ties, so a weight must be the double
// anybody can restate.
//
//   nbr_pair      one wavefront, one pair: the shorter sorted row in chunks of 64, every lane searches the longer row for its
//                 entry, the matches of a chunk come out of a ballot and their weights are added one by one in lane order
//   k_nbr_pairs   one wavefront per pair
//   k_nbr_rank    persistent blocks over the directed pairs (p, q).  The candidates of p that score above zero are the nodes
//                 two steps from p: the block walks z in N(p), c in N(z), claims every c once in a bitmap of its own
//                 (atomicOr: the first claimant decides), lists the claimed candidates in LDS, and its wavefronts score
//                 them with nbr_pair against s = nbr_pair(p, q) into integer counters.  Every other candidate scores
//                 exactly zero: they are counted, not visited.  The walk is repeated to clear the claimed bits.
//
// Read-only: rowptr, the sorted rows of svils_handle::pred and the scratch of svils_handle::nbr; needs no state.  The
// refusals, NONE, in_row and the way ranks go back to the caller are svils_pairs.h, shared with svils_predict.hip.
#include "svils_pairs.h"

namespace {

constexpr uint32_t LIST_CAP = 2048;           // candidates a block lists before its wavefronts score them
constexpr uint64_t NBR_BATCH = 1u << 16;      // pairs per internal batch (bounds the scratch, see include/svils.h)
constexpr uint32_t BLOCKS_PER_CU = 4;

// The score of (p, q) and the number of their common neighbours, the same value in every lane.  Called by a whole wavefront
// with p and q uniform.  The sum is sequential in ascending z whatever the row lengths: chunks ascend along the shorter
// row, lanes ascend within a chunk, and every lane adds the same weights in the same order (nothing is reduced across lanes).
__device__ inline double nbr_pair(const uint64_t *__restrict__ rowptr, const uint32_t *__restrict__ scol,
                                  const double *__restrict__ w, uint32_t p, uint32_t q, uint32_t lane, uint32_t *common) {
  uint64_t ab = rowptr[p], ae = rowptr[p + 1], bb = rowptr[q], be = rowptr[q + 1];
  if (ae - ab > be - bb) {
    uint64_t t = ab; ab = bb; bb = t;
    t = ae; ae = be; be = t;
  }
  double s = 0.0;
  uint32_t cnt = 0;
  for (uint64_t base = ab; base < ae; base += 64) {
    double wz = 0.0;
    bool hit = false;
    if (base + lane < ae) {
      const uint32_t z = scol[base + lane];
      hit = in_row(scol, bb, be, z);
      if (hit) wz = w[rowptr[z + 1] - rowptr[z]];
    }
    unsigned long long mask = __ballot(hit);
    cnt += (uint32_t)__popcll(mask);
    const int hi = __double2hiint(wz), lo = __double2loint(wz);
    while (mask) {
      const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(mask));
      mask &= mask - 1;
      s += __hiloint2double(__builtin_amdgcn_readlane(hi, j), __builtin_amdgcn_readlane(lo, j));
    }
  }
  *common = cnt;
  return s;
}

__global__ __launch_bounds__(256) void k_nbr_pairs(uint32_t np, const uint64_t *__restrict__ rowptr, const uint32_t *__restrict__ scol,
                                                   const double *__restrict__ w, const uint32_t *__restrict__ pairs,
                                                   double *__restrict__ score, uint32_t *__restrict__ common) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= np) return;
  uint32_t c;
  const double s = nbr_pair(rowptr, scol, w, pairs[2 * i], pairs[2 * i + 1], lane, &c);
  if (lane == 0) { score[i] = s; common[i] = c; }
}

// the nl listed candidates scored by the block's wavefronts, one candidate per wavefront at a time; the list is empty
// afterwards.  Called by the whole block behind a barrier, with nothing adding to the list.
__device__ inline void drain(const uint64_t *__restrict__ rowptr, const uint32_t *__restrict__ scol, const double *__restrict__ w,
                             uint32_t p, double s, const uint32_t *list, uint32_t *lcount, uint32_t nl, uint32_t wv, uint32_t lane,
                             uint32_t *above, uint32_t *tied, uint32_t *seen) {
  for (uint32_t k = wv; k < nl; k += 4) {
    uint32_t cm;
    const double sc = nbr_pair(rowptr, scol, w, p, list[k], lane, &cm);
    *above += sc > s ? 1u : 0u;
    *tied += sc == s ? 1u : 0u;
    ++*seen;
  }
  __syncthreads();
  if (threadIdx.x == 0) *lcount = 0;
  __syncthreads();
}

// Block b serves the pairs b, b + gridDim.x, ...; bitmap + b * words is its own (all zero on entry and on exit).  Wavefront
// wv walks the neighbours wv, wv + 4, ... of p, 64 entries of one neighbour's row per step; the steps of the four wavefronts
// run in lock step (a step adds at most 256 entries to the list, which is drained before it could overflow).  cnt[i] =
// above, tied, ncand of pair i; every combination is of integers.
__global__ __launch_bounds__(256) void k_nbr_rank(uint32_t np, uint32_t n, uint32_t words, const uint64_t *__restrict__ rowptr,
                                                  const uint32_t *__restrict__ scol, const double *__restrict__ w,
                                                  const uint32_t *__restrict__ pairs, uint32_t *__restrict__ bitmap,
                                                  double *__restrict__ score, uint32_t *__restrict__ cnt) {
  __shared__ uint32_t list[LIST_CAP];
  __shared__ uint32_t lcount;
  __shared__ uint32_t tot[3];
  const uint32_t t = threadIdx.x, wv = t >> 6, lane = t & 63;
  uint32_t *bm = bitmap + (size_t)blockIdx.x * words;
  for (uint32_t i = blockIdx.x; i < np; i += gridDim.x) {
    const uint32_t p = pairs[2 * i], q = pairs[2 * i + 1];
    const uint64_t pb = rowptr[p], pe = rowptr[p + 1];
    const uint32_t dp = (uint32_t)(pe - pb);
    if (t == 0) lcount = 0;
    if (t < 3) tot[t] = 0;
    uint32_t cm;
    const double s = nbr_pair(rowptr, scol, w, p, q, lane, &cm);
    __syncthreads();
    uint32_t above = 0, tied = 0, seen = 0;
    uint32_t zi = wv;
    uint64_t off = 0;
    for (;;) {
      const bool have = zi < dp;
      if (have) {
        const uint32_t z = scol[pb + zi];
        const uint64_t zb = rowptr[z], ze = rowptr[z + 1];
        bool keep = false;
        uint32_t c = NONE;
        if (zb + off + lane < ze) {
          c = scol[zb + off + lane];
          const uint32_t bit = 1u << (c & 31);
          const bool first = !(atomicOr(bm + (c >> 5), bit) & bit);
          keep = first && c != p && c != q && !in_row(scol, pb, pe, c);
        }
        const unsigned long long mask = __ballot(keep);
        if (mask) {
          uint32_t base = 0;
          if (lane == 0) base = atomicAdd(&lcount, (uint32_t)__popcll(mask));
          base = __builtin_amdgcn_readfirstlane(base);
          if (keep) list[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1))] = c;
        }
        off += 64;
        if (zb + off >= ze) { zi += 4; off = 0; }
      }
      const bool more = __syncthreads_or(have);
      const uint32_t nl = lcount;
      __syncthreads();   // everybody has read the count before the next step adds to it
      if (!more || nl > LIST_CAP - 256) drain(rowptr, scol, w, p, s, list, &lcount, nl, wv, lane, &above, &tied, &seen);
      if (!more) break;
    }
    // the same walk again, to clear the words that hold a claimed bit.  The barriers of the last drain put every claim
    // before these clears, the barrier at the end of the pair puts them before the next pair's claims (the bitmap is the
    // block's own).  One atomic per entry again, like the claims: the price of not remembering which words were touched.
    for (uint32_t y = wv; y < dp; y += 4) {
      const uint32_t z = scol[pb + y];
      const uint64_t ze = rowptr[z + 1];
      for (uint64_t e = rowptr[z] + lane; e < ze; e += 64) atomicAnd(bm + (scol[e] >> 5), 0u);
    }
    if (lane == 0) {
      atomicAdd(&tot[0], above);
      atomicAdd(&tot[1], tied);
      atomicAdd(&tot[2], seen);
    }
    __syncthreads();
    if (t == 0) {
      // candidates of p other than q: every node but p, p's neighbours and q.  Those not seen have no common neighbour
      // with p: they score exactly 0, the seen ones above 0.
      const uint32_t nc = n - 1 - dp - (in_row(scol, pb, pe, q) ? 0u : 1u);
      cnt[3 * (size_t)i] = tot[0];
      cnt[3 * (size_t)i + 1] = tot[1] + (s == 0.0 ? nc - tot[2] : 0u);
      cnt[3 * (size_t)i + 2] = nc;
      score[i] = s;
    }
    __syncthreads();
  }
}

// the refusals of both entry points (include/svils.h): those of svils_link_prob, without the state
int check(svils_handle *h, const char *name, int measure, const uint32_t *pairs, uint64_t npairs) {
  if (int rc = check_pair_handle(h, name, false)) return rc;
  if (measure != SVILS_NBR_CN && measure != SVILS_NBR_AA && measure != SVILS_NBR_RA)
    return fail(SVILS_ERR_ARG, "%s: unknown measure %d", name, measure);
  return check_pairs(h, name, pairs, npairs);
}

// w[d] for d = 0 .. the largest training degree, once per handle and measure.  Host arithmetic: 1.0 / std::log((double)d)
// is the value any caller can restate (the device's logarithm is another function).
int build_weights(svils_handle *h, int measure) {
  svils_handle::NbrScratch &s = h->nbr;
  if (s.w[measure]) return 0;
  uint64_t maxdeg = 0;
  for (uint32_t x = 0; x < h->geo.n; ++x) maxdeg = std::max(maxdeg, h->h_rowptr[x + 1] - h->h_rowptr[x]);
  std::vector<double> w(maxdeg + 1, 0.0);
  for (uint64_t d = 2; d <= maxdeg; ++d)
    w[d] = measure == SVILS_NBR_CN ? 1.0 : measure == SVILS_NBR_AA ? 1.0 / std::log((double)d) : 1.0 / (double)d;
  if (int rc = dalloc(h, &s.w[measure], w.size(), false)) return rc;
  HIPCHK(hipMemcpyAsync(s.w[measure], w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));   // w leaves scope
  return 0;
}

// sorted rows, the weights, and room for a batch of `m` pairs
int prepare(svils_handle *h, int measure, uint64_t m) {
  if (int rc = sorted_rows(h)) return rc;
  if (int rc = build_weights(h, measure)) return rc;
  svils_handle::NbrScratch &s = h->nbr;
  if (int rc = reserve(h, s.pairs, 2 * m)) return rc;
  if (int rc = reserve(h, s.score, m)) return rc;
  return reserve(h, s.cnt, 3 * m);
}

}  // namespace

extern "C" {

int svils_nbr_score(svils_handle *h, int measure, const uint32_t *pairs, uint64_t npairs, double *score, uint32_t *common) {
  if (int rc = check(h, "svils_nbr_score", measure, pairs, npairs)) return rc;
  if (!npairs) return 0;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (int rc = prepare(h, measure, std::min(npairs, NBR_BATCH))) return rc;
  svils_handle::NbrScratch &s = h->nbr;
  for (uint64_t b = 0; b < npairs; b += NBR_BATCH) {
    const uint32_t m = (uint32_t)std::min(NBR_BATCH, npairs - b);
    HIPCHK(hipMemcpyAsync(s.pairs.p, pairs + 2 * b, 2 * (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_nbr_pairs, dim3((m + 3) / 4), dim3(256), 0, h->stream, m, h->d.rowptr, h->pred.scol, s.w[measure],
                       s.pairs.p, s.score.p, s.cnt.p);
    HIPCHK(hipGetLastError());
    if (score) HIPCHK(hipMemcpyAsync(score + b, s.score.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (common) HIPCHK(hipMemcpyAsync(common + b, s.cnt.p, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

int svils_nbr_rank(svils_handle *h, int measure, const uint32_t *pairs, uint64_t npairs, uint32_t *above, uint32_t *tied,
                   uint32_t *ncand, double *score) {
  if (int rc = check(h, "svils_nbr_rank", measure, pairs, npairs)) return rc;
  if (!npairs) return 0;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (int rc = prepare(h, measure, std::min(npairs, NBR_BATCH))) return rc;
  svils_handle::NbrScratch &s = h->nbr;
  const uint32_t n = h->geo.n, words = (n + 31) / 32;
  if (!s.bitmap) {
    s.blocks = BLOCKS_PER_CU * cu_count(h->cfg.device);
    if (int rc = dalloc(h, &s.bitmap, (size_t)s.blocks * words, true)) return rc;   // zeroed once; every launch leaves it so
  }
  for (uint64_t b = 0; b < npairs; b += NBR_BATCH) {
    const uint32_t m = (uint32_t)std::min(NBR_BATCH, npairs - b);
    HIPCHK(hipMemcpyAsync(s.pairs.p, pairs + 2 * b, 2 * (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_nbr_rank, dim3(std::min(m, s.blocks)), dim3(256), 0, h->stream, m, n, words, h->d.rowptr, h->pred.scol,
                       s.w[measure], s.pairs.p, s.bitmap, s.score.p, s.cnt.p);
    HIPCHK(hipGetLastError());
    if (int rc = fetch_ranks(h->stream, s.cnt.p, s.score.p, m, b, above, tied, ncand, score)) return rc;
  }
  return 0;
}

}  // extern "C"
