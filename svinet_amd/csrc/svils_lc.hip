// svils_lc.hip -- -gml / -lcstats on the device: the link communities of a fitted model, the reference's
// MMSBGen::get_lc_stats and MMSBGen::gml (src/mmsbgen.cc:181-193, 230-285, 418-499, 700-729, 911-961).
//
//   k_beta        estimate_beta (src/mmsbgen.hh:213-222): beta_k = l0 / (l0 + l1)
//   k_node        one block per 256 nodes, the rows staged through LDS in tiles of TK columns (coalesced reads, any K):
//                 every lane sums its own row in k order (estimate_all, :700-716), writes pi = gamma / s over gamma in
//                 place, and takes most_likely_group (mmsbgen.hh:112-123) and bridgeness (:230-241) in k order
//   k_link        one wavefront per link, lanes across k (16-byte loads when K is even): x_k = (pi_p pi_q) beta_k, the
//                 first strict maximum u / idx by an exact wave reduction (max, then lowest index), s by a fixed tree
//                 (inner_prod_max, src/matrix.hh:460-476).  Links whose ratio u / s lies within 2 K eps ratio of 0.5 or
//                 0.9 -- the only ones whose decision can depend on the order of s -- go to a compacted list
//   k_recheck     those links again, one lane each, s in the reference's sequential k order
//   k_comm        per community: nodes, sum of degrees and (max, smallest node) as one 64-bit max, over deg_c columns
//   k_node_counts per node: memberships (#k with deg_c > 0) and influence deg_c[i][group]
//   k_gml_*       the GML edge list: an order-preserving compaction of the links (kept sorted by (p, q)) that pass 0.9
//
// Counts are integers, so the atomics of deg_c and of the community reductions are deterministic.
#include "svils_tool.h"

// No fused multiply-adds in this unit: the reference computes every product and sum separately (x86, no contraction);
// a contracted (pi_p pi_q) beta or (pi - 1/K)^2 + v changes the last bit of a ratio or a bridgeness.
#pragma clang fp contract(off)

namespace {

constexpr uint32_t TK = 16;               // columns per LDS tile of k_node (256 rows x 17 doubles = 34 KB)
constexpr uint32_t COMM_ROWS = 1024;      // rows per block of k_comm
constexpr uint32_t NONE = 0xffffffffu;
constexpr uint8_t F_JOIN = 1, F_GML = 2, F_BAND = 4;

__global__ __launch_bounds__(256) void k_beta(uint32_t K, const double *__restrict__ lam, double *__restrict__ beta) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k < K) beta[k] = lam[2 * k] / (lam[2 * k] + lam[2 * k + 1]);
}

__global__ __launch_bounds__(256) void k_node(uint32_t n, uint32_t K, double *__restrict__ pi, const uint32_t *__restrict__ deg,
                                              uint32_t *__restrict__ group, double *__restrict__ bridg) {
  __shared__ double tile[256][TK + 1];
  const uint32_t r0 = blockIdx.x * 256, t = threadIdx.x;
  const uint32_t rows = min(256u, n - r0);
  double s = 0;
  for (uint32_t k0 = 0; k0 < K; k0 += TK) {
    const uint32_t kw = min(TK, K - k0);
    for (uint32_t e = t; e < rows * kw; e += 256) {
      const uint32_t r = e / kw, c = e - r * kw;
      tile[r][c] = pi[(size_t)(r0 + r) * K + k0 + c];
    }
    __syncthreads();
    if (t < rows)
      for (uint32_t c = 0; c < kw; ++c) s += tile[t][c];
    __syncthreads();
  }
  const double inv = 1.0 / (double)K;
  double v = 0, mx = 0;
  uint32_t g = 0;
  for (uint32_t k0 = 0; k0 < K; k0 += TK) {
    const uint32_t kw = min(TK, K - k0);
    for (uint32_t e = t; e < rows * kw; e += 256) {
      const uint32_t r = e / kw, c = e - r * kw;
      tile[r][c] = pi[(size_t)(r0 + r) * K + k0 + c];
    }
    __syncthreads();
    if (t < rows)
      for (uint32_t c = 0; c < kw; ++c) {
        const double p = tile[t][c] / s;
        tile[t][c] = p;
        if (p > mx) {
          mx = p;
          g = k0 + c;
        }
        const double d = p - inv;
        v += d * d;
      }
    __syncthreads();
    for (uint32_t e = t; e < rows * kw; e += 256) {
      const uint32_t r = e / kw, c = e - r * kw;
      pi[(size_t)(r0 + r) * K + k0 + c] = tile[r][c];
    }
    __syncthreads();
  }
  if (t < rows) {
    group[r0 + t] = g;
    bridg[r0 + t] = (1 - sqrt(v * (double)K / (double)(K - 1))) * (double)deg[r0 + t];
  }
}

__device__ inline void decide(uint32_t p, uint32_t q, uint32_t K, double ratio, uint32_t idx, uint8_t extra, uint8_t *flags, uint64_t x,
                              uint32_t *__restrict__ degc) {
  // lc_current_draw_helper: `max < 0.5` leaves the link out; gml: `max < 0.9` is no edge.  A NaN ratio passes both.
  const bool join = !(ratio < 0.5), gml = !(ratio < 0.9);
  flags[x] = (uint8_t)((join ? F_JOIN : 0) | (gml ? F_GML : 0) | extra);
  if (join) {
    atomicAdd(&degc[(size_t)p * K + idx], 1u);
    atomicAdd(&degc[(size_t)q * K + idx], 1u);
  }
}

// one link per wavefront, four per block
template <bool VEC>
__global__ __launch_bounds__(256) void k_link(uint64_t E, uint32_t K, const uint32_t *__restrict__ links, const double *__restrict__ pi,
                                              const double *__restrict__ beta, double band, uint32_t *__restrict__ colour,
                                              uint8_t *__restrict__ flags, uint32_t *__restrict__ blist, uint32_t *__restrict__ counters,
                                              uint32_t *__restrict__ degc) {
  const uint64_t x = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (x >= E) return;   // whole wavefronts leave together
  const uint32_t p = links[2 * x], q = links[2 * x + 1];
  const double *a = pi + (size_t)p * K, *b = pi + (size_t)q * K;
  double s = 0, u = 0;
  uint32_t idx = NONE;
  if (VEC) {   // K even: rows are 16-byte aligned
    const double2 *a2 = (const double2 *)a, *b2 = (const double2 *)b, *c2 = (const double2 *)beta;
    for (uint32_t j = lane; j < K / 2; j += 64) {
      const double2 va = a2[j], vb = b2[j], vc = c2[j];
      const double x0 = (va.x * vb.x) * vc.x, x1 = (va.y * vb.y) * vc.y;
      s += x0;
      s += x1;
      if (x0 > u) { u = x0; idx = 2 * j; }
      if (x1 > u) { u = x1; idx = 2 * j + 1; }
    }
  } else {
    for (uint32_t k = lane; k < K; k += 64) {
      const double v = (a[k] * b[k]) * beta[k];
      s += v;
      if (v > u) { u = v; idx = k; }
    }
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  double m = u;
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  uint32_t w = (u == m) ? idx : NONE;   // the lowest index holding the maximum: the reference's first strict maximum
  for (int o = 32; o > 0; o >>= 1) w = min(w, (uint32_t)__shfl_xor((int)w, o, 64));
  if (lane != 0) return;
  if (w == NONE) w = 0;   // nothing beat 0 (all terms 0): idx stays 0, the ratio is 0 / 0
  colour[x] = w;
  const double ratio = m / s;
  const double tol = band * ratio;
  if (fabs(ratio - 0.5) <= tol || fabs(ratio - 0.9) <= tol) {
    blist[atomicAdd(&counters[0], 1u)] = (uint32_t)x;
    return;
  }
  decide(p, q, K, ratio, w, 0, flags, x, degc);
}

// the band links again, s in k order
__global__ __launch_bounds__(256) void k_recheck(const uint32_t *cnt, uint32_t K, const uint32_t *__restrict__ links,
                                                 const double *__restrict__ pi, const double *__restrict__ beta,
                                                 const uint32_t *__restrict__ blist, const uint32_t *__restrict__ colour,
                                                 uint8_t *__restrict__ flags, uint32_t *counters, uint32_t *__restrict__ degc) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= cnt[0]) return;
  const uint32_t x = blist[j], p = links[2 * (size_t)x], q = links[2 * (size_t)x + 1];
  const double *a = pi + (size_t)p * K, *b = pi + (size_t)q * K;
  double s = 0, u = 0;
  for (uint32_t k = 0; k < K; ++k) {
    const double v = (a[k] * b[k]) * beta[k];
    s += v;
    u = v > u ? v : u;
  }
  decide(p, q, K, u / s, colour[x], F_BAND, flags, x, degc);
}

// grid (ceil(K / 256), ceil(n / COMM_ROWS)): thread = column, a range of rows
__global__ __launch_bounds__(256) void k_comm(uint32_t n, uint32_t K, const uint32_t *__restrict__ degc, uint32_t *__restrict__ cnodes,
                                              unsigned long long *__restrict__ csum, unsigned long long *__restrict__ ckey) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const uint32_t i0 = blockIdx.y * COMM_ROWS, i1 = min(n, i0 + COMM_ROWS);
  uint32_t nodes = 0;
  unsigned long long sum = 0, key = 0;
  for (uint32_t i = i0; i < i1; ++i) {
    const uint32_t c = degc[(size_t)i * K + k];
    if (!c) continue;
    nodes++;
    sum += c;
    const unsigned long long kk = ((unsigned long long)c << 32) | (unsigned long long)(NONE - i);   // count desc, node asc
    key = kk > key ? kk : key;
  }
  if (nodes) {
    atomicAdd(&cnodes[k], nodes);
    atomicAdd(&csum[k], sum);
    atomicMax(&ckey[k], key);
  }
}

// one node per wavefront
__global__ __launch_bounds__(256) void k_node_counts(uint32_t n, uint32_t K, const uint32_t *__restrict__ degc,
                                                     const uint32_t *__restrict__ group, uint32_t *__restrict__ memb,
                                                     uint32_t *__restrict__ infl) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const uint32_t *row = degc + (size_t)i * K;
  uint32_t c = 0;
  for (uint32_t k = lane; k < K; k += 64) c += row[k] ? 1u : 0u;
  for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o, 64);
  if (lane == 0) {
    memb[i] = c;
    infl[i] = row[group[i]];
  }
}

// the GML edges: per block of 256 links its count, one block scans the counts, then every block writes its edges.  The
// count of links left out (ratio < 0.5) is summed here too: one atomic per block, not one per link
__global__ __launch_bounds__(256) void k_gml_count(uint64_t E, const uint8_t *__restrict__ flags, uint32_t *__restrict__ bcnt,
                                                   uint32_t *__restrict__ unlikely) {
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint8_t fl = x < E ? flags[x] : (uint8_t)F_JOIN;
  const int c = __syncthreads_count((fl & F_GML) != 0);
  const int u = __syncthreads_count(!(fl & F_JOIN));
  if (threadIdx.x == 0) {
    bcnt[blockIdx.x] = (uint32_t)c;
    if (u) atomicAdd(unlikely, (uint32_t)u);
  }
}

__global__ __launch_bounds__(1024) void k_gml_scan(uint32_t nb, const uint32_t *__restrict__ bcnt, unsigned long long *__restrict__ boff,
                                                   unsigned long long *__restrict__ total) {
  __shared__ unsigned long long part[1024];
  const uint32_t t = threadIdx.x, per = (nb + 1023) / 1024;
  const uint32_t b0 = min(nb, t * per), b1 = min(nb, b0 + per);
  unsigned long long s = 0;
  for (uint32_t b = b0; b < b1; ++b) s += bcnt[b];
  part[t] = s;
  __syncthreads();
  for (uint32_t o = 1; o < 1024; o <<= 1) {   // inclusive scan of the thread totals
    const unsigned long long v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  unsigned long long off = part[t] - s;
  for (uint32_t b = b0; b < b1; ++b) {
    boff[b] = off;
    off += bcnt[b];
  }
  if (t == 1023) total[0] = part[1023];
}

__global__ __launch_bounds__(256) void k_gml_write(uint64_t E, const uint8_t *__restrict__ flags, const uint32_t *__restrict__ links,
                                                   const uint32_t *__restrict__ colour, const unsigned long long *__restrict__ boff,
                                                   uint32_t *__restrict__ out) {
  __shared__ uint32_t wtot[4];
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool f = x < E && (flags[x] & F_GML);
  const uint64_t mask = __ballot(f);
  if (lane == 0) wtot[wv] = (uint32_t)__popcll(mask);
  __syncthreads();
  if (!f) return;
  uint64_t pos = boff[blockIdx.x] + (uint64_t)__popcll(mask & ((1ull << lane) - 1));
  for (uint32_t w = 0; w < wv; ++w) pos += wtot[w];
  out[3 * pos] = links[2 * x];
  out[3 * pos + 1] = links[2 * x + 1];
  out[3 * pos + 2] = colour[x];
}

}  // namespace

// events ev[4]: node pass, link pass (+ recheck), counts (+ GML list), end
struct svils_lc : ToolHandle {
  uint32_t n = 0, k = 0;
  bool timed = false;
  uint64_t E = 0;
  // graph (GRAPH scope): links sorted by (p, q); order[x] = the caller's index of sorted link x
  uint32_t *links = nullptr, *deg = nullptr;
  std::vector<uint32_t> order;
  bool identity = true;                  // the caller's links were sorted already
  uint32_t *colour = nullptr, *blist = nullptr, *bcnt = nullptr, *gml = nullptr;   // per link / per block of 256 links
  uint8_t *flags = nullptr;
  unsigned long long *boff = nullptr;
  // model / results (HANDLE scope)
  double *pi = nullptr, *lam = nullptr, *beta = nullptr, *bridg = nullptr;
  uint32_t *group = nullptr, *memb = nullptr, *infl = nullptr, *degc = nullptr, *counters = nullptr;
  uint32_t *cnodes = nullptr;
  unsigned long long *csum = nullptr, *ckey = nullptr, *gtotal = nullptr;
  bool have_graph = false, have_model = false, done = false;
  uint64_t n_gml = 0, n_band = 0, n_unlikely = 0;
};

namespace {

void free_graph(svils_lc *h) {
  h->release(ToolHandle::GRAPH);
  h->have_graph = h->done = false;
}

int check_done(svils_lc *h, const char *name) {
  if (int rc = check(h, name)) return rc;
  if (!h->done) return fail(SVILS_ERR_ARG, "%s: svils_lc_run has not run on the current graph and model", name);
  HIPCHK(hipStreamSynchronize(h->st));
  return 0;
}

}  // namespace

extern "C" {

int svils_lc_create(int device, uint32_t n, uint32_t k, svils_lc **out) {
  if (!out) return fail(SVILS_ERR_ARG, "svils_lc_create: null argument");
  *out = nullptr;
  if (int rc = open_device(device, n < 1 || k < 2 ? "svils_lc_create: need n >= 1 and k >= 2" : nullptr)) return rc;
  svils_lc *h = new (std::nothrow) svils_lc();
  if (!h) return fail(SVILS_ERR_NOMEM, "out of host memory");
  h->n = n;
  h->k = k;
  const auto scope = ToolHandle::HANDLE;
  const size_t nk = (size_t)n * k;
  int rc = h->open(device, 4);
  if (!rc) rc = h->dalloc(scope, &h->pi, nk);
  if (!rc) rc = h->dalloc(scope, &h->degc, nk);
  if (!rc) rc = h->dalloc(scope, &h->lam, 2 * (size_t)k);
  if (!rc) rc = h->dalloc(scope, &h->beta, (size_t)k + 1);
  if (!rc) rc = h->dalloc(scope, &h->bridg, (size_t)n);
  if (!rc) rc = h->dalloc(scope, &h->group, (size_t)n);
  if (!rc) rc = h->dalloc(scope, &h->memb, (size_t)n);
  if (!rc) rc = h->dalloc(scope, &h->infl, (size_t)n);
  if (!rc) rc = h->dalloc(scope, &h->cnodes, (size_t)k);
  if (!rc) rc = h->dalloc(scope, &h->csum, (size_t)k);
  if (!rc) rc = h->dalloc(scope, &h->ckey, (size_t)k);
  if (!rc) rc = h->dalloc(scope, &h->counters, 2);
  if (!rc) rc = h->dalloc(scope, &h->gtotal, 1);
  if (rc) {
    svils_lc_destroy(h);
    return rc;
  }
  *out = h;
  return 0;
}

int svils_lc_destroy(svils_lc *h) {
  delete h;   // ~ToolHandle: waits for the stream, frees both scopes
  return 0;
}

int svils_lc_set_graph(svils_lc *h, const uint32_t *links, uint64_t nlinks) {
  if (int rc = check(h, "svils_lc_set_graph")) return rc;
  if (nlinks && !links) return fail(SVILS_ERR_ARG, "svils_lc_set_graph: null argument");
  if (nlinks >= NONE) return fail(SVILS_ERR_UNSUPPORTED, "svils_lc_set_graph: %llu links (at most 2^32 - 2)", (unsigned long long)nlinks);
  const uint32_t n = h->n;
  bool sorted = true;
  for (uint64_t x = 0; x < nlinks; ++x) {
    const uint32_t p = links[2 * x], q = links[2 * x + 1];
    if (p >= q || q >= n)
      return fail(SVILS_ERR_ARG, "svils_lc_set_graph: link %llu (%u, %u) is not p < q < n = %u", (unsigned long long)x, p, q, n);
    if (x && (links[2 * x - 2] > p || (links[2 * x - 2] == p && links[2 * x - 1] >= q))) sorted = false;
  }
  HIPCHK(hipStreamSynchronize(h->st));
  free_graph(h);
  std::vector<uint32_t> deg(n, 0), sl;
  for (uint64_t x = 0; x < 2 * nlinks; ++x) deg[links[x]]++;
  h->order.clear();
  h->identity = sorted;
  const uint32_t *src = links;
  if (!sorted) {   // (p, q) order: the GML edge order; the caller's order comes back through h->order
    std::vector<uint64_t> key(nlinks);
    for (uint64_t x = 0; x < nlinks; ++x) key[x] = ((uint64_t)links[2 * x] << 32) | links[2 * x + 1];
    h->order.resize(nlinks);
    for (uint64_t x = 0; x < nlinks; ++x) h->order[x] = (uint32_t)x;
    std::sort(h->order.begin(), h->order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    sl.resize(2 * nlinks);
    for (uint64_t x = 0; x < nlinks; ++x) {
      sl[2 * x] = links[2 * (size_t)h->order[x]];
      sl[2 * x + 1] = links[2 * (size_t)h->order[x] + 1];
    }
    src = sl.data();
  }
  const uint64_t nb = std::max<uint64_t>(blocks(nlinks, 256), 1);
  const auto scope = ToolHandle::GRAPH;
  int rc = 0;
  if (!rc) rc = h->dalloc(scope, &h->links, 2 * nlinks);
  if (!rc) rc = h->dalloc(scope, &h->deg, (size_t)n);
  if (!rc) rc = h->dalloc(scope, &h->colour, nlinks);
  if (!rc) rc = h->dalloc(scope, &h->flags, nlinks);
  if (!rc) rc = h->dalloc(scope, &h->blist, nlinks);
  if (!rc) rc = h->dalloc(scope, &h->gml, 3 * nlinks);
  if (!rc) rc = h->dalloc(scope, &h->bcnt, nb);
  if (!rc) rc = h->dalloc(scope, &h->boff, nb);
  if (!rc && nlinks && hipMemcpy(h->links, src, 2 * nlinks * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(SVILS_ERR_DEVICE, "svils_lc_set_graph: upload failed");
  if (!rc && hipMemcpy(h->deg, deg.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(SVILS_ERR_DEVICE, "svils_lc_set_graph: upload failed");
  if (rc) {
    free_graph(h);
    return rc;
  }
  h->E = nlinks;
  h->have_graph = true;
  return 0;
}

int svils_lc_set_model(svils_lc *h, const double *gamma, const double *lambda) {
  if (int rc = check(h, "svils_lc_set_model")) return rc;
  if (!gamma || !lambda) return fail(SVILS_ERR_ARG, "svils_lc_set_model: null argument");
  HIPCHK(hipStreamSynchronize(h->st));
  HIPCHK(hipMemcpy(h->pi, gamma, (size_t)h->n * h->k * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->lam, lambda, 2 * (size_t)h->k * sizeof(double), hipMemcpyHostToDevice));
  h->have_model = true;
  h->done = false;
  return 0;
}

int svils_lc_run(svils_lc *h) {
  if (int rc = check(h, "svils_lc_run")) return rc;
  if (!h->have_graph || !h->have_model) return fail(SVILS_ERR_ARG, "svils_lc_run: set the graph and the model first");
  const uint32_t n = h->n, K = h->k;
  const uint64_t E = h->E;
  hipStream_t st = h->st;
  // node pass: pi replaces gamma in place (set the model again before another run)
  HIPCHK(hipEventRecord(h->ev[0], st));
  hipLaunchKernelGGL(k_beta, dim3(blocks(K, 256)), dim3(256), 0, st, K, h->lam, h->beta);
  hipLaunchKernelGGL(k_node, dim3(blocks(n, 256)), dim3(256), 0, st, n, K, h->pi, h->deg, h->group, h->bridg);
  HIPCHK(hipGetLastError());
  h->have_model = false;
  HIPCHK(hipEventRecord(h->ev[1], st));
  // link pass
  HIPCHK(hipMemsetAsync(h->degc, 0, (size_t)n * K * sizeof(uint32_t), st));
  HIPCHK(hipMemsetAsync(h->counters, 0, 2 * sizeof(uint32_t), st));
  const double band = 2.0 * (double)K * 2.220446049250313e-16;   // 2 K DBL_EPSILON
  if (E) {
    if (K % 2 == 0)
      hipLaunchKernelGGL(k_link<true>, dim3(blocks(E, 4)), dim3(256), 0, st, E, K, h->links, h->pi, h->beta, band, h->colour, h->flags,
                         h->blist, h->counters, h->degc);
    else
      hipLaunchKernelGGL(k_link<false>, dim3(blocks(E, 4)), dim3(256), 0, st, E, K, h->links, h->pi, h->beta, band, h->colour, h->flags,
                         h->blist, h->counters, h->degc);
    HIPCHK(hipGetLastError());
    // the band list has at most E entries; blocks past the count leave at once
    hipLaunchKernelGGL(k_recheck, dim3(blocks(E, 256)), dim3(256), 0, st, h->counters, K, h->links, h->pi, h->beta, h->blist, h->colour,
                       h->flags, h->counters, h->degc);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(h->ev[2], st));
  // counts
  HIPCHK(hipMemsetAsync(h->cnodes, 0, (size_t)K * sizeof(uint32_t), st));
  HIPCHK(hipMemsetAsync(h->csum, 0, (size_t)K * sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(h->ckey, 0, (size_t)K * sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(h->gtotal, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_comm, dim3(blocks(K, 256), blocks(n, COMM_ROWS)), dim3(256), 0, st, n, K, h->degc, h->cnodes, h->csum, h->ckey);
  hipLaunchKernelGGL(k_node_counts, dim3(blocks(n, 4)), dim3(256), 0, st, n, K, h->degc, h->group, h->memb, h->infl);
  HIPCHK(hipGetLastError());
  if (E) {
    const uint32_t nb = blocks(E, 256);
    hipLaunchKernelGGL(k_gml_count, dim3(nb), dim3(256), 0, st, E, h->flags, h->bcnt, h->counters + 1);
    hipLaunchKernelGGL(k_gml_scan, dim3(1), dim3(1024), 0, st, nb, h->bcnt, h->boff, h->gtotal);
    hipLaunchKernelGGL(k_gml_write, dim3(nb), dim3(256), 0, st, E, h->flags, h->links, h->colour, h->boff, h->gml);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(h->ev[3], st));
  uint32_t c[2] = {0, 0};
  unsigned long long g = 0;
  HIPCHK(hipMemcpyAsync(c, h->counters, sizeof c, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&g, h->gtotal, sizeof g, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  h->n_band = c[0];
  h->n_unlikely = c[1];
  h->n_gml = g;
  h->done = h->timed = true;
  return 0;
}

int svils_lc_get_nodes(svils_lc *h, uint32_t *group, double *bridgeness, uint32_t *memberships, uint32_t *influence) {
  if (int rc = check_done(h, "svils_lc_get_nodes")) return rc;
  const size_t n = h->n;
  if (group) HIPCHK(hipMemcpy(group, h->group, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (bridgeness) HIPCHK(hipMemcpy(bridgeness, h->bridg, n * sizeof(double), hipMemcpyDeviceToHost));
  if (memberships) HIPCHK(hipMemcpy(memberships, h->memb, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (influence) HIPCHK(hipMemcpy(influence, h->infl, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

int svils_lc_get_degrees(svils_lc *h, uint32_t *deg_c) {
  if (int rc = check_done(h, "svils_lc_get_degrees")) return rc;
  if (!deg_c) return fail(SVILS_ERR_ARG, "svils_lc_get_degrees: null argument");
  HIPCHK(hipMemcpy(deg_c, h->degc, (size_t)h->n * h->k * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

int svils_lc_get_pi(svils_lc *h, double *pi) {
  if (int rc = check_done(h, "svils_lc_get_pi")) return rc;
  if (!pi) return fail(SVILS_ERR_ARG, "svils_lc_get_pi: null argument");
  HIPCHK(hipMemcpy(pi, h->pi, (size_t)h->n * h->k * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int svils_lc_get_communities(svils_lc *h, uint32_t *nodes, uint64_t *degsum, uint32_t *max, uint32_t *argmax) {
  if (int rc = check_done(h, "svils_lc_get_communities")) return rc;
  const size_t K = h->k;
  std::vector<uint32_t> cn(K);
  std::vector<unsigned long long> key(K);
  HIPCHK(hipMemcpy(cn.data(), h->cnodes, K * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (nodes) memcpy(nodes, cn.data(), K * sizeof(uint32_t));
  if (degsum) HIPCHK(hipMemcpy(degsum, h->csum, K * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(key.data(), h->ckey, K * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  for (size_t k = 0; k < K; ++k) {   // an empty community: max 0, node 0 (Community::deg_stats never assigns them)
    if (max) max[k] = cn[k] ? (uint32_t)(key[k] >> 32) : 0;
    if (argmax) argmax[k] = cn[k] ? NONE - (uint32_t)key[k] : 0;
  }
  return 0;
}

int svils_lc_get_links(svils_lc *h, uint32_t *colour, uint8_t *flags, uint64_t counts[3]) {
  if (int rc = check_done(h, "svils_lc_get_links")) return rc;
  const uint64_t E = h->E;
  if (counts) {
    counts[0] = h->n_unlikely;
    counts[1] = h->n_gml;
    counts[2] = h->n_band;
  }
  if (!E || (!colour && !flags)) return 0;
  std::vector<uint32_t> c(colour ? E : 0);
  std::vector<uint8_t> f(flags ? E : 0);
  if (colour) HIPCHK(hipMemcpy(c.data(), h->colour, E * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (flags) HIPCHK(hipMemcpy(f.data(), h->flags, E, hipMemcpyDeviceToHost));
  for (uint64_t x = 0; x < E; ++x) {
    const uint64_t to = h->identity ? x : h->order[x];
    if (colour) colour[to] = c[x];
    if (flags) flags[to] = f[x];
  }
  return 0;
}

int svils_lc_get_gml(svils_lc *h, uint64_t *count, uint32_t *edges) {
  if (int rc = check_done(h, "svils_lc_get_gml")) return rc;
  if (count) *count = h->n_gml;
  if (edges && h->n_gml) HIPCHK(hipMemcpy(edges, h->gml, 3 * h->n_gml * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

int svils_lc_get_timing(svils_lc *h, double ms[3]) {
  if (int rc = check(h, "svils_lc_get_timing")) return rc;
  if (!ms) return fail(SVILS_ERR_ARG, "svils_lc_get_timing: null argument");
  HIPCHK(hipStreamSynchronize(h->st));
  for (int p = 0; p < 3; ++p) ms[p] = h->elapsed_ms(p, p + 1, h->timed);
  return 0;
}

}  // extern "C"
