// svils_findk.hip -- -findk on the device: the reference's FastInit::batch_infer (src/fastinit.cc:240-289), a label
// propagation over a top-5 sparse gamma.  Every node holds 5 (label, value) slots; slot 0's label is its current label.
//
//   k_top_wave      nodes of training degree <= 64, one wavefront each: the neighbours' labels in lanes, a bitonic sort
//                   across the wavefront, run lengths from a ballot of the run heads, then 5 rounds of a wave arg-max
//                   over (count desc, label asc)
//   k_top_block     larger nodes, one block each: an open-addressing hash (label -> count) in LDS (degree <= 2048) or in
//                   global scratch (hubs, any degree up to n - 1), then every thread's private top 5 over its slots and
//                   5 rounds of a block arg-max
//   k_compact       nodes with 1 .. 4 distinct labels: (node, count, labels) records for the host's padding draws
//   k_apply         set_gamma (src/fastinit.cc:200-236): counted slots get count + alpha, pads (k_pads) 2 alpha
//   k_pi            estimate_all_pi (src/fastinit.hh:460-476)
//   k_edge_ll       edge_likelihood (src/fastinit.cc:416-446) of links (y = 1) or held-out pairs
//   k_part_sum      fixed-order sums: 4096 items per block, then one block over the partials (deterministic run to run)
//   k_groups        compute_and_log_groups (src/fastinit.cc:291-414): both directions of every link; the winning label is
//                   one of each endpoint's 5 slots, so membership is a 5-bit mask per node (atomicOr)
//
// The sort order (count desc, label asc) is what the reference's qsort with cmppairval gives over a std::map's ascending
// labels under glibc's merge sort: a stable descending sort.
#include "svils_tool.h"
#include "svils_waveutil.h"

// No fused multiply-adds in this unit: the reference computes every product and sum separately (x86, no contraction);
// an FMA inside `u > max` compares the exact product and moves the winning label of a tie in compute_and_log_groups.
#pragma clang fp contract(off)

namespace {

constexpr uint32_t S = 5;                  // slots per node (FastInit::_k)
constexpr uint32_t NONE = 0xffffffffu;
constexpr uint32_t WAVE_MAX = 64;          // degrees up to this: k_top_wave
constexpr uint32_t LDS_SLOTS = 4096;       // hash slots in LDS (32 KB): degrees up to LDS_SLOTS / 2 take k_top_block<true>
constexpr uint32_t SUM_CHUNK = 4096;       // items per partial sum
constexpr uint32_t SENTINEL = 65535;       // compute_and_log_groups drops a label equal to its "no maximum" value

__device__ inline uint64_t key_of(uint32_t count, uint32_t label) { return ((uint64_t)count << 32) | (uint64_t)(NONE - label); }
__device__ inline uint32_t label_of(uint64_t key) { return NONE - (uint32_t)key; }

// nodes[] of training degree 1 .. 64; four per block of 256
__global__ __launch_bounds__(256) void k_top_wave(uint32_t cnt, const uint32_t *__restrict__ nodes, const uint64_t *__restrict__ rowptr,
                                                  const uint32_t *__restrict__ col, const uint32_t *__restrict__ labels,
                                                  uint32_t *__restrict__ top_lab, uint32_t *__restrict__ top_cnt,
                                                  uint32_t *__restrict__ ndist) {
  const uint32_t x = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (x >= cnt) return;   // whole wavefronts leave together
  const uint32_t i = nodes[x];
  const uint64_t b = rowptr[i];
  const uint32_t d = (uint32_t)(rowptr[i + 1] - b);
  uint32_t v = lane < d ? labels[(size_t)col[b + lane] * S] : NONE;
  for (uint32_t k = 2; k <= 64; k <<= 1)   // bitonic sort, ascending across the wavefront
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)v, (int)j, 64);
      const bool up = (lane & k) == 0, lower = (lane & j) == 0;
      v = (lower == up) ? min(v, o) : max(v, o);
    }
  const uint32_t prev = (uint32_t)__shfl_up((int)v, 1, 64);
  const bool head = v != NONE && (lane == 0 || v != prev);
  const uint64_t heads = __ballot(head);
  const uint64_t after = lane == 63 ? 0 : heads >> (lane + 1);
  const uint32_t next = after ? lane + 1 + (uint32_t)__builtin_ctzll(after) : d;
  uint64_t key = head ? key_of(next - lane, v) : 0;
  for (uint32_t r = 0; r < S; ++r) {
    const uint64_t m = wave_max_u64(key);
    if (lane == 0) {
      top_lab[(size_t)i * S + r] = m ? label_of(m) : NONE;
      top_cnt[(size_t)i * S + r] = (uint32_t)(m >> 32);
    }
    if (key == m) key = 0;
  }
  if (lane == 0) ndist[i] = (uint32_t)__popcll(heads);
}

__device__ inline void top5_insert(uint64_t x, uint64_t &t0, uint64_t &t1, uint64_t &t2, uint64_t &t3, uint64_t &t4) {
  if (x <= t4) return;
  t4 = x;
  uint64_t s;
  if (t4 > t3) { s = t3; t3 = t4; t4 = s; } else return;
  if (t3 > t2) { s = t2; t2 = t3; t3 = s; } else return;
  if (t2 > t1) { s = t1; t1 = t2; t2 = s; } else return;
  if (t1 > t0) { s = t0; t0 = t1; t1 = s; }
}

// one node per block.  IN_LDS: the hash lives in LDS (LDS_SLOTS slots, degree <= LDS_SLOTS / 2); otherwise it lives at
// scratch + soff[x] (a power of two >= 2 x degree slots, keys then counts)
template <bool IN_LDS>
__global__ __launch_bounds__(256) void k_top_block(const uint32_t *__restrict__ nodes, const uint64_t *__restrict__ soff,
                                                   uint32_t *__restrict__ scratch, const uint64_t *__restrict__ rowptr,
                                                   const uint32_t *__restrict__ col, const uint32_t *__restrict__ labels,
                                                   uint32_t *__restrict__ top_lab, uint32_t *__restrict__ top_cnt,
                                                   uint32_t *__restrict__ ndist) {
  __shared__ uint32_t lds[IN_LDS ? 2 * LDS_SLOTS : 1];
  __shared__ uint64_t red[4];
  __shared__ uint32_t redc[4];
  const uint32_t x = blockIdx.x, t = threadIdx.x, w = t >> 6, lane = t & 63;
  const uint32_t i = nodes[x];
  const uint64_t b = rowptr[i];
  const uint32_t d = (uint32_t)(rowptr[i + 1] - b);
  uint32_t *keys, *cnts;
  uint32_t T;
  if (IN_LDS) {
    keys = lds;
    cnts = lds + LDS_SLOTS;
    T = LDS_SLOTS;
  } else {
    T = (uint32_t)((soff[x + 1] - soff[x]) / 2);
    keys = scratch + soff[x];
    cnts = keys + T;
  }
  for (uint32_t s = t; s < T; s += 256) { keys[s] = NONE; cnts[s] = 0; }
  __syncthreads();
  const uint32_t mask = T - 1;
  for (uint32_t e = t; e < d; e += 256) {
    const uint32_t lab = labels[(size_t)col[b + e] * S];
    uint32_t h = (lab * 2654435761u) & mask;
    while (true) {
      const uint32_t old = atomicCAS(&keys[h], NONE, lab);
      if (old == NONE || old == lab) { atomicAdd(&cnts[h], 1u); break; }
      h = (h + 1) & mask;
    }
  }
  __syncthreads();
  uint64_t t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
  uint32_t distinct = 0;
  for (uint32_t s = t; s < T; s += 256) {   // atomic loads: the slots were last written by atomics (L2 for the global hash)
    const uint32_t k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == NONE) continue;
    ++distinct;
    top5_insert(key_of(__hip_atomic_load(&cnts[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), k), t0, t1, t2, t3, t4);
  }
  distinct = wave_sum_u32(distinct);
  if (lane == 0) redc[w] = distinct;
  for (uint32_t r = 0; r < S; ++r) {
    const uint64_t m = wave_max_u64(t0);
    __syncthreads();
    if (lane == 0) red[w] = m;
    __syncthreads();
    uint64_t g = red[0];
    for (int q = 1; q < 4; ++q) g = red[q] > g ? red[q] : g;
    if (t == 0) {
      top_lab[(size_t)i * S + r] = g ? label_of(g) : NONE;
      top_cnt[(size_t)i * S + r] = (uint32_t)(g >> 32);
    }
    if (g && t0 == g) { t0 = t1; t1 = t2; t2 = t3; t3 = t4; t4 = 0; }   // keys are unique: one thread owns the winner
  }
  if (t == 0) ndist[i] = redc[0] + redc[1] + redc[2] + redc[3];
}

// records [node, ndistinct, label0..3] of the nodes that need padding (1 .. 4 distinct labels); order is the host's to fix
__global__ __launch_bounds__(256) void k_compact(uint32_t n, const uint32_t *__restrict__ ndist, const uint32_t *__restrict__ top_lab,
                                                 uint32_t *__restrict__ count, uint32_t *__restrict__ rec) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t d = ndist[i];
  if (d == 0 || d >= S) return;
  const uint32_t at = atomicAdd(count, 1u);
  uint32_t *r = rec + (size_t)at * 6;
  r[0] = i;
  r[1] = d;
  for (uint32_t j = 0; j < 4; ++j) r[2 + j] = top_lab[(size_t)i * S + j];
}

// set_gamma's counted slots: (label, count + alpha); nodes without a counted label keep their slots (:205-206)
__global__ __launch_bounds__(256) void k_apply(uint32_t n, double alpha, const uint32_t *__restrict__ ndist,
                                               const uint32_t *__restrict__ top_lab, const uint32_t *__restrict__ top_cnt,
                                               uint32_t *__restrict__ labels, double *__restrict__ values) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t d = ndist[i];
  if (d == 0) return;
  for (uint32_t j = 0; j < S && j < d; ++j) {
    labels[(size_t)i * S + j] = top_lab[(size_t)i * S + j];
    values[(size_t)i * S + j] = (double)top_cnt[(size_t)i * S + j] + alpha;
  }
}

// the padding slots: recs [m][6] as k_compact wrote them, pads [m][4] in the same order (the first 5 - ndistinct used)
__global__ __launch_bounds__(256) void k_pads(uint32_t m, double alpha, const uint32_t *__restrict__ rec, const uint32_t *__restrict__ pads,
                                              uint32_t *__restrict__ labels, double *__restrict__ values) {
  const uint32_t x = blockIdx.x * 256 + threadIdx.x;
  if (x >= m) return;
  const uint32_t i = rec[(size_t)x * 6], d = rec[(size_t)x * 6 + 1];
  for (uint32_t j = d; j < S; ++j) {
    labels[(size_t)i * S + j] = pads[(size_t)x * 4 + (j - d)];
    values[(size_t)i * S + j] = alpha + alpha;
  }
}

// pi = value / (sum of the 5 values + (n - 5) alpha), the reference's order of operations (uint32 n - 5)
__global__ __launch_bounds__(256) void k_pi(uint32_t n, double alpha, const double *__restrict__ values, double *__restrict__ pi) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double *v = values + (size_t)i * S;
  double s = .0;
  for (uint32_t j = 0; j < S; ++j) s += v[j];
  s += (double)(uint32_t)(n - S) * alpha;
  for (uint32_t j = 0; j < S; ++j) pi[(size_t)i * S + j] = v[j] / s;
}

__device__ inline double edge_ll(const uint32_t *labels, const double *pi, uint32_t p, uint32_t q, bool y) {
  uint32_t lp[S], lq[S];
  double pp[S], pq[S];
  for (uint32_t j = 0; j < S; ++j) {
    lp[j] = labels[(size_t)p * S + j]; lq[j] = labels[(size_t)q * S + j];
    pp[j] = pi[(size_t)p * S + j]; pq[j] = pi[(size_t)q * S + j];
  }
  double s = .0;
  for (uint32_t k1 = 0; k1 < S; ++k1)
    for (uint32_t k2 = 0; k2 < S; ++k2)
      if ((lp[k1] == lq[k2]) == y) s += pp[k1] * pq[k2];
  if (s < 1e-30) s = 1e-30;
  return log(s);
}

// pairs [m][stride]: (p, q[, y]); stride 2 = links (y = 1)
__global__ __launch_bounds__(256) void k_edge_ll(uint64_t m, uint32_t stride, const uint32_t *__restrict__ pairs,
                                                 const uint32_t *__restrict__ labels, const double *__restrict__ pi,
                                                 double *__restrict__ out) {
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= m) return;
  const uint32_t *r = pairs + x * stride;
  out[x] = edge_ll(labels, pi, r[0], r[1], stride == 2 ? true : r[2] != 0);
}

// partial[b] = sum of v[x] over the SUM_CHUNK items of block b (sel: only those with pairs[3x + 2] == want); a fixed tree
template <bool FINAL>
__global__ __launch_bounds__(256) void k_part_sum(uint64_t m, const double *__restrict__ v, const uint32_t *__restrict__ pairs,
                                                  int want, double *__restrict__ out) {
  __shared__ double red[256];
  const uint32_t t = threadIdx.x;
  const uint64_t b0 = FINAL ? 0 : (uint64_t)blockIdx.x * SUM_CHUNK;
  const uint64_t b1 = FINAL ? m : min(m, b0 + SUM_CHUNK);
  double s = .0;
  for (uint64_t x = b0 + t; x < b1; x += 256)
    if (want < 0 || (int)pairs[3 * x + 2] == want) s += v[x];
  red[t] = s;
  __syncthreads();
  for (uint32_t o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) out[FINAL ? 0 : blockIdx.x] = red[0];
}

// both directed entries (i, m) of every link: the loop of compute_and_log_groups (:305-348)
__global__ __launch_bounds__(256) void k_groups(uint64_t E, double thresh, const uint32_t *__restrict__ links,
                                                const uint32_t *__restrict__ labels, const double *__restrict__ pi,
                                                uint32_t *__restrict__ masks, uint32_t *__restrict__ unlikely) {
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t bad = 0;
  if (x < E) {
    for (int dir = 0; dir < 2; ++dir) {
      const uint32_t i = links[2 * x + dir], m = links[2 * x + 1 - dir];
      uint32_t li[S], lm[S];
      double pi_i[S], pi_m[S];
      for (uint32_t j = 0; j < S; ++j) {
        li[j] = labels[(size_t)i * S + j]; lm[j] = labels[(size_t)m * S + j];
        pi_i[j] = pi[(size_t)i * S + j]; pi_m[j] = pi[(size_t)m * S + j];
      }
      uint32_t max_k = SENTINEL, s1 = 0, s2 = 0;
      double mx = .0, sum = .0;
      for (uint32_t k1 = 0; k1 < S; ++k1)
        for (uint32_t k2 = 0; k2 < S; ++k2)
          if (li[k1] == lm[k2]) {
            const double u = pi_i[k1] * pi_m[k2];
            sum += u;
            if (u > mx) { mx = u; max_k = li[k1]; s1 = k1; s2 = k2; }
          }
      mx = sum > .0 ? mx / sum : .0;
      if (mx < thresh) { ++bad; continue; }
      if (max_k != SENTINEL) {
        if (!(masks[i] & (1u << s1))) atomicOr(&masks[i], 1u << s1);
        if (!(masks[m] & (1u << s2))) atomicOr(&masks[m], 1u << s2);
      }
    }
  }
  bad = wave_sum_u32(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(unlikely, bad);
}

}  // namespace

// events ev[7]: count, compact + records, apply, end of apply, likelihoods, groups, end
struct svils_findk : ToolHandle {
  uint32_t n = 0;
  double alpha = 0, thresh = 0.5;
  bool timed[4] = {};                       // phases with a measurement: count, apply, likelihoods, groups
  uint64_t E = 0, H = 0;
  // graph (GRAPH scope)
  uint32_t *links = nullptr;                // [E][2] p < q, every link
  uint32_t *held = nullptr;                 // [H][3] p, q, y: the held-out pairs in map order
  uint64_t *rowptr = nullptr;               // training CSR (links not held out)
  uint32_t *col = nullptr;
  uint32_t *bin_wave = nullptr, *bin_lds = nullptr, *bin_hub = nullptr;
  uint32_t n_wave = 0, n_lds = 0, n_hub = 0;
  uint64_t *hub_off = nullptr;              // [n_hub + 1] offsets into hub_scratch (uint32 words)
  uint32_t *hub_scratch = nullptr;
  double *ll = nullptr, *part = nullptr;    // [max(E, H)] likelihoods, their partial sums
  // state (HANDLE scope)
  uint32_t *labels = nullptr;               // [n][5]
  double *values = nullptr, *pi = nullptr;  // [n][5]
  uint32_t *top_lab = nullptr, *top_cnt = nullptr, *ndist = nullptr;
  uint32_t *rec = nullptr, *pads = nullptr, *counter = nullptr;   // counter[0]: records, counter[1]: unlikely
  uint32_t *masks = nullptr;
  double *sums = nullptr;                   // [4] training, held-out all / y = 0 / y = 1
  uint32_t npad = 0;
  bool have_graph = false, have_state = false, counted = false;
  std::vector<uint32_t> h_rec;
};

namespace {

void free_graph(svils_findk *f) {
  f->release(ToolHandle::GRAPH);
  f->have_graph = false;
}

}  // namespace

extern "C" {

int svils_findk_create(int device, uint32_t n, double alpha, double link_thresh, svils_findk **out) {
  if (!out) return fail(SVILS_ERR_ARG, "svils_findk_create: null argument");
  *out = nullptr;
  if (int rc = open_device(device, n < 2 || !(alpha > 0) ? "svils_findk_create: need n >= 2 and alpha > 0" : nullptr)) return rc;
  svils_findk *f = new (std::nothrow) svils_findk();
  if (!f) return fail(SVILS_ERR_NOMEM, "out of host memory");
  f->n = n;
  f->alpha = alpha;
  f->thresh = link_thresh;
  const auto scope = ToolHandle::HANDLE;
  const size_t ns = (size_t)n * S;
  int rc = f->open(device, 7);
  if (!rc) rc = f->dalloc(scope, &f->labels, ns);
  if (!rc) rc = f->dalloc(scope, &f->values, ns);
  if (!rc) rc = f->dalloc(scope, &f->pi, ns);
  if (!rc) rc = f->dalloc(scope, &f->top_lab, ns);
  if (!rc) rc = f->dalloc(scope, &f->top_cnt, ns);
  if (!rc) rc = f->dalloc(scope, &f->ndist, (size_t)n);
  if (!rc) rc = f->dalloc(scope, &f->rec, (size_t)n * 6);
  if (!rc) rc = f->dalloc(scope, &f->pads, (size_t)n * 4);
  if (!rc) rc = f->dalloc(scope, &f->masks, (size_t)n);
  if (!rc) rc = f->dalloc(scope, &f->counter, 2);
  if (!rc) rc = f->dalloc(scope, &f->sums, 4);
  if (rc) {
    svils_findk_destroy(f);
    return rc;
  }
  *out = f;
  return 0;
}

int svils_findk_destroy(svils_findk *f) {
  delete f;   // ~ToolHandle: waits for the stream, frees both scopes
  return 0;
}

int svils_findk_set_graph(svils_findk *f, const uint32_t *links, uint64_t nlinks, const uint8_t *held_out,
                          const uint32_t *heldout_pairs, uint64_t nheldout) {
  if (int rc = check(f, "svils_findk_set_graph")) return rc;
  if ((nlinks && !links) || (nheldout && !heldout_pairs)) return fail(SVILS_ERR_ARG, "svils_findk_set_graph: null argument");
  const uint32_t n = f->n;
  for (uint64_t x = 0; x < nlinks; ++x)
    if (links[2 * x] >= n || links[2 * x + 1] >= n || links[2 * x] == links[2 * x + 1])
      return fail(SVILS_ERR_ARG, "svils_findk_set_graph: link %llu (%u, %u) is a self pair or names a node >= n = %u",
                  (unsigned long long)x, links[2 * x], links[2 * x + 1], n);
  for (uint64_t x = 0; x < nheldout; ++x)
    if (heldout_pairs[3 * x] >= n || heldout_pairs[3 * x + 1] >= n)
      return fail(SVILS_ERR_ARG, "svils_findk_set_graph: held-out pair %llu names a node >= n", (unsigned long long)x);
  HIPCHK(hipStreamSynchronize(f->st));
  free_graph(f);
  // the training CSR: the links not held out, both directions (the count of batch_infer, :258-271)
  std::vector<uint64_t> rp((size_t)n + 1, 0);
  for (uint64_t x = 0; x < nlinks; ++x)
    if (!held_out || !held_out[x]) { rp[links[2 * x] + 1]++; rp[links[2 * x + 1] + 1]++; }
  for (uint32_t i = 0; i < n; ++i) rp[i + 1] += rp[i];
  std::vector<uint32_t> col(rp[n]);
  {
    std::vector<uint64_t> at(rp.begin(), rp.end() - 1);
    for (uint64_t x = 0; x < nlinks; ++x)
      if (!held_out || !held_out[x]) {
        const uint32_t p = links[2 * x], q = links[2 * x + 1];
        col[at[p]++] = q;
        col[at[q]++] = p;
      }
  }
  // degree bins; hubs get a hash of a power of two >= 2 x degree slots (keys and counts: twice that many words)
  std::vector<uint32_t> bw, bl, bh;
  std::vector<uint64_t> hoff(1, 0);
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t d = rp[i + 1] - rp[i];
    if (d == 0) continue;
    if (d <= WAVE_MAX) bw.push_back(i);
    else if (d <= LDS_SLOTS / 2) bl.push_back(i);
    else {
      bh.push_back(i);
      uint64_t T = 1;
      while (T < 2 * d) T <<= 1;
      hoff.push_back(hoff.back() + 2 * T);
    }
  }
  std::vector<uint32_t> lk(links, links + 2 * nlinks), hp(heldout_pairs, heldout_pairs + 3 * nheldout);
  const auto scope = ToolHandle::GRAPH;
  int rc = 0;
  if (!rc) rc = f->upload(scope, &f->links, lk);
  if (!rc) rc = f->upload(scope, &f->held, hp);
  if (!rc) rc = f->upload(scope, &f->rowptr, rp);
  if (!rc) rc = f->upload(scope, &f->col, col);
  if (!rc) rc = f->upload(scope, &f->bin_wave, bw);
  if (!rc) rc = f->upload(scope, &f->bin_lds, bl);
  if (!rc) rc = f->upload(scope, &f->bin_hub, bh);
  if (!rc) rc = f->upload(scope, &f->hub_off, hoff);
  if (!rc) rc = f->dalloc(scope, &f->hub_scratch, hoff.back());
  const uint64_t mx = std::max<uint64_t>(std::max<uint64_t>(nlinks, nheldout), 1);
  if (!rc) rc = f->dalloc(scope, &f->ll, mx);
  if (!rc) rc = f->dalloc(scope, &f->part, blocks(mx, SUM_CHUNK));
  if (!rc && hipStreamSynchronize(f->st) != hipSuccess) rc = fail(SVILS_ERR_DEVICE, "svils_findk_set_graph: upload failed");
  if (rc) {
    free_graph(f);
    return rc;
  }
  f->E = nlinks;
  f->H = nheldout;
  f->n_wave = (uint32_t)bw.size();
  f->n_lds = (uint32_t)bl.size();
  f->n_hub = (uint32_t)bh.size();
  f->have_graph = true;
  f->counted = false;
  return 0;
}

int svils_findk_init_state(svils_findk *f, const uint32_t *labels, const double *values) {
  if (int rc = check(f, "svils_findk_init_state")) return rc;
  if (!labels || !values) return fail(SVILS_ERR_ARG, "svils_findk_init_state: null argument");
  const size_t ns = (size_t)f->n * S;
  for (size_t x = 0; x < ns; ++x)
    if (labels[x] >= f->n) return fail(SVILS_ERR_ARG, "svils_findk_init_state: label %u >= n = %u", labels[x], f->n);
  HIPCHK(hipMemcpyAsync(f->labels, labels, ns * sizeof(uint32_t), hipMemcpyHostToDevice, f->st));
  HIPCHK(hipMemcpyAsync(f->values, values, ns * sizeof(double), hipMemcpyHostToDevice, f->st));
  hipLaunchKernelGGL(k_pi, dim3(blocks(f->n, 256)), dim3(256), 0, f->st, f->n, f->alpha, f->values, f->pi);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(f->st));
  f->have_state = true;
  f->counted = false;
  return 0;
}

int svils_findk_count(svils_findk *f, uint32_t *npad) {
  if (int rc = check(f, "svils_findk_count")) return rc;
  if (!npad) return fail(SVILS_ERR_ARG, "svils_findk_count: null argument");
  if (!f->have_graph || !f->have_state) return fail(SVILS_ERR_ARG, "svils_findk_count: set the graph and the state first");
  const uint32_t n = f->n;
  HIPCHK(hipEventRecord(f->ev[0], f->st));
  HIPCHK(hipMemsetAsync(f->ndist, 0, (size_t)n * sizeof(uint32_t), f->st));
  if (f->n_wave)
    hipLaunchKernelGGL(k_top_wave, dim3(blocks(f->n_wave, 4)), dim3(256), 0, f->st, f->n_wave, f->bin_wave, f->rowptr, f->col,
                       f->labels, f->top_lab, f->top_cnt, f->ndist);
  if (f->n_lds)
    hipLaunchKernelGGL(k_top_block<true>, dim3(f->n_lds), dim3(256), 0, f->st, f->bin_lds, (const uint64_t *)nullptr,
                       (uint32_t *)nullptr, f->rowptr, f->col, f->labels, f->top_lab, f->top_cnt, f->ndist);
  if (f->n_hub)
    hipLaunchKernelGGL(k_top_block<false>, dim3(f->n_hub), dim3(256), 0, f->st, f->bin_hub, f->hub_off, f->hub_scratch, f->rowptr,
                       f->col, f->labels, f->top_lab, f->top_cnt, f->ndist);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(f->ev[1], f->st));
  HIPCHK(hipMemsetAsync(f->counter, 0, sizeof(uint32_t), f->st));
  hipLaunchKernelGGL(k_compact, dim3(blocks(n, 256)), dim3(256), 0, f->st, n, f->ndist, f->top_lab, f->counter, f->rec);
  HIPCHK(hipGetLastError());
  uint32_t m = 0;
  HIPCHK(hipMemcpyAsync(&m, f->counter, sizeof m, hipMemcpyDeviceToHost, f->st));
  HIPCHK(hipStreamSynchronize(f->st));
  f->h_rec.resize((size_t)m * 6);
  if (m) HIPCHK(hipMemcpy(f->h_rec.data(), f->rec, (size_t)m * 6 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  // the padding draws run in node order: sort the records by node (k_compact appends them in no fixed order)
  std::vector<uint32_t> order(m);
  for (uint32_t x = 0; x < m; ++x) order[x] = x;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return f->h_rec[(size_t)a * 6] < f->h_rec[(size_t)b * 6]; });
  std::vector<uint32_t> sorted((size_t)m * 6);
  for (uint32_t x = 0; x < m; ++x) memcpy(&sorted[(size_t)x * 6], &f->h_rec[(size_t)order[x] * 6], 6 * sizeof(uint32_t));
  f->h_rec.swap(sorted);
  if (m) HIPCHK(hipMemcpy(f->rec, f->h_rec.data(), (size_t)m * 6 * sizeof(uint32_t), hipMemcpyHostToDevice));
  f->npad = m;
  f->counted = true;
  f->timed[0] = true;
  *npad = m;
  return 0;
}

int svils_findk_pad_requests(svils_findk *f, uint32_t *nodes, uint32_t *ndistinct, uint32_t *labels) {
  if (int rc = check(f, "svils_findk_pad_requests")) return rc;
  if (!f->counted) return fail(SVILS_ERR_ARG, "svils_findk_pad_requests: no svils_findk_count since the last apply");
  if (f->npad && (!nodes || !ndistinct || !labels)) return fail(SVILS_ERR_ARG, "svils_findk_pad_requests: null argument");
  for (uint32_t x = 0; x < f->npad; ++x) {
    const uint32_t *r = &f->h_rec[(size_t)x * 6];
    nodes[x] = r[0];
    ndistinct[x] = r[1];
    for (uint32_t j = 0; j < 4; ++j) labels[(size_t)x * 4 + j] = j < r[1] ? r[2 + j] : NONE;
  }
  return 0;
}

int svils_findk_apply(svils_findk *f, const uint32_t *pads) {
  if (int rc = check(f, "svils_findk_apply")) return rc;
  if (!f->counted) return fail(SVILS_ERR_ARG, "svils_findk_apply: no svils_findk_count since the last apply");
  if (f->npad && !pads) return fail(SVILS_ERR_ARG, "svils_findk_apply: null argument");
  const uint32_t n = f->n;
  for (uint32_t x = 0; x < f->npad; ++x)
    for (uint32_t j = f->h_rec[(size_t)x * 6 + 1]; j < S; ++j)
      if (pads[(size_t)x * 4 + (j - f->h_rec[(size_t)x * 6 + 1])] >= n)
        return fail(SVILS_ERR_ARG, "svils_findk_apply: pad label of record %u >= n", x);
  HIPCHK(hipEventRecord(f->ev[2], f->st));
  if (f->npad) HIPCHK(hipMemcpyAsync(f->pads, pads, (size_t)f->npad * 4 * sizeof(uint32_t), hipMemcpyHostToDevice, f->st));
  hipLaunchKernelGGL(k_apply, dim3(blocks(n, 256)), dim3(256), 0, f->st, n, f->alpha, f->ndist, f->top_lab, f->top_cnt, f->labels,
                     f->values);
  if (f->npad)
    hipLaunchKernelGGL(k_pads, dim3(blocks(f->npad, 256)), dim3(256), 0, f->st, f->npad, f->alpha, f->rec, f->pads, f->labels, f->values);
  hipLaunchKernelGGL(k_pi, dim3(blocks(n, 256)), dim3(256), 0, f->st, n, f->alpha, f->values, f->pi);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(f->ev[3], f->st));
  HIPCHK(hipStreamSynchronize(f->st));
  f->counted = false;
  f->timed[1] = true;
  return 0;
}

int svils_findk_report(svils_findk *f, double *training_ll, double *heldout_sums, uint32_t *unlikely, uint32_t *masks) {
  if (int rc = check(f, "svils_findk_report")) return rc;
  if (!f->have_graph || !f->have_state) return fail(SVILS_ERR_ARG, "svils_findk_report: set the graph and the state first");
  if ((unlikely == nullptr) != (masks == nullptr)) return fail(SVILS_ERR_ARG, "svils_findk_report: unlikely and masks go together");
  HIPCHK(hipEventRecord(f->ev[4], f->st));
  HIPCHK(hipMemsetAsync(f->sums, 0, 4 * sizeof(double), f->st));
  if (f->E) {
    hipLaunchKernelGGL(k_edge_ll, dim3(blocks(f->E, 256)), dim3(256), 0, f->st, f->E, 2u, f->links, f->labels, f->pi, f->ll);
    const uint32_t nb = blocks(f->E, SUM_CHUNK);
    hipLaunchKernelGGL(k_part_sum<false>, dim3(nb), dim3(256), 0, f->st, f->E, f->ll, (const uint32_t *)nullptr, -1, f->part);
    hipLaunchKernelGGL(k_part_sum<true>, dim3(1), dim3(256), 0, f->st, (uint64_t)nb, f->part, (const uint32_t *)nullptr, -1, f->sums);
  }
  if (f->H) {
    hipLaunchKernelGGL(k_edge_ll, dim3(blocks(f->H, 256)), dim3(256), 0, f->st, f->H, 3u, f->held, f->labels, f->pi, f->ll);
    const uint32_t nb = blocks(f->H, SUM_CHUNK);
    for (int want = -1; want <= 1; ++want) {
      hipLaunchKernelGGL(k_part_sum<false>, dim3(nb), dim3(256), 0, f->st, f->H, f->ll, f->held, want, f->part);
      hipLaunchKernelGGL(k_part_sum<true>, dim3(1), dim3(256), 0, f->st, (uint64_t)nb, f->part, (const uint32_t *)nullptr, -1,
                         f->sums + 2 + want);
    }
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(f->ev[5], f->st));
  if (masks) {
    HIPCHK(hipMemsetAsync(f->masks, 0, (size_t)f->n * sizeof(uint32_t), f->st));
    HIPCHK(hipMemsetAsync(f->counter + 1, 0, sizeof(uint32_t), f->st));
    if (f->E)
      hipLaunchKernelGGL(k_groups, dim3(blocks(f->E, 256)), dim3(256), 0, f->st, f->E, f->thresh, f->links, f->labels, f->pi, f->masks,
                         f->counter + 1);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(f->ev[6], f->st));
  double s[4];
  HIPCHK(hipMemcpyAsync(s, f->sums, sizeof s, hipMemcpyDeviceToHost, f->st));
  if (masks) {
    HIPCHK(hipMemcpyAsync(unlikely, f->counter + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, f->st));
    HIPCHK(hipMemcpyAsync(masks, f->masks, (size_t)f->n * sizeof(uint32_t), hipMemcpyDeviceToHost, f->st));
  }
  HIPCHK(hipStreamSynchronize(f->st));
  if (training_ll) *training_ll = f->E ? s[0] / (double)f->E : 0.0;
  if (heldout_sums) { heldout_sums[0] = s[1]; heldout_sums[1] = s[2]; heldout_sums[2] = s[3]; }
  f->timed[2] = true;
  f->timed[3] = masks != nullptr;
  return 0;
}

int svils_findk_get_state(svils_findk *f, uint32_t *labels, double *values, double *pi) {
  if (int rc = check(f, "svils_findk_get_state")) return rc;
  if (!f->have_state) return fail(SVILS_ERR_ARG, "svils_findk_get_state: no state");
  const size_t ns = (size_t)f->n * S;
  if (labels) HIPCHK(hipMemcpyAsync(labels, f->labels, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, f->st));
  if (values) HIPCHK(hipMemcpyAsync(values, f->values, ns * sizeof(double), hipMemcpyDeviceToHost, f->st));
  if (pi) HIPCHK(hipMemcpyAsync(pi, f->pi, ns * sizeof(double), hipMemcpyDeviceToHost, f->st));
  HIPCHK(hipStreamSynchronize(f->st));
  return 0;
}

int svils_findk_get_timing(svils_findk *f, double ms[4]) {
  if (int rc = check(f, "svils_findk_get_timing")) return rc;
  if (!ms) return fail(SVILS_ERR_ARG, "svils_findk_get_timing: null argument");
  HIPCHK(hipStreamSynchronize(f->st));
  static const int from[4] = {0, 2, 4, 5}, to[4] = {1, 3, 5, 6};
  for (int p = 0; p < 4; ++p) ms[p] = f->elapsed_ms(from[p], to[p], f->timed[p]);
  return 0;
}

}  // extern "C"
