// svils_orig_elbo.hip -- -orig -logl: the reference's MMSBInferOrig::approx_log_likelihood (src/mmsbinferorig.cc:624-726, under
// GLOBALPHIS) of the CURRENT state on the device: s = P + N.  beta is a point estimate in this model, so
// there is no term of the block rates.  One pass is
//
//   k_orig_dir_exp, k_orig_tables   (svils_orig.hip) Elogpi of the current gamma and the fixed point's L tables, into buffers of
//                                   the pass; k_orig_tables once more with eps = 1e-10: T0 = log((1 - beta) + 1e-10),
//                                   T1 = log(beta + 1e-10), the reference's log(fd[g][h] + 1e-10)
//   k_orig_elbo_nodes               one wavefront per node: the node's term of N (svils_elbo.h, shared with svils_batch_elbo)
//   per launch of the sweep's row cut:
//     k_orig_pairs<KP,LREG>         (svils_orig.hip, as it stands) the fixed points from 1 / K into the handle's phi buffers, with a
//                                   counter block of the pass's own
//     k_orig_elbo_terms<KP>         one workgroup per row p of the launch; wavefront j takes the tiles t = j (mod 4) of the row, 16
//                                   slots (p, 16 t .. 16 t + 15) each, in the pair kernel's MFMA mapping: B = Phi2, A = 16-row
//                                   blocks of T0 / T1, a pair's column zero in the product that is not its own, so the
//                                   accumulators hold exactly T_y phi2.  Register r of block b of lane (g, c) is row
//                                   h = 16 b + 4 r + g of pair c -- the entry of phi1 the lane holds in operand layout -- so
//                                   phi1^T T_y phi2 is an elementwise multiply-add behind the MFMA chain: no cross-lane move.  Cross
//                                   terms and entropies per lane.  A lane adds its tiles in ascending order, one butterfly at the
//                                   end, one double per (row, j): el_part [n][4]
//   k_orig_elbo_reduce              one block: P = the 4 n partials, N = the n node terms, each thread its entries in ascending
//                                   order, then a fixed tree
//
// No floating-point atomics, and a partial belongs to a piece of a row that depends on n alone: the three outputs have the same
// bits whatever svils_orig_set_launch_rows cut the pass into.  The pass writes el_* and the phi buffers (which every sweep
// overwrites before it reads them) and nothing else: gamma, beta, the handle's counters, Elogpi, tabs and state_gen stay.
#include "svils_devutil.h"
#include "svils_elbo.h"
#include "svils_orig.h"
#include "svils_waveutil.h"

using namespace svils_impl;

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr uint32_t ROW_PIECES = 4;   // partial sums per row: the wavefronts of a workgroup

__global__ __launch_bounds__(256) void k_orig_elbo_nodes(uint32_t n, uint32_t K, double alpha, const double *__restrict__ gamma,
                                                         const double *__restrict__ elogpi, double *__restrict__ out) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;   // whole wavefronts leave together
  const double t = elbo_node_term(gamma + (size_t)i * K, elogpi + (size_t)i * K, K, alpha, lane);
  if (lane == 0) out[i] = t;
}

struct TermArgs {
  uint32_t n, K, p0, tpr;             // the launch's first row; tpr = ceil(n / 16)
  const double *elogpi;               // [n][K]
  const double *tabs;                 // [2][KP][ld] T0, T1 in the layout of k_orig_tables
  const double *phi1, *phi2;          // [rows n][KP] of this launch
  const uint8_t *yv;                  // [rows n]
  double *part;                       // [n][ROW_PIECES]
};

// The tables in registers (KP <= 32) or LDS, as the pair kernel's split
template <int KP>
__global__ __launch_bounds__(256) void k_orig_elbo_terms(TermArgs x) {
  constexpr bool LREG = KP <= 32;
  constexpr int R = KP / 16, S = KP / 4, LD = tab_ld(KP);
  __shared__ double lt[LREG ? 1 : 2 * KP * LD];
  const uint32_t t = threadIdx.x, w = t >> 6, l = t & 63, g = l >> 4, c = l & 15;
  const uint32_t K = x.K, n = x.n, pr = blockIdx.x, p = x.p0 + pr;
  double a0r[LREG ? R * S : 1], a1r[LREG ? R * S : 1];
  if (LREG) {
#pragma unroll
    for (int b = 0; b < R; ++b)
#pragma unroll
      for (int s = 0; s < S; ++s) {
        a0r[LREG ? b * S + s : 0] = x.tabs[(4 * s + g) * LD + 16 * b + c];
        a1r[LREG ? b * S + s : 0] = x.tabs[KP * LD + (4 * s + g) * LD + 16 * b + c];
      }
  } else {
    for (uint32_t i = t; i < 2 * KP * LD; i += 256) lt[LREG ? 0 : i] = x.tabs[i];
    __syncthreads();
  }
  const double *ep = x.elogpi + (size_t)p * K;
  double acc = 0.0;
  for (uint32_t ti = w; ti < x.tpr; ti += ROW_PIECES) {   // wave-uniform
    const uint32_t q = ti * TILE_PAIRS + c;
    const bool in = q < n;
    const size_t slot = (size_t)pr * n + (in ? q : 0);
    const bool y = in && x.yv[slot];
    const double *eq = x.elogpi + (size_t)(in ? q : 0) * K;
    const double *f1 = x.phi1 + slot * KP + g, *f2 = x.phi2 + slot * KP + g;
    const bool any1 = __any(y), any0 = __any(in && !y);
    double phi2[S];
#pragma unroll
    for (int s = 0; s < S; ++s) phi2[s] = in ? f2[4 * s] : 0.0;   // (zero past K and for a slot that is not visited)
    d4 u[R];
#pragma unroll
    for (int b = 0; b < R; ++b) u[b] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const double z2 = y ? 0.0 : phi2[s], y2 = y ? phi2[s] : 0.0;
#pragma unroll
      for (int b = 0; b < R; ++b) {
        const double a0 = LREG ? a0r[LREG ? b * S + s : 0] : lt[LREG ? 0 : (4 * s + g) * LD + 16 * b + c];
        const double a1 = LREG ? a1r[LREG ? b * S + s : 0] : lt[LREG ? 0 : KP * LD + (4 * s + g) * LD + 16 * b + c];
        if (any0) u[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, z2, u[b], 0, 0, 0);
        if (any1) u[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, y2, u[b], 0, 0, 0);
      }
    }
    // this lane's share of the tile.  u[b][r] is row h = 16 b + 4 r + g of T_y phi2: the entry s = 4 b + r of phi1 in operand
    // layout.  Rows h >= K: phi1 and phi2 are 0 there, and so are the table's rows
    double tl = 0.0;
#pragma unroll
    for (int b = 0; b < R; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = 4 * b + r;
        const bool ok = in && (uint32_t)(4 * s) + g < K;
        const double p1 = ok ? f1[4 * s] : 0.0, p2 = phi2[s];
        const double e1 = ok ? ep[4 * s + g] : 0.0, e2 = ok ? eq[4 * s + g] : 0.0;
        tl += p1 * (u[b][r] + e1) + p2 * e2 - xlogx(p1) - xlogx(p2);
      }
    acc += tl;
  }
  acc = wave_sum_f64(acc);
  if (l == 0) x.part[(size_t)p * ROW_PIECES + w] = acc;
}

// out: total, P, N.  The order of every sum depends on n alone
__global__ __launch_bounds__(256) void k_orig_elbo_reduce(uint32_t n, const double *__restrict__ part, const double *__restrict__ node,
                                                          double *__restrict__ out) {
  __shared__ double red[2][256];
  const uint32_t t = threadIdx.x;
  double sp = 0.0, sn = 0.0;
  for (uint64_t e = t; e < (uint64_t)ROW_PIECES * n; e += 256) sp += part[e];
  for (uint32_t i = t; i < n; i += 256) sn += node[i];
  red[0][t] = sp;
  red[1][t] = sn;
  __syncthreads();
  for (uint32_t o = 128; o > 0; o >>= 1) {
    if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; }
    __syncthreads();
  }
  if (t == 0) {
    out[0] = red[0][0] + red[1][0];
    out[1] = red[0][0];
    out[2] = red[1][0];
  }
}

template <int KP>
void launch_terms(svils_orig *h, uint32_t rows, const TermArgs &a) {
  hipLaunchKernelGGL((k_orig_elbo_terms<KP>), dim3(rows), dim3(256), 0, h->st, a);
}

}  // namespace

namespace svils_impl {

void free_elbo(svils_orig *h) {
  for (hipEvent_t e : h->ev_elbo)
    if (e) (void)hipEventDestroy(e);
  h->ev_elbo.clear();
}

}  // namespace svils_impl

extern "C" {

int svils_orig_elbo(svils_orig *h, double out[3]) {
  const char *name = "svils_orig_elbo";
  if (int rc = check(h, name)) return rc;
  if (!out) return fail(SVILS_ERR_ARG, "%s: null argument", name);
  if (!h->have_graph || !h->have_state) return fail(SVILS_ERR_ARG, "%s: set the graph and the state first", name);
  if (int rc = settle(h, name)) return rc;   // the degenerate flag: the state is what the last applied sweep left
  const uint32_t n = h->n, K = h->k, KP = h->kp;
  const size_t tab = (size_t)KP * h->ld;
  const auto scope = ToolHandle::HANDLE;
  if (int rc = h->reserve(scope, &h->el_elogpi, (size_t)n * K)) return rc;
  if (int rc = h->reserve(scope, &h->el_tabs, 4 * tab)) return rc;
  if (int rc = h->reserve(scope, &h->el_part, (size_t)ROW_PIECES * n)) return rc;
  if (int rc = h->reserve(scope, &h->el_node, (size_t)n)) return rc;
  if (int rc = h->reserve(scope, &h->el_out, (size_t)3)) return rc;
  if (int rc = h->reserve(scope, &h->el_ctr, (size_t)CTR_COUNT)) return rc;
  const uint32_t nlaunch = (n + h->rows - 1) / h->rows;
  while (h->ev_elbo.size() < 2 + 2 * (size_t)nlaunch) {
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreate(&e));
    h->ev_elbo.push_back(e);
  }
  h->timed_elbo = false;
  // the pass's counter block: zero, with the handle's degenerate flag mirrored (down here: settle() has looked)
  HIPCHK(hipMemsetAsync(h->el_ctr, 0, CTR_COUNT * sizeof(u64), h->st));
  HIPCHK(hipMemcpyAsync(h->el_ctr + CTR_FLAG, h->ctr + CTR_PENDING, sizeof(u64), hipMemcpyDeviceToDevice, h->st));
  HIPCHK(hipEventRecord(h->ev_elbo[0], h->st));
  if (int rc = orig_launch_prologue(h, h->el_elogpi, h->el_tabs, 0.0)) return rc;
  if (int rc = orig_launch_prologue(h, nullptr, h->el_tabs + 2 * tab, 1e-10)) return rc;
  hipLaunchKernelGGL(k_orig_elbo_nodes, dim3(blocks(n, 4)), dim3(256), 0, h->st, n, K, h->alpha, h->gamma, h->el_elogpi, h->el_node);
  HIPCHK(hipGetLastError());
  uint32_t b = 0;
  const uint32_t tpr = (n + TILE_PAIRS - 1) / TILE_PAIRS;
  for (uint32_t p0 = 0; p0 < n; p0 += h->rows, ++b) {
    const uint32_t rows = std::min(h->rows, n - p0);
    PairArgs a{n, K, h->nw, p0, rows, tpr, h->adj, h->skip, h->el_elogpi, h->el_tabs, h->phi1, h->phi2, h->yv, h->el_ctr};
    if (int rc = orig_launch_pairs(h, name, a)) return rc;
    HIPCHK(hipEventRecord(h->ev_elbo[1 + 2 * b], h->st));
    TermArgs ta{n, K, p0, tpr, h->el_elogpi, h->el_tabs + 2 * tab, h->phi1, h->phi2, h->yv, h->el_part};
    switch (KP) {
      case 16: launch_terms<16>(h, rows, ta); break;
      case 32: launch_terms<32>(h, rows, ta); break;
      case 48: launch_terms<48>(h, rows, ta); break;
      case 64: launch_terms<64>(h, rows, ta); break;
      default: return fail(SVILS_ERR_UNSUPPORTED, "%s: no term kernel for padded K = %u", name, KP);   // a missing kernel is an error
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev_elbo[2 + 2 * b], h->st));
  }
  hipLaunchKernelGGL(k_orig_elbo_reduce, dim3(1), dim3(256), 0, h->st, n, h->el_part, h->el_node, h->el_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev_elbo[1 + 2 * b], h->st));
  h->el_nlaunch = b;
  h->timed_elbo = true;
  u64 c[CTR_COUNT] = {0};
  double o[3] = {0, 0, 0};
  HIPCHK(hipMemcpyAsync(c, h->el_ctr, sizeof c, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipMemcpyAsync(o, h->el_out, sizeof o, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  if (c[CTR_NORM])
    return fail(SVILS_ERR_UNSUPPORTED, "%s: %llu pair(s) of the pass with a normaliser not > 0 (the reference asserts s > 0 there)", name,
                c[CTR_NORM]);
  for (int i = 0; i < 3; ++i) out[i] = o[i];
  return 0;
}

int svils_orig_get_elbo_stats(svils_orig *h, uint64_t *pairs_done, uint64_t *rounds_total, uint32_t *rounds_max, uint64_t *bad_normalisers) {
  if (int rc = check(h, "svils_orig_get_elbo_stats")) return rc;
  u64 c[CTR_COUNT] = {0};
  if (h->el_ctr) {
    HIPCHK(hipMemcpyAsync(c, h->el_ctr, sizeof c, hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
  }
  if (pairs_done) *pairs_done = c[CTR_PAIRS];
  if (rounds_total) *rounds_total = c[CTR_ROUNDS];
  if (rounds_max) *rounds_max = (uint32_t)c[CTR_MAXR];
  if (bad_normalisers) *bad_normalisers = c[CTR_NORM];
  return 0;
}

int svils_orig_get_elbo_timing(svils_orig *h, double ms[3]) {
  if (int rc = check(h, "svils_orig_get_elbo_timing")) return rc;
  if (!ms) return fail(SVILS_ERR_ARG, "svils_orig_get_elbo_timing: null argument");
  HIPCHK(hipStreamSynchronize(h->st));
  ms[0] = ms[1] = ms[2] = -1.0;
  if (!h->timed_elbo) return 0;
  auto between = [&](size_t a, size_t b) {
    float t = 0;
    return hipEventElapsedTime(&t, h->ev_elbo[a], h->ev_elbo[b]) == hipSuccess ? (double)t : -1.0;
  };
  ms[0] = between(0, 1 + 2 * (size_t)h->el_nlaunch);
  ms[1] = ms[2] = 0.0;
  for (uint32_t b = 0; b < h->el_nlaunch; ++b) {
    ms[1] += between(b ? 2 * (size_t)b : 0, 1 + 2 * (size_t)b);   // (the first launch's bracket includes Elogpi, the tables and the node terms)
    ms[2] += between(1 + 2 * (size_t)b, 2 + 2 * (size_t)b);
  }
  return 0;
}

}  // extern "C"
