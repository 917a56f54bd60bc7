// svils_elbo.h -- what the two variational lower bounds share on the device (svils_batch_elbo, DESIGN.md section 4k;
// svils_orig_elbo, section 4n): the entropy term and the node term N_p.
#pragma once
#include "svils_waveutil.h"

namespace svils {

// phi log phi; an entry that has underflowed to exactly 0 adds 0 (the reference's log(phi) * phi is NaN there)
__device__ __forceinline__ double xlogx(double p) { return p > 0.0 ? p * log(p) : 0.0; }

// One wavefront per node.  The node's term of N (src/mmsbinfer.cc:2036-2056, src/mmsbinferorig.cc:668-688):
//   lnGamma(K alpha) - K lnGamma(alpha) + (alpha - 1) sum_k Elogpi_k - [lnGamma(sum_k gamma_k) - sum_k lnGamma(max(gamma_k, 1e-30))]
//   - sum_k (gamma_k - 1) Elogpi_k
// g, e: the node's rows of gamma and Elogpi.  The same bits in every lane
__device__ inline double elbo_node_term(const double *__restrict__ g, const double *__restrict__ e, uint32_t K, double alpha,
                                        uint32_t lane) {
  double se = 0.0, sg = 0.0, sl = 0.0, sge = 0.0;
  for (uint32_t k = lane; k < K; k += 64) {
    se += e[k];
    sg += g[k];
    sl += lgamma(fmax(g[k], 1e-30));
    sge += (g[k] - 1.0) * e[k];
  }
  se = wave_sum_f64(se);
  sg = wave_sum_f64(sg);
  sl = wave_sum_f64(sl);
  sge = wave_sum_f64(sge);
  return lgamma((double)K * alpha) - (double)K * lgamma(alpha) + (alpha - 1.0) * se - (lgamma(sg) - sl) - sge;
}

}  // namespace svils
