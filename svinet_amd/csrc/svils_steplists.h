// svils_steplists.h -- what the list entry points of svils_batch.hip (svils_batch_step_pairs, _step_star, _step_strat) check
// of a call's step lists.  Plain host code: no device, no handle.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/svils.h"

namespace svils_impl {

// Declared in svils_handle.h.  Repeated here so that this header needs neither the HIP runtime nor RCCL's types, which
// svils_handle.h brings in: a host-only program can include it and supply its own fail().  svils_batch.hip includes both;
// should the two declarations ever part, that file no longer builds or the library no longer loads
int fail(int code, const char *fmt, ...);

// off[0] == 0; then step by step: rho_open (where a step size of 1 is refused: strat steps) below 1, off not decreasing,
// scale a positive number, start (where the steps have start nodes) a node of n; then the lists there if they have
// entries (have_lists) and fewer than 2^30 entries (`what`) in all.  Out: the entries of the call and of its longest step
inline int check_step_lists(const char *name, const char *what, uint32_t n, uint32_t nsteps, const uint64_t *off, const double *scale,
                            const uint32_t *start, const double *rho_open, bool have_lists, uint64_t *total, uint64_t *most) {
  if (off[0] != 0) return fail(SVILS_ERR_ARG, "%s: off[0] is not 0", name);
  *most = 0;
  for (uint32_t s = 0; s < nsteps; ++s) {
    if (rho_open && !(rho_open[s] < 1.0))
      return fail(SVILS_ERR_ARG, "%s: rho_gamma[%u] is not in (0, 1) (log1p(-1) has no value)", name, s);
    if (off[s + 1] < off[s]) return fail(SVILS_ERR_ARG, "%s: off[%u] decreases", name, s + 1);
    if (!(scale[s] > 0.0) || !std::isfinite(scale[s])) return fail(SVILS_ERR_ARG, "%s: scale[%u] is not a positive number", name, s);
    if (start && start[s] >= n) return fail(SVILS_ERR_ARG, "%s: start[%u] = %u is not < n = %u", name, s, start[s], n);
    *most = std::max(*most, off[s + 1] - off[s]);
  }
  *total = off[nsteps];
  if (*total && !have_lists) return fail(SVILS_ERR_ARG, "%s: null argument", name);
  if (*total >= ((uint64_t)1 << 30)) return fail(SVILS_ERR_UNSUPPORTED, "%s: more than 2^30 %s in one call", name, what);
  return 0;
}

}  // namespace svils_impl
