// svils_waveutil.h -- what the standalone device engines (svils_batch, svils_orig, svils_findk) share on the device
// side: the wavefront-wide reductions, one copy of each butterfly so that every unit sums in the same order, and the
// exit rule of the all-pairs fixed points.
//
// These would sit next to group_sum / cross_group_sum, but svils_devutil.h is one of the kernel sources whose hashes
// stand behind the sweep's measured HBM traffic (bench.py: KERNEL_SOURCES, profiles/traffic.json): a byte changed there
// voids that record.  Nothing of the sweep path needs what is here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace svils {

// All-reduce over the 64 lanes of a wavefront: a butterfly in the fixed order xor 32, 16, .. 1; every lane ends with the
// same bits
__device__ inline double wave_sum_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline uint32_t wave_sum_u32(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ inline uint64_t wave_sum_u64(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((long long)v, o, 64);
  return v;
}
__device__ inline uint32_t wave_max_u32(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ inline uint64_t wave_max_u64(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t w = (uint64_t)__shfl_xor((long long)v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// the exit rule of a pair's fixed point (PhiComp of -batch-gpu and its steps, PhiComp2 of -orig)
constexpr uint32_t MAX_ROUNDS = 50;                 // src/env.hh:415 online_iterations
constexpr double MEAN_CHANGE_THRESH = 0.00001;      // src/env.hh:337 meanchangethresh

}  // namespace svils
