// micro-benchmark: the sustained rate of v_mfma_f64_16x16x4_f64 (the instruction of k_topk_tiles, svils_predict.hip).
// Every wavefront runs ITERS rounds of CH independent accumulator chains (16 x 16 x 4 x 2 = 2048 flop per instruction)
// from registers only; grids of 1 .. 8 wavefronts per SIMD on every CU.  One JSON line per configuration, the best first
// repetition of three discarded.
//   hipcc --offload-arch=gfx950 -O3 -o /tmp/f64mfma tools/ubench/f64mfma.hip && /tmp/f64mfma
#include <hip/hip_runtime.h>
#include <cstdio>
#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

typedef double d4 __attribute__((ext_vector_type(4)));

template <int CH>
__global__ __launch_bounds__(256) void k(int iters, double *out) {
  d4 acc[CH];
  const double a = 1.0 + 1e-9 * threadIdx.x, b = 1.0 - 1e-9 * blockIdx.x;
#pragma unroll
  for (int c = 0; c < CH; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < iters; ++i)
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[c], 0, 0, 0);
  double s = 0;
#pragma unroll
  for (int c = 0; c < CH; ++c) s += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
  if (s == 0.5) out[blockIdx.x] = s;   // never true: keeps the chains alive
}

template <int CH>
static int run(int cus, int waves_per_simd, double *out) {
  const int iters = 4096, blocks = cus * waves_per_simd;   // 256 threads = one wavefront on each of the four SIMDs
  hipEvent_t e0, e1;
  CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
  float best = 1e30f;
  for (int rep = 0; rep < 4; ++rep) {
    CHK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL((k<CH>), dim3(blocks), dim3(256), 0, 0, iters, out);
    CHK(hipEventRecord(e1, 0));
    CHK(hipEventSynchronize(e1));
    float ms = 0;
    CHK(hipEventElapsedTime(&ms, e0, e1));
    if (rep > 0 && ms < best) best = ms;
  }
  const double flop = (double)blocks * 4 * iters * CH * 2048.0;
  printf("{\"instr\": \"v_mfma_f64_16x16x4_f64\", \"chains\": %d, \"waves_per_simd\": %d, \"cus\": %d, \"ms\": %.4f, \"tflops\": %.2f}\n",
         CH, waves_per_simd, cus, best, flop / (best * 1e-3) / 1e12);
  return 0;
}

int main() {
  int cus = 0;
  CHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  double *out = nullptr;
  CHK(hipMalloc(&out, 1 << 20));
  for (int w : {1, 2, 4, 8}) {
    if (run<1>(cus, w, out) || run<4>(cus, w, out) || run<8>(cus, w, out)) return 1;
  }
  CHK(hipFree(out));
  return 0;
}
