// Micro-benchmark: the rate of v_mfma_f64_16x16x4_f64 beside v_fma_f64 on MI355X, registers only (no memory traffic), at
// 1..3 waves per SIMD - what a Gram kernel (erpl_surrogate.hip) could gain from the matrix instruction at the most.
// Diagnostic tool (not part of the product):
//   hipcc --offload-arch=gfx950 -O3 mfma_f64.hip -o mfma_f64
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)

typedef double double4v __attribute__((ext_vector_type(4)));

// KIND 0: 8 independent v_fma_f64 chains (64 fused multiply-adds per instruction and wave)
// KIND 1: 4 independent accumulators of v_mfma_f64_16x16x4_f64 (1024 fused multiply-adds per instruction and wave)
// KIND 2: 8 independent accumulators of the same
template <int KIND>
__global__ __launch_bounds__(64) void k(double* out, int iters, double seed) {
  double a = seed + 1e-9 * threadIdx.x, b = 1.0 - 1e-9 * threadIdx.x;
  double r = 0.0;
  if (KIND == 0) {
    double c[8];
    for (int i = 0; i < 8; ++i) c[i] = seed + i;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = __builtin_fma(c[i], b, a);
    }
    for (int i = 0; i < 8; ++i) r += c[i];
  } else {
    constexpr int N = KIND == 1 ? 4 : 8;
    double4v c[N];
    for (int i = 0; i < N; ++i) c[i] = double4v{seed, seed + i, 0.0, 1.0};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int u = 0; u < 64 / N; ++u)
#pragma unroll
        for (int i = 0; i < N; ++i) c[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c[i], 0, 0, 0);
    }
    for (int i = 0; i < N; ++i) r += c[i].x + c[i].y + c[i].z + c[i].w;
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = r;
}

template <int KIND>
void run(const char* name, double* d, int cus, double fma_per_instr) {
  const int iters = 4000;
  for (int w = 1; w <= 3; ++w) {
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    hipLaunchKernelGGL(k<KIND>, dim3(cus * 4 * w), dim3(64), 0, 0, d, 300, 1e-3);
    CHECK(hipDeviceSynchronize());
    CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL(k<KIND>, dim3(cus * 4 * w), dim3(64), 0, 0, d, iters, 1e-3);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
    const double instr = (double)iters * 64, waves = (double)cus * 4 * w;
    printf("%-44s waves/SIMD=%d  %8.3f ms  %7.2f cyc/instr/SIMD  %7.2f TFLOP/s\n", name, w, ms, ms * 1e-3 * 2.4e9 / (instr * w),
           2.0 * fma_per_instr * instr * waves / (ms * 1e-3) / 1e12);
  }
}

int main() {
  hipDeviceProp_t p; CHECK(hipGetDeviceProperties(&p, 0));
  const int cus = p.multiProcessorCount;
  printf("device %s, %d CUs (cycles are nominal 2.4 GHz cycles)\n", p.name, cus);
  double* d; CHECK(hipMalloc(&d, (size_t)cus * 4 * 3 * 64 * sizeof(double)));
  run<0>("v_fma_f64, 8 chains", d, cus, 64.0);
  run<1>("v_mfma_f64_16x16x4_f64, 4 accumulators", d, cus, 1024.0);
  run<2>("v_mfma_f64_16x16x4_f64, 8 accumulators", d, cus, 1024.0);
  return 0;
}
