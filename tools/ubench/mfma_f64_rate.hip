// mfma_f64_rate.hip -- the issue rate of v_mfma_f64_16x16x4_f64 on the card (gfx950), the ceiling
// of the correlation matrix's sums (deequ_amd/csrc/dq_corrmat.hip).  A register-only loop: every wave
// runs kChains independent accumulators through kIters MFMAs each, one or two waves per SIMD, so
// the number is the matrix pipe's throughput: cycles per MFMA per SIMD = elapsed shader cycles /
// (MFMAs per wave * waves per SIMD), and FLOP/s of the chip = 2048 FLOP * MFMAs / elapsed time.
// Build: hipcc -O3 --offload-arch=gfx950 mfma_f64_rate.hip -o mfma_f64_rate
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

using f64x4 = __attribute__((ext_vector_type(4))) double;
constexpr int kIters = 4096;
constexpr int kChains = 8;

struct Stamp { unsigned long long t0, t1; };

__global__ __launch_bounds__(512) void k_mfma_f64(Stamp* st, double* sink, double seed) {
  f64x4 acc[kChains];
  for (int c = 0; c < kChains; ++c) acc[c] = f64x4{seed, 0.0, 0.0, (double)c};
  const double a = seed + threadIdx.x * 1e-9, b = 1.0 - seed;
  __syncthreads();
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int i = 0; i < kIters; ++i) {
#pragma unroll
    for (int c = 0; c < kChains; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[c], 0, 0, 0);
  }
  __syncthreads();
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) st[blockIdx.x] = {t0, t1};
  double r = 0.0;
  for (int c = 0; c < kChains; ++c) r += acc[c][0] + acc[c][3];
  if (r == 0.12345) sink[0] = r;
}

int main() {
  hipDeviceProp_t p;
  CHK(hipGetDeviceProperties(&p, 0));
  const int cus = p.multiProcessorCount;
  Stamp* d_st;
  double* d_sink;
  CHK(hipMalloc(&d_st, sizeof(Stamp) * cus));
  CHK(hipMalloc(&d_sink, 8));
  for (int threads : {256, 512}) {  // one and two waves per SIMD
    hipEvent_t e0, e1;
    CHK(hipEventCreate(&e0));
    CHK(hipEventCreate(&e1));
    std::vector<float> ms;
    for (int rep = 0; rep < 6; ++rep) {
      CHK(hipEventRecord(e0));
      hipLaunchKernelGGL(k_mfma_f64, dim3(cus), dim3(threads), 0, 0, d_st, d_sink, 0.5);
      CHK(hipEventRecord(e1));
      CHK(hipEventSynchronize(e1));
      float t;
      CHK(hipEventElapsedTime(&t, e0, e1));
      if (rep) ms.push_back(t);
    }
    std::vector<Stamp> st(cus);
    CHK(hipMemcpy(st.data(), d_st, sizeof(Stamp) * cus, hipMemcpyDeviceToHost));
    std::vector<double> cyc;
    for (const Stamp& s : st) cyc.push_back((double)(s.t1 - s.t0));
    std::sort(cyc.begin(), cyc.end());
    std::sort(ms.begin(), ms.end());
    const double per_wave = (double)kIters * kChains, waves_per_simd = threads / 256.0;
    const double mfmas = per_wave * (threads / 64.0) * cus;
    printf("{\"threads\": %d, \"cus\": %d, \"memtime_ticks_per_mfma_per_simd\": %.2f, \"ms_min\": %.3f, \"ms_median\": %.3f, "
           "\"ms_max\": %.3f, \"tflops_median\": %.1f, \"mfma_per_s_median\": %.4g}\n",
           threads, cus, cyc[cyc.size() / 2] / (per_wave * waves_per_simd), ms.front(), ms[ms.size() / 2], ms.back(),
           2048.0 * mfmas / (ms[ms.size() / 2] * 1e-3) / 1e12, mfmas / (ms[ms.size() / 2] * 1e-3));
  }
  return 0;
}
