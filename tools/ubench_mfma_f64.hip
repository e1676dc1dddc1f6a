// ubench_mfma_f64.hip -- the fp64 matrix-core rate of gfx950: back-to-back v_mfma_f64_16x16x4_f64 (2 * 16 * 16 * 4 = 2048 FLOP each)
// on one SIMD and on every SIMD of the chip.  The guides give no fp64 matrix peak; tools/bench_poisson.py divides by this one.
//   hipcc -O3 --offload-arch=gfx950 tools/ubench_mfma_f64.hip -o /tmp/ubench_mfma_f64 && /tmp/ubench_mfma_f64 [out.json]
// Each wave runs 8 INDEPENDENT accumulator chains (inline asm, so the instruction is exactly the one named), timed with s_memtime
// inside the kernel (one wave on one SIMD: cycles per MFMA) and with hipEvents around a chip-wide launch (4 waves per CU, one per
// SIMD, every CU, and 8 waves per CU): FLOP / s.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

typedef double d4 __attribute__((ext_vector_type(4)));

#define CHECK(x)                                                              \
  do {                                                                        \
    hipError_t e = (x);                                                       \
    if (e != hipSuccess) {                                                    \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e)); \
      return 1;                                                               \
    }                                                                         \
  } while (0)

#define MF(C) "v_mfma_f64_16x16x4_f64 %" #C ", %8, %9, %" #C "\n"

__global__ void __launch_bounds__(512) mfma_f64(double* out, unsigned long long* cycles, int iters, double seed) {
  d4 c0 = {seed, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0, c4 = c0, c5 = c0, c6 = c0, c7 = c0;
  const double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
  __syncthreads();
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int k = 0; k < iters; ++k) {
    asm volatile(MF(0) MF(1) MF(2) MF(3) MF(4) MF(5) MF(6) MF(7)
                 : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7)
                 : "v"(a), "v"(b));
  }
  asm volatile("s_nop 7\ns_nop 7" ::: "memory");
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  const d4 s = c0 + c1 + c2 + c3 + c4 + c5 + c6 + c7;
  if (s.x == 12345.678) out[threadIdx.x] = s.y;   // (never: keeps the chains live)
  if (threadIdx.x == 0 && blockIdx.x == 0) cycles[0] = t1 - t0;
}

int main(int argc, char** argv) {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  double* out;
  unsigned long long* cyc;
  CHECK(hipMalloc(&out, 512 * sizeof(double)));
  CHECK(hipMalloc(&cyc, sizeof(unsigned long long)));
  const int iters = 20000;   // x 8 MFMAs per wave

  // one wave on one SIMD: cycles (s_memtime ticks at the 100 MHz constant clock are converted with the shader clock below)
  hipLaunchKernelGGL(mfma_f64, dim3(1), dim3(64), 0, 0, out, cyc, 100, 1.0);
  CHECK(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  CHECK(hipEventRecord(e0));
  hipLaunchKernelGGL(mfma_f64, dim3(1), dim3(64), 0, 0, out, cyc, iters, 1.0);
  CHECK(hipEventRecord(e1));
  CHECK(hipEventSynchronize(e1));
  float ms1 = 0;
  CHECK(hipEventElapsedTime(&ms1, e0, e1));
  unsigned long long ticks = 0;
  CHECK(hipMemcpy(&ticks, cyc, sizeof(ticks), hipMemcpyDeviceToHost));
  const double n1 = (double)iters * 8;
  const double one_simd_flops = n1 * 2048.0 / (ms1 * 1e-3);
  const double clk_hz = prop.clockRate * 1e3;   // (the rated shader clock)
  const double cyc_per_mfma = (ms1 * 1e-3) * clk_hz / n1;

  // chip-wide: one wave per SIMD (256 threads per CU) and two (512)
  double chip[2];
  for (int v = 0; v < 2; ++v) {
    const int threads = v == 0 ? 256 : 512;
    hipLaunchKernelGGL(mfma_f64, dim3(cus), dim3(threads), 0, 0, out, cyc, 100, 1.0);
    CHECK(hipDeviceSynchronize());
    CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL(mfma_f64, dim3(cus), dim3(threads), 0, 0, out, cyc, iters, 1.0);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    chip[v] = (double)cus * (threads / 64) * n1 * 2048.0 / (ms * 1e-3);
  }
  printf("v_mfma_f64_16x16x4_f64, 8 independent chains per wave, %d x 8 MFMAs per wave\n", iters);
  printf("  one wave, one SIMD: %.3f ms -> %.2f GFLOP/s, %.1f cycles per MFMA at the rated %.0f MHz (s_memtime ticks %llu)\n", ms1,
         one_simd_flops * 1e-9, cyc_per_mfma, clk_hz * 1e-6, ticks);
  printf("  chip-wide, %d CUs, 1 wave per SIMD: %.2f TFLOP/s\n", cus, chip[0] * 1e-12);
  printf("  chip-wide, %d CUs, 2 waves per SIMD: %.2f TFLOP/s\n", cus, chip[1] * 1e-12);
  if (argc > 1) {
    FILE* f = fopen(argv[1], "w");
    if (f) {
      fprintf(f, "{\"instruction\": \"v_mfma_f64_16x16x4_f64\", \"one_simd_gflops\": %.3f, \"cycles_per_mfma_at_rated_clock\": %.2f, "
                 "\"rated_clock_mhz\": %.0f, \"chip_tflops_1wave_per_simd\": %.3f, \"chip_tflops_2waves_per_simd\": %.3f, \"cus\": %d}\n",
              one_simd_flops * 1e-9, cyc_per_mfma, clk_hz * 1e-6, chip[0] * 1e-12, chip[1] * 1e-12, cus);
      fclose(f);
    }
  }
  CHECK(hipFree(out));
  CHECK(hipFree(cyc));
  return 0;
}
