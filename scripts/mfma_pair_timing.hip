// Stand-alone timing of the two fp16 MFMA forms the persistent decoder's split products can issue on
// ("K-pair products"): 64 back-to-back v_mfma_f32_16x16x16_f16 against 32
// v_mfma_f32_16x16x32_f16 -- the same 64 k-groups of work -- one wave per SIMD (one work-group of 4
// waves), operands in registers, NACC accumulators in rotation (2 = kg_mfma_x3_pre's c0 / c1).
//   hipcc -O3 --offload-arch=gfx950 scripts/mfma_pair_timing.hip -o mfma_pair_timing && ./mfma_pair_timing
// Prints shader-clock cycles (s_memtime) and ns (s_memrealtime, 100 MHz) per batch, minimum over REPS.
#include <hip/hip_runtime.h>

#include <cstdio>

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int REPS = 64, INNER = 16;  // INNER batches between two clock reads

template <int NACC, bool X32>
__global__ __launch_bounds__(256) void k_time(const float* in, float* out, long long* cyc, long long* rt) {
  const int lane = threadIdx.x & 63;
  f16x8 a8, b8;
  for (int e = 0; e < 8; ++e) {
    a8[e] = (_Float16)in[lane * 8 + e];
    b8[e] = (_Float16)in[512 + lane * 8 + e];
  }
  const f16x4 a4 = {a8[0], a8[1], a8[2], a8[3]}, b4 = {b8[0], b8[1], b8[2], b8[3]};
  f32x4 c[NACC];
  for (int i = 0; i < NACC; ++i) c[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  long long best = 1LL << 62, bestrt = 1LL << 62;
  for (int r = 0; r < REPS; ++r) {
    __builtin_amdgcn_sched_barrier(0);
    const long long r0 = __builtin_amdgcn_s_memrealtime();
    const long long t0 = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
    for (int q = 0; q < INNER; ++q) {
      if constexpr (X32) {
#pragma unroll
        for (int i = 0; i < 32; ++i) c[i % NACC] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, b8, c[i % NACC], 0, 0, 0);
      } else {
#pragma unroll
        for (int i = 0; i < 64; ++i) c[i % NACC] = __builtin_amdgcn_mfma_f32_16x16x16f16(a4, b4, c[i % NACC], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15\n s_nop 15" ::: "memory");  // the last MFMA's result is not waited for otherwise
    const long long t1 = __builtin_amdgcn_s_memtime();
    const long long r1 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_sched_barrier(0);
    if (t1 - t0 < best) best = t1 - t0;
    if (r1 - r0 < bestrt) bestrt = r1 - r0;
  }
  float s = 0.f;
  for (int i = 0; i < NACC; ++i) s += c[i][0] + c[i][1] + c[i][2] + c[i][3];
  out[threadIdx.x] = s;
  if (lane == 0) {
    cyc[threadIdx.x >> 6] = best;
    rt[threadIdx.x >> 6] = bestrt;
  }
}

#define CHECK(x)                                                      \
  do {                                                                \
    hipError_t e_ = (x);                                              \
    if (e_ != hipSuccess) {                                           \
      std::printf("%s: %s\n", #x, hipGetErrorString(e_));             \
      return 1;                                                       \
    }                                                                 \
  } while (0)

template <int NACC, bool X32>
int run(const char* name, float* in, float* out, long long* cyc, long long* rt) {
  long long hc[4], hr[4];
  for (int k = 0; k < 2; ++k) {  // the second launch is the measurement (clocks up, code resident)
    k_time<NACC, X32><<<1, 256>>>(in, out, cyc, rt);
    CHECK(hipDeviceSynchronize());
  }
  CHECK(hipMemcpy(hc, cyc, sizeof(hc), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(hr, rt, sizeof(hr), hipMemcpyDeviceToHost));
  const int n = X32 ? 32 : 64;
  std::printf("%-28s acc=%d  %d MFMAs: %7.1f memtime ticks, %7.1f ns per batch (wave 0; waves 1..3: %.1f %.1f %.1f ticks)\n", name,
              NACC, n, (double)hc[0] / INNER, 10.0 * hr[0] / INNER, (double)hc[1] / INNER, (double)hc[2] / INNER,
              (double)hc[3] / INNER);
  return 0;
}

int main() {
  float *in, *out;
  long long *cyc, *rt;
  CHECK(hipMalloc(&in, 1024 * sizeof(float)));
  CHECK(hipMalloc(&out, 256 * sizeof(float)));
  CHECK(hipMalloc(&cyc, 4 * sizeof(long long)));
  CHECK(hipMalloc(&rt, 4 * sizeof(long long)));
  float h[1024];
  for (int i = 0; i < 1024; ++i) h[i] = 0.001f * (float)((i * 37) % 101 - 50);
  CHECK(hipMemcpy(in, h, sizeof(h), hipMemcpyHostToDevice));
  int rc = 0;
  rc |= run<2, false>("v_mfma_f32_16x16x16_f16", in, out, cyc, rt);
  rc |= run<2, true>("v_mfma_f32_16x16x32_f16", in, out, cyc, rt);
  rc |= run<4, false>("v_mfma_f32_16x16x16_f16", in, out, cyc, rt);
  rc |= run<4, true>("v_mfma_f32_16x16x32_f16", in, out, cyc, rt);
  (void)hipFree(in);
  (void)hipFree(out);
  (void)hipFree(cyc);
  (void)hipFree(rt);
  return rc;
}
