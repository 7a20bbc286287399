// qsad_rate.hip — issue cost of v_qsad_pk_u16_u8 against the v_alignbyte_b32 + v_sad_u8 form of
// the sliding 4-position SAD step used by k_coarse_me / k_inter_me (csrc/gpu/k_inter.hip).
//
// One "row step" = the SADs of an 8-pixel source row (s0, s1) against 4 horizontally adjacent
// positions of a 12-byte window row (w0, w1, w2):
//   legacy   6 v_alignbyte_b32 + 8 v_sad_u8, 4 x u32 accumulators
//   packed   2 v_qsad_pk_u16_u8, one 4 x u16 accumulator
// Each loop pass runs 4 independent row steps (no dependence between them, accumulator chains
// of length 2 inside one), 4096 passes.  Both forms are first checked against each other on
// random words, then timed at 1 and at 8 waves per SIMD.
//
//   hipcc -O3 --offload-arch=gfx950 tools/native/qsad_rate.hip -o qsad_rate && ./qsad_rate
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                             \
  do {                                                                    \
    hipError_t e_ = (x);                                                  \
    if (e_ != hipSuccess) {                                               \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));        \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

constexpr int kSets = 4, kPasses = 4096;

__device__ __forceinline__ void opaque(uint32_t& v) { asm volatile("" : "+v"(v)); }

template <bool kPacked>
__global__ void __launch_bounds__(256) k_rate(const uint32_t* in, uint32_t* out, long long* cyc, int passes) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  uint32_t w[kSets][3], s[kSets][2];
#pragma unroll
  for (int i = 0; i < kSets; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) w[i][j] = in[(threadIdx.x * 5 * kSets + 5 * i + j) & 4095];
    s[i][0] = in[(threadIdx.x * 5 * kSets + 5 * i + 3) & 4095];
    s[i][1] = in[(threadIdx.x * 5 * kSets + 5 * i + 4) & 4095];
  }
  uint32_t acc[kSets][4] = {};
  uint64_t pk[kSets] = {};
  const long long t0 = clock64();
  for (int p = 0; p < passes; ++p) {
#pragma unroll
    for (int i = 0; i < kSets; ++i) {
      // the operands change every pass as far as the compiler knows: nothing is hoisted
      opaque(w[i][0]);
      opaque(w[i][1]);
      opaque(w[i][2]);
      const uint32_t w0 = w[i][0], w1 = w[i][1], w2 = w[i][2], s0 = s[i][0], s1 = s[i][1];
      if (kPacked) {
        pk[i] = __builtin_amdgcn_qsad_pk_u16_u8((uint64_t)w1 << 32 | w0, s0, pk[i]);
        pk[i] = __builtin_amdgcn_qsad_pk_u16_u8((uint64_t)w2 << 32 | w1, s1, pk[i]);
      } else {
        acc[i][0] = __builtin_amdgcn_sad_u8(w1, s1, __builtin_amdgcn_sad_u8(w0, s0, acc[i][0]));
#pragma unroll
        for (int sft = 1; sft < 4; ++sft) {
          const uint32_t lo = __builtin_amdgcn_alignbyte(w1, w0, sft);
          const uint32_t hi = __builtin_amdgcn_alignbyte(w2, w1, sft);
          acc[i][sft] = __builtin_amdgcn_sad_u8(hi, s1, __builtin_amdgcn_sad_u8(lo, s0, acc[i][sft]));
        }
      }
    }
  }
  const long long t1 = clock64();
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < kSets; ++i) {
    if (kPacked) {
      r += (uint32_t)pk[i] + (uint32_t)(pk[i] >> 32);
    } else {
      r += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    }
  }
  out[gid] = r;
  if ((threadIdx.x & 63) == 0) cyc[gid >> 6] = t1 - t0;
}

// one row step in both forms, for the equality check
__global__ void k_check(const uint32_t* in, uint32_t* legacy, uint32_t* packed, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t w0 = in[5 * i], w1 = in[5 * i + 1], w2 = in[5 * i + 2], s0 = in[5 * i + 3], s1 = in[5 * i + 4];
  uint32_t a[4];
  a[0] = __builtin_amdgcn_sad_u8(w1, s1, __builtin_amdgcn_sad_u8(w0, s0, 0u));
#pragma unroll
  for (int sft = 1; sft < 4; ++sft)
    a[sft] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w2, w1, sft), s1,
                                     __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w1, w0, sft), s0, 0u));
  uint64_t pk = __builtin_amdgcn_qsad_pk_u16_u8((uint64_t)w1 << 32 | w0, s0, 0ull);
  pk = __builtin_amdgcn_qsad_pk_u16_u8((uint64_t)w2 << 32 | w1, s1, pk);
#pragma unroll
  for (int sft = 0; sft < 4; ++sft) {
    legacy[4 * i + sft] = a[sft];
    packed[4 * i + sft] = (uint32_t)(pk >> (16 * sft)) & 0xffffu;
  }
}

template <bool kPacked>
static void run(const char* name, const uint32_t* d_in, uint32_t* d_out, long long* d_cyc, int waves_per_simd, double mhz) {
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int blocks = prop.multiProcessorCount * waves_per_simd;  // a 256-thread block = 1 wave on each SIMD of a CU
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  k_rate<kPacked><<<blocks, 256>>>(d_in, d_out, d_cyc, 64);  // warm-up
  CK(hipEventRecord(e0));
  k_rate<kPacked><<<blocks, 256>>>(d_in, d_out, d_cyc, kPasses);
  CK(hipEventRecord(e1));
  CK(hipEventSynchronize(e1));
  float ms = 0;
  CK(hipEventElapsedTime(&ms, e0, e1));
  std::vector<long long> cyc((size_t)blocks * 4);
  CK(hipMemcpy(cyc.data(), d_cyc, cyc.size() * sizeof(long long), hipMemcpyDeviceToHost));
  double sum = 0;
  long long mx = 0;
  for (long long c : cyc) {
    sum += (double)c;
    mx = c > mx ? c : mx;
  }
  const double steps = (double)kPasses * kSets;  // row steps per wave
  const int per_step = kPacked ? 2 : 14;
  // a SIMD issues for waves_per_simd waves in the kernel's time: cycles per instruction seen by the SIMD
  const double cyc_evt = ms * 1e-3 * mhz * 1e6 / (steps * waves_per_simd);
  std::printf(
      "%-7s waves/SIMD %d: %.3f ms, %.2f clk/row-step/SIMD (%.2f clk/instr at %.0f MHz); per-wave counter: mean %.0f max %lld "
      "ticks = %.3f ticks/row-step\n",
      name, waves_per_simd, ms, cyc_evt, cyc_evt / per_step, mhz, sum / cyc.size(), mx, sum / cyc.size() / steps);
}

int main() {
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const double mhz = prop.clockRate / 1000.0;
  std::printf("%s, %d CUs, %.0f MHz\n", prop.gcnArchName, prop.multiProcessorCount, mhz);
  const int n = 1 << 16;
  std::vector<uint32_t> h((size_t)5 * n);
  uint32_t x = 12345;
  for (auto& v : h) {
    x = x * 1664525u + 1013904223u;
    v = x ^ (x >> 15);
  }
  // saturating rows too: all 0 against all 255
  for (int j = 0; j < 5; ++j) h[j] = j < 3 ? 0u : 0xffffffffu;
  uint32_t *d_in, *d_a, *d_b, *d_out;
  long long* d_cyc;
  CK(hipMalloc(&d_in, h.size() * 4));
  CK(hipMalloc(&d_a, (size_t)4 * n * 4));
  CK(hipMalloc(&d_b, (size_t)4 * n * 4));
  CK(hipMalloc(&d_out, (size_t)prop.multiProcessorCount * 8 * 256 * 4));
  CK(hipMalloc(&d_cyc, (size_t)prop.multiProcessorCount * 8 * 4 * sizeof(long long)));
  CK(hipMemcpy(d_in, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  k_check<<<n / 256, 256>>>(d_in, d_a, d_b, n);
  std::vector<uint32_t> a((size_t)4 * n), b((size_t)4 * n);
  CK(hipMemcpy(a.data(), d_a, a.size() * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(b.data(), d_b, b.size() * 4, hipMemcpyDeviceToHost));
  long bad = 0;
  for (size_t i = 0; i < a.size(); ++i) bad += a[i] != b[i];
  std::printf("check: %zu SADs, %ld differ (first row: %u %u %u %u)\n", a.size(), bad, b[0], b[1], b[2], b[3]);
  if (bad) return 2;
  for (int wps : {1, 8}) {
    run<false>("legacy", d_in, d_out, d_cyc, wps, mhz);
    run<true>("packed", d_in, d_out, d_cyc, wps, mhz);
  }
  return 0;
}
