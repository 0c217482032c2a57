// k_lora_delta for gfx950 (CDNA4 / MI355X): the per-row low-rank term of one projection of the fused decode step
// (docs/LORA.md).
//
//   delta[m][n] = sum_r B'_a[n][r] * bf16(sum_k A'_a[r][k] * x[m][k]),  a = aid[m];  exactly 0.0f where aid[m] = -1
//
// for up to 64 rows that may each name another adapter. It runs ahead of the projection's k_skinny<.., LORA = 1> on
// the same stream, which adds delta to its fp32 accumulator ahead of its epilogue.
//
// Grid (column tiles of delta, 16-row tiles of the step); a workgroup is kWaves waves and owns 16 rows by
// kWaves * kColTiles * 16 columns. Per distinct adapter of its row tile (rows of other adapters, of no adapter and
// past M are masked to zero in the A operand, as k_attn_chunk masks mixed cache slots):
//   shrink  t[16][R] = x_tile * A'^T on v_mfma_f32_16x16x32_bf16, k_skinny's pattern: the waves split K, each lane
//           streams its A' rows with 16-byte buffer loads straight into B fragments, two k-steps of loads in flight
//           ahead of their MFMAs, and the partials are summed through LDS. One pass over x serves kRankGroup 16-rank
//           tiles (64 ranks), so R = 192 takes three passes. Every workgroup of a row tile recomputes t: A' is small
//           and stays in L2 / MALL. Measured, this costs more than a second dependent launch would: the shrink,
//           all of A' through one CU per workgroup, dominates the step's added time (docs/LORA.md).
//   t       is rounded to bf16 once, as PEFT's bf16 forward rounds the output of lora_A, and kept in LDS in the MFMA's
//           A-operand order (row m, rank r contiguous).
//   expand  each wave multiplies t into its kColTiles 16-column subtiles of B' on the same MFMA with K = R (B' rows
//           streamed with 16-byte loads, no reduction: a wave owns its columns) and accumulates over the tile's
//           adapters: a row is non-zero in one pass only.
// A row tile without any adapter writes zeros and loads no adapter bytes. No atomics, no host read-back: capturable,
// and the result does not depend on the grid.
// Every global load goes through a buffer descriptor sized from the arguments (rows past M, ranks past R, columns
// past N and k-steps past a wave's share read as zeros, without a memory access); the stores are guarded by M and N.
#include "decode_lora.h"

#include "bf16_common.h"

namespace {

using namespace p2pt_gpu;
using namespace p2pt_lora;

typedef short frag8 __attribute__((ext_vector_type(8)));
typedef float frag4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kOob = 0x80000000u;  // the host keeps every operand below 2 GiB
constexpr int kTStride = kMaxRank + 8;  // bf16 per row of t in LDS: 400 bytes, rows stay 16-byte aligned
static_assert(kRankGroup == kWaves, "wave g sums rank tile g of a shrink pass");
static_assert((kTStride * 2) % 16 == 0 && kTStride >= ((kMaxRank + 31) & ~31), "t rows: aligned, whole k-steps");

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint4 buf_ld16(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}
__device__ __forceinline__ frag8 as_frag(const uint4& v) { return __builtin_bit_cast(frag8, v); }

__global__ __launch_bounds__(kWaves * 64) void k_lora_delta(LoraArgs a) {
  __shared__ float red[kWaves][kRankGroup][4][kWave];
  __shared__ __attribute__((aligned(16))) uint16_t t_s[16][kTStride];
  __shared__ int aid_s[16];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = blockIdx.y << 4;
  const int c = lane & 15, lrow0 = (lane >> 4) << 2, kq = (lane >> 4) << 3;
  const int col0 = (blockIdx.x * kWaves + wv) * (kColTiles * 16);  // this wave's first delta column
  const int K = a.K, R = a.R, N = a.N;

  // The adapter of MFMA row c, the same in all four lane groups of every wave, so the ballots below are uniform over
  // the workgroup. Rows past M and ids outside the table count as no adapter.
  const int mrow = m0 + c;
  int my_aid = mrow < a.M ? a.aid[mrow] : -1;
  if (my_aid < 0 || my_aid >= a.n_adapters) my_aid = -1;
  if (threadIdx.x < 16) aid_s[threadIdx.x] = my_aid;
  // t's columns from R up to the next whole k-step are read by the expand and never written: zero them once.
  for (int i = threadIdx.x; i < 16 * kTStride / 2; i += kWaves * 64) reinterpret_cast<uint32_t*>(&t_s[0][0])[i] = 0u;
  __syncthreads();

  frag4 out[kColTiles];
#pragma unroll
  for (int t = 0; t < kColTiles; t++) out[t] = frag4{0.f, 0.f, 0.f, 0.f};

  if (__ballot(my_aid >= 0) != 0ull) {
    const int S = K >> 5, s0 = wv * S / kWaves, s1 = (wv + 1) * S / kWaves;  // this wave's k-steps of the shrink
    const __amdgpu_buffer_rsrc_t rx = rsrc(a.x, uint32_t(a.M) * uint32_t(K) * 2u);
    for (int ad = 0; ad < a.n_adapters; ad++) {
      if (__ballot(my_aid == ad) == 0ull) continue;
      const uint32_t xoff = my_aid == ad ? (uint32_t(mrow) * uint32_t(K) + uint32_t(kq)) * 2u : kOob;
      const __amdgpu_buffer_rsrc_t rA = rsrc(a.A + size_t(ad) * R * K, uint32_t(R) * uint32_t(K) * 2u);
      const __amdgpu_buffer_rsrc_t rB = rsrc(a.B + size_t(ad) * N * R, uint32_t(N) * uint32_t(R) * 2u);

      // Shrink: 64 ranks per pass over the wave's share of K.
      for (int rb = 0; rb < R; rb += 16 * kRankGroup) {
        frag4 acc[kRankGroup];
        uint32_t aoff[kRankGroup];
#pragma unroll
        for (int g = 0; g < kRankGroup; g++) {
          acc[g] = frag4{0.f, 0.f, 0.f, 0.f};
          const int r = rb + 16 * g + c;
          aoff[g] = r < R ? (uint32_t(r) * uint32_t(K) + uint32_t(kq)) * 2u : kOob;
        }
        for (int s = s0; s < s1; s += 2) {
          uint4 xv[2], av[2][kRankGroup];
#pragma unroll
          for (int u = 0; u < 2; u++) {
            const bool in = s + u < s1;
            const uint32_t su = uint32_t(s + u) * 64u;
            xv[u] = buf_ld16(rx, in && xoff != kOob ? xoff + su : kOob);
#pragma unroll
            for (int g = 0; g < kRankGroup; g++) av[u][g] = buf_ld16(rA, in && aoff[g] != kOob ? aoff[g] + su : kOob);
          }
          __builtin_amdgcn_sched_barrier(0);  // every load of the batch ahead of the first MFMA, as in k_skinny
#pragma unroll
          for (int u = 0; u < 2; u++)
#pragma unroll
            for (int g = 0; g < kRankGroup; g++)
              acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(xv[u]), as_frag(av[u][g]), acc[g], 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < kRankGroup; g++)
#pragma unroll
          for (int r = 0; r < 4; r++) red[wv][g][r][lane] = acc[g][r];
        __syncthreads();
        // Wave g sums rank tile g (C layout: row lrow0 + r, rank rb + 16 g + c) and rounds it to bf16 once. Rows of
        // other adapters are stored as zeros whatever A' holds.
        const int rank = rb + 16 * wv + c;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          float sum = 0.f;
#pragma unroll
          for (int w = 0; w < kWaves; w++) sum += red[w][wv][r][lane];
          if (rank < R) t_s[lrow0 + r][rank] = aid_s[lrow0 + r] == ad ? uint16_t(f2bf_bits(sum)) : uint16_t(0);
        }
        __syncthreads();
      }

      // Expand: this wave's columns, K = R. The next adapter's first store to t comes after a barrier every wave
      // reaches only with its expand behind it.
      for (int s = 0; s < (R + 31) >> 5; s++) {
        const int k0 = 32 * s + kq;
        const uint4 tv = *reinterpret_cast<const uint4*>(&t_s[c][k0]);
        uint4 bv[kColTiles];
#pragma unroll
        for (int t = 0; t < kColTiles; t++) {
          const int n = col0 + 16 * t + c;
          bv[t] = buf_ld16(rB, n < N && k0 < R ? (uint32_t(n) * uint32_t(R) + uint32_t(k0)) * 2u : kOob);
        }
#pragma unroll
        for (int t = 0; t < kColTiles; t++)
          out[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(tv), as_frag(bv[t]), out[t], 0, 0, 0);
      }
    }
  }

  // C layout: row lrow0 + r, column col0 + 16 t + c. A row without an adapter gets 0.0f whatever B' holds.
#pragma unroll
  for (int t = 0; t < kColTiles; t++) {
    const int n = col0 + 16 * t + c;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int m = m0 + lrow0 + r;
      if (m < a.M && n < N) a.delta[size_t(m) * N + n] = aid_s[lrow0 + r] >= 0 ? out[t][r] : 0.f;
    }
  }
}

}  // namespace

namespace p2pt_lora {

bool shapes_ok(int M, int N, int K, int R, int n_adapters) {
  if (M < 1 || M > 64 || N < 16 || N % 16 || K < 32 || K % 32 || R < 16 || R % 16 || R > kMaxRank) return false;
  if (n_adapters < 1 || n_adapters > kMaxAdapters) return false;
  // 32-bit byte offsets below kOob into x, one adapter's A' and one adapter's B'.
  return size_t(M) * K * 2 < kOob && size_t(R) * K * 2 < kOob && size_t(N) * R * 2 < kOob;
}

LoraPlan plan(int M, int N, int K, int R) {
  (void)K;
  const int cols = kWaves * kColTiles * 16;
  return {(N + cols - 1) / cols, (M + 15) >> 4, kWaves, cols, (R + 16 * kRankGroup - 1) / (16 * kRankGroup)};
}

hipError_t launch_delta(const LoraArgs& a, hipStream_t s) {
  if (!shapes_ok(a.M, a.N, a.K, a.R, a.n_adapters)) return hipErrorInvalidValue;
  if (!a.x || !a.aid || !a.A || !a.B || !a.delta) return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(a.x) % 16 || reinterpret_cast<uintptr_t>(a.A) % 16 ||
      reinterpret_cast<uintptr_t>(a.B) % 16)
    return hipErrorInvalidValue;
  const LoraPlan p = plan(a.M, a.N, a.K, a.R);
  hipLaunchKernelGGL(k_lora_delta, dim3(p.grid_x, p.grid_y), dim3(p.waves * 64), 0, s, a);
  return hipGetLastError();
}

}  // namespace p2pt_lora

extern "C" {

// Standalone k_lora_delta (ops.lora_delta; tests, benchmarks) on caller tensors: LoraArgs' shapes.
int p2pt_lora_delta(const void* x, const int* aid, const void* A, const void* B, float* delta, int M, int N, int K,
                    int R, int n_adapters, void* stream) {
  const p2pt_lora::LoraArgs a{static_cast<const uint16_t*>(x), aid, static_cast<const uint16_t*>(A),
                              static_cast<const uint16_t*>(B), delta, M, N, K, R, n_adapters};
  return int(p2pt_lora::launch_delta(a, static_cast<hipStream_t>(stream)));
}

// What it launches (host only: no device is touched).
int p2pt_lora_plan(int M, int N, int K, int R, int n_adapters, p2pt_lora::LoraPlan* out) {
  if (!p2pt_lora::shapes_ok(M, N, K, R, n_adapters)) return int(hipErrorInvalidValue);
  *out = p2pt_lora::plan(M, N, K, R);
  return 0;
}

int p2pt_lora_max_adapters() { return p2pt_lora::kMaxAdapters; }
int p2pt_lora_max_rank() { return p2pt_lora::kMaxRank; }

}  // extern "C"
