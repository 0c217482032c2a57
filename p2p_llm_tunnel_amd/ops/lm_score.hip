// Prompt scoring for the inference endpoint (gfx950 / CDNA4): the LM-head GEMM over the fused step's final residual,
// fused with an online log-sum-exp, a target pick and an argmax. fp32 from the MFMA accumulator to the result: no
// logit is rounded to bf16 and none is stored (docs/PROMPT_LOGPROBS.md).
//
//   p2pt_lm_score   resid: bf16 [rows <= 64][dim], what the last layer's down projection left. w: the table's LM head,
//     [V][dim] with the final-norm weight folded in, bf16 (w8 = 0) or e4m3 bytes with fp32 row scales (w8 = 1).
//     target: int32 [rows]; a row with a negative target is off and none of its outputs is touched. For every other
//     row m, with z[v] = ((sum_k x[m][k] W'[v][k]) * scale[v]) * (1/rms_m):
//
//       lse[m] = log sum_v exp(z[v])     z_target[m] = z[target[m]]     z_top[m] = max_v z[v]     id_top[m] = its
//       lowest id
//
//   k_lm_score, one workgroup per (vocab slab of 256 columns, 16-row tile), the tile the fast index of a 1-D grid so
//   that the up to four tiles of a slab run side by side and share its rows of W in the caches; 4 waves. Wave w owns the slab's columns
//   [64 w, 64 w + 64) as four 16-column MFMA tiles and walks all of K for them, so no partial sum ever crosses a
//   wave. B fragments stream straight from global memory (16-byte loads; 8-byte loads of e4m3 bytes decoded exactly
//   to bf16 ahead of the MFMA) through a buffer descriptor that covers this slab's rows of W only: columns past V read
//   zeros from its range check and the descriptor never nears 32-bit limits, whatever V * dim is. The A fragment is
//   loaded per k-step (16 bytes per lane, one load beside the four B loads): the 16 x dim tile is read by every
//   wave of the slab's workgroup and stays in cache, LDS staging would cap dim at what 16 rows fit (and cost a
//   barrier ahead of the stream), and the per-step load keeps dim free up to 16384.
//   1/rms is recomputed from the bf16 rows in fp32 ahead of the stream, one wave per row (embed_pool.hip's order).
//   Epilogue: each lane folds its 4 rows x 4 columns into (max, sum exp(z - max), best z, best id, target's z), the
//   16 lanes of a row merge by DPP, the four waves through LDS in wave order, and thread r < 16 stores the
//   workgroup's partial of row r. A tile whose rows are all off exits at once.
//   k_lm_score_merge, one wave per row: lane l folds slabs l, l + 64, ... in ascending order, the lanes merge by a
//   fixed tree. Every order is fixed, so a row's result depends on the row alone: not on scheduling, not on where
//   in the step it sits, not on the other rows. Plain vector stores only; no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bf16_common.h"

// exp(z - max) and the rescaling products are single fp32 operations, as the test's bound counts them.
#pragma clang fp contract(off)

namespace {

using namespace p2pt_gpu;

constexpr int kMaxRows = 64;  // rows of resid (decode_fused.hip's kMaxM)
constexpr int kWaves = 4, kThreads = kWaves * kWave;
constexpr int kTN = 4;                       // 16-column MFMA tiles per wave
constexpr int kSlab = kWaves * kTN * 16;     // vocabulary columns per workgroup
constexpr int kUM = 4;                       // k-steps per load batch
constexpr int kMaxDim = 16384;
constexpr float kDown = 0x1p-96f;            // embed_pool.hip's rescue scaling of a row whose sum of squares overflows
constexpr uint32_t kOob = 0x80000000u;       // past every descriptor here: the load returns zeros

typedef short frag8 __attribute__((ext_vector_type(8)));
typedef float frag4 __attribute__((ext_vector_type(4)));
typedef float float2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint4 buf_ld16(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}
__device__ __forceinline__ uint2 buf_ld8(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
}
__device__ __forceinline__ frag8 as_frag(const uint4& v) { return __builtin_bit_cast(frag8, v); }

// Eight e4m3 bytes as eight bf16 (v_cvt_pk_f32_fp8; exact: the low 16 bits of every decoded fp32 are zero).
__device__ __forceinline__ uint4 e4m3x8_to_bf16x8(const uint2& v) {
  const float2v a = __builtin_amdgcn_cvt_pk_f32_fp8(int(v.x), false), b = __builtin_amdgcn_cvt_pk_f32_fp8(int(v.x), true);
  const float2v c = __builtin_amdgcn_cvt_pk_f32_fp8(int(v.y), false), d = __builtin_amdgcn_cvt_pk_f32_fp8(int(v.y), true);
  auto pk = [](float lo, float hi) { return (__float_as_uint(hi) & 0xffff0000u) | (__float_as_uint(lo) >> 16); };
  return make_uint4(pk(a[0], a[1]), pk(b[0], b[1]), pk(c[0], c[1]), pk(d[0], d[1]));
}

// Sum over one bf16 row of (x * scale)^2: lane-strided 16-byte chunks, then the wave (embed_pool.hip's row_sumsq).
__device__ __forceinline__ float row_sumsq(const uint4* __restrict__ x, int words, float scale) {
  float ss = 0.f;
  for (int i = threadIdx.x % kWave; i < words; i += kWave) {
    float f[8];
    unpack8(x[i], f);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const float v = f[k] * scale;
      ss += v * v;
    }
  }
  return wave_sum(ss);
}

// The running state of one row over a set of columns. m = -inf: no column yet (s is then 0).
struct Fold {
  float m, s, best, zt;
  int id;
};
__device__ __forceinline__ Fold fold_empty() { return Fold{-INFINITY, 0.f, -INFINITY, -INFINITY, 0x7fffffff}; }
// exp(a - b) for a <= b, 0 when a is -inf (also when both are: an empty set joins an empty set).
__device__ __forceinline__ float exp_down(float a, float b) { return a == -INFINITY ? 0.f : expf(a - b); }
// a then b, in that order: sum = a.s * exp(a.m - M) + b.s * exp(b.m - M).
__device__ __forceinline__ Fold fold_join(const Fold& a, const Fold& b) {
  Fold r;
  r.m = fmaxf(a.m, b.m);
  r.s = a.s * exp_down(a.m, r.m) + b.s * exp_down(b.m, r.m);
  r.best = a.best;
  r.id = a.id;
  am_take(r.best, r.id, b.best, b.id);
  r.zt = fmaxf(a.zt, b.zt);  // at most one side has seen the target
  return r;
}

template <int W8>
__global__ __launch_bounds__(kThreads) void k_lm_score(const uint16_t* __restrict__ resid, const uint8_t* __restrict__ w,
                                                       const float* __restrict__ wscale, const int* __restrict__ target,
                                                       float4* __restrict__ part, int* __restrict__ part_id, int rows,
                                                       int V, int dim, float eps) {
  __shared__ float s_inv[16];
  __shared__ float4 s_f[kWaves][16];
  __shared__ int s_id[kWaves][16];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // The row tile is the fast index of the 1-D grid: the tiles of one slab are dispatched side by side.
  const int tiles = (rows + 15) >> 4, slabs = gridDim.x / tiles;
  const int slab = blockIdx.x / tiles, m0 = (blockIdx.x % tiles) << 4;
  const int tile_rows = min(16, rows - m0);

  // A tile without a scoring row has nothing to do (uniform over the workgroup).
  bool any = false;
  for (int r = 0; r < tile_rows; r++) any |= target[m0 + r] >= 0;
  if (!any) return;

  // 1/rms of the tile's rows, one wave per row, the same arithmetic in every workgroup of the tile.
  const int words = dim >> 3;
  for (int r = wv; r < tile_rows; r += kWaves) {
    const uint4* __restrict__ x = reinterpret_cast<const uint4*>(resid) + size_t(m0 + r) * words;
    float scale = 1.f;
    float ss = row_sumsq(x, words, scale);
    if (!(ss <= 3.402823466e38f)) {  // overflowed (wave-uniform): measure x * 2^-96; eps vanishes next to it
      scale = kDown;
      ss = row_sumsq(x, words, scale);
    }
    if (lane == 0) s_inv[r] = rsqrtf(ss / float(dim) + (scale == 1.f ? eps : 0.f)) * scale;
  }

  // A fragment: row lane & 15, k = 32 s + 8 (lane >> 4) + j; B fragment: column lane & 15 of the tile, the same k.
  constexpr uint32_t kWb = W8 ? 1u : 2u;  // bytes per weight element
  const int col0 = slab * kSlab, slab_cols = min(kSlab, V - col0);
  const __amdgpu_buffer_rsrc_t ra = rsrc(resid, uint32_t(rows) * uint32_t(dim) * 2u);
  const __amdgpu_buffer_rsrc_t rw =
      rsrc(w + size_t(col0) * size_t(dim) * kWb, uint32_t(slab_cols) * uint32_t(dim) * kWb);
  const uint32_t kq = uint32_t(lane >> 4) << 3;
  const uint32_t xoff = m0 + (lane & 15) < rows ? (uint32_t(m0 + (lane & 15)) * uint32_t(dim) + kq) * 2u : kOob;
  uint32_t woff[kTN];
#pragma unroll
  for (int t = 0; t < kTN; t++)  // past the slab's rows of W: past the descriptor, zeros
    woff[t] = (uint32_t(wv * (kTN * 16) + t * 16 + (lane & 15)) * uint32_t(dim) + kq) * kWb;

  frag4 acc[kTN];
#pragma unroll
  for (int t = 0; t < kTN; t++) acc[t] = frag4{0.f, 0.f, 0.f, 0.f};
  const int S = dim >> 5;
  for (int s = 0; s < S; s += kUM) {
    uint4 af[kUM];
    std::conditional_t<W8 != 0, uint2, uint4> bf[kUM][kTN];
#pragma unroll
    for (int u = 0; u < kUM; u++) {
      const bool in = s + u < S;
      const uint32_t su = uint32_t(s + u) * 64u;  // bytes per 32-wide k-step of bf16; half for e4m3
#pragma unroll
      for (int t = 0; t < kTN; t++) {
        if constexpr (W8 != 0) bf[u][t] = buf_ld8(rw, in ? woff[t] + (su >> 1) : kOob);
        else bf[u][t] = buf_ld16(rw, in ? woff[t] + su : kOob);
      }
      af[u] = buf_ld16(ra, in && xoff != kOob ? xoff + su : kOob);
    }
    __builtin_amdgcn_sched_barrier(0);  // every load of the batch ahead of its first MFMA
#pragma unroll
    for (int u = 0; u < kUM; u++)
#pragma unroll
      for (int t = 0; t < kTN; t++) {
        uint4 b;
        if constexpr (W8 != 0) b = e4m3x8_to_bf16x8(bf[u][t]);
        else b = bf[u][t];
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(af[u]), as_frag(b), acc[t], 0, 0, 0);
      }
  }
  __syncthreads();  // s_inv

  // C layout: row 4 (lane >> 4) + r, column lane & 15 of tile t.
  const int lrow0 = (lane >> 4) << 2, c = lane & 15;
  float wsc[kTN];
#pragma unroll
  for (int t = 0; t < kTN; t++) {
    const int col = col0 + wv * (kTN * 16) + t * 16 + c;
    wsc[t] = W8 != 0 && col < V ? wscale[col] : 1.f;
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = lrow0 + r;  // uniform over the lane's 16-lane row
    const bool row_ok = row < tile_rows;
    const float inv = row_ok ? s_inv[row] : 0.f;
    const int tgt = row_ok ? target[m0 + row] : -1;
    // This lane's four columns, ascending.
    float z[kTN];
    Fold f = fold_empty();
#pragma unroll
    for (int t = 0; t < kTN; t++) {
      const int col = col0 + wv * (kTN * 16) + t * 16 + c;
      float v = acc[t][r];
      if constexpr (W8 != 0) v *= wsc[t];  // the scale first, as k_skinny<.., W8 = 1> has it
      z[t] = col < V ? v * inv : -INFINITY;
      f.m = fmaxf(f.m, z[t]);
      if (z[t] > f.best) {
        f.best = z[t];
        f.id = col;
      }
      if (col == tgt) f.zt = z[t];
    }
#pragma unroll
    for (int t = 0; t < kTN; t++) f.s += exp_down(z[t], f.m);
    // The 16 lanes of the row: the maximum first, then every lane's sum on that maximum.
    const float m16 = row16_max(f.m);
    f.s = row16_sum(f.s * exp_down(f.m, m16));
    f.m = m16;
    row16_argmax(f.best, f.id);
    f.zt = row16_max(f.zt);
    if (c == 0) {
      s_f[wv][row] = make_float4(f.m, f.s, f.best, f.zt);
      s_id[wv][row] = f.id;
    }
  }
  __syncthreads();
  if (threadIdx.x < tile_rows) {  // one thread per row: the waves in order
    const int row = threadIdx.x;
    Fold f = fold_empty();
#pragma unroll
    for (int q = 0; q < kWaves; q++) {
      const float4 p = s_f[q][row];
      f = fold_join(f, Fold{p.x, p.y, p.z, p.w, s_id[q][row]});
    }
    part[size_t(m0 + row) * slabs + slab] = make_float4(f.m, f.s, f.best, f.zt);
    part_id[size_t(m0 + row) * slabs + slab] = f.id;
  }
}

// One wave per row: the slabs' partials in a fixed order.
__global__ __launch_bounds__(kWave) void k_lm_score_merge(const float4* __restrict__ part,
                                                          const int* __restrict__ part_id,
                                                          const int* __restrict__ target, int slabs,
                                                          float* __restrict__ lse, float* __restrict__ z_target,
                                                          float* __restrict__ z_top, int* __restrict__ id_top) {
  const int row = blockIdx.x, lane = threadIdx.x;
  if (target[row] < 0) return;
  Fold f = fold_empty();
  for (int i = lane; i < slabs; i += kWave) {
    const float4 p = part[size_t(row) * slabs + i];
    f = fold_join(f, Fold{p.x, p.y, p.z, p.w, part_id[size_t(row) * slabs + i]});
  }
  const float m = wave_max(f.m);
  const float s = wave_sum(f.s * exp_down(f.m, m));
  wave_argmax(f.best, f.id);
  const float zt = wave_max(f.zt);
  if (lane == 0) {
    lse[row] = m + logf(s);
    z_target[row] = zt;
    z_top[row] = f.best;
    id_top[row] = f.id;
  }
}

}  // namespace

extern "C" {

// What p2pt_lm_score launches (mirrored with ctypes): k_lm_score on slabs * tiles workgroups of `threads`, then
// k_lm_score_merge on one wave per row over `slabs` partials; work_words 4-byte words of scratch.
struct LmScorePlan {
  int slab, slabs, tiles, threads, work_words;
};

// The grids of p2pt_lm_score for these shapes (host only).
int p2pt_lm_score_plan(int V, int dim, int rows, LmScorePlan* plan) {
  if (!plan || V < 1 || dim < 32 || dim % 32 || dim > kMaxDim || rows < 1 || rows > kMaxRows) return -1;
  plan->slab = kSlab;
  plan->slabs = (V + kSlab - 1) / kSlab;
  plan->tiles = (rows + 15) / 16;
  plan->threads = kThreads;
  plan->work_words = 5 * kMaxRows * plan->slabs;
  return 0;
}

// resid: bf16 [rows][dim]; w: [V][dim] bf16 (w8 = 0) or e4m3 bytes (w8 = 1) with wscale fp32 [V]; target: int32
// [rows], checked against V by the caller (the Python wrapper raises first; a target at or past V matches no column
// and leaves z_target at -inf). work: plan.work_words 4-byte words, 16-byte aligned; lse, z_target, z_top: fp32
// [rows]; id_top: int32 [rows]. Two launches on `stream`, neither allocating nor synchronising.
int p2pt_lm_score(const void* resid, int rows, int dim, const void* w, const void* wscale, int w8, int V, float eps,
                  const int* target, void* work, size_t work_words, float* lse, float* z_target, float* z_top,
                  int* id_top, void* stream) {
  LmScorePlan p;
  if (p2pt_lm_score_plan(V, dim, rows, &p) != 0 || !resid || !w || !target || !work || !lse || !z_target || !z_top ||
      !id_top || (w8 != 0 && w8 != 1) || (w8 == 1) != (wscale != nullptr) || !(eps >= 0.f) ||
      work_words < size_t(p.work_words))
    return int(hipErrorInvalidValue);
  if ((reinterpret_cast<uintptr_t>(resid) | reinterpret_cast<uintptr_t>(work)) & 15 ||
      reinterpret_cast<uintptr_t>(w) & (w8 ? 7 : 15))
    return int(hipErrorInvalidValue);
  float4* part = static_cast<float4*>(work);
  int* part_id = reinterpret_cast<int*>(part + size_t(kMaxRows) * p.slabs);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(p.slabs * p.tiles);  // tile fastest
  if (w8)
    hipLaunchKernelGGL(k_lm_score<1>, grid, dim3(kThreads), 0, st, static_cast<const uint16_t*>(resid),
                       static_cast<const uint8_t*>(w), static_cast<const float*>(wscale), target, part, part_id, rows, V,
                       dim, eps);
  else
    hipLaunchKernelGGL(k_lm_score<0>, grid, dim3(kThreads), 0, st, static_cast<const uint16_t*>(resid),
                       static_cast<const uint8_t*>(w), static_cast<const float*>(nullptr), target, part, part_id, rows,
                       V, dim, eps);
  const int rc = int(hipGetLastError());
  if (rc != 0) return rc;
  hipLaunchKernelGGL(k_lm_score_merge, dim3(rows), dim3(kWave), 0, st, part, part_id, target, p.slabs, lse, z_target,
                     z_top, id_top);
  return int(hipGetLastError());
}

}  // extern "C"
