// Fused Llama decode step for gfx950 (CDNA4 / MI355X).
//
// The unfused step (kernels.hip + hipBLASLt) is ~50 kernels per token for a
// 4-layer model; at decode batch sizes every one of them is a few-µs latency
// chain (dispatch, one HBM round trip, write back) and the step is bound by
// kernel count, not bytes. This file rebuilds the step as 5 kernels per layer
// plus 3, the GEMMs weight-streaming MFMA kernels with their neighbours fused in:
//
//   k_embed              token gather -> residual stream, per-row sum of squares
//   per layer:
//     k_skinny<ROPE>     RMSNorm (attn_norm) -> QKV GEMM -> RoPE on q/k,
//                        q to the attention buffer, k/v appended to the cache
//     (QKV-bias models:  k_skinny<ROPE_BIAS>, the same with a bias on q, k and v)
//     (scaled RoPE:      k_skinny<ROPE_TAB> / <ROPE_BIAS_TAB>, the same with the frequencies
//                        read from an fp32 table [D/2] instead of computed inline)
//     (QK-norm models:   k_skinny<STORE> writes the raw projection instead, and
//      k_qknorm_rope     norms every q and k head, rotates and appends: a sixth kernel)
//     (FP8 KV cache:     the _KV8 counterpart of whichever kernel appends writes e4m3 bytes,
//                        and k_attn<D, G, true> reads them: the same kernel count)
//     k_attn            GQA flash-decoding split-K; the last split to finish
//                        for a (sequence, KV head) merges the partials in-kernel
//     (sliding window:   a layer with a window runs k_attn<D, G, KV8, true> over its last W positions)
//     (FP8 weights:      every k_skinny is its W8 instantiation: e4m3 weight bytes, 8-byte loads, and the
//                        column's fp32 scale on the accumulator ahead of 1/rms: the same kernel count)
//     (MXFP4 weights:    a layer's four k_skinny are their W8 = 2 instantiations: OCP Microscaling FP4, 32-element
//                        blocks of e2m1 nibbles with one e8m0 scale byte, 4-byte loads and a 1-byte scale load per
//                        k-step, decoded exactly by v_cvt_scalef32_pk_bf16_fp4 ahead of the MFMA; no scale in the
//                        epilogue. The LM head stays FP8. The same kernel count: docs/WEIGHT_MXFP4.md)
//     k_skinny<RESID>    O projection -> residual add -> per-row sum-of-squares
//                        partials for the next norm
//     k_skinny<SILU>     RMSNorm (ffn_norm) -> gate/up GEMM -> SwiGLU
//     k_skinny<RESID>    down projection -> residual add -> sum-of-squares
//   k_skinny<ARGMAX>     RMSNorm (final norm) -> LM head -> logits and
//                        per-block greedy winners
//   k_argmax_merge       one block per row merges the winners
//
// k_skinny<NW, TN, EPI, UM, W8>, k_attn<D, G, KV8, WIN> and k_qknorm_rope<D, TAB, KV8> are templates; which instantiations
// exist is stated once, as lists of parameter values and one predicate, in decode_fused.hip, and a plan that names
// any other is refused there. The RoPE epilogue of a model is rope_epi(bias, table, kv8) below.
//
// Skinny GEMM (M <= 64 tokens): Y[M,N] = A[M,K] * W[N,K]^T on
// v_mfma_f32_16x16x32_bf16. A workgroup owns 16*TN output columns of one
// 16-row tile (blockIdx.y; prefill-heavy steps carry up to 4) and splits K
// over its NW waves; each lane streams its weight rows with 16-byte loads
// straight into MFMA B fragments (no LDS staging: every weight byte is used
// exactly once, by exactly one lane), the K-split partials are summed through
// LDS and wave 0 runs the epilogue. RMSNorm is folded away: its weight g is
// multiplied into the columns of the following projection once at load time
// (W'[n][k] = W[n][k] g[k]), and the per-row 1/rms factors out of the dot
// product, so the GEMM streams the raw residual and the epilogue scales the
// accumulator. 1/rms comes from per-block partial sums of squares written by
// the residual producer (deterministic: fixed order, no float atomics).
// The attention splits merge in-kernel through write-through stores and an
// arrival ticket, never an L2 write-back fence. QKV and gate/up weights have
// their rows interleaved in pairs (RoPE partners; gate_j/up_j) so that one
// 16-column tile holds both members of every pair (lanes c, c^1).
//
// Numerics: GEMM outputs, the residual and the attention output are rounded
// to bf16 where the unfused path rounds them; the normed activation is not
// materialised (rounding differs at the bf16-ulp level); fp32 accumulation.
//
// This header is the device side: kernel arguments, the kernels, the attention
// grid rules and the record of what was measured and rejected. decode_fused.hip
// includes it and holds the host side (planning, workspace, the instantiation set, launches).
#pragma once
#include "bf16_common.h"

#include <algorithm>
#include <type_traits>

namespace {

using namespace p2pt_gpu;

constexpr int kMaxM = 64;  // token rows per step: up to 4 MFMA row tiles (blockIdx.y)

typedef short frag8 __attribute__((ext_vector_type(8)));
typedef float frag4 __attribute__((ext_vector_type(4)));

// EPI_ROPE_BIAS: EPI_ROPE with a per-column bias on q, k and v (Qwen2). A variant of its own, so that
// models without a bias keep the EPI_ROPE kernels as they are, with no run-time test of a pointer.
// EPI_ROPE_TAB, EPI_ROPE_BIAS_TAB: EPI_ROPE and EPI_ROPE_BIAS with inv_freq[i] read from a table in device
// memory (llama3 / linear RoPE scaling: the host computes the table once per model). Variants of their own for
// the same reason: models with default RoPE keep the inline exp2f and launch exactly what they did.
// EPI_ROPE_KV8, EPI_ROPE_BIAS_KV8, EPI_ROPE_TAB_KV8, EPI_ROPE_BIAS_TAB_KV8: the four RoPE epilogues for an FP8
// (OCP e4m3fn; scale 1, or per-head scales: GemmArgs::k_rscale) KV cache: q is written as before, the K and V rows as one byte per element, rounded once
// from the epilogue's fp32 value (f32_to_e4m3x2). Variants of their own, kEpiKv8 above their bf16 counterparts, so
// that a bf16 cache launches exactly the kernels it did.
constexpr int kEpiKv8 = 8;
enum Epi : int {
  EPI_STORE = 0, EPI_ROPE = 1, EPI_SILU = 2, EPI_RESID = 3, EPI_ARGMAX = 4, EPI_ROPE_BIAS = 5, EPI_ROPE_TAB = 6,
  EPI_ROPE_BIAS_TAB = 7,
  EPI_ROPE_KV8 = kEpiKv8 + EPI_ROPE, EPI_ROPE_BIAS_KV8 = kEpiKv8 + EPI_ROPE_BIAS,
  EPI_ROPE_TAB_KV8 = kEpiKv8 + EPI_ROPE_TAB, EPI_ROPE_BIAS_TAB_KV8 = kEpiKv8 + EPI_ROPE_BIAS_TAB
};
constexpr bool epi_kv8(int epi) {
  return epi == EPI_ROPE_KV8 || epi == EPI_ROPE_BIAS_KV8 || epi == EPI_ROPE_TAB_KV8 || epi == EPI_ROPE_BIAS_TAB_KV8;
}
constexpr int epi_base(int epi) { return epi_kv8(epi) ? epi - kEpiKv8 : epi; }  // the bf16-cache counterpart
constexpr bool epi_is_rope(int epi) {
  return epi_base(epi) == EPI_ROPE || epi_base(epi) == EPI_ROPE_BIAS || epi_base(epi) == EPI_ROPE_TAB ||
         epi_base(epi) == EPI_ROPE_BIAS_TAB;
}
constexpr bool epi_has_bias(int epi) { return epi_base(epi) == EPI_ROPE_BIAS || epi_base(epi) == EPI_ROPE_BIAS_TAB; }
constexpr bool epi_has_table(int epi) { return epi_base(epi) == EPI_ROPE_TAB || epi_base(epi) == EPI_ROPE_BIAS_TAB; }
// The RoPE epilogue with these traits (host: plan_step), and the proof that the traits above are its inverse.
constexpr int rope_epi(bool bias, bool table, bool kv8) {
  return (table ? (bias ? EPI_ROPE_BIAS_TAB : EPI_ROPE_TAB) : (bias ? EPI_ROPE_BIAS : EPI_ROPE)) + (kv8 ? kEpiKv8 : 0);
}
constexpr bool rope_epi_inverts(bool bias, bool table, bool kv8) {
  const int e = rope_epi(bias, table, kv8);
  return epi_is_rope(e) && epi_has_bias(e) == bias && epi_has_table(e) == table && epi_kv8(e) == kv8;
}
static_assert(rope_epi_inverts(0, 0, 0) && rope_epi_inverts(1, 0, 0) && rope_epi_inverts(0, 1, 0) &&
              rope_epi_inverts(1, 1, 0) && rope_epi_inverts(0, 0, 1) && rope_epi_inverts(1, 0, 1) &&
              rope_epi_inverts(0, 1, 1) && rope_epi_inverts(1, 1, 1));

struct GemmArgs {
  const uint16_t* x;  // A [M][K]
  const uint16_t* w;  // W [N][K]; for a normed input, W[n][k] * g[k] folded in
  int M, N, K;
  // RMSNorm of A's rows (ss_part == nullptr: A used as is). The norm weight g
  // is folded into W offline, so only the per-row 1/rms remains, and that
  // factors out of the dot product: it scales the accumulator in the epilogue.
  const float* ss_part;  // [ss_parts][16] partial row sums of squares
  int ss_parts;
  float eps;
  // epilogue
  uint16_t* out;   // STORE/ARGMAX: [M][N] logits; SILU: [M][N/2]; RESID: residual [M][N], in place
  float* ss_out;   // RESID: [gridDim.x][16]
  const int* pos;   // ROPE: cache position of each row
  const int* slot;  // ROPE: cache slot of each row (nullptr: row m -> slot m)
  int nslots;
  uint16_t* q_out;
  uint16_t* kc;  // the _KV8 epilogues: e4m3 bytes, the same [slot][pos][Hkv][D] order
  uint16_t* vc;
  const uint16_t* bias;  // ROPE_BIAS(_TAB): [N], in the row order of W (interleaved like its rows)
  const float* inv_freq;  // ROPE_TAB, ROPE_BIAS_TAB: [D / 2] RoPE frequencies (the others compute them from log2_theta)
  int H, Hkv, D, Smax;
  float log2_theta;
  float* am_val;  // ARGMAX: [gridDim.x][16]
  int* am_idx;
  // K parts (kpl = log2 P, 0: off; TN = 1, M * P <= 16). A subtile then holds
  // 16 / P output columns instead of 16, so a small-N projection lands on P
  // times the workgroups and its weight stream spreads over every CU (one CU
  // streams ~10 B/cycle; a 2048-wide projection in 16-column tiles reaches
  // only 128 of the 256 CUs). Lanes past the tile width take the other K
  // parts of the same columns, and MFMA rows m * P + p carry activation row
  // m's K part p, so every lane streams unique weight bytes. The diagonal
  // blocks of the 16 x 16 accumulator are summed in the epilogue. It needs
  // spare MFMA rows: a decode step of <= 16 / P tokens.
  int kpl;
  // FP8 weights (k_skinny<.., W8 = 1>): w holds N * K e4m3 bytes and wscale the fp32 scale of each output row,
  // [N] in the row order of w (interleaved like its rows). Not read by the bf16 kernels.
  const float* wscale;
  // FP8 cache with scales (the _KV8 epilogues): fp32 [Hkv] each, the reciprocals 1 / k_scale and 1 / v_scale of this
  // layer's KV heads, which multiply the value ahead of its one rounding. Both nullptr: scale 1. Not read otherwise.
  const float* k_rscale;
  const float* v_rscale;
  // MXFP4 weights (k_skinny<.., W8 = 2>): w holds N * K / 2 bytes, two e2m1 nibbles each (the lower k in the low
  // nibble), and wexp the e8m0 scale byte of every 32-element block, [N][K / 32] in the row order of w. Not read by
  // the other kernels.
  const uint8_t* wexp;
};

// log2 of the output columns per 16-lane subtile: 16, 8 or 4 for 1, 2 or 4 K parts.
__host__ __device__ __forceinline__ int tile_cwl(int kpl) { return 4 - kpl; }

__device__ __forceinline__ frag8 as_frag(const uint4& v) { return __builtin_bit_cast(frag8, v); }

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
// v_dot2_f32_bf16: c + a.lo * b.lo + a.hi * b.hi, products and sum in fp32.
__device__ __forceinline__ float dot2_bf16(uint32_t a, uint32_t b, float c) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a), __builtin_bit_cast(bf16x2_t, b), c, false);
}

// FP8 KV cache: OCP e4m3fn (4 exponent bits, bias 7, 3 mantissa bits, no infinities, 0x7f / 0xff NaN, largest
// finite value 448), scale 1. Two fp32 values to two bytes (a in bits 0..7, b in 8..15), each rounded once to
// nearest-even by v_cvt_pk_fp8_f32, subnormals (multiples of 2^-9) included. Finite values are clamped to +-448
// first (v_med3_f32): what the conversion alone does above 448 (saturate, or NaN) depends on the wave's FP16_OVFL
// mode bit, and the stored byte must not. NaN stays NaN: v_med3 would turn it into a bound, so it is passed by.
__device__ __forceinline__ float e4m3_clamp(float x) {
  const float c = __builtin_amdgcn_fmed3f(x, -448.f, 448.f);
  return x != x ? x : c;
}
__device__ __forceinline__ uint16_t f32_to_e4m3x2(float a, float b) {
  return uint16_t(__builtin_amdgcn_cvt_pk_fp8_f32(e4m3_clamp(a), e4m3_clamp(b), 0, false));
}
typedef float float2v __attribute__((ext_vector_type(2)));
// Eight e4m3 bytes to fp32 (v_cvt_pk_f32_fp8: exact, every e4m3 value is an fp32 value).
__device__ __forceinline__ void unpack8_e4m3(const uint2& v, float* f) {
  const float2v a = __builtin_amdgcn_cvt_pk_f32_fp8(int(v.x), false), b = __builtin_amdgcn_cvt_pk_f32_fp8(int(v.x), true);
  const float2v c = __builtin_amdgcn_cvt_pk_f32_fp8(int(v.y), false), d = __builtin_amdgcn_cvt_pk_f32_fp8(int(v.y), true);
  f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1];
  f[4] = c[0]; f[5] = c[1]; f[6] = d[0]; f[7] = d[1];
}
// Eight e4m3 bytes as eight bf16 (exact: the low 16 bits of every decoded fp32 are zero).
__device__ __forceinline__ uint4 e4m3x8_to_bf16x8(const uint2& v) {
  float f[8];
  unpack8_e4m3(v, f);
  auto pk = [](float lo, float hi) { return (__float_as_uint(hi) & 0xffff0000u) | (__float_as_uint(lo) >> 16); };
  return make_uint4(pk(f[0], f[1]), pk(f[2], f[3]), pk(f[4], f[5]), pk(f[6], f[7]));
}

// Cross-workgroup hand-off without L2 write-back/invalidate fences: payload
// stores are agent-scope relaxed atomics (write-through, `sc1`), drained with
// s_waitcnt before the arrival ticket; the last arriver reads them back with
// agent-scope loads that bypass stale cache lines (MI355X_MICROARCH handoff-flag).
template <typename T>
__device__ __forceinline__ void st_wt(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ T ld_wt(const T* p) {
  return __hip_atomic_load(const_cast<T*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void drain_stores() {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  __builtin_amdgcn_s_waitcnt(0);
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}
__device__ __forceinline__ unsigned arrive(unsigned* ctr) {
  return __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Output column of lane column c (0..15) in subtile t of block bx, for
// subtiles of 2^cwl columns (lanes past 2^cwl: the same columns' other K parts).
template <int TN>
__device__ __forceinline__ int tile_col(int bx, int t, int c, int cwl) {
  return ((bx * TN + t) << cwl) + (c & ((1 << cwl) - 1));
}

// Operand loads go through buffer descriptors (wave-uniform base and size
// from the kernel arguments): a lane whose byte offset lies past the buffer
// gets zeros from the range check without a memory access. Rows past M and
// k-steps past a wave's share use that (kOob), so a batch is branch-free and a
// decode step at batch 1 fetches its one activation row once per k-step
// instead of for all 16 MFMA rows.
constexpr uint32_t kOob = 0x80000000u;  // host keeps every operand below 2 GiB

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint4 buf_ld16(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}
__device__ __forceinline__ uint2 buf_ld8(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
}
__device__ __forceinline__ uint32_t buf_ld4(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0);
}
__device__ __forceinline__ uint32_t buf_ld1(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_amdgcn_raw_buffer_load_b8(r, off, 0, 0);
}

// MXFP4: four bytes (eight e2m1 nibbles, the lower k in the low nibble of its byte) and the block's e8m0 scale byte E
// as eight bf16, by v_cvt_scalef32_pk_bf16_fp4 with the scale 2^(E - 127) passed as the fp32 of bits E << 23. Exact:
// every e2m1 value has at most one mantissa bit, and the quantiser keeps E where 0.5 * 2^(E - 127) and 6 * 2^(E - 127)
// are normal bf16 numbers. E = 0 with zero nibbles (what a load past the buffer returns) decodes to zeros.
__device__ __forceinline__ uint4 fp4x8_to_bf16x8(uint32_t v, uint32_t e) {
  const float sc = __uint_as_float(e << 23);
  auto cv = [&](auto sel) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, decltype(sel)::value));
  };
  return make_uint4(cv(std::integral_constant<int, 0>{}), cv(std::integral_constant<int, 1>{}),
                    cv(std::integral_constant<int, 2>{}), cv(std::integral_constant<int, 3>{}));
}

// One batch of up to UM consecutive 32-wide k-steps [s, min(s + UM, s1)):
// every load of the batch is issued before any of it is used.
// W8 (FP8 weights): the lane's B fragment of a k-step is its 8 k-values as 8 e4m3 bytes, one 8-byte load at a
// k-step stride of 32 bytes, decoded to the bf16 fragment (e4m3x8_to_bf16x8: exact) just ahead of its MFMA. The A
// operand, the order of the k-steps and the MFMA are the bf16 kernel's, so on the decoded weights the accumulator
// is the bf16 kernel's bit for bit.
// W8 = 2 (MXFP4 weights): the 8 k-values are 4 bytes, one 4-byte load at a k-step stride of 16 bytes, and the k-step
// is one 32-element block, so its scale is one byte at a stride of 1 (soff, through the descriptor rs; the four
// k-groups of a column read the same byte). Both are decoded together just ahead of the MFMA (fp4x8_to_bf16x8: exact
// for every scale), and nothing after the MFMA knows the format: on the dequantised weights the whole kernel is the
// bf16 kernel's bit for bit. soff and rs are not read otherwise.
template <int UM, int TN, int W8>
struct Batch {
  std::conditional_t<W8 == 2, uint32_t, std::conditional_t<W8 == 1, uint2, uint4>> b[UM][TN];
  uint32_t e[W8 == 2 ? UM : 1][TN];  // W8 = 2: the block's e8m0 scale byte
  uint4 a[UM];
};

template <int UM, int TN, int W8>
__device__ __forceinline__ void load_batch(Batch<UM, TN, W8>& bt, __amdgpu_buffer_rsrc_t ra, uint32_t xoff,
                                           __amdgpu_buffer_rsrc_t rw, const uint32_t (&woff)[TN],
                                           __amdgpu_buffer_rsrc_t rs, const uint32_t (&soff)[TN], int s, int s1) {
#pragma unroll
  for (int u = 0; u < UM; u++) {
    const bool in = s + u < s1;
    const uint32_t su = uint32_t(s + u) * 64u;  // bytes per 32-wide k-step (bf16; half for e4m3, a quarter for MXFP4)
#pragma unroll
    for (int t = 0; t < TN; t++) {
      if constexpr (W8 == 2) {
        bt.b[u][t] = buf_ld4(rw, in ? woff[t] + (su >> 2) : kOob);
        bt.e[u][t] = buf_ld1(rs, in ? soff[t] + uint32_t(s + u) : kOob);
      } else if constexpr (W8 == 1) bt.b[u][t] = buf_ld8(rw, in ? woff[t] + (su >> 1) : kOob);
      else bt.b[u][t] = buf_ld16(rw, in ? woff[t] + su : kOob);
    }
    bt.a[u] = buf_ld16(ra, in ? xoff + su : kOob);
  }
}

template <int UM, int TN, int W8>
__device__ __forceinline__ void mma_apply(frag4 (&acc)[TN], const Batch<UM, TN, W8>& bt) {
#pragma unroll
  for (int u = 0; u < UM; u++)
#pragma unroll
    for (int t = 0; t < TN; t++) {
      uint4 b;
      if constexpr (W8 == 2) b = fp4x8_to_bf16x8(bt.b[u][t], bt.e[u][t]);
      else if constexpr (W8 == 1) b = e4m3x8_to_bf16x8(bt.b[u][t]);
      else b = bt.b[u][t];
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(bt.a[u]), as_frag(b), acc[t], 0, 0, 0);
    }
}

// The wave's k-steps [s0, s1), one batch at a time.
template <int UM, int TN, int W8>
__device__ __forceinline__ void mma_stream(frag4 (&acc)[TN], __amdgpu_buffer_rsrc_t ra, uint32_t xoff,
                                           __amdgpu_buffer_rsrc_t rw, const uint32_t (&woff)[TN],
                                           __amdgpu_buffer_rsrc_t rs, const uint32_t (&soff)[TN], int s0, int s1) {
  for (int s = s0; s < s1; s += UM) {
    Batch<UM, TN, W8> p;
    load_batch<UM, TN, W8>(p, ra, xoff, rw, woff, rs, soff, s, s1);
    // Keep every load of the batch ahead of the first MFMA: left alone, the
    // scheduler interleaves them and the batch pays several memory latencies.
    __builtin_amdgcn_sched_barrier(0);
    mma_apply<UM, TN, W8>(acc, p);
  }
}

// Skinny GEMM + fused epilogue. NW waves split K; TN subtiles of 2^cwl
// columns per block; UM k-steps per load batch (host: >= each wave's share
// when possible). Steps of more than 16 rows put each 16-row tile on its own
// workgroup (blockIdx.y). ROPE and SILU take weights whose rows are
// interleaved in pairs (RoPE partners d, d + D/2 of a head; gate_j, up_j), so
// a pair sits in lanes c, c^1.
// W8: the weight is N * K e4m3 bytes with one fp32 scale per output row (GemmArgs::wscale). The stream is as above
// with 8-byte B loads (Batch); the scale of the lane's column multiplies the accumulator once, in fp32, after the
// K-split reduction and the K-parts diagonal sum and ahead of 1/rms: v = (v * s[col]) * rs. Everything after that
// is the bf16 kernel's epilogue. With power-of-two scales the product is exact, so the kernel matches the bf16
// kernel on the weights decode(q) * s bit for bit.
// W8 = 2: the weight is N * K / 2 bytes of e2m1 nibbles with one e8m0 byte per 32-element block (GemmArgs::wexp,
// N * K / 32 bytes). The stream is as above with 4-byte B loads and a 1-byte scale load per k-step (Batch); under K
// parts both offsets carry the part. There is no scale in the epilogue: the decoded fragment is the dequantised
// weight itself, so the kernel matches the bf16 kernel on those weights bit for bit, for every scale.
template <int NW, int TN, int EPI, int UM, int W8 = 0>
__global__ __launch_bounds__(NW * 64) void k_skinny(GemmArgs a) {
  __shared__ float red[NW][TN][4][kWave];
  __shared__ float red_ss[NW][kWave];
  // The wave index is uniform: held in an SGPR, the k-step bounds and loop
  // counter derived from it stay out of the VGPR budget.
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = blockIdx.y << 4;  // first row of this workgroup's 16-row tile
  const int bx = blockIdx.x;       // column tile
  const int cwl = tile_cwl(a.kpl);
  const bool norm = a.ss_part != nullptr;

  // Row sums of squares for the folded RMSNorm, spread over every wave (lane:
  // row lane & 15, partials (lane >> 4) + 4 * wave + 4 * NW * i): up to 8
  // loads per lane issued ahead of the weight stream and summed only after
  // it, so they never stall it; combined through LDS before the epilogue.
  constexpr int kSsRegs = 8;
  float ssv[kSsRegs];
  const int ss_p0 = (lane >> 4) + 4 * wv;
  if (norm) {
#pragma unroll
    for (int i = 0; i < kSsRegs; i++) {
      const int p = ss_p0 + 4 * NW * i;
      ssv[i] = p < a.ss_parts ? a.ss_part[p * kMaxM + m0 + (lane & 15)] : 0.f;
    }
  }

  // A fragment: row lane & 15, k = 32*s + 8*(lane>>4) + j; B fragment: W row n, same k.
  // The K steps are split evenly over the NW waves.
  const int kparts = 1 << a.kpl, Kp = a.K >> a.kpl;  // Kp: K elements per part
  const int m_a = (lane & 15) >> a.kpl;              // activation row of this lane's MFMA row
  const int p_a = (lane & 15) & (kparts - 1);        // ... and the K part it carries
  const bool a_ok = m0 + m_a < a.M;
  const int kq = (lane >> 4) << 3;
  const int S = Kp >> 5;
  const int s0 = wv * S / NW, s1 = (wv + 1) * S / NW;
  // Byte offsets of this lane's A row and weight rows at k-step 0; rows past
  // M read as zeros (kOob).
  const __amdgpu_buffer_rsrc_t ra = rsrc(a.x, uint32_t(a.M) * uint32_t(a.K) * 2u);
  constexpr uint32_t kWb = W8 ? 1u : 2u;   // bytes per weight element ...
  constexpr uint32_t kWs = W8 == 2 ? 1u : 0u;  // ... halved once more for MXFP4's nibbles
  const __amdgpu_buffer_rsrc_t rw = rsrc(a.w, (uint32_t(a.N) * uint32_t(a.K) * kWb) >> kWs);
  // MXFP4: the scale bytes, [N][K / 32]; the other formats never load through it.
  const __amdgpu_buffer_rsrc_t rs = W8 == 2 ? rsrc(a.wexp, uint32_t(a.N) * uint32_t(a.K >> 5)) : rw;
  const uint32_t xoff = a_ok ? (uint32_t(m0 + m_a) * uint32_t(a.K) + uint32_t(p_a * Kp + kq)) * 2u : kOob;
  const int p_b = (lane & 15) >> cwl;  // K part of this lane's weight column
  uint32_t woff[TN], soff[TN];
#pragma unroll
  for (int t = 0; t < TN; t++) {
    const uint32_t col = uint32_t(tile_col<TN>(bx, t, lane & 15, cwl));
    woff[t] = ((col * uint32_t(a.K) + uint32_t(p_b * Kp + kq)) * kWb) >> kWs;
    soff[t] = col * uint32_t(a.K >> 5) + uint32_t(p_b * (Kp >> 5));  // the block of k-step 0 of this lane's K part
  }

  // C layout: row m = m0 + 4*(lane>>4) + r, column = tile_col(.., lane & 15).
  const int lrow0 = (lane >> 4) << 2, mrow0 = m0 + lrow0;
  const int c = lane & 15;
  const bool col_ok = c < (1 << cwl);  // lanes past the tile width carry the other K parts

  // RESID: the residual values this lane's epilogue updates, loaded by wave 0
  // ahead of the weight stream (they do not depend on it) instead of after
  // the reduction, which would add a dependent memory round trip.
  float rprev[EPI == EPI_RESID ? TN : 1][4];
  if constexpr (EPI == EPI_RESID) {
    if (wv == 0) {
#pragma unroll
      for (int t = 0; t < TN; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int m = min(mrow0 + r, a.M - 1);
          rprev[t][r] = bf2f(a.out[size_t(m) * a.N + tile_col<TN>(bx, t, c, cwl)]);
        }
    }
  }

  // ROPE_BIAS: this lane's column bias, loaded by wave 0 ahead of the weight
  // stream like rprev. The host keeps kpl == 0 here, so the column is < N.
  float bias = 0.f;
  if constexpr (epi_has_bias(EPI)) {
    if (wv == 0) bias = bf2f(a.bias[tile_col<TN>(bx, 0, c, cwl)]);
  }

  // ROPE_TAB: this lane's RoPE frequency, inv_freq[i] of its column's pair i = (col % D) / 2, loaded ahead of
  // the weight stream for the same reason: after it, a 4-byte load, cache hit or not, would sit between the
  // last MFMA and the sincosf. The index is < D / 2, the table's length, for any column whatever. plan_step
  // gives QKV no K parts (k_parts = false), so these epilogues are planned and tested at kpl == 0 only.
  // Measured on MI355X and rejected: col & (D - 1) for col % D (D is 64 or 128). Without the integer division
  // the QKV kernel was slower, not faster: 6.32 us per launch against 6.22 with the division and 6.10 for
  // EPI_ROPE (Llama-3.2-1B's shape, batch 1, kernel trace); the step +4.1 us against +1.4 us.
  float tab_freq = 0.f;
  if constexpr (epi_has_table(EPI)) {
    if (wv == 0) tab_freq = a.inv_freq[(tile_col<TN>(bx, 0, c, cwl) % a.D) >> 1];
  }

  // W8: this lane's column scales, loaded by wave 0 ahead of the weight stream like bias and tab_freq. tile_col
  // masks the lane column to the tile width, so under K parts the lanes past it index their own column's scale,
  // below N like every column of the grid (grid_x * TN * 2^cwl == N).
  float wsc[W8 == 1 ? TN : 1];
  if constexpr (W8 == 1) {
    if (wv == 0) {
#pragma unroll
      for (int t = 0; t < TN; t++) wsc[t] = a.wscale[tile_col<TN>(bx, t, c, cwl)];
    }
  }

  // _KV8 with scales: the reciprocal scale of this workgroup's head, loaded ahead of the weight stream like bias
  // and tab_freq. A tile's 16 columns lie in one head (D is a multiple of 16 and QKV has no K parts), so the head
  // and the load are uniform: one scalar load per workgroup. q heads, and a model without scales, keep 1.
  float kv_rs = 1.f;
  if constexpr (epi_kv8(EPI)) {
    const int kvh = tile_col<TN>(bx, 0, 0, cwl) / a.D - a.H;  // < 2 Hkv: every column of the grid is below N
    if (wv == 0 && kvh >= 0 && a.k_rscale != nullptr) kv_rs = kvh < a.Hkv ? a.k_rscale[kvh] : a.v_rscale[kvh - a.Hkv];
  }

  frag4 acc[TN];
#pragma unroll
  for (int t = 0; t < TN; t++) acc[t] = frag4{0.f, 0.f, 0.f, 0.f};
  mma_stream<UM, TN, W8>(acc, ra, xoff, rw, woff, rs, soff, s0, s1);

  if (norm) {
    float ssum = 0.f;
#pragma unroll
    for (int i = 0; i < kSsRegs; i++) ssum += ssv[i];
    for (int p = ss_p0 + 4 * NW * kSsRegs; p < a.ss_parts; p += 4 * NW) ssum += a.ss_part[p * kMaxM + m0 + (lane & 15)];
    red_ss[wv][lane] = ssum;
  }
  // K-split reduction through LDS (lane-contiguous: conflict-free).
#pragma unroll
  for (int t = 0; t < TN; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) red[wv][t][r][lane] = acc[t][r];
  __syncthreads();
  if (wv != 0) return;
  float v[TN][4];
#pragma unroll
  for (int t = 0; t < TN; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      float sum = 0.f;
#pragma unroll
      for (int w = 0; w < NW; w++) sum += red[w][t][r][lane];
      v[t][r] = sum;
    }

  if (a.kpl) {
    // Sum the diagonal blocks: output (row m, column c < 2^cwl) is
    // sum_p C[m * P + p][c + p * 2^cwl]. Wave 0 alone from here on: the
    // reduction buffer (its own reads are done) holds C [16][17].
    float* cbuf = &red[0][0][0][0];
#pragma unroll
    for (int r = 0; r < 4; r++) cbuf[(lrow0 + r) * 17 + c] = v[0][r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = lrow0 + r;
      float sum = 0.f;
      if (row < (16 >> a.kpl) && col_ok)
        for (int p = 0; p < kparts; p++) sum += cbuf[(row * kparts + p) * 17 + c + (p << cwl)];
      v[0][r] = sum;
    }
  }

  if constexpr (W8 == 1) {
#pragma unroll
    for (int t = 0; t < TN; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) v[t][r] *= wsc[t];
  }

  if (norm) {
    float ssum = 0.f;
#pragma unroll
    for (int w = 0; w < NW; w++) ssum += red_ss[w][lane];
    ssum = xor32_sum(xor16_sum(ssum));
    const float rs_row = rsqrtf(ssum * (1.f / float(a.K)) + a.eps);  // for row m0 + (lane & 15)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const float rs = __shfl(rs_row, lrow0 + r, kWave);
#pragma unroll
      for (int t = 0; t < TN; t++) v[t][r] *= rs;
    }
  }

  if constexpr (EPI == EPI_STORE || EPI == EPI_ARGMAX) {
    // Logits (bf16) and, for ARGMAX, this block's per-row winner (first index on ties).
    float best[4];
    int bi[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      best[r] = -INFINITY;
      bi[r] = 0x7fffffff;
    }
#pragma unroll
    for (int t = 0; t < TN; t++) {
      const int n = tile_col<TN>(bx, t, c, cwl);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int m = mrow0 + r;
        const float lv = bf_round(v[t][r]);
        if (m < a.M && col_ok) a.out[size_t(m) * a.N + n] = uint16_t(f2bf_bits(lv));
        if (lv > best[r] || (lv == best[r] && n < bi[r])) {
          best[r] = lv;
          bi[r] = n;
        }
      }
    }
    if constexpr (EPI == EPI_ARGMAX) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        row16_argmax(best[r], bi[r]);
        if (c == 0) {
          a.am_val[bx * kMaxM + mrow0 + r] = best[r];
          a.am_idx[bx * kMaxM + mrow0 + r] = bi[r];
        }
      }
    }
  } else if constexpr (EPI == EPI_SILU) {
    // Interleaved rows: even lane = gate_j, odd lane = up_j, j = column / 2.
    const int n = tile_col<TN>(bx, 0, c, cwl);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const float mine = bf_round(v[0][r]);
      const float other = dpp<kDppXor1>(mine);
      if ((c & 1) || !col_ok || mrow0 + r >= a.M) continue;
      a.out[size_t(mrow0 + r) * (a.N >> 1) + (n >> 1)] = uint16_t(f2bf_bits(mine / (1.f + __expf(-mine)) * other));
    }
  } else if constexpr (epi_is_rope(EPI)) {
    // Interleaved rows within each head: column 2i = dim i, 2i+1 = dim i + D/2.
    // ROPE_BIAS adds the column's bias in fp32 after the 1/rms scale and before
    // the one rounding ahead of the rotation: q, k and v alike. The _TAB variants take the frequency from the
    // table (loaded above) and are otherwise this code.
    const int half = a.D >> 1;
    const int col = tile_col<TN>(bx, 0, c, cwl);
    const int head = col / a.D, i = (col % a.D) >> 1;
    const bool second = c & 1;
    float inv_freq;
    if constexpr (epi_has_table(EPI)) inv_freq = tab_freq;
    else inv_freq = exp2f(-a.log2_theta * (2.f * i) / a.D);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int m = mrow0 + r;
      const float mine = bf_round(epi_has_bias(EPI) ? v[0][r] + bias : v[0][r]);
      const float other = dpp<kDppXor1>(mine);
      if (m >= a.M || !col_ok) continue;
      // Host validates; clamped anyway so a bad index can never write outside the cache.
      const int p = min(max(a.pos[m], 0), a.Smax - 1);
      const int sl = a.slot ? min(max(a.slot[m], 0), a.nslots - 1) : m;
      const int d = i + (second ? half : 0);
      if constexpr (epi_kv8(EPI)) {
        // The head is the same for the whole workgroup (16 columns of one head) and m for the 16 lanes of a row,
        // so the four lanes of a quad are always here together: lane c + 2 holds dim d + 1, and lanes with
        // (c & 2) == 0 store dims d, d + 1 as one 2-byte word (d is even there). K: the rotated fp32 value; V: the
        // fp32 projection (+ bias) itself, not its bf16 rounding.
        float val = epi_has_bias(EPI) ? v[0][r] + bias : v[0][r];
        if (head < a.H + a.Hkv) {
          float sn, cs;
          sincosf(float(p) * inv_freq, &sn, &cs);
          const float x1 = second ? other : mine, x2 = second ? mine : other;
          val = second ? x2 * cs + x1 * sn : x1 * cs - x2 * sn;
        }
        // K and V: times the head's reciprocal scale (exactly val at scale 1), still ahead of the one rounding.
        const float sval = val * kv_rs;
        const float next = dpp<kDppXor2>(sval);
        if (head < a.H) {
          a.q_out[(size_t(m) * a.H + head) * a.D + d] = uint16_t(f2bf_bits(val));
        } else if (!(c & 2)) {
          const bool is_k = head < a.H + a.Hkv;
          uint8_t* row = reinterpret_cast<uint8_t*>(is_k ? a.kc : a.vc) +
                         ((size_t(sl) * a.Smax + p) * a.Hkv + (head - a.H - (is_k ? 0 : a.Hkv))) * a.D;
          *reinterpret_cast<uint16_t*>(row + d) = f32_to_e4m3x2(sval, next);
        }
      } else if (head < a.H + a.Hkv) {
        float sn, cs;
        sincosf(float(p) * inv_freq, &sn, &cs);
        const float x1 = second ? other : mine, x2 = second ? mine : other;
        const float o = second ? x2 * cs + x1 * sn : x1 * cs - x2 * sn;
        uint16_t* dst = head < a.H ? a.q_out + (size_t(m) * a.H + head) * a.D
                                   : a.kc + ((size_t(sl) * a.Smax + p) * a.Hkv + (head - a.H)) * a.D;
        dst[d] = uint16_t(f2bf_bits(o));
      } else {
        a.vc[((size_t(sl) * a.Smax + p) * a.Hkv + (head - a.H - a.Hkv)) * a.D + d] = uint16_t(f2bf_bits(mine));
      }
    }
  } else if constexpr (EPI == EPI_RESID) {
    float sq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TN; t++) {
      const int n = tile_col<TN>(bx, t, c, cwl);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int m = mrow0 + r;
        if (m >= a.M || !col_ok) continue;
        const float nv = bf_round(rprev[t][r] + bf_round(v[t][r]));
        a.out[size_t(m) * a.N + n] = uint16_t(f2bf_bits(nv));
        sq[r] += nv * nv;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      sq[r] = row16_sum(sq[r]);
      if (c == 0) a.ss_out[bx * kMaxM + mrow0 + r] = sq[r];
    }
  }
}

// Greedy sampling, second stage: one block per row merges the LM-head blocks'
// winners (first index on ties).
__global__ __launch_bounds__(256) void k_argmax_merge(const float* __restrict__ am_val, const int* __restrict__ am_idx,
                                                      int parts, int64_t* __restrict__ ids) {
  const int m = blockIdx.x;
  float b = -INFINITY;
  int i = 0x7fffffff;
  for (int p0 = threadIdx.x; p0 < parts; p0 += 8 * 256) {
    float pv[8];
    int pi[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {  // 8 loads in flight per thread
      const int p = p0 + j * 256;
      pv[j] = p < parts ? am_val[p * kMaxM + m] : -INFINITY;
      pi[j] = p < parts ? am_idx[p * kMaxM + m] : 0x7fffffff;
    }
#pragma unroll
    for (int j = 0; j < 8; j++)
      if (pv[j] > b || (pv[j] == b && pi[j] < i)) {
        b = pv[j];
        i = pi[j];
      }
  }
  wave_argmax(b, i);
  __shared__ float sb[4];
  __shared__ int si[4];
  if ((threadIdx.x & 63) == 0) {
    sb[threadIdx.x >> 6] = b;
    si[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++)
      if (sb[w] > b || (sb[w] == b && si[w] < i)) {
        b = sb[w];
        i = si[w];
      }
    ids[m] = i == 0x7fffffff ? 0 : i;  // a row of NaN logits has no winner: id 0, never out of range
  }
}

// ------------------------------------------------------------ embedding gather
// One block per token: residual row = embed[token]; ss_out[0][b] = sum of squares.
__global__ __launch_bounds__(256) void k_embed(const uint16_t* __restrict__ embed, const int64_t* __restrict__ tok,
                                               uint16_t* __restrict__ resid, float* __restrict__ ss_out, int dim,
                                               int vocab) {
  const int b = blockIdx.x;
  int64_t t = tok[b];
  t = t < 0 ? 0 : (t >= vocab ? vocab - 1 : t);
  const uint4* src = reinterpret_cast<const uint4*>(embed + size_t(t) * dim);
  uint4* dst = reinterpret_cast<uint4*>(resid + size_t(b) * dim);
  float ss = 0.f;
  for (int i = threadIdx.x; i < dim / 8; i += 256) {
    const uint4 v = src[i];
    dst[i] = v;
    float f[8];
    unpack8(v, f);
#pragma unroll
    for (int j = 0; j < 8; j++) ss += f[j] * f[j];
  }
  __shared__ float red[4];
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  if (threadIdx.x == 0) ss_out[b] = red[0] + red[1] + red[2] + red[3];
}

// ------------------------------------------------------------ per-head QK RMSNorm + RoPE + cache append
// QK-norm models (Qwen3): an RMSNorm over head_dim with a learned [D] weight on
// every q and k head, after the projection and before RoPE. A head is spread
// over 4 or 8 workgroups of the QKV GEMM, so the norm cannot sit in its
// epilogue; the GEMM stores the raw projection (EPI_STORE, plain row order) and
// this kernel finishes it: norm, rotate-half RoPE, q to the attention buffer,
// k appended to the cache, v copied bit for bit. D / 4 lanes per head (2 or 4
// heads per wave): lane j holds dims 2j, 2j + 1 and their RoPE partners
// 2j + D/2, 2j + 1 + D/2 as two 4-byte loads, so the rotation needs no lane
// exchange and the sum of squares is one DPP row sum (plus one half-swap at
// D = 128). fp32 throughout, rounded to bf16 once. No LDS, no barrier.
struct QkNormArgs {
  const uint16_t* qkv;  // [M][(H + 2 Hkv) * D], plain head order
  const uint16_t* gq;   // [D] q_norm weight
  const uint16_t* gk;   // [D] k_norm weight
  const int* pos;
  const int* slot;  // nullptr: row m -> slot m
  int nslots;
  uint16_t* q_out;  // [M][H][D]
  uint16_t* kc;     // [nslots][Smax][Hkv][D]; k_qknorm_rope<D, TAB, true>: e4m3 bytes
  uint16_t* vc;
  int H, Hkv, Smax;
  float eps, log2_theta;
  const float* inv_freq;  // k_qknorm_rope<D, true>: [D / 2] RoPE frequencies, 8-byte aligned
  // k_qknorm_rope<D, TAB, true> with scales: [Hkv] each, 1 / k_scale and 1 / v_scale (GemmArgs); both nullptr: scale 1.
  const float* k_rscale;
  const float* v_rscale;
};

constexpr int kQkNormWaves = 4;  // waves per workgroup of k_qknorm_rope

// Heads one workgroup of k_qknorm_rope covers.
__host__ __device__ __forceinline__ int qknorm_heads_per_wg(int D) { return kQkNormWaves * kWave / (D / 4); }

// TAB: the frequencies of dims 2j and 2j + 1 come from a.inv_freq as one 8-byte load (scaled RoPE) instead
// of exp2f; 2j + 1 < D / 2 for every lane.
// KV8: an FP8 (e4m3) cache. q is written as bf16 as before; k goes from the rotated fp32 value to e4m3 in one
// rounding, v from the bf16 value read (exactly an fp32 value) likewise: two 2-byte stores per lane instead of two
// 4-byte ones. With scales, k and v are multiplied by their head's reciprocal scale ahead of that rounding (a lane
// group's own head: one 4-byte load per lane, issued with the norm weights).
template <int D, bool TAB = false, bool KV8 = false>
__global__ __launch_bounds__(kQkNormWaves * 64) void k_qknorm_rope(QkNormArgs a) {
  constexpr int LPH = D / 4, half = D / 2;  // lanes per head
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.y;
  const int heads = a.H + 2 * a.Hkv;
  const int head = (blockIdx.x * kQkNormWaves * 64 + threadIdx.x) / LPH;
  // Lane groups past the last head follow it (every lane stays in the
  // cross-lane sums) and store nothing.
  const int hc = min(head, heads - 1);
  const int j = lane % LPH;
  const uint16_t* src = a.qkv + (size_t(m) * heads + hc) * D + 2 * j;
  const uint32_t lo = *reinterpret_cast<const uint32_t*>(src);
  const uint32_t hi = *reinterpret_cast<const uint32_t*>(src + half);
  const bool is_q = hc < a.H, is_v = hc >= a.H + a.Hkv;
  const uint16_t* g = (is_q ? a.gq : a.gk) + 2 * j;
  const uint32_t glo = *reinterpret_cast<const uint32_t*>(g);
  const uint32_t ghi = *reinterpret_cast<const uint32_t*>(g + half);
  float kv_rs = 1.f;
  if constexpr (KV8) {
    if (!is_q && a.k_rscale != nullptr) kv_rs = is_v ? a.v_rscale[hc - a.H - a.Hkv] : a.k_rscale[hc - a.H];
  }
  float2 tab_freq = make_float2(0.f, 0.f);
  if constexpr (TAB) tab_freq = *reinterpret_cast<const float2*>(a.inv_freq + 2 * j);
  // Host validates; clamped anyway so a bad index can never write outside the cache.
  const int p = min(max(a.pos[m], 0), a.Smax - 1);
  const int sl = a.slot ? min(max(a.slot[m], 0), a.nslots - 1) : m;

  const float x1[2] = {bf_lo(lo), bf_hi(lo)}, x2[2] = {bf_lo(hi), bf_hi(hi)};
  float ss = x1[0] * x1[0] + x1[1] * x1[1] + x2[0] * x2[0] + x2[1] * x2[1];
  ss = row16_sum(ss);
  if constexpr (LPH == 32) ss = xor16_sum(ss);
  const float rs = rsqrtf(ss * (1.f / float(D)) + a.eps);
  if (head >= heads) return;

  uint32_t olo = lo, ohi = hi;  // v: copied as is
  float o1[2] = {x1[0], x1[1]}, o2[2] = {x2[0], x2[1]};
  if (!is_v) {
    const float g1[2] = {bf_lo(glo), bf_hi(glo)}, g2[2] = {bf_lo(ghi), bf_hi(ghi)};
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const int i = 2 * j + e;
      float inv_freq;
      if constexpr (TAB) inv_freq = e ? tab_freq.y : tab_freq.x;
      else inv_freq = exp2f(-a.log2_theta * (2.f * i) / D);
      float sn, cs;
      sincosf(float(p) * inv_freq, &sn, &cs);
      const float n1 = x1[e] * rs * g1[e], n2 = x2[e] * rs * g2[e];
      o1[e] = n1 * cs - n2 * sn;
      o2[e] = n2 * cs + n1 * sn;
    }
    olo = pack2(o1[0], o1[1]);
    ohi = pack2(o2[0], o2[1]);
  }
  const size_t row = (size_t(sl) * a.Smax + p) * a.Hkv;
  if constexpr (KV8) {
    if (!is_q) {
      uint8_t* dst8 = reinterpret_cast<uint8_t*>(is_v ? a.vc : a.kc) + (row + (hc - a.H - (is_v ? a.Hkv : 0))) * D;
      *reinterpret_cast<uint16_t*>(dst8 + 2 * j) = f32_to_e4m3x2(o1[0] * kv_rs, o1[1] * kv_rs);
      *reinterpret_cast<uint16_t*>(dst8 + 2 * j + half) = f32_to_e4m3x2(o2[0] * kv_rs, o2[1] * kv_rs);
      return;
    }
  }
  uint16_t* dst = is_q   ? a.q_out + (size_t(m) * a.H + hc) * D
                  : is_v ? a.vc + (row + (hc - a.H - a.Hkv)) * D
                         : a.kc + (row + (hc - a.H)) * D;
  *reinterpret_cast<uint32_t*>(dst + 2 * j) = olo;
  *reinterpret_cast<uint32_t*>(dst + 2 * j + half) = ohi;
}

// ------------------------------------------------------------ attention
// GQA flash-decoding with a fixed grid of (span slot, row b, KV head)
// workgroups: graph-captured steps launch the same grid whatever the context
// length, so the grid is sized by the batch (about one round of workgroups on
// the chip), not by the cache capacity — idle workgroups were a third of the
// kernel at 1k tokens. Each slot covers a span of >= 64 tokens of row b; its
// 8 waves walk the span in 32-token pieces with an online softmax.
// A piece is loaded straight into registers with 16-byte loads whose lanes
// tile whole K/V rows (D/8 lanes per row: every instruction reads full cache
// lines); nothing is staged through LDS. A lane keeps one 8-dim group of every
// query head of the KV head (K/V are read once per GQA group), computes its
// dot products with v_dot2_f32_bf16 and finishes them with in-row DPP sums,
// and ends up holding the softmax weights of exactly the tokens whose V it
// loaded: P.V needs no data exchange until the final cross-row sum. Scores and
// P.V are fp32 VALU (G is only a compile-time loop bound): with G <= 8 query rows an MFMA tile would be >= half
// padding; the kernel is bound by the K/V stream and latency.
// The 8 waves of a slot merge through LDS; only spans split over several
// slots publish a partial (write-through + arrival ticket) that the last slot
// to finish merges, its waves taking different heads.
// Row b reads cache slot slot[b] (rows may share a slot: chunked prefill) and
// attends to positions 0..pos[b]; the output is bf16 [B][H*D].
constexpr int kAttnSlotCap = 16;  // span slots per (row, KV head) at most
// Workgroups one launch aims at: one 512-thread, 234-VGPR workgroup per CU.
// More slots per row are slower: b16 0.522 / 0.567 / 0.597 / 0.645 ms at
// 256 / 512 / 768 / 1024 (profiles/r03/decode/attn_grid_sweep_head.log).
constexpr int kAttnTargetWgs = 256;
// Smallest token span of one workgroup (a multiple of the 32-token wave
// piece). 64 (two busy waves) puts a short context on 4x the workgroups of
// 256 (one piece per wave): at batch 1 and 1k tokens the decode step went
// 396 -> 380 us on MI355X, unchanged at batch 16.
constexpr int kAttnMinSpan = 64;
constexpr int kAttnPiece = 32;  // tokens per wave piece

// Tokens per span slot for a row of `len` tokens on `slots` slots (gridDim.x):
// an even share in whole wave pieces, at least kAttnMinSpan.
__host__ __device__ __forceinline__ int attn_span(int len, unsigned slots) {
  const int span = (len + slots - 1) / slots;
  return std::max(kAttnMinSpan, (span + kAttnPiece - 1) / kAttnPiece * kAttnPiece);
}

// KV8: an FP8 (e4m3) cache. The same lane -> (token, 8-dim group) map and the same reductions; a lane
// loads its 8 dims as 8 bytes instead of 16 and decodes them with v_cvt_pk_f32_fp8 (exact). For the scores the
// decoded K is packed to bf16 pairs (exact too: 3 mantissa bits, and e4m3's exponents lie inside bf16's), so the
// dot products are the bf16 kernel's v_dot2_f32_bf16 chain against the packed q, product and sum in fp32; P.V
// takes the decoded V in fp32. The softmax and everything after the span loop are the bf16 kernel's code.
// Scales (k_scale, v_scale: fp32 [Hkv] of this layer, both nullptr for scale 1; the bf16 kernels never read them):
// the bytes hold x / s, and the KV head's two scalars undo that where it is free. K's joins the score scale
// (scale * k_scale[kvh]), V's the final normalisation (v_scale[kvh] / L for 1.f / L) at the single-slot exit and in
// the cross-slot merge, and nowhere else. At scale 1 both expressions are the unscaled ones bit for bit.
// WIN: sliding-window attention (docs/SLIDING_WINDOW.md). Row b attends to positions [lo, len) with lo = max(0, len -
// window): `window` tokens, its own included (kv_idx > q_idx - window). The span geometry is that of a row of
// len - lo tokens shifted up by lo: span and nact from len - lo, s0 = lo + sl * span. Rows below lo are never loaded
// (the piece loop starts at s0 >= lo and a lane past a piece's end re-reads that piece's last row), so what they
// hold is of no account; lo need be a multiple of nothing, since every load is a whole row's own 16 (or 8) bytes.
// Everything after the span loop is the code below, unchanged. Without WIN `window` is not read.
template <int D, int G, bool KV8 = false, bool WIN = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(1))) void k_attn(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ kc, const uint16_t* __restrict__ vc,
    const int* __restrict__ pos, const int* __restrict__ slot, int nslots, float* __restrict__ part_o,
    float* __restrict__ part_ml, unsigned* __restrict__ counters, uint16_t* __restrict__ out, int H, int Hkv, int Smax,
    int nsplit, float scale, const float* __restrict__ k_scale, const float* __restrict__ v_scale, int window) {
  constexpr int NWV = 8;
  constexpr int TOK = kAttnPiece;
  constexpr int DPL = D / kWave;  // merges: dims per lane
  constexpr int MAXC = 16;        // partials merged per load batch
  constexpr int LPR = D / 8, RPI = kWave / LPR, NI = TOK / RPI;
  __shared__ __attribute__((aligned(16))) float pacc[NWV][G][D];
  __shared__ float pml[NWV][G][2];
  __shared__ unsigned s_ticket;

  const int b = blockIdx.y / Hkv, kvh = blockIdx.y % Hkv;
  const int len = min(max(pos[b], 0), Smax - 1) + 1;
  int lo = 0;  // first position the row attends to
  if constexpr (WIN) lo = max(0, len - max(window, 1));
  const int span = attn_span(len - lo, gridDim.x);
  const int nact = (len - lo + span - 1) / span;  // slots with tokens
  const int sl = blockIdx.x;
  if (sl >= nact) return;
  const int s0 = lo + sl * span, s1 = min(len, s0 + span);
  const int sb = slot ? min(max(slot[b], 0), nslots - 1) : b;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int dg = lane % LPR, ri = lane / LPR;
  float vnum = 1.f;  // the numerator of the final normalisation
  if constexpr (KV8) {
    if (k_scale != nullptr) {
      scale *= k_scale[kvh];
      vnum = v_scale[kvh];
    }
  }

  const size_t tok_stride = size_t(Hkv) * D;
  const uint16_t* kbase = kc + size_t(sb) * Smax * tok_stride + size_t(kvh) * D + 8 * dg;
  const uint16_t* vbase = vc + size_t(sb) * Smax * tok_stride + size_t(kvh) * D + 8 * dg;
  // KV8: the same element offsets, one byte per element.
  const uint8_t* kbase8 = reinterpret_cast<const uint8_t*>(kc) + size_t(sb) * Smax * tok_stride + size_t(kvh) * D + 8 * dg;
  const uint8_t* vbase8 = reinterpret_cast<const uint8_t*>(vc) + size_t(sb) * Smax * tok_stride + size_t(kvh) * D + 8 * dg;
  // This lane's 8 query dims of every head as bf16 pairs (v_dot2 operands).
  uint4 qpk[G];
  {
    const uint16_t* qp = q + (size_t(b) * H + size_t(kvh) * G) * D + 8 * dg;
#pragma unroll
    for (int g = 0; g < G; g++) qpk[g] = *reinterpret_cast<const uint4*>(qp + size_t(g) * D);
  }

  // Running state over this wave's pieces. m is wave-uniform per head; l and
  // acc hold this lane's tokens only and are summed across rows at the end.
  float mg[G], lg[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; g++) {
    mg[g] = -INFINITY;
    lg[g] = 0.f;
#pragma unroll
    for (int k = 0; k < 8; k++) acc[g][k] = 0.f;
  }
  for (int p0 = s0 + wv * TOK; p0 < s1; p0 += NWV * TOK) {
    const int ntok = min(TOK, s1 - p0);
    // Issue the piece (lanes past the end re-read the last valid row).
    uint4 kr[KV8 ? 1 : NI], vr[KV8 ? 1 : NI];
    uint2 kr8[KV8 ? NI : 1], vr8[KV8 ? NI : 1];
#pragma unroll
    for (int j = 0; j < NI; j++) {
      const size_t t = size_t(p0 + min(j * RPI + ri, ntok - 1)) * tok_stride;
      if constexpr (KV8) kr8[j] = *reinterpret_cast<const uint2*>(kbase8 + t);
      else kr[j] = *reinterpret_cast<const uint4*>(kbase + t);
    }
#pragma unroll
    for (int j = 0; j < NI; j++) {
      const size_t t = size_t(p0 + min(j * RPI + ri, ntok - 1)) * tok_stride;
      if constexpr (KV8) vr8[j] = *reinterpret_cast<const uint2*>(vbase8 + t);
      else vr[j] = *reinterpret_cast<const uint4*>(vbase + t);
    }
    // Scores: lane (ri, dg) ends with token j*RPI + ri's score for every head.
    float sc[G][NI];
#pragma unroll
    for (int j = 0; j < NI; j++) {
      uint4 kj;
      if constexpr (KV8) kj = e4m3x8_to_bf16x8(kr8[j]);
      else kj = kr[j];
#pragma unroll
      for (int g = 0; g < G; g++) {
        float d = 0.f;
        d = dot2_bf16(qpk[g].x, kj.x, d);
        d = dot2_bf16(qpk[g].y, kj.y, d);
        d = dot2_bf16(qpk[g].z, kj.z, d);
        d = dot2_bf16(qpk[g].w, kj.w, d);
        d = (LPR == 16 ? row16_sum(d) : row8_sum(d)) * scale;
        sc[g][j] = (j * RPI + ri < ntok) ? d : -INFINITY;
      }
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
      float pm = -INFINITY;
#pragma unroll
      for (int j = 0; j < NI; j++) pm = fmaxf(pm, sc[g][j]);
      if constexpr (LPR == 8) pm = xor8_max(pm);
      pm = xor32_max(xor16_max(pm));
      const float mnew = fmaxf(mg[g], pm);
      const float corr = __expf(mg[g] - mnew);  // 0 on the first piece (mg = -inf)
      mg[g] = mnew;
      float ls = 0.f;
#pragma unroll
      for (int j = 0; j < NI; j++) {
        sc[g][j] = __expf(sc[g][j] - mnew);  // now p (0 for masked tokens)
        ls += sc[g][j];
      }
      lg[g] = lg[g] * corr + ls;
#pragma unroll
      for (int k = 0; k < 8; k++) acc[g][k] *= corr;
    }
    // P.V: the lane's own tokens times its 8 dims.
#pragma unroll
    for (int j = 0; j < NI; j++) {
      float f[8];
      if constexpr (KV8) unpack8_e4m3(vr8[j], f);
      else unpack8(vr[j], f);
#pragma unroll
      for (int g = 0; g < G; g++)
#pragma unroll
        for (int k = 0; k < 8; k++) acc[g][k] += sc[g][j] * f[k];
    }
  }
  // Sum across rows (lanes with the same dim group).
#pragma unroll
  for (int g = 0; g < G; g++) {
    float l = lg[g];
    if constexpr (LPR == 8) l = xor8_sum(l);
    lg[g] = xor32_sum(xor16_sum(l));
#pragma unroll
    for (int k = 0; k < 8; k++) {
      float v = acc[g][k];
      if constexpr (LPR == 8) v = xor8_sum(v);
      acc[g][k] = xor32_sum(xor16_sum(v));
    }
  }
  // Publish this wave to the workgroup (waves without pieces: m = -inf, l = 0).
  if (ri == 0) {
#pragma unroll
    for (int g = 0; g < G; g++) {
      *reinterpret_cast<float4*>(&pacc[wv][g][8 * dg]) = make_float4(acc[g][0], acc[g][1], acc[g][2], acc[g][3]);
      *reinterpret_cast<float4*>(&pacc[wv][g][8 * dg + 4]) = make_float4(acc[g][4], acc[g][5], acc[g][6], acc[g][7]);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int g = 0; g < G; g++) {
      pml[wv][g][0] = mg[g];
      pml[wv][g][1] = lg[g];
    }
  }
  __syncthreads();

  // Slot merge through LDS: wave w takes heads w, w + 8, ...
  const size_t hb0 = size_t(b) * H + size_t(kvh) * G;
  for (int g = wv; g < G; g += NWV) {
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < NWV; w++) M = fmaxf(M, pml[w][g][0]);
    float L = 0.f, o[DPL];
#pragma unroll
    for (int k = 0; k < DPL; k++) o[k] = 0.f;
#pragma unroll
    for (int w = 0; w < NWV; w++) {
      const float ww = pml[w][g][1] > 0.f ? __expf(pml[w][g][0] - M) : 0.f;
      L += pml[w][g][1] * ww;
#pragma unroll
      for (int k = 0; k < DPL; k++) o[k] += ww * pacc[w][g][lane + k * kWave];
    }
    const size_t hb = hb0 + g;
    if (nact == 1) {
      const float inv = KV8 ? vnum / L : 1.f / L;
#pragma unroll
      for (int k = 0; k < DPL; k++) out[hb * D + lane + k * kWave] = uint16_t(f2bf_bits(o[k] * inv));
    } else {
      float* po = part_o + (hb * nsplit + sl) * D;
#pragma unroll
      for (int k = 0; k < DPL; k++) st_wt(po + lane + k * kWave, o[k]);
      if (lane == 0) {
        st_wt(part_ml + (hb * nsplit + sl) * 2 + 0, M);
        st_wt(part_ml + (hb * nsplit + sl) * 2 + 1, L);
      }
    }
  }
  if (nact == 1) return;
  drain_stores();
  __syncthreads();
  if (threadIdx.x == 0) s_ticket = arrive(&counters[blockIdx.y]);
  __syncthreads();
  if (s_ticket != unsigned(nact - 1)) return;

  // Last slot: merge the slot partials, heads spread over the waves. Each
  // batch of up to MAXC partials (maxima, sums and vectors together) is loaded
  // before any of it is used and folded in with a running maximum, so a merge
  // of <= MAXC slots is one memory round trip (a separate pass for the global
  // maximum first cost a second one).
  for (int g = wv; g < G; g += NWV) {
    const size_t hb = hb0 + g;
    const float* ml = part_ml + hb * nsplit * 2;
    float M = -INFINITY;
    float L = 0.f, o[DPL];
#pragma unroll
    for (int k = 0; k < DPL; k++) o[k] = 0.f;
    for (int c0 = 0; c0 < nact; c0 += MAXC) {
      float pv[MAXC][DPL], wl[MAXC], ll[MAXC];
#pragma unroll
      for (int j = 0; j < MAXC; j++) {
        const bool ok = c0 + j < nact;
        const int c = min(c0 + j, nact - 1);
        wl[j] = ld_wt(ml + 2 * c);
        ll[j] = ok ? ld_wt(ml + 2 * c + 1) : 0.f;
#pragma unroll
        for (int k = 0; k < DPL; k++) pv[j][k] = ld_wt(part_o + (hb * nsplit + c) * D + lane + k * kWave);
      }
      float Mb = M;
#pragma unroll
      for (int j = 0; j < MAXC; j++)
        if (ll[j] > 0.f) Mb = fmaxf(Mb, wl[j]);
      const float rs = M == -INFINITY ? 0.f : __expf(M - Mb);  // rescale what is folded in so far
      L *= rs;
#pragma unroll
      for (int k = 0; k < DPL; k++) o[k] *= rs;
      M = Mb;
#pragma unroll
      for (int j = 0; j < MAXC; j++) {
        const float ww = ll[j] > 0.f ? __expf(wl[j] - M) : 0.f;
        L += ll[j] * ww;
#pragma unroll
        for (int k = 0; k < DPL; k++) o[k] += ww * pv[j][k];
      }
    }
    const float inv = KV8 ? vnum / L : 1.f / L;
#pragma unroll
    for (int k = 0; k < DPL; k++) out[hb * D + lane + k * kWave] = uint16_t(f2bf_bits(o[k] * inv));
  }
  if (threadIdx.x == 0) st_wt(&counters[blockIdx.y], 0u);
}

// Partial slots per head in part_o / part_ml (k_attn's nsplit): the most span
// slots a launch can have. k_attn writes slot sl < nact <= gridDim.x <= stride:
// span >= ceil(len / gridDim.x), so nact = ceil(len / span) <= gridDim.x, and
// attn_slots() never exceeds the stride.
int attn_part_stride(int max_seq) { return std::min(kAttnSlotCap, (max_seq + kAttnMinSpan - 1) / kAttnMinSpan); }

// Span slots per (row, KV head), k_attn's gridDim.x: about one round of
// workgroups on the chip. Sized by the batch; the context enters through pos.
int attn_slots(int B, int Hkv, int max_seq) {
  return std::max(1, std::min(kAttnTargetWgs / std::max(1, B * Hkv), attn_part_stride(max_seq)));
}
// ... of a layer with a sliding window: a row has min(max_seq, window) tokens at most, so the slots are those of a
// cache that long. Never more than attn_slots(B, Hkv, max_seq), so within kAttnSlotCap and the partials' stride,
// which stays attn_part_stride(max_seq) for every layer.
int attn_window_slots(int B, int Hkv, int max_seq, int window) {
  return attn_slots(B, Hkv, std::min(max_seq, std::max(window, 1)));
}

// Measured on MI355X and rejected; the code is gone, the findings stay. This
// file reads no environment variables: what ships is the one path below.
//  - Split-K over workgroups (write-through slabs, arrival ticket, last
//    arriver combines): the seam costs more than the extra workgroups win at
//    d_model <= 2048. QKV 8.7 -> 13.5 us, O 7.4 -> 12.0, down 17.3 -> 17.3
//    (2048-wide config, batch 8).
//  - Narrow duplicate-column tiles (8 or 4 columns, the other lanes repeating
//    them): O alone 5.8 -> 5.5 us at batch 1, QKV 6.1 -> 7.8; O and down at
//    one workgroup per CU 1-4 % slower end to end. 16 everywhere is fastest.
//  - K parts on QKV and gate/up: batch 1, QKV at 4 columns 0.360 -> 0.373 ms
//    per step, gate/up 0.368 (8 columns) and 0.391 (4). Their grids already
//    cover the chip. K parts stay on O and down only (0.372 -> 0.359 ms).
//  - A 16-token attention piece (128 instead of 234 VGPRs, two workgroups per
//    CU): small, ctx 1024, b1 0.358 -> 0.365 ms, b16 0.522 -> 0.531, b64
//    1.125 -> 1.134 (profiles/r03/decode/attn_tok_ab_head.log).
//  - 8-step load batches: at most 4 k-steps per batch keeps more waves
//    resident. Batch 1 396 -> 389 us per step, batch 16 unchanged.
//  - 16-wave workgroups: 8 beats 16 by 20-30 % at K = 5632 (down 9.4 ->
//    10.5 us); the reduction and barrier cost more than the loads in flight.
//  - Non-temporal weight loads: 1.75x slower on the 4-layer config, 5 % slower
//    on the 0.85 GB config (profiles/r02/decode/decode_sweep_s9.log). A decode
//    step replays the same weights, and the 256 MB MALL keeps them resident.
//  - One workgroup sharing each weight fragment across the four tiles of a
//    64-row step: small, 64 rows 1.19 -> 1.26 ms; 16 streams 3.0 K -> 2.7 K
//    tok/s (profiles/r02/decode/decode_sweep_s10_rowtiles.log). The load
//    path, not HBM, becomes the limit.
//  - The argmax merge folded into the LM head's last block: 0.359 -> 0.366 ms
//    at batch 1, 0.522 -> 0.554 at 16. 1,000 arrivals on one counter cost more
//    than the launch.
//  - A persistent O -> gate/up -> down kernel (in-order tile queue,
//    write-through hand-offs): small b1 0.358 -> 0.61-1.09 ms in every variant
//    (profiles/r03/decode_block/).
//  - FP8 KV cache, k_attn<D, G, true>: fp32 FMAs against q unpacked to fp32 (8 G more registers, <128,8> spilled
//    232 bytes per lane) gave way before any run to packing the decoded K to bf16 for the v_dot2 chain
//    (<128,4> 184 VGPRs, <128,8> 72 bytes). A layout with 16-byte loads (D / 16 lanes per row) was not tried.
//    What ships, against bf16 (profiles/kv_fp8.json): batch 16 at 32k tokens 1.987 -> 1.479 ms (small) and
//    4.298 -> 3.701 (Llama-3.2-1B's shape); batch 1 0.2-0.6 % slower at every context.
//  - FP8 weights, k_skinny<.., W8 = 1>: what ships is 8-byte B loads at a 32-byte k-step stride, decoded to the bf16
//    fragment ahead of the MFMA (at most 88 VGPRs, no spills; the bf16 instantiations keep their register counts).
//    Against bf16 (profiles/weight_fp8.json, ctx 1024): Llama-3.1-8B's shape 3.210 -> 2.835 ms at batch 1 and
//    4.713 -> 4.338 at 16, small 0.368 -> 0.339 and 0.521 -> 0.498, tiny 0.140 -> 0.136: never slower, far from 2x.
//    A weight layout with K permuted offline so that one 16-byte load feeds two k-steps was not tried and not
//    measured; neither was decoding through FP8 or scaled MFMA (the activation stays bf16).
//  - MXFP4 weights, k_skinny<.., W8 = 2>: what ships is the natural byte order, one 4-byte B load and one 1-byte scale
//    load per lane, k-step and subtile, decoded by v_cvt_scalef32_pk_bf16_fp4 ahead of the MFMA. It is correct bit for
//    bit and it is slow: a quarter of the bytes in twice the load instructions of bf16, each fetching a quarter of a
//    16-byte one. Against bf16 and FP8 (docs/WEIGHT_MXFP4_raw.json, ctx 1024, ms per step): Llama-3.1-8B's shape
//    3.193 / 2.839 / 4.291 at batch 1 and 4.764 / 4.356 / 5.864 at 16, Llama-3.2-1B's 0.816 / 0.737 / 0.940 and
//    1.191 / 1.133 / 1.410, small 0.368 / 0.339 / 0.393 and 0.523 / 0.502 / 0.595, tiny 0.140 / 0.136 / 0.147 and
//    0.187 / 0.177 / 0.196: slower than both at every shape measured. The blocked order (K permuted offline so that one
//    16-byte load feeds a lane's four k-steps, and the four scale bytes one 4-byte load) was not built and not
//    measured; it is the first thing to try, and the format's bytes on the device would be the same.
//  - A two-deep load-batch pipeline (every projection +0.5-1.8 us) and one
//    workgroup per CU forced through padded LDS (QKV 5.9 -> 9.9 us)
//    (profiles/r02/decode/decode_sweep_s8.log).
}  // namespace
