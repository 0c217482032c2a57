// The set of kernel instantiations of the fused decode step, stated once: decode_fused.hip (every format but grouped
// int4 and block-scaled FP8), decode_w4g.hip (grouped int4, compiled without packed fp32 instructions), decode_f8g.hip
// (block-scaled FP8) and decode_lora.hip (the LoRA-delta variants) all instantiate from these lists and these predicates, and nothing else.
#pragma once
#include "decode_fused_kernels.h"

#include <type_traits>
#include <utility>

namespace {

// ------------------------------------------------------------ the kernels that exist
// Stated once: a list of values per template parameter and, for k_skinny, one predicate over their product. The
// three *_kernel() lookups instantiate exactly this set; the launchers, p2pt_llama_plan_kernels and dims_ok read
// nothing else.
template <int... V>
using Ints = std::integer_sequence<int, V...>;
using HeadDims = Ints<64, 128>;  // D of k_attn and k_qknorm_rope
// G of k_attn, the GQA ratio H / Hkv (models/checkpoint.py mirrors it as _GQA_RATIOS). 5, 6 and 7 are the Qwen2 /
// Qwen2.5 family's (40/8, 12/2, 14/2 and 28/4). 3 is absent: no checkpoint the loader accepts uses it.
using GqaRatios = Ints<1, 2, 4, 5, 6, 7, 8>;
using Flags = Ints<0, 1>;  // KV8 and WIN of k_attn; TAB and KV8 of k_qknorm_rope
using SkinnyFormats = Ints<0, 1, 2>;  // W8 of k_skinny in decode_fused.hip: bf16, FP8, MXFP4
constexpr int kW4g = 3;  // W8 of k_skinny in decode_w4g.hip: grouped int4 (docs/WEIGHT_INT4.md)
constexpr int kF8g = 4;  // W8 of k_skinny in decode_f8g.hip: block-scaled FP8 (docs/WEIGHT_FP8G128.md)
using SkinnyWaves = Ints<4, 8>;
using SkinnyTiles = Ints<1, 2>;
using SkinnyBatches = Ints<1, 2, 4>;
using SkinnyEpis = Ints<EPI_STORE, EPI_ROPE, EPI_SILU, EPI_RESID, EPI_ARGMAX, EPI_ROPE_BIAS, EPI_ROPE_TAB,
                        EPI_ROPE_BIAS_TAB, EPI_ROPE_KV8, EPI_ROPE_BIAS_KV8, EPI_ROPE_TAB_KV8, EPI_ROPE_BIAS_TAB_KV8>;
constexpr bool skinny_exists(int nw, int tn, int epi, int um, int w8) {
  // Two subtiles for the LM head and the standalone GEMM (plain STORE has both), one for every other epilogue.
  if (tn != (epi == EPI_ARGMAX ? 2 : 1) && !(epi == EPI_STORE && tn == 2)) return false;
  // FP8 weights run the five GEMMs of a step only (the standalone GEMM stays bf16), so they carry what plan_gemm
  // can give those: the LM head's fixed 4 waves with any load batch, and for the others the (nw, um) pairs of
  // fixed_nw == 0 below. 47 instantiations beside the 66 of bf16.
  if (w8 && epi == EPI_STORE && tn == 2) return false;
  // MXFP4 weights run a layer's four GEMMs only (the LM head stays FP8): every epilogue those can be planned with,
  // the eight RoPE ones, SILU, RESID and, for QK-norm models, STORE with one subtile, never ARGMAX, each with the
  // (nw, um) pairs of fixed_nw == 0. 44 instantiations beside the 47 of FP8 and the 66 of bf16.
  // Grouped int4 weights likewise (the LM head stays bf16): the same 44, in decode_w4g.hip. Block-scaled FP8 weights
  // likewise: the same 44, in decode_f8g.hip.
  if (w8 >= 2 && epi == EPI_ARGMAX) return false;
  if (w8 && epi == EPI_ARGMAX) return nw == 4;
  if (w8) return nw == 4 || um == 4;
  // The table and FP8-cache epilogues run QKV projections only, so they carry just the (nw, um) pairs plan_gemm
  // can give one (fixed_nw == 0): 4 waves up to 16 k-steps with um 1, 2 or 4, and 8 waves from 17 on, where a
  // wave's share is at least 3 k-steps and um is 4.
  if (epi_has_table(epi) || epi_kv8(epi)) return nw == 4 || um == 4;
  return true;
}
// k_skinny<.., W8 = 0, LORA = 1> in decode_lora.hip (docs/LORA.md): bf16 weights and the epilogues a layer's four
// projections of a model without QK-norm can be planned with, the eight RoPE ones, SILU and RESID, one subtile, each
// with the (nw, um) pairs its base kernel has: 48 instantiations.
constexpr bool skinny_lora_exists(int nw, int tn, int epi, int um) {
  return tn == 1 && (epi_is_rope(epi) || epi == EPI_SILU || epi == EPI_RESID) && skinny_exists(nw, tn, epi, um, 0);
}
template <int... V>
constexpr bool contains(Ints<V...>, int v) {
  return ((v == V) || ...);
}

// pick(f, v0, Ints<...>{}, v1, Ints<...>{}, ...) calls f(c0, c1, ...), each c a std::integral_constant equal to
// its run-time v, and calls nothing when some v is in no list.
template <typename F>
void pick(F&& f) {
  f();
}
template <typename F, int... V, typename... Rest>
void pick(F&& f, int v, Ints<V...>, Rest... rest) {
  ((v == V ? pick([&](auto... c) { f(std::integral_constant<int, V>{}, c...); }, rest...) : void()), ...);
}

}  // namespace
