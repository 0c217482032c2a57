// The routed-expert FFN's kernel instantiations and launches (docs/MOE.md). The kernels are in decode_moe_kernels.h;
// planning, the workspace and the entry points are decode_fused.hip's, which calls launch_moe once per layer. A
// translation unit of its own: build.py compiles it without packed fp32 instructions (why: decode_fused_kernels.h, at
// P2PT_NO_PK_F32), the rest of the library as before, so no existing kernel's code changes. That per-function
// attribute was not taken here: under it only always_inline code is inlined, and these kernels use bf16_common.h's
// conversions and reductions, __expf, rsqrtf, __ballot and __syncthreads, which would each have to be spelled out
// again as builtins. The price: this unit compiles decode_fused_kernels.h's two non-template kernels (k_embed,
// k_argmax_merge) a second time, unused.
#include "decode_moe_kernels.h"

namespace {

using p2pt_moe::MoePlan;
using MoeKernel = void (*)(MoeArgs);

// k_moe_gate_up / k_moe_down<NW, RT, UM, W8> exist for NW in {4, 8}, RT in {1, 2, 4}, UM in {1, 2, 4}, W8 in {0, 1, 2}:
// what plan_moe can name, in every expert format. nullptr for anything else. An FP8 kernel's load batch is counted in
// k-step pairs (decode_moe_kernels.h), so a plan's um of 1 runs 2 k-steps a batch: the <.., 2, 1> instantiation. An
// MXFP4 kernel's is one k-step quad at every um, so every um the plan can name runs the <.., 1, 2> instantiation.
template <bool DOWN, int NW, int RT, int W8>
MoeKernel by_um(int um) {
  if constexpr (W8 == 2) {
    if (um == 1 || um == 2 || um == 4) return DOWN ? k_moe_down<NW, RT, 1, 2> : k_moe_gate_up<NW, RT, 1, 2>;
    return nullptr;
  } else {
    switch (um) {
      case 1:
        if constexpr (W8 != 0) return DOWN ? k_moe_down<NW, RT, 2, W8> : k_moe_gate_up<NW, RT, 2, W8>;
        else return DOWN ? k_moe_down<NW, RT, 1> : k_moe_gate_up<NW, RT, 1>;
      case 2: return DOWN ? k_moe_down<NW, RT, 2, W8> : k_moe_gate_up<NW, RT, 2, W8>;
      case 4: return DOWN ? k_moe_down<NW, RT, 4, W8> : k_moe_gate_up<NW, RT, 4, W8>;
    }
    return nullptr;
  }
}
template <bool DOWN, int NW, int W8>
MoeKernel by_rt(int rt, int um) {
  switch (rt) {
    case 1: return by_um<DOWN, NW, 1, W8>(um);
    case 2: return by_um<DOWN, NW, 2, W8>(um);
    case 4: return by_um<DOWN, NW, 4, W8>(um);
  }
  return nullptr;
}
template <bool DOWN, int W8>
MoeKernel by_nw(int nw, int rt, int um) {
  return nw == 4 ? by_rt<DOWN, 4, W8>(rt, um) : nw == 8 ? by_rt<DOWN, 8, W8>(rt, um) : nullptr;
}
template <bool DOWN>
MoeKernel moe_kernel(int nw, int rt, int um, int w8 = 0) {
  return w8 == 0   ? by_nw<DOWN, 0>(nw, rt, um)
         : w8 == 1 ? by_nw<DOWN, 1>(nw, rt, um)
         : w8 == 2 ? by_nw<DOWN, 2>(nw, rt, um)
                   : nullptr;
}

int log2_exact(int v) { return v == 4 ? 2 : v == 8 ? 3 : v == 16 ? 4 : -1; }

}  // namespace

namespace p2pt_moe {

bool moe_kernels_exist(const MoePlan& p, ExpertFormat f) {
  return moe_kernel<false>(p.gu_nw, p.gu_rt, p.gu_um, f.w8) && moe_kernel<true>(p.dn_nw, p.dn_rt, p.dn_um, f.w8) &&
         p.route_waves == kRouteWaves && p.cb_waves == kCombineWaves && log2_exact(p.cb_cols) > 0;
}

hipError_t launch_moe(const MoePlan& p, const MoeArgs& a, hipStream_t s, ExpertFormat f) {
  if (!moe_kernels_exist(p, f)) return hipErrorInvalidValue;
  // What the kernels index without a test of their own.
  if (a.B < 1 || a.B > kMaxM || a.E < 1 || a.E > kMaxExperts || a.top_k < 1 || a.top_k > kMaxTopK || a.top_k > a.E)
    return hipErrorInvalidValue;
  if (a.dim < 32 || a.dim % 32 || a.ffn < 32 || a.ffn % 32 || a.ss_in < 1) return hipErrorInvalidValue;
  // Each expert's slice, and both activation buffers, below kOob.
  if (size_t(2) * a.ffn * a.dim * 2 >= kOob || size_t(kMaxPairs) * a.ffn * 2 >= kOob || size_t(kMaxM) * a.dim * 2 >= kOob)
    return hipErrorInvalidValue;
  if (p.route_grid != a.B || p.gu_grid_x * 16 != 2 * a.ffn || p.dn_grid_x * 16 != a.dim || p.gu_grid_y != a.E ||
      p.dn_grid_y != a.E || p.cb_grid * p.cb_cols != a.dim)
    return hipErrorInvalidValue;
  if (!a.resid || !a.ss || !a.router || !a.w_gate_up || !a.w_down || !a.route_id || !a.route_w || !a.route_rs ||
      !a.moe_h || !a.moe_part)
    return hipErrorInvalidValue;
  // FP8 experts: whole k-step pairs of both K (the kernels split and load K by the pair), each expert's slice in bytes
  // below kOob (half the bf16 slice above, tested on its own all the same), and the row scales there exactly then.
  if (f.w8 == 1 && (a.dim % 64 || a.ffn % 64 || size_t(2) * a.ffn * a.dim >= kOob)) return hipErrorInvalidValue;
  if ((f.w8 == 1) != (a.gate_up_scale != nullptr) || (f.w8 == 1) != (a.down_scale != nullptr))
    return hipErrorInvalidValue;
  // MXFP4 experts: whole k-step quads of both K, each expert's nibble slice (and so its scale slice, a sixteenth of
  // it) below kOob, the e8m0 scales there exactly then, and no fp32 scales (the test above).
  if (f.w8 == 2 && (a.dim % 128 || a.ffn % 128 || size_t(a.ffn) * a.dim >= kOob)) return hipErrorInvalidValue;
  if ((f.w8 == 2) != (a.gate_up_exp != nullptr) || (f.w8 == 2) != (a.down_exp != nullptr))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_moe_route, dim3(p.route_grid), dim3(kRouteWaves * 64), 0, s, a);
  hipLaunchKernelGGL(moe_kernel<false>(p.gu_nw, p.gu_rt, p.gu_um, f.w8), dim3(p.gu_grid_x, p.gu_grid_y), dim3(p.gu_nw * 64), 0,
                     s, a);
  hipLaunchKernelGGL(moe_kernel<true>(p.dn_nw, p.dn_rt, p.dn_um, f.w8), dim3(p.dn_grid_x, p.dn_grid_y), dim3(p.dn_nw * 64), 0,
                     s, a);
  hipLaunchKernelGGL(k_moe_combine, dim3(p.cb_grid), dim3(kCombineWaves * 64), 0, s, a, log2_exact(p.cb_cols));
  return hipGetLastError();
}

}  // namespace p2pt_moe
