// Routed-expert FFN of the fused decode step (docs/MOE.md): what decode_fused.hip (planning, workspace, entry points)
// and decode_moe.hip (the four kernels' instantiations and launches) share. The kernels themselves are in
// decode_moe_kernels.h. decode_moe.hip is a translation unit of its own because it is compiled without packed fp32
// instructions (build.py), which the rest of the library keeps.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace p2pt_moe {

constexpr int kMaxExperts = 128;  // E: a lane of k_moe_route holds experts lane and lane + 64
constexpr int kMaxTopK = 8;       // experts per token: route_id holds at most kMaxM * 8 ints
constexpr int kRouteWaves = 4, kCombineWaves = 4;  // waves per workgroup of k_moe_route and k_moe_combine

// The mixture-of-experts shape of a model, beside the plans as WeightFormat and Windows are (mirrored with ctypes).
// With it, LlamaDims::ffn is the per-expert intermediate size.
struct MoeDims {
  int n_experts;  // E
  int top_k;      // experts per token
  int norm_topk;  // 1: the top-k probabilities are renormalised to sum to one (Mixtral)
};

// The format of the stacked expert matrices (w_gate_up, w_down), beside MoeDims as WeightFormat is beside the plans
// (mirrored with ctypes; docs/MOE_FP8.md). 0: bf16. 1: OCP e4m3fn bytes in k-step-pair order with one fp32 scale per
// (expert, output row). 2 (docs/MOE_MXFP4.md): OCP MXFP4, e2m1 nibbles two to a byte in k-step-quad order with one
// e8m0 scale byte per 32-element block of a row, and no fp32 scale. It changes no field of MoePlan: the grids, wave
// counts, row tiles and load batches are the bf16 kernels'. The router, the attention projections and the LM head are
// bf16 either way.
struct ExpertFormat {
  int w8;
};

// What the four kernels launch for B rows (mirrored with ctypes): every field a function of (B, dims, MoeDims).
struct MoePlan {
  int route_grid, route_waves;      // k_moe_route: one workgroup per row
  int gu_grid_x, gu_grid_y;         // k_moe_gate_up<gu_nw, gu_rt, gu_um>: (16-column tiles of [2 ffn_e], expert)
  int gu_nw, gu_rt, gu_um;
  int dn_grid_x, dn_grid_y;         // k_moe_down<dn_nw, dn_rt, dn_um>: (16-column tiles of [dim], expert)
  int dn_nw, dn_rt, dn_um;
  int cb_grid, cb_cols, cb_waves;   // k_moe_combine: cb_grid workgroups of cb_cols columns; cb_grid is the ss_in of
                                    // the next layer's QKV GEMM and of the LM head
};

// One layer's pointers. Shapes: dims of the model, E / top_k of MoeDims, B rows.
struct MoeArgs {
  uint16_t* resid;          // bf16 [B][dim], updated in place by k_moe_combine
  float* ss;                // fp32 [parts][kMaxM]: read (ss_in partials) by k_moe_route, rewritten (cb_grid) by combine
  int ss_in;                // partials the residual's producer left
  const uint16_t* router;   // bf16 [E][dim], the FFN norm weight folded in
  const void* w_gate_up;    // bf16 [E][2 ffn_e][dim], folded, rows interleaved (gate_j, up_j) per expert; with
                            // ExpertFormat::w8 = 1 e4m3 bytes of the same shape, every row in k-step-pair order;
                            // with w8 = 2 nibble bytes [E][2 ffn_e][dim / 2], every row in k-step-quad order
  const void* w_down;       // bf16 (or e4m3 bytes, or nibble bytes of half the count, likewise) [E][dim][ffn_e]
  int* route_id;            // int32 [B][top_k], descending probability
  float* route_w;           // fp32 [B][top_k]
  float* route_rs;          // fp32 [B]: 1 / rms of the row, as the router used it
  uint16_t* moe_h;          // bf16 [B * top_k][ffn_e]
  float* moe_part;          // fp32 [B][top_k][dim]
  int B, dim, ffn, E, top_k, norm_topk;
  float eps;
  const float* gate_up_scale;  // ExpertFormat::w8 = 1: fp32 [E][2 ffn_e], the row scales of w_gate_up; else nullptr
  const float* down_scale;     // ExpertFormat::w8 = 1: fp32 [E][dim]; else nullptr
  const uint8_t* gate_up_exp;  // ExpertFormat::w8 = 2: e8m0 [E][2 ffn_e][dim / 32], natural order; else nullptr
  const uint8_t* down_exp;     // ExpertFormat::w8 = 2: e8m0 [E][dim][ffn_e / 32]; else nullptr
};

// The four launches of one MoE layer, in order, on stream s; a plan that names a kernel which is not instantiated, or
// arguments outside what the kernels index, are hipErrorInvalidValue and nothing is launched. f: the experts' format;
// the GEMM kernels are then its instantiations, the fp32 scales must be there exactly when it is FP8 and the e8m0
// scales exactly when it is MXFP4.
hipError_t launch_moe(const MoePlan& p, const MoeArgs& a, hipStream_t s, ExpertFormat f = ExpertFormat{0});
// Whether the plan's kernels exist in format f (host only).
bool moe_kernels_exist(const MoePlan& p, ExpertFormat f = ExpertFormat{0});

}  // namespace p2pt_moe
