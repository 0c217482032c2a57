// Grouped int4 weights of the fused decode step (docs/WEIGHT_INT4.md): what decode_fused.hip (planning, workspace, weight
// table, launches) and decode_w4g.hip (the k_skinny<.., W8 = 3> instantiations and k_embed_xg) share. decode_w4g.hip is
// a translation unit of its own because it is compiled without packed fp32 instructions (build.py), which the rest of
// the library keeps; the kernels themselves are decode_fused_kernels.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace p2pt_w4g {

// The host handle of k_skinny<nw, tn, epi, um, 3>, to be launched with a GemmArgs; nullptr where decode_fused_set.h's
// skinny_exists has no such instantiation.
const void* skinny_kernel(int nw, int tn, int epi, int um);

// k_embed_xg on B workgroups: the embedding gather that also stores xg = bf16(row * g).
hipError_t launch_embed_xg(const uint16_t* embed, const int64_t* tok, uint16_t* resid, float* ss_out, int dim, int vocab,
                           const uint16_t* g, uint16_t* xg, int B, hipStream_t s);

}  // namespace p2pt_w4g
