// Grouped int4 weights of the fused decode step for gfx950 (docs/WEIGHT_INT4.md): the k_skinny<.., W8 = 3>
// instantiations that decode_fused_set.h's predicate names, and k_embed_xg. Planning, the workspace, the weight table
// and the launches are decode_fused.hip's, which looks its kernels up here. This file is compiled without packed fp32
// instructions (build.py): the decode is eight scalar fmas per word.
#include "decode_w4g.h"

#include "decode_fused_set.h"

namespace p2pt_w4g {

const void* skinny_kernel(int nw, int tn, int epi, int um) {
  const void* k = nullptr;
  pick([&](auto cnw, auto ctn, auto cepi, auto cum) {
    if constexpr (skinny_exists(cnw, ctn, cepi, cum, kW4g))
      k = reinterpret_cast<const void*>(&k_skinny<cnw, ctn, cepi, cum, kW4g>);
  }, nw, SkinnyWaves{}, tn, SkinnyTiles{}, epi, SkinnyEpis{}, um, SkinnyBatches{});
  return k;
}

hipError_t launch_embed_xg(const uint16_t* embed, const int64_t* tok, uint16_t* resid, float* ss_out, int dim, int vocab,
                           const uint16_t* g, uint16_t* xg, int B, hipStream_t s) {
  if (!g || !xg || B <= 0 || dim % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_embed_xg<0>, dim3(B), dim3(256), 0, s, embed, tok, resid, ss_out, dim, vocab, g, xg);
  return hipGetLastError();
}

}  // namespace p2pt_w4g
