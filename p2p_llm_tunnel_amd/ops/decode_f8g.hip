// Block-scaled FP8 weights of the fused decode step for gfx950 (docs/WEIGHT_FP8G128.md): the k_skinny<.., W8 = 4>
// instantiations that decode_fused_set.h's predicate names. Planning, the weight table and the launches are
// decode_fused.hip's, which looks its kernels up here.
#include "decode_f8g.h"

#include "decode_fused_set.h"

namespace p2pt_f8g {

const void* skinny_kernel(int nw, int tn, int epi, int um) {
  const void* k = nullptr;
  pick([&](auto cnw, auto ctn, auto cepi, auto cum) {
    if constexpr (skinny_exists(cnw, ctn, cepi, cum, kF8g))
      k = reinterpret_cast<const void*>(&k_skinny<cnw, ctn, cepi, cum, kF8g>);
  }, nw, SkinnyWaves{}, tn, SkinnyTiles{}, epi, SkinnyEpis{}, um, SkinnyBatches{});
  return k;
}

}  // namespace p2pt_f8g
