// LoRA adapters in the fused decode step for gfx950 (docs/LORA.md): the k_skinny<.., W8 = 0, LORA = 1> instantiations
// that decode_fused_set.h's skinny_lora_exists names. Planning, the workspace and the launches are decode_fused.hip's,
// which looks its kernels up here; a translation unit of its own so that decode_fused.hip instantiates what it did.
#include "decode_lora.h"

#include "decode_fused_set.h"

namespace p2pt_lora {

const void* skinny_kernel(int nw, int tn, int epi, int um) {
  const void* k = nullptr;
  pick([&](auto cnw, auto ctn, auto cepi, auto cum) {
    if constexpr (skinny_lora_exists(cnw, ctn, cepi, cum))
      k = reinterpret_cast<const void*>(&k_skinny<cnw, ctn, cepi, cum, 0, 1>);
  }, nw, SkinnyWaves{}, tn, SkinnyTiles{}, epi, SkinnyEpis{}, um, SkinnyBatches{});
  return k;
}

}  // namespace p2pt_lora
