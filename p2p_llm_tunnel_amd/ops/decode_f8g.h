// Block-scaled FP8 weights of the fused decode step (docs/WEIGHT_FP8G128.md): what decode_fused.hip (planning, weight
// table, launches) and decode_f8g.hip (the k_skinny<.., W8 = 4> instantiations) share. The instantiations are a
// translation unit of their own so that decode_fused.hip compiles the kernels it always did; the kernels themselves are
// decode_fused_kernels.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace p2pt_f8g {

// The host handle of k_skinny<nw, tn, epi, um, 4>, to be launched with a GemmArgs; nullptr where decode_fused_set.h's
// skinny_exists has no such instantiation.
const void* skinny_kernel(int nw, int tn, int epi, int um);

}  // namespace p2pt_f8g
