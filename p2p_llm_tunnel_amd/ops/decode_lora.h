// LoRA adapters in the fused decode step (docs/LORA.md): what decode_fused.hip (planning, workspace, launches),
// decode_lora.hip (the k_skinny<.., LORA = 1> instantiations) and lora_delta.hip (k_lora_delta) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace p2pt_lora {

constexpr int kMaxAdapters = 8;  // adapters beside one base model
constexpr int kMaxRank = 192;    // R of one projection: three stacked parts of PEFT rank <= 64
constexpr int kWaves = 4;        // per workgroup of k_lora_delta: they split K in the shrink, the columns in the expand
constexpr int kColTiles = 4;     // 16-column subtiles of delta per wave: a workgroup owns kWaves * kColTiles * 16 columns
constexpr int kRankGroup = 4;    // 16-row tiles of A' per shrink pass: 64 ranks share one pass over x

// What k_lora_delta launches for M rows of a projection [N][K] at padded rank R (mirrored with ctypes).
struct LoraPlan {
  int grid_x, grid_y;  // (column tiles of delta, 16-row tiles of the step)
  int waves;           // per workgroup
  int cols;            // delta columns per workgroup
  int passes;          // shrink passes per adapter of a tile: ceil(R / 64)
};

// One projection's adapters. A [n_adapters][R][K] and B [n_adapters][N][R], bf16, 16-byte aligned; R a multiple of
// 16 up to kMaxRank; K a multiple of 32; N a multiple of 16; x [M][K] bf16; aid int32 [M], -1 (or anything outside
// 0..n_adapters-1): no adapter; delta fp32 [M][N].
struct LoraArgs {
  const uint16_t* x;
  const int* aid;
  const uint16_t* A;
  const uint16_t* B;
  float* delta;
  int M, N, K, R, n_adapters;
};

// Whether the shapes can be launched at all (host only).
bool shapes_ok(int M, int N, int K, int R, int n_adapters);
LoraPlan plan(int M, int N, int K, int R);
// k_lora_delta on plan()'s grid; hipErrorInvalidValue for shapes it refuses or a null pointer.
hipError_t launch_delta(const LoraArgs& a, hipStream_t s);

// The host handle of k_skinny<nw, tn, epi, um, 0, 1>, to be launched with a GemmArgs; nullptr where
// decode_fused_set.h's skinny_lora_exists has no such instantiation.
const void* skinny_kernel(int nw, int tn, int epi, int um);

}  // namespace p2pt_lora
