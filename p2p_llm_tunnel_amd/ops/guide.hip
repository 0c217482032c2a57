// Guided decoding for the on-node inference endpoint (gfx950 / CDNA4): a
// token-level automaton per sequence, on device, inside the captured decode
// step, after the penalties (when the engine has them) and ahead of the sampler.
//
//   p2pt_guide   one 1024-thread workgroup (16 waves of 64) per row, the row's
//     only owner. `arena` is int16 [arena_states, V]: the tables of the resident
//     patterns, one after the other. A slot's table starts at arena row base[s]
//     (-1: the slot is not guided) and its entries are states of that table,
//     counted from its first row: arena[base + c][t] is the state after token t
//     in state c, or -1 when t is not allowed there. cur[s] is the slot's state.
//     A row whose slot is out of range, whose base is negative or whose
//     base + cur lies outside the arena is OFF: work[r] becomes a bit-for-bit
//     copy of x[r] (nothing moves when the two are one buffer), ids[r], base and
//     cur are not touched. A row that is ON:
//       1. advance: a decode row's input token tok[r] was sampled by the
//          previous step, whose host has not seen it yet. With dec[r] set,
//          t = arena[base + cur][tok]; cur = t when t >= 0 (and inside the
//          arena), otherwise the state stands. EVERY lane reads cur[s] and the
//          transition, then a barrier, then lane 0 alone writes cur[s] back: no
//          lane reads another lane's store. A prompt row (the last one emits the
//          first token) advances nothing.
//       2. mask: work[v] = arena[base + cur][v] >= 0 ? x[v] : -inf, the kept
//          elements bit for bit. x may be work itself (the penalty kernel's
//          output, masked in place): each lane stores only elements it loaded.
//       3. ids[r] = argmax of the stored row by row_common.h's rules (take_bits,
//          block_argmax; k_argmax_merge's too: lowest id on ties, NaN never wins,
//          a row with nothing above -inf gives 0), kept in registers while
//          storing. The sampler reads work, so greedy decoding and sampling see
//          the same numbers.
//     16-byte loads of x with ONE 16-byte load of the table row per 8 elements
//     when V % 8 == 0 (every row of x, work and the arena then starts on a
//     16-byte boundary); any other V runs element by element.
//
//   p2pt_guide_reset   admission of a request into a slot, never captured: one
//     lane stores base[slot] (-1 switches the slot off) and cur[slot] = 0.
#include "row_common.h"

namespace {

using namespace p2pt_gpu;

constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr uint32_t kNegInf = 0xFF80u;  // bf16 -inf

// 8 elements from loaded vectors: mask, store, keep the lane's argmax. A table entry is allowed when its sign
// bit is clear.
__device__ __forceinline__ void mask_chunk(int c, const uint4& lv, const uint4& tv, uint4* w4, float& b, int& bi) {
  uint32_t raw[8], o[8];
  bits8(lv, raw);
  const uint32_t neg[8] = {tv.x & 0x8000u, tv.x & 0x80000000u, tv.y & 0x8000u, tv.y & 0x80000000u,
                           tv.z & 0x8000u, tv.z & 0x80000000u, tv.w & 0x8000u, tv.w & 0x80000000u};
#pragma unroll
  for (int j = 0; j < 8; j++) {
    o[j] = neg[j] ? kNegInf : raw[j];
    take_bits(b, bi, o[j], c * 8 + j);
  }
  w4[c] = pack_bits8(o);
}

__global__ __launch_bounds__(kThreads) void k_guide(const uint16_t* x, uint16_t* work, int64_t* __restrict__ ids,
                                                    const int64_t* __restrict__ tok, const int64_t* __restrict__ dec,
                                                    const int64_t* __restrict__ slot, const int* __restrict__ base,
                                                    int* cur, int n_slots, const int16_t* __restrict__ arena,
                                                    int arena_states, int V) {
  const int row = blockIdx.x;
  const uint16_t* lr = x + size_t(row) * V;
  uint16_t* wr = work + size_t(row) * V;
  const bool vec = (V & 7) == 0;
  const int nvec = V >> 3;
  const int64_t s64 = slot[row];
  // Everything below is uniform over the workgroup (it depends on the row only).
  int b0 = -1, c = 0;
  if (s64 >= 0 && s64 < n_slots) {
    b0 = base[s64];
    c = cur[s64];
  }
  if (b0 < 0 || c < 0 || b0 >= arena_states || c >= arena_states - b0) {  // off: copy the row
    if (lr == wr) return;
    copy_row(lr, wr, V, kThreads);
    return;
  }
  const int64_t t64 = tok[row];
  if (dec[row] != 0 && t64 >= 0 && t64 < V) {
    const int t = arena[size_t(b0 + c) * V + size_t(t64)];
    if (t >= 0 && t < arena_states - b0) {  // a transition that dies, or leaves the arena, lets the state stand
      __syncthreads();                      // every lane has read cur[s]
      if (threadIdx.x == 0) cur[s64] = t;
      c = t;
    }
  }
  const int16_t* tr = arena + size_t(b0 + c) * V;

  float b = -INFINITY;
  int bi = 0x7fffffff;
  if (vec) {
    const uint4* l4 = reinterpret_cast<const uint4*>(lr);
    const uint4* t4 = reinterpret_cast<const uint4*>(tr);
    uint4* w4 = reinterpret_cast<uint4*>(wr);
    // Two chunks per trip, their four loads issued before the first use.
    for (int c0 = threadIdx.x; c0 < nvec; c0 += 2 * kThreads) {
      const int c1 = c0 + kThreads;
      const bool two = c1 < nvec;
      const int c1r = two ? c1 : c0;  // past the end: chunk c0 again, in bounds; nothing is stored for it
      const uint4 lv0 = l4[c0], tv0 = t4[c0];
      const uint4 lv1 = l4[c1r], tv1 = t4[c1r];
      mask_chunk(c0, lv0, tv0, w4, b, bi);
      if (two) mask_chunk(c1, lv1, tv1, w4, b, bi);
    }
  } else {
    for (int i = threadIdx.x; i < V; i += kThreads) {
      const uint32_t o = tr[i] < 0 ? kNegInf : uint32_t(lr[i]);
      wr[i] = uint16_t(o);
      take_bits(b, bi, o, i);
    }
  }

  __shared__ float s_b[kWaves];
  __shared__ int s_i[kWaves];
  block_argmax<kWaves>(b, bi, s_b, s_i);
  if (threadIdx.x == 0) ids[row] = bi == 0x7fffffff ? 0 : bi;  // no winner (all -inf / NaN): id 0, never out of range
}

__global__ void k_guide_reset(int* __restrict__ base, int* __restrict__ cur, int first) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    *base = first;
    *cur = 0;
  }
}

}  // namespace

extern "C" {

// x, work: bf16 [B, V] (one buffer, or two that do not overlap); ids, tok: int64 [B]; dec, slot: int64 [>= B];
// base, cur: int32 [n_slots]; arena: int16 [arena_states, V]. With V % 8 == 0 x, work and arena must be 16-byte
// aligned.
int p2pt_guide(const void* x, void* work, int64_t* ids, const int64_t* tok, const int64_t* dec, const int64_t* slot,
               const int* base, int* cur, int n_slots, const void* arena, int arena_states, int B, int V,
               void* stream) {
  if (!x || !work || !ids || !tok || !dec || !slot || !base || !cur || !arena || B <= 0 || V < 32 || n_slots <= 0 ||
      arena_states <= 0)
    return int(hipErrorInvalidValue);
  if (V % 8 == 0 && !(aligned16(x) && aligned16(work) && aligned16(arena))) return int(hipErrorInvalidValue);
  hipLaunchKernelGGL(k_guide, dim3(B), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint16_t*>(x), static_cast<uint16_t*>(work), ids, tok, dec, slot, base, cur,
                     n_slots, static_cast<const int16_t*>(arena), arena_states, V);
  return int(hipGetLastError());
}

// first: the arena row the slot's table starts at, or -1 for a slot that is not guided.
int p2pt_guide_reset(int* base, int* cur, int n_slots, int slot, int first, int arena_states, void* stream) {
  if (!base || !cur || n_slots <= 0 || slot < 0 || slot >= n_slots || arena_states <= 0 || first < -1 ||
      first >= arena_states)
    return int(hipErrorInvalidValue);
  hipLaunchKernelGGL(k_guide_reset, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), base + slot, cur + slot,
                     first);
  return int(hipGetLastError());
}

}  // extern "C"
