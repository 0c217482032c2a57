// Helpers shared by the kernels that run one workgroup per row of bf16 logits
// (k_sample, k_logprobs, k_penalize, k_guide, k_argmax): block reductions over
// a caller's LDS array, the radix-select bucket scan, 8 x bf16 bit patterns in
// and out of a uint4, the off-row copy, and the row argmax with its one rule:
// lowest id on ties, NaN never wins, ascending index within a lane, and
// 0x7fffffff left in thread 0 when the row has no winner (each kernel turns
// that into its own answer: id 0, or ids[row] left alone).
#pragma once
#include "bf16_common.h"

namespace p2pt_gpu {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Max / sum over a workgroup of WAVES waves through red[WAVES]; every thread gets the result. The leading
// barrier lets a caller use `red` again right after an earlier call.
template <int WAVES>
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; w++) m = fmaxf(m, red[w]);
  return m;
}

template <int WAVES>
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < WAVES; w++) s += red[w];
  return s;
}

// Among 256 buckets (descending digit order), the digit where the running sum from the top first reaches
// `need`: *digit = that digit, *above = the sum of the buckets above it, *total (unless null) = the sum of all
// buckets. One wave: lane j holds digits 255-4j .. 252-4j.
template <class T>
__device__ __forceinline__ void find_bucket(const T* hist, T need, uint32_t* digit, T* above, T* total) {
  const int lane = threadIdx.x & 63;
  T v[4], s = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    v[q] = hist[255 - 4 * lane - q];
    s += v[q];
  }
  T incl = s;  // inclusive prefix over lanes
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    T o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  const T excl = incl - s;
  const bool hit = excl < need && incl >= need;
  const uint64_t b = __ballot(hit);
  // No hit: the integer select always has one where its result is used (need <= the level's total: k < V in
  // k_sample; k_logprobs reads *total and, where its narrowed first scan holds fewer than N, scans the whole row
  // again). The float select can miss when the totals, re-accumulated at this level by unordered atomics, fall
  // short of the `need` carried down, i.e. when p * Z lies within rounding of the enclosing bucket's end. Lane 63
  // then takes digit 0 (q == 3 below) with everything else above it, and so on down: the cut ends at the bottom
  // of the enclosing bucket's key range. No key lies between that and the bucket's lowest token, so the kept set
  // is the bucket and all above it, whose mass is `need` to within those roundings: the cut an exact sum could
  // have chosen. At the first level the same reasoning keeps everything (p * Z within rounding of Z).
  const int first = b ? __ffsll((unsigned long long)b) - 1 : 63;
  if (lane == first) {
    T run = excl;
    uint32_t dg = 255 - 4 * lane - 3;
    T ab = run;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (run + v[q] >= need || q == 3) {
        dg = 255 - 4 * lane - q;
        ab = run;
        break;
      }
      run += v[q];
    }
    *digit = dg;
    *above = ab;
  }
  if (total && lane == 63) *total = incl;
}

// The eight bf16 bit patterns of a 16-byte vector, and back.
__device__ __forceinline__ void bits8(const uint4& v, uint32_t (&h)[8]) {
  h[0] = v.x & 0xffffu; h[1] = v.x >> 16;
  h[2] = v.y & 0xffffu; h[3] = v.y >> 16;
  h[4] = v.z & 0xffffu; h[5] = v.z >> 16;
  h[6] = v.w & 0xffffu; h[7] = v.w >> 16;
}
__device__ __forceinline__ uint4 pack_bits8(const uint32_t (&o)[8]) {
  return make_uint4(o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16));
}

// A lane's argmax step on a bf16 bit pattern. Strict: with ascending i within a lane the first of equals stays,
// and neither NaN nor -inf replaces the initial (-inf, 0x7fffffff).
__device__ __forceinline__ void take_bits(float& b, int& bi, uint32_t bits, int i) {
  const float v = bf2f(uint16_t(bits));
  if (v > b) {
    b = v;
    bi = i;
  }
}

// work row = logits row, bit for bit, by a workgroup of `threads`: 16-byte vectors when V % 8 == 0 (the caller's
// launcher has checked the alignment), element by element otherwise.
__device__ __forceinline__ void copy_row(const uint16_t* lr, uint16_t* wr, int V, int threads) {
  if ((V & 7) == 0) {
    const uint4* l4 = reinterpret_cast<const uint4*>(lr);
    uint4* w4 = reinterpret_cast<uint4*>(wr);
    for (int c = threadIdx.x; c < (V >> 3); c += threads) w4[c] = l4[c];
  } else {
    for (int i = threadIdx.x; i < V; i += threads) wr[i] = lr[i];
  }
}

// Every lane's (b, bi) -> the workgroup's winner in thread 0 (other threads hold their wave's), through
// s_b[WAVES] and s_i[WAVES]. bi == 0x7fffffff there: no element of the row is above -inf.
template <int WAVES>
__device__ __forceinline__ void block_argmax(float& b, int& bi, float* s_b, int* s_i) {
  wave_argmax(b, bi);
  if ((threadIdx.x & 63) == 0) {
    s_b[threadIdx.x >> 6] = b;
    s_i[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < WAVES; w++) am_take(b, bi, s_b[w], s_i[w]);
  }
}

}  // namespace p2pt_gpu
