// Token log-probabilities for the on-node inference endpoint (gfx950 / CDNA4):
// the chosen token's logprob and the top N (token, logprob) pairs of a bf16
// logits row, on device, inside the captured decode step.
//
//   p2pt_logprobs   one 1024-thread workgroup (16 waves of 64) per row:
//     z_i = float(logit_i);  lse = m + log(sum_i exp(z_i - m)),  m = max_i z_i
//     logprob_i = z_i - lse                                (fp32, precise expf / logf)
//   The distribution is the model's own softmax(logits): it does not depend on
//   temperature, top-k or top-p (vLLM's default too), so the sampler's
//   parameters are no input here.
//
//   Top N = the first N elements ordered by (bf16 value descending, id
//   ascending). Ties are the normal case (8 mantissa bits), so the selection is
//   deterministic by construction: the N-th largest 16-bit order-preserving key
//   by radix select (2 passes of 8 bits, LDS histograms; the first pass counts
//   only keys within two high-byte buckets of the maximum and is redone over
//   the whole row if those hold fewer than N), then every element above that
//   key, then elements equal to it in ascending id order (a block scan over
//   consecutive 8192-element chunks) until there are N. The at most 20 results
//   are ranked in LDS. Atomics build the histograms and hand out LDS slots to
//   the elements above the key; the ranking then orders them, so no atomic
//   decides which ids are returned or in what order.
//
//   Rows with want == 0 return before touching memory. -inf logits give -inf
//   logprobs (never NaN); -0 orders as +0. The block reductions, the radix
//   select's bucket scan (find_bucket) and the uint4 unpack are row_common.h's.
#include "row_common.h"

namespace {

using namespace p2pt_gpu;

constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr int kMaxTop = 20;           // out_ids columns; out_lp has kMaxTop + 1
constexpr int kChunk = kThreads * 8;  // elements per block-wide step: 8 consecutive per thread

// Order-preserving 16-bit key of a bf16 bit pattern (-0 canonicalised to +0), and back.
__device__ __forceinline__ uint32_t okey16(uint32_t b) {
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
}
__device__ __forceinline__ float key_value(uint32_t key) {
  return bf2f(uint16_t((key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu)));
}

// Elements i .. i+7 of the row as bf16 bit patterns; returns how many lie inside the row (i < V).
__device__ __forceinline__ int load8(const uint16_t* __restrict__ lr, int i, int V, bool aligned, uint32_t (&h)[8]) {
  if (aligned && i + 8 <= V) {
    bits8(*reinterpret_cast<const uint4*>(lr + i), h);
    return 8;
  }
  const int n = V - i < 8 ? V - i : 8;
#pragma unroll
  for (int e = 0; e < 8; e++) h[e] = e < n ? uint32_t(lr[i + e]) : 0u;
  return n;
}

__global__ __launch_bounds__(kThreads) void k_logprobs(const uint16_t* __restrict__ logits,
                                                       const int64_t* __restrict__ ids,
                                                       const int64_t* __restrict__ want, float* __restrict__ out_lp,
                                                       int32_t* __restrict__ out_ids, int V) {
  const int row = blockIdx.x;
  const int64_t w = want[row];
  if (w <= 0) return;  // row is off: its outputs keep whatever they held
  const int N = int(w - 1 < kMaxTop ? w - 1 : kMaxTop);
  const uint16_t* lr = logits + size_t(row) * V;
  const bool aligned = (reinterpret_cast<uintptr_t>(lr) & 15) == 0;
  const int tid = threadIdx.x;

  __shared__ float red[kWaves];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_find[3];
  __shared__ uint32_t s_wtot[kWaves];
  __shared__ uint32_t s_cnt;
  __shared__ uint32_t s_key[kMaxTop];
  __shared__ int s_id[kMaxTop];

  uint32_t h[8];

  // ---- pass 1: the row maximum
  float m = -INFINITY;
  for (int i = tid * 8; i < V; i += kChunk) {
    const int n = load8(lr, i, V, aligned, h);
#pragma unroll
    for (int e = 0; e < 8; e++)
      if (e < n) m = fmaxf(m, bf2f(uint16_t(h[e])));
  }
  m = block_max<kWaves>(m, red);
  const float mm = m == -INFINITY ? 0.f : m;  // an all -inf row: exp(-inf - 0) = 0, lse = -inf

  // ---- pass 2: sum of exp(z - m), and the histogram of the keys' high bytes
  const uint32_t kmax = okey16(f2bf_bits(m));
  uint32_t lo = (kmax & 0xFF00u) >= 0x100u ? (kmax & 0xFF00u) - 0x100u : 0u;  // count keys >= lo only
  uint32_t d1 = 0, above = 0;
  float s = 0.f;
  for (int attempt = 0;; attempt++) {
    for (int d = tid; d < 256; d += kThreads) hist[d] = 0;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (int i = tid * 8; i < V; i += kChunk) {
      const int n = load8(lr, i, V, aligned, h);
#pragma unroll
      for (int e = 0; e < 8; e++) {
        if (e >= n) continue;
        if (attempt == 0) s += expf(bf2f(uint16_t(h[e])) - mm);
        const uint32_t key = okey16(h[e]);
        if (N > 0 && key >= lo) atomicAdd(&hist[key >> 8], 1u);
      }
    }
    __syncthreads();
    if (N == 0) break;
    if (tid < 64) find_bucket<uint32_t>(hist, uint32_t(N), &s_find[0], &s_find[1], &s_find[2]);
    __syncthreads();
    d1 = s_find[0];
    above = s_find[1];
    if (s_find[2] >= uint32_t(N) || lo == 0) break;  // V >= 32 > N: the whole row always holds N
    lo = 0;
    __syncthreads();
  }
  const float lse = mm + logf(block_sum<kWaves>(s, red));

  if (tid == 0) {  // the chosen token: wherever it ranks
    const int64_t c = ids[row];
    float lp = __uint_as_float(0x7FC00000u);  // an id outside the row: NaN
    if (c >= 0 && c < V) {
      const float z = bf2f(lr[c]);
      lp = z == -INFINITY ? -INFINITY : z - lse;
    }
    out_lp[size_t(row) * (kMaxTop + 1)] = lp;
  }
  if (N == 0) return;

  // ---- pass 3: the low byte of the N-th largest key, among keys with high byte d1
  for (int d = tid; d < 256; d += kThreads) hist[d] = 0;
  __syncthreads();
  for (int i = tid * 8; i < V; i += kChunk) {
    const int n = load8(lr, i, V, aligned, h);
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const uint32_t key = okey16(h[e]);
      if (e < n && (key >> 8) == d1) atomicAdd(&hist[key & 0xFFu], 1u);
    }
  }
  __syncthreads();
  if (tid < 64) find_bucket<uint32_t>(hist, uint32_t(N) - above, &s_find[0], &s_find[1], &s_find[2]);
  __syncthreads();
  const uint32_t kth = (d1 << 8) | s_find[0];
  const uint32_t n_above = above + s_find[1];          // keys > kth: all taken, < N of them
  const uint32_t need_eq = uint32_t(N) - n_above;      // keys == kth: the lowest ids, >= 1 of them

  // ---- pass 4: gather. Keys above kth take LDS slots [0, n_above) in any order
  // (ranked below); keys equal to kth take slots n_above.. in ascending id order.
  uint32_t eq_taken = 0;  // the same in every thread
  const int lane = tid & 63, wave = tid >> 6;
  for (int base = 0; base < V; base += kChunk) {
    const int i = base + tid * 8;
    uint32_t eqmask = 0, c = 0;
    if (i < V) {
      const int n = load8(lr, i, V, aligned, h);
#pragma unroll
      for (int e = 0; e < 8; e++) {
        if (e >= n) continue;
        const uint32_t key = okey16(h[e]);
        if (key > kth) {
          const uint32_t slot = atomicAdd(&s_cnt, 1u);
          if (slot < uint32_t(kMaxTop)) {
            s_key[slot] = key;
            s_id[slot] = i + e;
          }
        } else if (key == kth) {
          eqmask |= 1u << e;
          c++;
        }
      }
    }
    if (eq_taken < need_eq) {  // block-uniform
      uint32_t incl = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
      }
      if (lane == 63) s_wtot[wave] = incl;
      __syncthreads();
      uint32_t before = 0, total = 0;
#pragma unroll
      for (int q = 0; q < kWaves; q++) {
        const uint32_t t = s_wtot[q];
        if (q < wave) before += t;
        total += t;
      }
      uint32_t rank = eq_taken + before + incl - c;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        if (!(eqmask & (1u << e))) continue;
        if (rank < need_eq) {
          s_key[n_above + rank] = kth;
          s_id[n_above + rank] = i + e;
        }
        rank++;
      }
      eq_taken += total;
      __syncthreads();
    }
  }
  __syncthreads();

  // ---- rank the N entries by (key descending, id ascending) and write them out
  if (tid < N) {
    const uint32_t key = s_key[tid];
    const int id = s_id[tid];
    int rank = 0;
    for (int j = 0; j < N; j++) rank += (s_key[j] > key || (s_key[j] == key && s_id[j] < id)) ? 1 : 0;
    const float z = key_value(key);
    out_lp[size_t(row) * (kMaxTop + 1) + 1 + rank] = z == -INFINITY ? -INFINITY : z - lse;
    out_ids[size_t(row) * kMaxTop + rank] = id;
  }
}

}  // namespace

extern "C" {

// logits: bf16 [B, V], rows contiguous; ids: int64 [B], the chosen ids (after
// the sampler); want: int64 [>= B], per row 0 = off, 1 + N = the chosen token
// and the top N (N in 0..20; larger values count as 20); out_lp: float32
// [B, 21], column 0 the chosen token's logprob, columns 1..N the top N in
// descending order; out_ids: int32 [B, 20], their ids. Columns past N and rows
// that are off are left as they were.
int p2pt_logprobs(const void* logits, const int64_t* ids, const int64_t* want, float* out_lp, int32_t* out_ids, int B,
                  int V, void* stream) {
  if (B < 1 || V < 32 || V > (1 << 30)) return int(hipErrorInvalidValue);
  hipLaunchKernelGGL(k_logprobs, dim3(B), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint16_t*>(logits), ids, want, out_lp, out_ids, V);
  return int(hipGetLastError());
}

}  // extern "C"
