// Stochastic sampling for the on-node inference endpoint (gfx950 / CDNA4):
// temperature, top-k and top-p (nucleus) over a bf16 logits row, on device,
// inside the captured decode step.
//
//   p2pt_sample   one 1024-thread workgroup (16 waves of 64) per row:
//     z_i = logit_i / T                                   (fp32)
//     top-k: the k-th largest z by radix select on order-preserving keys
//            (4 passes of 8 bits, LDS histograms)         -> keep z >= z_(k)
//     top-p: the smallest set of the largest kept z whose softmax mass
//            reaches p, by the same radix select over mass (LDS fp32
//            histograms of exp(z - max))                  -> keep z >= z_(p)
//     draw:  Gumbel-max over the kept set: argmax_i z_i - log(-log u_i), u_i
//            from a counter-based hash of (seed, counter, i), i.e. an exact
//            draw from softmax(z) restricted to the kept set (HF / vLLM
//            order: temperature, then top-k, then top-p; ties at a cut are
//            kept, as HF's `logits < kth` filter does).
//   Rows with T <= 0 keep the greedy id already in `ids` (the fused LM head's
//   argmax): greedy decoding stays bit-exact and costs one early-exit wave.
//
// params: int64 [5, ld] — float32 bits of T, top_k (<= 0: off), float32 bits
// of top_p (>= 1: off), seed, counter (the request's token index, so each
// draw of a request uses fresh noise and a fixed seed replays the same text).
//
//   p2pt_sample_minp   the same kernel's MINP instantiation, params int64
//     [6, ld]: row 5 holds the float32 bits of ln(min_p), computed on the host
//     in fp64 and rounded once (-inf: off), so the device takes no
//     transcendental at this cut:
//     min_p: t = m + ln(min_p), one fp32 add on the block maximum m of z that
//            the kernel already holds                     -> keep z >= t
//     (a token whose z equals t is kept, as at the other cuts). The final cut
//     is max(top-k, top-p, min_p): HF's order, temperature, top-k, top-p, then
//     min_p. p_i / p_max = exp(z_i - m) does not depend on the set the softmax
//     is normalised over, so after top-k and top-p the min_p filter is exactly
//     this threshold; the top-p mass is taken over the top-k set as without
//     min_p, not narrowed by it. One add and one key per row: no pass over the
//     logits and no LDS beyond p2pt_sample's. p2pt_sample launches the
//     MINP = false instantiation, whose code the flag does not touch.
// The block reductions, the radix select's bucket scan (find_bucket) and the
// argmax tail of the draw are row_common.h's.
#include "row_common.h"

namespace {

using namespace p2pt_gpu;

constexpr int kThreads = 1024, kWaves = kThreads / 64;

__device__ __forceinline__ uint32_t okey(float f) {  // order-preserving float -> uint32
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // SplitMix64 finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Gumbel(0, 1) noise for element i of draw (seed, ctr). In double: the
// winners of a Gumbel-max come from u near 1, where -log(u) ~ 1 - u is tiny
// and the fast single-precision log's absolute error is of its own size (a
// measurable bias in the 12,800-draw chi-square test).
__device__ __forceinline__ float gumbel(uint64_t seed, uint64_t ctr, uint32_t i) {
  uint64_t h = mix64(seed + mix64(ctr * 0x9E3779B97F4A7C15ull + i + 1));
  double u = (double(h >> 11) + 0.5) * (1.0 / 9007199254740992.0);  // (0, 1), 53 bits
  return float(-log(-log(u)));
}

template <bool MINP>
__global__ __launch_bounds__(kThreads) void k_sample(const uint16_t* __restrict__ logits, int64_t* __restrict__ ids,
                                                     const int64_t* __restrict__ params, int ld, int V) {
  const int row = blockIdx.x;
  const int B = ld;  // params rows are `ld` long (a view of the engine's staging block)
  const float T = __uint_as_float(uint32_t(params[row]));
  if (!(T >= 1e-4f)) return;  // greedy row (or T -> 0, whose limit is greedy): the fused argmax stands
  int64_t k = params[B + row];
  float p = __uint_as_float(uint32_t(params[2 * B + row]));
  const uint64_t seed = uint64_t(params[3 * B + row]), ctr = uint64_t(params[4 * B + row]);
  if (k <= 0 || k > V) k = V;
  if (!(p > 0.f && p < 1.f)) p = 1.f;
  const float invT = 1.0f / T;
  const uint16_t* lr = logits + size_t(row) * V;

  __shared__ float red[kWaves];
  __shared__ uint32_t hist_u[256];
  __shared__ float hist_f[256];
  __shared__ uint32_t s_digit;
  __shared__ uint32_t s_above_u;
  __shared__ float s_above_f;
  __shared__ float s_best[kWaves];
  __shared__ int s_bi[kWaves];

  float m = -INFINITY;
  for (int i = threadIdx.x; i < V; i += kThreads) m = fmaxf(m, bf2f(lr[i]) * invT);
  m = block_max<kWaves>(m, red);

  // ---- top-k: the k-th largest key
  uint32_t kth = 0;  // keep key >= kth (0: everything)
  if (k < V) {
    uint32_t prefix = 0, mask = 0, need = uint32_t(k);
    for (int shift = 24; shift >= 0; shift -= 8) {
      for (int d = threadIdx.x; d < 256; d += kThreads) hist_u[d] = 0;
      __syncthreads();
      for (int i = threadIdx.x; i < V; i += kThreads) {
        const uint32_t key = okey(bf2f(lr[i]) * invT);
        if ((key & mask) == prefix) atomicAdd(&hist_u[(key >> shift) & 0xFF], 1u);
      }
      __syncthreads();
      if (threadIdx.x < 64) find_bucket<uint32_t>(hist_u, need, &s_digit, &s_above_u, nullptr);
      __syncthreads();
      need -= s_above_u;
      prefix |= s_digit << shift;
      mask |= 0xFFu << shift;
      __syncthreads();
    }
    kth = prefix;
  }

  // ---- top-p over the kept set: mass radix select
  uint32_t pth = 0;
  if (p < 1.f) {
    float z = 0.f;
    for (int i = threadIdx.x; i < V; i += kThreads) {
      const float zi = bf2f(lr[i]) * invT;
      if (okey(zi) >= kth) z += __expf(zi - m);
    }
    float need = p * block_sum<kWaves>(z, red);
    uint32_t prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
      for (int d = threadIdx.x; d < 256; d += kThreads) hist_f[d] = 0.f;
      __syncthreads();
      for (int i = threadIdx.x; i < V; i += kThreads) {
        const float zi = bf2f(lr[i]) * invT;
        const uint32_t key = okey(zi);
        if (key >= kth && (key & mask) == prefix) atomicAdd(&hist_f[(key >> shift) & 0xFF], __expf(zi - m));
      }
      __syncthreads();
      if (threadIdx.x < 64) find_bucket<float>(hist_f, need, &s_digit, &s_above_f, nullptr);
      __syncthreads();
      need -= s_above_f;
      prefix |= s_digit << shift;
      mask |= 0xFFu << shift;
      __syncthreads();
    }
    pth = prefix;
  }
  uint32_t cut = kth > pth ? kth : pth;
  if constexpr (MINP) {
    const float lnp = __uint_as_float(uint32_t(params[5 * B + row]));
    if (lnp != -INFINITY) {  // -inf: off (the cut stays what it is without min_p)
      const uint32_t mth = okey(m + lnp);
      cut = cut > mth ? cut : mth;
    }
  }

  // ---- Gumbel-max over the kept set
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < V; i += kThreads) {
    const float zi = bf2f(lr[i]) * invT;
    if (okey(zi) < cut) continue;
    am_take(best, bi, zi + gumbel(seed, ctr, uint32_t(i)), i);
  }
  block_argmax<kWaves>(best, bi, s_best, s_bi);
  if (threadIdx.x == 0 && bi != 0x7fffffff) ids[row] = bi;  // no winner: the greedy id stands
}

}  // namespace

extern "C" {

// ids: int64 [B] (in: greedy ids; out: samples for rows with T > 0);
// params: int64 [5, ld] (ld >= B, row k of parameter p at params[p * ld + k]);
// logits: bf16 [B, V] rows contiguous.
int p2pt_sample(const void* logits, int64_t* ids, const int64_t* params, int B, int ld, int V, void* stream) {
  if (B <= 0 || V <= 0 || ld < B) return int(hipErrorInvalidValue);
  hipLaunchKernelGGL(k_sample<false>, dim3(B), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint16_t*>(logits), ids, params, ld, V);
  return int(hipGetLastError());
}

// As p2pt_sample with params: int64 [6, ld], whose row 5 holds the float32 bits of ln(min_p) (-inf: off).
int p2pt_sample_minp(const void* logits, int64_t* ids, const int64_t* params, int B, int ld, int V, void* stream) {
  if (B <= 0 || V <= 0 || ld < B) return int(hipErrorInvalidValue);
  hipLaunchKernelGGL(k_sample<true>, dim3(B), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint16_t*>(logits), ids, params, ld, V);
  return int(hipGetLastError());
}

}  // extern "C"
