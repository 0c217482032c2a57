// Pooling of the fused step's final residual into sentence embeddings for the
// inference endpoint's embedding routes (gfx950 / CDNA4).
//
//   p2pt_embed_pool   up to 16 jobs per launch, one workgroup each. A job is
//     (row0, n, acc, flags, out_row): rows [row0, row0 + n) of resid (bf16
//     [rows <= 64, dim], what the last layer's down projection left) are
//     normalised with the final-norm weight g and added, in fp32 and in row
//     order, to the running sum a of one sequence:
//
//       inv_r = rsqrt(sum_c x_rc^2 / dim + eps)      (from the bf16 row itself)
//       a_c  += (x_rc * inv_r) * g_c                 r ascending, one add per row
//
//     flags bit 0 ("first piece"): a starts at zero, acc_buf is not read;
//     otherwise a starts at acc_buf[acc]. flags bit 1 ("last piece"):
//     out[out_row] = a / sqrt(sum_c a_c^2) (zeros when that norm is 0 or not
//     finite) and acc_buf is not written; otherwise acc_buf[acc] = a. Each
//     column belongs to one lane, so the chain of additions of a sequence is the
//     same however its rows are split over launches (bit-identical results), and
//     every reduction has a fixed order (reruns are bit-identical too).
//
//   A row whose fp32 sum of squares overflows (|x| around 1e19 and up) is
//   measured again on x * 2^-96, an exact scaling, so every finite bf16 row
//   gets its true 1/rms.
//
//   The jobs travel by value in the kernel arguments, as kv_copy.hip's do: no
//   device table, no H2D copy, no allocation and no sync, so a launch can sit
//   between two graph replays on one stream. Nothing outside acc_buf[acc] of
//   the jobs without "last" and out[out_row] of the jobs with it is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16_common.h"

// "One fp32 add per row": keep the multiply and the add apart.
#pragma clang fp contract(off)

namespace {

using namespace p2pt_gpu;

constexpr int kMaxJobs = 16;
constexpr int kMaxRows = 64;  // rows of resid (decode_fused.hip's kMaxM)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxDim = 16384;
// Rescue scaling of a row whose sum of squares overflows: 16384 * (2^128 * 2^-96)^2 = 2^78 fits.
constexpr float kDown = 0x1p-96f;

struct EmbedJobs {
  int row0[kMaxJobs], n[kMaxJobs], acc[kMaxJobs], flags[kMaxJobs], out_row[kMaxJobs];
};

__device__ __forceinline__ void load8(const float* p, float* a) {
  const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
  a[0] = lo.x; a[1] = lo.y; a[2] = lo.z; a[3] = lo.w;
  a[4] = hi.x; a[5] = hi.y; a[6] = hi.z; a[7] = hi.w;
}
__device__ __forceinline__ void store8(float* p, const float* a) {
  *reinterpret_cast<float4*>(p) = make_float4(a[0], a[1], a[2], a[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(a[4], a[5], a[6], a[7]);
}

// Sum over one bf16 row of (x * scale)^2: lane-strided 16-byte chunks, then the wave.
__device__ __forceinline__ float row_sumsq(const uint4* __restrict__ x, int words, float scale) {
  float ss = 0.f;
  for (int i = threadIdx.x % kWave; i < words; i += kWave) {
    float f[8];
    unpack8(x[i], f);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const float v = f[k] * scale;
      ss += v * v;
    }
  }
  return wave_sum(ss);
}

__global__ __launch_bounds__(kThreads) void k_embed_pool(const uint4* __restrict__ resid, const uint4* __restrict__ g,
                                                         float* __restrict__ acc_buf, float* __restrict__ out, int dim,
                                                         float eps, EmbedJobs jobs) {
  __shared__ float s_inv[kMaxRows], s_scale[kMaxRows], s_part[kWaves];
  const int job = blockIdx.x, words = dim / 8;
  const int n = jobs.n[job], flags = jobs.flags[job];
  const uint4* __restrict__ x0 = resid + size_t(jobs.row0[job]) * words;
  const int wave = threadIdx.x / kWave;

  // 1/rms of each row of the job, one wave per row.
  for (int r = wave; r < n; r += kWaves) {
    const uint4* __restrict__ x = x0 + size_t(r) * words;
    float scale = 1.f;
    float ss = row_sumsq(x, words, scale);
    if (!(ss <= 3.402823466e38f)) {  // overflowed (wave-uniform): measure x * 2^-96; eps vanishes next to it
      scale = kDown;
      ss = row_sumsq(x, words, scale);
    }
    if (threadIdx.x % kWave == 0) {
      s_inv[r] = rsqrtf(ss / float(dim) + (scale == 1.f ? eps : 0.f));
      s_scale[r] = scale;
    }
  }
  __syncthreads();

  const bool first = flags & 1, last = flags & 2;
  float* dst = last ? out + size_t(jobs.out_row[job]) * dim : acc_buf + size_t(jobs.acc[job]) * dim;
  const float* src = acc_buf + size_t(jobs.acc[job]) * dim;
  float part = 0.f;
  for (int i = threadIdx.x; i < words; i += kThreads) {  // this lane's columns [8 i, 8 i + 8)
    float a[8], gw[8];
    if (first) {
#pragma unroll
      for (int k = 0; k < 8; k++) a[k] = 0.f;
    } else {
      load8(src + 8 * i, a);
    }
    unpack8(g[i], gw);
#pragma unroll 4
    for (int r = 0; r < n; r++) {
      float f[8];
      unpack8(x0[size_t(r) * words + i], f);
      const float inv = s_inv[r], scale = s_scale[r];
#pragma unroll
      for (int k = 0; k < 8; k++) a[k] += ((f[k] * scale) * inv) * gw[k];
    }
    store8(dst + 8 * i, a);  // "last": unnormalised for now; this lane reads it back below
    if (last) {
#pragma unroll
      for (int k = 0; k < 8; k++) part += a[k] * a[k];
    }
  }
  if (!last) return;  // uniform over the workgroup

  part = wave_sum(part);
  if (threadIdx.x % kWave == 0) s_part[wave] = part;
  __syncthreads();
  float total = s_part[0];
#pragma unroll
  for (int w = 1; w < kWaves; w++) total += s_part[w];
  const bool ok = total > 0.f && total <= 3.402823466e38f;
  const float norm = sqrtf(total);
  for (int i = threadIdx.x; i < words; i += kThreads) {
    float a[8];
    load8(dst + 8 * i, a);
#pragma unroll
    for (int k = 0; k < 8; k++) a[k] = ok ? a[k] / norm : 0.f;
    store8(dst + 8 * i, a);
  }
}

}  // namespace

extern "C" {

int p2pt_max_embed_jobs() { return kMaxJobs; }

// resid: bf16 [rows, dim]; g: bf16 [dim]; acc_buf: fp32 [n_acc, dim]; out: fp32
// [n_out, dim]; all 16-byte aligned. jobs: HOST array of n_jobs (row0, n, acc,
// flags, out_row) quintuples, read here and passed on by value. Every argument
// is checked again (the Python wrapper raises first).
int p2pt_embed_pool(const void* resid, int rows, int dim, const void* g, void* acc_buf, int n_acc, void* out,
                    int n_out, float eps, int n_jobs, const int* jobs, void* stream) {
  if (!resid || !g || !acc_buf || !out || !jobs || rows < 1 || rows > kMaxRows || dim < 8 || dim % 8 ||
      dim > kMaxDim || n_acc < 1 || n_out < 1 || n_jobs < 1 || n_jobs > kMaxJobs || !(eps >= 0.f))
    return int(hipErrorInvalidValue);
  if ((reinterpret_cast<uintptr_t>(resid) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(acc_buf) |
       reinterpret_cast<uintptr_t>(out)) & 15)
    return int(hipErrorInvalidValue);
  EmbedJobs ej = {};
  for (int j = 0; j < n_jobs; j++) {
    const int row0 = jobs[5 * j], n = jobs[5 * j + 1], acc = jobs[5 * j + 2], flags = jobs[5 * j + 3],
              out_row = jobs[5 * j + 4];
    if (row0 < 0 || n < 1 || n > rows || row0 > rows - n || acc < 0 || acc >= n_acc || flags < 0 || flags > 3)
      return int(hipErrorInvalidValue);
    if ((flags & 2) ? (out_row < 0 || out_row >= n_out) : out_row != -1) return int(hipErrorInvalidValue);
    for (int q = 0; q < j; q++)
      if (ej.acc[q] == acc || ((flags & 2) && (ej.flags[q] & 2) && ej.out_row[q] == out_row))
        return int(hipErrorInvalidValue);
    ej.row0[j] = row0;
    ej.n[j] = n;
    ej.acc[j] = acc;
    ej.flags[j] = flags;
    ej.out_row[j] = out_row;
  }
  hipLaunchKernelGGL(k_embed_pool, dim3(n_jobs), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint4*>(resid), static_cast<const uint4*>(g), static_cast<float*>(acc_buf),
                     static_cast<float*>(out), dim, eps, ej);
  return int(hipGetLastError());
}

}  // extern "C"
