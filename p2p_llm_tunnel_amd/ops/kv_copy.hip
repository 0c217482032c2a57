// Slot-to-slot copy of K/V cache rows for the inference endpoint's prefix
// cache (gfx950 / CDNA4): a request whose prompt begins like the rows another
// slot already holds takes those rows instead of prefilling them again.
//
//   p2pt_kv_copy   up to 8 jobs per launch; a job is "rows [0, len) of slot
//     src -> slot dst, every layer, K and V". The caches are
//     [n_layers, n_slots, max_seq, row_elems] bf16, so per (layer, job, K|V)
//     the region is ONE contiguous run of len * row_elems * 2 bytes, a
//     multiple of 16 (the launcher checks it).
//
//   The jobs travel by value in the kernel arguments: the launcher reads the
//   host triples and there is no device table, no H2D copy, no allocation and
//   no sync, so a launch can sit between two graph replays on one stream.
//
//   Grid (chunk, layer x {K, V}, job), capped near 2048 workgroups; a
//   workgroup grid-strides over its run in chunks of kThreads * kUnroll
//   16-byte words, kUnroll loads in flight per lane before the first store.
//   Lanes past the end of a run store nothing, a job with len == 0 does
//   nothing, and nothing outside the destination runs is written. src and dst
//   slots differ (checked), so a run never overlaps its source.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kMaxJobs = 8;
constexpr int kThreads = 256;
constexpr int kUnroll = 4;                     // 16-byte loads in flight per lane (written out in the kernel)
constexpr int kChunk = kThreads * kUnroll;     // 16-byte words per workgroup per stride: 16 KiB
constexpr int kMaxBlocks = 2048;               // memory-bound: ~8 workgroups per CU, grid-stride the rest

struct KvJobs {
  int src[kMaxJobs], dst[kMaxJobs], len[kMaxJobs];
};

__global__ __launch_bounds__(kThreads) void k_kv_copy(uint4* __restrict__ k_cache, uint4* __restrict__ v_cache,
                                                      int n_slots, size_t slot_words, int row_words, KvJobs jobs) {
  const int job = blockIdx.z;
  const size_t total = size_t(jobs.len[job]) * row_words;  // 16-byte words of this run
  uint4* cache = (blockIdx.y & 1) ? v_cache : k_cache;
  const size_t layer = size_t(blockIdx.y >> 1) * n_slots;
  const uint4* __restrict__ s = cache + (layer + jobs.src[job]) * slot_words;
  uint4* __restrict__ d = cache + (layer + jobs.dst[job]) * slot_words;
  for (size_t base = size_t(blockIdx.x) * kChunk; base < total; base += size_t(gridDim.x) * kChunk) {
    // Every lane loads (past the end: the run's last word again, in bounds), so
    // the loads stay unconditional and all in flight; only the stores are masked.
    const size_t i0 = base + threadIdx.x, i1 = i0 + kThreads, i2 = i1 + kThreads, i3 = i2 + kThreads;
    const size_t last = total - 1;
    const uint4 r0 = s[i0 < total ? i0 : last];
    const uint4 r1 = s[i1 < total ? i1 : last];
    const uint4 r2 = s[i2 < total ? i2 : last];
    const uint4 r3 = s[i3 < total ? i3 : last];
    if (i0 < total) d[i0] = r0;
    if (i1 < total) d[i1] = r1;
    if (i2 < total) d[i2] = r2;
    if (i3 < total) d[i3] = r3;
  }
}

}  // namespace

extern "C" {

int p2pt_max_kv_copy_jobs() { return kMaxJobs; }

// k_cache, v_cache: bf16 [n_layers, n_slots, max_seq, row_elems], 16-byte
// aligned; jobs: HOST array of n_jobs (src, dst, len) triples, read here and
// passed on by value. Every argument is checked again (the Python wrapper
// raises first): slots in range, src != dst, 0 <= len <= max_seq, rows a
// multiple of 16 bytes. Sources and destinations of one call must be disjoint
// sets and no destination may repeat (the wrapper's rule; checked here too).
int p2pt_kv_copy(void* k_cache, void* v_cache, int n_layers, int n_slots, int max_seq, int row_elems, int n_jobs,
                 const int* jobs, void* stream) {
  if (!k_cache || !v_cache || !jobs || n_layers < 1 || n_layers > 32767 || n_slots < 2 || max_seq < 1 ||
      row_elems < 8 || row_elems % 8 || n_jobs < 1 || n_jobs > kMaxJobs)
    return int(hipErrorInvalidValue);
  if ((reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache)) & 15)
    return int(hipErrorInvalidValue);
  KvJobs kj = {};
  int max_len = 0;
  for (int j = 0; j < n_jobs; j++) {
    const int src = jobs[3 * j], dst = jobs[3 * j + 1], len = jobs[3 * j + 2];
    if (src < 0 || src >= n_slots || dst < 0 || dst >= n_slots || src == dst || len < 0 || len > max_seq)
      return int(hipErrorInvalidValue);
    for (int q = 0; q < j; q++)
      if (kj.dst[q] == dst || kj.dst[q] == src || kj.src[q] == dst) return int(hipErrorInvalidValue);
    kj.src[j] = src;
    kj.dst[j] = dst;
    kj.len[j] = len;
    max_len = len > max_len ? len : max_len;
  }
  if (max_len == 0) return int(hipSuccess);  // nothing to move
  const int row_words = row_elems / 8;  // 8 bf16 per 16-byte word
  const size_t slot_words = size_t(max_seq) * row_words;
  const int yz = 2 * n_layers * n_jobs;
  const size_t chunks = (size_t(max_len) * row_words + kChunk - 1) / kChunk;
  const int cap = kMaxBlocks / yz > 0 ? kMaxBlocks / yz : 1;
  const int gx = int(chunks < size_t(cap) ? chunks : size_t(cap));
  hipLaunchKernelGGL(k_kv_copy, dim3(gx, 2 * n_layers, n_jobs), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), static_cast<uint4*>(k_cache), static_cast<uint4*>(v_cache),
                     n_slots, slot_words, row_words, kj);
  return int(hipGetLastError());
}

}  // extern "C"
