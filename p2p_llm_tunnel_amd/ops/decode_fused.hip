// Host side of the fused Llama decode step for gfx950 (CDNA4 / MI355X): which
// kernel variant runs on which grid (plan_step, a pure function), the
// workspace, the set of kernel instantiations (lists and one predicate), the
// lookups and launches that follow a plan into that set, and the C entry
// points. The kernels and the design notes are in decode_fused_kernels.h.
#include "decode_fused_kernels.h"

#include <type_traits>
#include <utility>

namespace {

struct LlamaDims {
  int vocab, dim, n_layers, H, Hkv, D, ffn, max_seq, max_batch;
  float eps, theta;
  // The KV cache holds OCP e4m3fn bytes (scale 1, or per-head scales: KvScales) instead of bf16: the _KV8 epilogues and k_attn<D, G, true>. It sits
  // ahead of the three family flags, whose order (qkv_bias last) the plan tests of those families pin.
  int kv_fp8;  // per-head scales, where a model has them, travel beside the plans (KvScales), not here
  int rope_table;  // RoPE frequencies from an fp32 table [D/2] (llama3 / linear scaling): the table's inv_freq entry
  int qk_norm;  // per-head RMSNorm on q and k before RoPE (Qwen3): a sixth kernel per layer
  int qkv_bias;  // a bias on the q, k and v projections (Qwen2): added in the QKV GEMM's epilogue
};

constexpr int kTnResid = 1, kTnStore = 2;  // LM head: two 16-column subtiles per block
constexpr int kCUs = 256;  // MI355X compute units: K-parts tiling aims at one workgroup per CU
constexpr int kMaxKpl = 2;  // at most 4 K parts: 4-column subtiles

// ------------------------------------------------------------ the plan
// Everything a launch depends on besides pointers, as plain ints (mirrored with
// ctypes in ops/__init__.py). A consumer's ss_in is its producer's grid_x.
struct GemmPlan {
  int epi, nw, tn, um, kpl;  // k_skinny<nw, tn, epi, um>, 1 << kpl K parts
  int grid_x, grid_y;
  int ss_in;  // sum-of-squares partials read (0: no norm)
  int M, N, K;
};
struct AttnPlan {
  int D, G;    // k_attn<D, G>
  int slots;   // gridDim.x
  int stride;  // partial slots per head in part_o / part_ml (k_attn's nsplit)
  int grid_y;
};
struct StepPlan {
  int rows, emit_rows;
  GemmPlan qkv_first, qkv, o, gate_up, down, lm_head;  // qkv_first: layer 0 reads k_embed's one partial
  AttnPlan attn;
  int am_parts;  // per-row winners k_argmax_merge reads
  int qk_norm_grid;  // k_qknorm_rope's gridDim.x (gridDim.y: rows); 0: not launched
  int qk_norm_table;  // k_qknorm_rope<D, true>: frequencies from the table (a QK-norm model with scaled RoPE)
};
// The FP8-cache choices of a step, beside StepPlan (whose layout the plan tests of earlier families pin int for
// int): which k_attn and which k_qknorm_rope variant run. The _KV8 epilogue is StepPlan's own qkv.epi.
struct KvPlan {
  int attn_kv8;     // k_attn<D, G, true>: the cache is e4m3
  int qk_norm_kv8;  // k_qknorm_rope<D, TAB, true>: k and v appended as e4m3 (a QK-norm model with an FP8 cache)
};
KvPlan plan_kv(const LlamaDims& d) { return {d.kv_fp8, d.qk_norm ? d.kv_fp8 : 0}; }
// The weight format of a step, beside StepPlan for the same reason. It is no field of LlamaDims either (whose
// layout is pinned too): it travels as an argument of its own through the _w entry points. StepPlan does not
// depend on it: FP8 weights change no grid, wave count, load batch or K part.
struct WeightPlan {
  int w8;  // k_skinny<.., 1>: the five GEMM weights are e4m3 bytes with an fp32 scale per output row
};
bool weights_ok(const WeightPlan& w) { return w.w8 == 0 || w.w8 == 1; }
// The weight formats of a step, beside the plans as WeightPlan is, and what the step itself follows: WeightPlan's one
// field (pinned by tests, as is its refusal of w8 = 2) cannot say that the layers and the LM head differ, so the _fmt
// entry points take this and the WeightPlan ones are the same call with {w8, w8}. 0 bf16, 1 FP8 (e4m3 bytes, an fp32
// scale per output row), 2 MXFP4 (OCP Microscaling: e2m1 nibbles, an e8m0 scale byte per 32-element block). MXFP4
// is a format of the four layer GEMMs only, and its LM head is FP8 (docs/WEIGHT_MXFP4.md). StepPlan does not depend
// on it: no format changes a grid, wave count, load batch or K part.
struct WeightFormat {
  int layers;   // wqkv, wo, w_gate_up, w_down: k_skinny<.., layers>
  int lm_head;  // k_skinny<.., EPI_ARGMAX, .., lm_head>
};
bool format_ok(const WeightFormat& f) {
  return (f.layers == 0 && f.lm_head == 0) || (f.layers == 1 && f.lm_head == 1) || (f.layers == 2 && f.lm_head == 1);
}
// The scales of an FP8 cache, beside the plans as WeightPlan is and for the same reason: no field of LlamaDims, no
// entry of the weight table, so a model without scales plans, lays out and launches what it did. One device buffer,
// fp32 [4][n_layers][Hkv]: 1 / k_scale, 1 / v_scale (what the writers multiply by, computed once on the host),
// then k_scale, v_scale (what k_attn undoes them with). nullptr: scale 1. It changes no plan: the kernels are the
// same instantiations with or without it.
struct KvScales {
  const float* table;
  enum Part : int { K_RECIP, V_RECIP, K, V };
  // [Hkv] of one part for layer L; nullptr without scales.
  const float* at(const LlamaDims& d, Part p, int L) const {
    return table ? table + (size_t(p) * d.n_layers + L) * d.Hkv : nullptr;
  }
};

// The sliding windows of a model's layers, beside the plans as WeightPlan and KvScales are and for the same reason: no
// field of LlamaDims or of a plan struct, so a model without windows plans, lays out and launches what it did. A host
// array of n_layers ints: 0 is full attention, W >= 1 attends to the last W positions, the row's own included
// (docs/SLIDING_WINDOW.md). nullptr: no layer has a window.
struct Windows {
  const int* per_layer;
  int at(int L) const { return per_layer ? per_layer[L] : 0; }
};
bool windows_ok(const LlamaDims& d, const Windows& w) {
  for (int L = 0; w.per_layer && L < d.n_layers; L++)
    if (w.per_layer[L] < 0) return false;
  return true;
}
// What one layer's window changes of a step (mirrored with ctypes): the attention variant, its launch argument and
// its span slots. Everything else of the layer is StepPlan's, and a layer with window 0 is StepPlan's attn as it is.
struct WindowPlan {
  int win;     // k_attn<D, G, KV8, true>
  int window;  // its launch argument (0 without)
  int slots;   // gridDim.x: those of a cache of min(max_seq, window) rows; the partials' stride stays AttnPlan's
};
WindowPlan plan_window(const LlamaDims& d, int B, int window) {
  if (window <= 0) return {0, 0, attn_slots(B, d.Hkv, d.max_seq)};
  return {1, window, attn_window_slots(B, d.Hkv, d.max_seq, window)};
}

// One workgroup per tn subtiles of 16 >> kpl columns of one 16-row tile.
//  - K parts (GemmArgs::kpl), where asked for (the d_model-wide O and down
//    projections): the widest tile (16, 8 or 4 columns) whose column tiles
//    reach one workgroup per CU, or 4 columns if none does; none where
//    16-column tiles already get there, the spare MFMA rows do not allow it
//    (M * P > 16) or K does not split into P parts of whole k-steps.
//  - Waves per workgroup, unless fixed: 4 up to 16 k-steps per workgroup, 8
//    above. Measured on MI355X (scripts/bench_skinny.py, M = 8): 4 and 8 waves
//    tie up to K = 2048.
//  - Load batch um: each wave's share of k-steps, rounded up to a power of two,
//    at most 4 (fewer registers, more resident waves).
// A K without a whole k-step leaves nw = 0, which launch() refuses.
GemmPlan plan_gemm(int epi, int tn, int M, int N, int K, bool k_parts = false, int fixed_nw = 0) {
  GemmPlan p{};
  p.epi = epi, p.tn = tn, p.M = M, p.N = N, p.K = K;
  if (k_parts && tn == 1 && (N >> 4) < kCUs) {
    const int kpl = std::min((N >> 3) >= kCUs ? 1 : 2, kMaxKpl);
    if ((M << kpl) <= 16 && K % (32 << kpl) == 0) p.kpl = kpl;
  }
  const int steps = (K >> p.kpl) >> 5;
  if (steps <= 0) return p;
  p.nw = fixed_nw ? fixed_nw : steps <= 16 ? 4 : 8;
  const int per_wave = (steps + p.nw - 1) / p.nw;
  p.um = per_wave <= 1 ? 1 : per_wave <= 2 ? 2 : 4;
  p.grid_x = N / (tn << tile_cwl(p.kpl));
  p.grid_y = (M + 15) >> 4;
  return p;
}

// 4 waves x 2 subtiles: the fastest LM-head shape measured (vocab 32000, K 2048: 22.6 vs 29.6 us).
GemmPlan plan_lm_head(const LlamaDims& d, int rows) {
  return plan_gemm(EPI_ARGMAX, kTnStore, rows, d.vocab, d.dim, false, 4);
}

AttnPlan plan_attn(int B, int H, int Hkv, int D, int max_seq) {
  return {D, Hkv > 0 ? H / Hkv : 0, attn_slots(B, Hkv, max_seq), attn_part_stride(max_seq), B * Hkv};
}

StepPlan plan_step(const LlamaDims& d, int B, int emit_rows) {
  StepPlan p{};
  p.rows = B;
  p.emit_rows = emit_rows <= 0 || emit_rows > B ? B : emit_rows;
  // QK-norm models: the GEMM stores the raw projection and k_qknorm_rope finishes it.
  // QKV-bias models: the RoPE epilogue with the bias add. No K parts on QKV (launch() refuses them with a bias).
  // Scaled RoPE (rope_table): the table counterpart of whichever kernel rotates; nothing else moves.
  // FP8 cache (kv_fp8): the _KV8 counterpart of whichever kernel appends, and of k_attn; nothing else moves.
  const int qkv_epi = d.qk_norm ? EPI_STORE : rope_epi(d.qkv_bias, d.rope_table, d.kv_fp8);
  p.qkv = plan_gemm(qkv_epi, 1, B, (d.H + 2 * d.Hkv) * d.D, d.dim);
  if (d.qk_norm) {
    const int per_wg = qknorm_heads_per_wg(d.D);
    p.qk_norm_grid = (d.H + 2 * d.Hkv + per_wg - 1) / per_wg;
    p.qk_norm_table = d.rope_table;
  }
  p.attn = plan_attn(B, d.H, d.Hkv, d.D, d.max_seq);
  p.o = plan_gemm(EPI_RESID, kTnResid, B, d.dim, d.H * d.D, true);
  p.gate_up = plan_gemm(EPI_SILU, 1, B, 2 * d.ffn, d.dim);
  p.down = plan_gemm(EPI_RESID, kTnResid, B, d.dim, d.ffn, true);
  p.lm_head = plan_lm_head(d, p.emit_rows);
  p.qkv_first = p.qkv;
  p.qkv_first.ss_in = 1;
  p.gate_up.ss_in = p.o.grid_x;
  p.qkv.ss_in = p.lm_head.ss_in = p.down.grid_x;
  p.am_parts = p.lm_head.grid_x;
  return p;
}

// ------------------------------------------------------------ workspace
size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

struct Workspace {
  uint16_t *resid, *q, *attn, *h, *qkv;
  float *ss, *part_o, *part_ml, *am_val;
  int* am_idx;
  unsigned* counters;  // [kMaxM * H] attention split tickets (self-resetting)
  size_t bytes;
};

// The workspace buffers in layout order (p2pt_llama_ws_layout reports them in this order).
enum WsBuf : int { WS_RESID, WS_Q, WS_ATTN, WS_H, WS_SS, WS_PART_O, WS_PART_ML, WS_AM_VAL, WS_AM_IDX, WS_COUNTERS, WS_QKV, WS_NBUF };

struct WsLayout {
  size_t off[WS_NBUF];    // byte offset from the workspace base (256-byte aligned)
  size_t count[WS_NBUF];  // elements: bf16 resid/q/attn/h/qkv, fp32 ss/part_o/part_ml/am_val, int32 am_idx, uint32 counters
  size_t bytes;
};

// The one place that knows the workspace layout. The counts that depend on a
// grid are the plan's own, at their worst case over the row count.
WsLayout ws_layout(const LlamaDims& d) {
  WsLayout l{};
  size_t off = 0;
  auto take = [&](WsBuf b, size_t count, size_t elem) {
    l.off[b] = off;
    l.count[b] = count;
    off += align256(count * elem);
  };
  const int nsplit = attn_part_stride(d.max_seq);
  const int ss_parts = d.dim / (kTnResid << tile_cwl(kMaxKpl));  // a residual producer's grid_x at the most K parts
  const int am_parts = plan_lm_head(d, kMaxM).grid_x;
  take(WS_RESID, size_t(kMaxM) * d.dim, 2);
  take(WS_Q, size_t(kMaxM) * d.H * d.D, 2);
  take(WS_ATTN, size_t(kMaxM) * d.H * d.D, 2);
  take(WS_H, size_t(kMaxM) * d.ffn, 2);
  take(WS_SS, size_t(std::max(ss_parts, 1)) * kMaxM, 4);
  take(WS_PART_O, size_t(kMaxM) * d.H * nsplit * d.D, 4);
  take(WS_PART_ML, size_t(kMaxM) * d.H * nsplit * 2, 4);
  take(WS_AM_VAL, size_t(am_parts) * kMaxM, 4);
  take(WS_AM_IDX, size_t(am_parts) * kMaxM, 4);
  take(WS_COUNTERS, size_t(kMaxM * d.H), 4);
  // The raw QKV projection of a QK-norm model; empty otherwise (the layout of other models is unchanged).
  take(WS_QKV, d.qk_norm ? size_t(kMaxM) * (d.H + 2 * d.Hkv) * d.D : 0, 2);
  l.bytes = off;
  return l;
}

Workspace carve(const LlamaDims& d, uint8_t* base) {
  const WsLayout l = ws_layout(d);
  Workspace w{};
  auto at = [&](WsBuf b) { return base ? base + l.off[b] : nullptr; };
  w.resid = reinterpret_cast<uint16_t*>(at(WS_RESID));
  w.q = reinterpret_cast<uint16_t*>(at(WS_Q));
  w.attn = reinterpret_cast<uint16_t*>(at(WS_ATTN));
  w.h = reinterpret_cast<uint16_t*>(at(WS_H));
  w.ss = reinterpret_cast<float*>(at(WS_SS));
  w.part_o = reinterpret_cast<float*>(at(WS_PART_O));
  w.part_ml = reinterpret_cast<float*>(at(WS_PART_ML));
  w.am_val = reinterpret_cast<float*>(at(WS_AM_VAL));
  w.am_idx = reinterpret_cast<int*>(at(WS_AM_IDX));
  w.counters = reinterpret_cast<unsigned*>(at(WS_COUNTERS));
  w.qkv = reinterpret_cast<uint16_t*>(at(WS_QKV));
  w.bytes = l.bytes;
  return w;
}

// ------------------------------------------------------------ weight table
// The one place in C that knows the layout of the pointer list w (ops/__init__.py's WeightTable is the Python one;
// p2pt_llama_weight_layout reports this one so that the two can be compared): embed, final_norm, lm_head, inv_freq
// if rope_table, then per layer the six, + q_norm, k_norm (qk_norm) or + bqkv (qkv_bias), then with FP8 weights the
// fp32 row scales: lm_head's, then per layer wqkv's, wo's, w_gate_up's and w_down's. An MXFP4 table has the same
// entries: lm_head as in an FP8 table, each layer GEMM as N * K / 2 bytes, and after the table lm_head's fp32 row
// scales, then per layer the four e8m0 scale tensors [N][K / 32] where the FP8 table has row scales.
enum Role : int { R_EMBED, R_FINAL_NORM, R_LM_HEAD, R_INV_FREQ, R_ATTN_NORM, R_WQKV, R_WO, R_FFN_NORM, R_W_GATE_UP,
                  R_W_DOWN, R_BQKV, R_Q_NORM, R_K_NORM, R_NROLES };
struct WeightTable {
  LlamaDims d;
  WeightFormat f;
  const void* const* w;
  int per_layer() const { return d.qk_norm ? 8 : d.qkv_bias ? 7 : 6; }
  int scales0() const { return 3 + d.rope_table + per_layer() * d.n_layers; }
  int size() const { return scales0() + (f.lm_head ? 1 + 4 * d.n_layers : 0); }
  // The format of a GEMM weight's role (0 for every other role).
  int format(Role r) const {
    return r == R_LM_HEAD ? f.lm_head : r == R_WQKV || r == R_WO || r == R_W_GATE_UP || r == R_W_DOWN ? f.layers : 0;
  }
  // Index of a role (of layer L, which the four global roles ignore); -1: this table has none.
  int index(Role r, int L = 0) const {
    if (r <= R_LM_HEAD) return r;
    if (r == R_INV_FREQ) return d.rope_table ? 3 : -1;
    const int base = 3 + d.rope_table + per_layer() * L;
    if (r <= R_W_DOWN) return base + (r - R_ATTN_NORM);
    if (r == R_BQKV) return d.qkv_bias && !d.qk_norm ? base + 6 : -1;
    return d.qk_norm ? base + 6 + (r - R_Q_NORM) : -1;
  }
  // Index of the scales of a GEMM weight (fp32 row scales, or an MXFP4 weight's e8m0 block scales); -1 for a bf16
  // table (where launch() wants none) or another role.
  int scale_index(Role r, int L = 0) const {
    const int j = r == R_WQKV ? 1 : r == R_WO ? 2 : r == R_W_GATE_UP ? 3 : r == R_W_DOWN ? 4 : 0;
    return !format(r) ? -1 : scales0() + (j ? 4 * L + j : 0);
  }
  const void* get(Role r, int L = 0) const { return at(index(r, L)); }  // nullptr where the table has none
  const void* scale(Role r, int L = 0) const { return at(scale_index(r, L)); }
  const void* at(int i) const { return i < 0 ? nullptr : w[i]; }
};

// ------------------------------------------------------------ kernel arguments
// A stage's GemmArgs is one expression: gemm(x, w) + norm(...) + its
// epilogue. Each helper takes every field of its group, so none stays zero by
// omission; launch() checks that a plan with a norm got one.
template <typename Set>
GemmArgs operator+(GemmArgs a, Set set) {
  set(a);
  return a;
}
// M, N, K and kpl are the plan's: launch() fills them in. scale: what the table holds for the weight's scales, the
// fp32 row scales of an FP8 weight (fmt 1) or the e8m0 block scales of an MXFP4 one (fmt 2); nullptr: bf16.
GemmArgs gemm(const void* x, const void* w, const void* scale = nullptr, int fmt = 1) {
  GemmArgs a{};
  a.x = static_cast<const uint16_t*>(x), a.w = static_cast<const uint16_t*>(w);
  if (fmt == 2) a.wexp = static_cast<const uint8_t*>(scale);
  else a.wscale = static_cast<const float*>(scale);
  return a;
}
auto norm(const float* ss, int parts, float eps) {
  return [=](GemmArgs& a) { a.ss_part = ss, a.ss_parts = parts, a.eps = eps; };
}
auto store(void* out) {  // STORE, SILU
  return [=](GemmArgs& a) { a.out = static_cast<uint16_t*>(out); };
}
// Every RoPE epilogue. bias and inv_freq: nullptr where the epilogue reads none (launch() refuses a bias or
// table epilogue without its pointer).
// k_rscale, v_rscale: the layer's reciprocal cache scales (KvScales), nullptr for scale 1 and for a bf16 cache.
auto rope(const LlamaDims& d, const int* pos, const int* slot, uint16_t* q, uint16_t* kc, uint16_t* vc,
          const void* bias, const void* inv_freq, const float* k_rscale, const float* v_rscale) {
  return [=](GemmArgs& a) {
    a.pos = pos, a.slot = slot, a.nslots = d.max_batch, a.q_out = q, a.kc = kc, a.vc = vc;
    a.k_rscale = k_rscale, a.v_rscale = v_rscale;
    a.bias = static_cast<const uint16_t*>(bias), a.inv_freq = static_cast<const float*>(inv_freq);
    a.H = d.H, a.Hkv = d.Hkv, a.D = d.D, a.Smax = d.max_seq, a.log2_theta = log2f(d.theta);
  };
}
auto resid(uint16_t* r, float* ss_out) {
  return [=](GemmArgs& a) { a.out = r, a.ss_out = ss_out; };
}
auto argmax(void* logits, float* am_val, int* am_idx) {
  return [=](GemmArgs& a) { a.out = static_cast<uint16_t*>(logits), a.am_val = am_val, a.am_idx = am_idx; };
}

// ------------------------------------------------------------ the kernels that exist
// Stated once: a list of values per template parameter and, for k_skinny, one predicate over their product. The
// three *_kernel() lookups instantiate exactly this set; the launchers, p2pt_llama_plan_kernels and dims_ok read
// nothing else.
template <int... V>
using Ints = std::integer_sequence<int, V...>;
using HeadDims = Ints<64, 128>;  // D of k_attn and k_qknorm_rope
// G of k_attn, the GQA ratio H / Hkv (models/checkpoint.py mirrors it as _GQA_RATIOS). 5, 6 and 7 are the Qwen2 /
// Qwen2.5 family's (40/8, 12/2, 14/2 and 28/4). 3 is absent: no checkpoint the loader accepts uses it.
using GqaRatios = Ints<1, 2, 4, 5, 6, 7, 8>;
using Flags = Ints<0, 1>;  // KV8 and WIN of k_attn; TAB and KV8 of k_qknorm_rope
using SkinnyFormats = Ints<0, 1, 2>;  // W8 of k_skinny: bf16, FP8, MXFP4
using SkinnyWaves = Ints<4, 8>;
using SkinnyTiles = Ints<1, 2>;
using SkinnyBatches = Ints<1, 2, 4>;
using SkinnyEpis = Ints<EPI_STORE, EPI_ROPE, EPI_SILU, EPI_RESID, EPI_ARGMAX, EPI_ROPE_BIAS, EPI_ROPE_TAB,
                        EPI_ROPE_BIAS_TAB, EPI_ROPE_KV8, EPI_ROPE_BIAS_KV8, EPI_ROPE_TAB_KV8, EPI_ROPE_BIAS_TAB_KV8>;
constexpr bool skinny_exists(int nw, int tn, int epi, int um, int w8) {
  // Two subtiles for the LM head and the standalone GEMM (plain STORE has both), one for every other epilogue.
  if (tn != (epi == EPI_ARGMAX ? 2 : 1) && !(epi == EPI_STORE && tn == 2)) return false;
  // FP8 weights run the five GEMMs of a step only (the standalone GEMM stays bf16), so they carry what plan_gemm
  // can give those: the LM head's fixed 4 waves with any load batch, and for the others the (nw, um) pairs of
  // fixed_nw == 0 below. 47 instantiations beside the 66 of bf16.
  if (w8 && epi == EPI_STORE && tn == 2) return false;
  // MXFP4 weights run a layer's four GEMMs only (the LM head stays FP8): every epilogue those can be planned with,
  // the eight RoPE ones, SILU, RESID and, for QK-norm models, STORE with one subtile, never ARGMAX, each with the
  // (nw, um) pairs of fixed_nw == 0. 44 instantiations beside the 47 of FP8 and the 66 of bf16.
  if (w8 == 2 && epi == EPI_ARGMAX) return false;
  if (w8 && epi == EPI_ARGMAX) return nw == 4;
  if (w8) return nw == 4 || um == 4;
  // The table and FP8-cache epilogues run QKV projections only, so they carry just the (nw, um) pairs plan_gemm
  // can give one (fixed_nw == 0): 4 waves up to 16 k-steps with um 1, 2 or 4, and 8 waves from 17 on, where a
  // wave's share is at least 3 k-steps and um is 4.
  if (epi_has_table(epi) || epi_kv8(epi)) return nw == 4 || um == 4;
  return true;
}
template <int... V>
constexpr bool contains(Ints<V...>, int v) {
  return ((v == V) || ...);
}

// pick(f, v0, Ints<...>{}, v1, Ints<...>{}, ...) calls f(c0, c1, ...), each c a std::integral_constant equal to
// its run-time v, and calls nothing when some v is in no list.
template <typename F>
void pick(F&& f) {
  f();
}
template <typename F, int... V, typename... Rest>
void pick(F&& f, int v, Ints<V...>, Rest... rest) {
  ((v == V ? pick([&](auto... c) { f(std::integral_constant<int, V>{}, c...); }, rest...) : void()), ...);
}

// The kernel a plan names, or nullptr where it is not instantiated.
using SkinnyKernel = void (*)(GemmArgs);
SkinnyKernel skinny_kernel(const GemmPlan& p, int w8 = 0) {
  SkinnyKernel k = nullptr;
  pick([&](auto nw, auto tn, auto epi, auto um, auto f8) {
    if constexpr (skinny_exists(nw, tn, epi, um, f8)) k = k_skinny<nw, tn, epi, um, f8>;
  }, p.nw, SkinnyWaves{}, p.tn, SkinnyTiles{}, p.epi, SkinnyEpis{}, p.um, SkinnyBatches{}, w8, SkinnyFormats{});
  return k;
}
using AttnKernel = decltype(&k_attn<64, 1, false>);
AttnKernel attn_kernel(int D, int G, int kv8, int win = 0) {
  AttnKernel k = nullptr;
  pick([&](auto d, auto g, auto f8, auto wn) { k = k_attn<d, g, f8 != 0, wn != 0>; }, D, HeadDims{}, G, GqaRatios{},
       kv8, Flags{}, win, Flags{});
  return k;
}
using QkNormKernel = void (*)(QkNormArgs);
QkNormKernel qknorm_kernel(int D, int table, int kv8) {
  QkNormKernel k = nullptr;
  pick([&](auto d, auto tab, auto f8) { k = k_qknorm_rope<d, tab != 0, f8 != 0>; }, D, HeadDims{}, table, Flags{},
       kv8, Flags{});
  return k;
}

// ------------------------------------------------------------ launches
// Each checks its arguments, looks its kernel up and launches it; a plan that names no kernel is hipErrorInvalidValue.
// w8: the weight's format (WeightFormat): 1, the FP8-weight instantiation, reads a.wscale and is refused without it;
// 2, the MXFP4 one, reads a.wexp likewise. A scale pointer the format does not read is refused too.
hipError_t launch(const GemmPlan& p, GemmArgs a, hipStream_t s, int w8 = 0) {
  if ((w8 == 1) != (a.wscale != nullptr) || (w8 == 2) != (a.wexp != nullptr)) return hipErrorInvalidValue;
  if (p.kpl < 0 || p.kpl > kMaxKpl || (p.ss_in > 0) != (a.ss_part != nullptr)) return hipErrorInvalidValue;
  if (p.kpl && (p.tn != 1 || (p.M << p.kpl) > 16 || p.K % (32 << p.kpl))) return hipErrorInvalidValue;
  // The bias is added once, after the K-split reduction: never with K parts, never without a bias.
  if (epi_has_bias(p.epi) && (p.kpl != 0 || a.bias == nullptr)) return hipErrorInvalidValue;
  // A table epilogue reads its table unconditionally: never without one.
  if (epi_has_table(p.epi) && a.inv_freq == nullptr) return hipErrorInvalidValue;
  // Cache scales come in pairs, and only to the epilogues that write an FP8 cache.
  if ((a.k_rscale != nullptr) != (a.v_rscale != nullptr) || (a.k_rscale && !epi_kv8(p.epi))) return hipErrorInvalidValue;
  const SkinnyKernel k = skinny_kernel(p, w8);
  if (!k) return hipErrorInvalidValue;
  a.M = p.M, a.N = p.N, a.K = p.K, a.kpl = p.kpl;
  hipLaunchKernelGGL(k, dim3(p.grid_x, p.grid_y), dim3(p.nw * 64), 0, s, a);
  return hipGetLastError();
}

// (span slot, row, KV head) workgroups of 8 waves. Row b reads cache slot
// slot[b] (nullptr: slot b) of nslots. kv8: the caches hold e4m3 bytes (KvPlan::attn_kv8). k_scale, v_scale: the
// layer's cache scales [Hkv] (KvScales), both nullptr for scale 1; refused with a bf16 cache. wp: the layer's
// window (WindowPlan); nullptr, or one without a window, launches the plan's own slots and the kernel without WIN.
// A windowed layer's slots must fit the partials' stride.
hipError_t launch_attn(const AttnPlan& p, int kv8, const void* q, const void* kc, const void* vc, const int* pos,
                       const int* slot, int nslots, float* part_o, float* part_ml, unsigned* counters, void* out,
                       int H, int Hkv, int Smax, hipStream_t s, const float* k_scale = nullptr,
                       const float* v_scale = nullptr, const WindowPlan* wp = nullptr) {
  const bool win = wp && wp->win;
  const AttnKernel k = attn_kernel(p.D, p.G, kv8, win);
  if (!k) return hipErrorInvalidValue;
  if ((k_scale != nullptr) != (v_scale != nullptr) || (k_scale && !kv8)) return hipErrorInvalidValue;
  if (win && (wp->window < 1 || wp->slots < 1 || wp->slots > p.stride)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k, dim3(win ? wp->slots : p.slots, p.grid_y), dim3(512), 0, s, static_cast<const uint16_t*>(q),
                     static_cast<const uint16_t*>(kc), static_cast<const uint16_t*>(vc), pos, slot, nslots, part_o,
                     part_ml, counters, static_cast<uint16_t*>(out), H, Hkv, Smax, p.stride, 1.f / sqrtf(float(p.D)),
                     k_scale, v_scale, win ? wp->window : 0);
  return hipGetLastError();
}

// (row, head group) workgroups of k_qknorm_rope: grid_x groups of qknorm_heads_per_wg(D) heads.
// table: the k_qknorm_rope<D, true> variant, which reads a.inv_freq (8-byte loads) and is refused without it.
// kv8: the variants that append k and v to an e4m3 cache.
hipError_t launch_qknorm(int grid_x, int rows, int D, bool table, bool kv8, const QkNormArgs& a, hipStream_t s) {
  const QkNormKernel k = qknorm_kernel(D, table, kv8);
  if (!k) return hipErrorInvalidValue;
  if (grid_x <= 0 || rows <= 0 || grid_x * qknorm_heads_per_wg(D) < a.H + 2 * a.Hkv) return hipErrorInvalidValue;
  if (table && (a.inv_freq == nullptr || reinterpret_cast<uintptr_t>(a.inv_freq) % 8)) return hipErrorInvalidValue;
  if ((a.k_rscale != nullptr) != (a.v_rscale != nullptr) || (a.k_rscale && !kv8)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k, dim3(grid_x, rows), dim3(kQkNormWaves * 64), 0, s, a);
  return hipGetLastError();
}

bool dims_ok(const LlamaDims& d) {
  if (!contains(HeadDims{}, d.D)) return false;
  if (d.qk_norm != 0 && d.qk_norm != 1) return false;
  if (d.qkv_bias != 0 && d.qkv_bias != 1) return false;
  if (d.rope_table != 0 && d.rope_table != 1) return false;
  // An e4m3 row of D in {64, 128} bytes stays a multiple of 16 bytes (k_attn's 8-byte loads, kv_copy's 16-byte ones).
  if (d.kv_fp8 != 0 && d.kv_fp8 != 1) return false;
  // No family has both, and the EPI_STORE + k_qknorm_rope route would need the bias elsewhere.
  if (d.qkv_bias && d.qk_norm) return false;
  // GEMM operands are addressed with 32-bit byte offsets below kOob (2 GiB):
  // each weight's own N x K bf16 extent (LM head vocab x dim, QKV, gate/up,
  // O, down), not the widest N times the largest K of different GEMMs.
  const size_t dim = size_t(d.dim), ffn = size_t(d.ffn), hd = size_t(d.H) * d.D;
  const size_t gemm_bytes[] = {size_t(d.vocab) * dim * 2, size_t(d.H + 2 * d.Hkv) * d.D * dim * 2,
                               2 * ffn * dim * 2, dim * hd * 2, dim * ffn * 2};
  for (size_t b : gemm_bytes)
    if (b >= kOob) return false;
  if (d.Hkv <= 0 || d.H % d.Hkv || !contains(GqaRatios{}, d.H / d.Hkv)) return false;
  if (d.dim % 32 || (d.H * d.D) % 32 || d.ffn % 32) return false;
  if (d.dim % (16 * kTnResid) || d.vocab % (16 * kTnStore) || d.ffn % 16) return false;
  if (d.max_batch <= 0 || d.max_seq <= 0 || d.n_layers <= 0) return false;
  return true;
}

bool rows_ok(int B) { return B > 0 && B <= kMaxM; }

}  // namespace

extern "C" {

// Workspace bytes for p2pt_llama_decode; it must be zero-filled once before first use
// (the in-kernel arrival counters reset themselves afterwards).
size_t p2pt_llama_ws_bytes(const LlamaDims* d) {
  if (!dims_ok(*d)) return 0;
  return carve(*d, nullptr).bytes;
}

// Where each workspace buffer lies (tests read the step's intermediates through
// this): byte offsets and element counts of resid, q, attn, h, ss, part_o,
// part_ml, am_val, am_idx, counters, qkv (empty unless qk_norm), in that order, into off[n] / count[n].
// Returns the number of buffers, or 0 for unsupported dims or n too small.
int p2pt_llama_ws_layout(const LlamaDims* d, size_t* off, size_t* count, int n) {
  if (!dims_ok(*d) || n < WS_NBUF) return 0;
  const WsLayout l = ws_layout(*d);
  for (int b = 0; b < WS_NBUF; b++) {
    off[b] = l.off[b];
    count[b] = l.count[b];
  }
  return WS_NBUF;
}

// What p2pt_llama_decode launches for B rows (host only: no device is touched).
// Refuses the dims and row counts that the step refuses.
int p2pt_llama_plan(const LlamaDims* d, int B, int emit_rows, StepPlan* out) {
  if (!dims_ok(*d) || !rows_ok(B)) return int(hipErrorInvalidValue);
  *out = plan_step(*d, B, emit_rows);
  return 0;
}

// The FP8-cache variants p2pt_llama_decode launches beside the plan above (host only); both 0 for a bf16 cache.
int p2pt_llama_kv_plan(const LlamaDims* d, KvPlan* out) {
  if (!dims_ok(*d)) return int(hipErrorInvalidValue);
  *out = plan_kv(*d);
  return 0;
}

// Whether every stage of the plans above names a kernel that exists, by the launchers' own lookups (host only).
// 0: all do; 1 + n: stage n, counting qkv_first, qkv, qk_norm, attn, o, gate_up, down, lm_head, is the first that
// does not; -1: dims or row count refused.
// windows: the per-layer windows (Windows), nullptr for none: every layer's attention variant must exist, and a
// windowed layer's slots must fit the partials' stride. A negative window is refused (-1).
// fmt: the weight formats (WeightFormat); one that is no supported pair is refused (-1).
int p2pt_llama_plan_kernels_fmt(const LlamaDims* d, int B, int emit_rows, const WeightFormat* fmt, const int* windows) {
  if (!dims_ok(*d) || !rows_ok(B) || !format_ok(*fmt) || !windows_ok(*d, Windows{windows})) return -1;
  const StepPlan P = plan_step(*d, B, emit_rows);
  const KvPlan KV = plan_kv(*d);
  const int w8 = fmt->layers;
  bool attn = true;
  for (int L = 0; L < d->n_layers; L++) {
    const WindowPlan wn = plan_window(*d, B, Windows{windows}.at(L));
    attn = attn && attn_kernel(P.attn.D, P.attn.G, KV.attn_kv8, wn.win) != nullptr && wn.slots >= 1 &&
           wn.slots <= P.attn.stride;
  }
  const bool found[] = {skinny_kernel(P.qkv_first, w8) != nullptr,
                        skinny_kernel(P.qkv, w8) != nullptr,
                        !P.qk_norm_grid || qknorm_kernel(d->D, P.qk_norm_table, KV.qk_norm_kv8) != nullptr,
                        attn,
                        skinny_kernel(P.o, w8) != nullptr,
                        skinny_kernel(P.gate_up, w8) != nullptr,
                        skinny_kernel(P.down, w8) != nullptr,
                        skinny_kernel(P.lm_head, fmt->lm_head) != nullptr};
  for (int n = 0; n < 8; n++)
    if (!found[n]) return 1 + n;
  return 0;
}
// The same with one format for the five GEMMs (WeightPlan: bf16 or FP8; anything else is refused).
int p2pt_llama_plan_kernels_win(const LlamaDims* d, int B, int emit_rows, const WeightPlan* wp, const int* windows) {
  if (!weights_ok(*wp)) return -1;
  const WeightFormat f{wp->w8, wp->w8};
  return p2pt_llama_plan_kernels_fmt(d, B, emit_rows, &f, windows);
}
int p2pt_llama_plan_kernels_w(const LlamaDims* d, int B, int emit_rows, const WeightPlan* wp) {
  return p2pt_llama_plan_kernels_win(d, B, emit_rows, wp, nullptr);
}
// What a layer with sliding window `window` (0: none) launches for attention at B rows, beside the plans above
// (host only).
int p2pt_llama_window_plan(const LlamaDims* d, int B, int window, WindowPlan* out) {
  if (!dims_ok(*d) || !rows_ok(B) || window < 0) return int(hipErrorInvalidValue);
  *out = plan_window(*d, B, window);
  return 0;
}
int p2pt_llama_plan_kernels(const LlamaDims* d, int B, int emit_rows) {
  const WeightPlan bf16{0};
  return p2pt_llama_plan_kernels_w(d, B, emit_rows, &bf16);
}

// The weight format of a step for weight_fp8 in {0, 1} (host only), beside the plans above.
int p2pt_llama_weight_plan(const LlamaDims* d, int weight_fp8, WeightPlan* out) {
  const WeightPlan w{weight_fp8};
  if (!dims_ok(*d) || !weights_ok(w)) return int(hipErrorInvalidValue);
  *out = w;
  return 0;
}

// The weight formats of a step for (layers, lm_head) in {(0, 0), (1, 1), (2, 1)} (host only), beside the plans above.
int p2pt_llama_weight_format(const LlamaDims* d, int layers, int lm_head, WeightFormat* out) {
  const WeightFormat f{layers, lm_head};
  if (!dims_ok(*d) || !format_ok(f)) return int(hipErrorInvalidValue);
  *out = f;
  return 0;
}

// The weight table of (dims, weight formats) as the step reads it (host only): its length, and into index[L * 13 + r]
// and scale_index[L * 13 + r] where role r (enum Role) of layer L and its scales (fp32 row scales, or the e8m0 block
// scales of an MXFP4 weight) sit, -1 where there is none.
// n: ints each array holds, at least 13 * n_layers. -1: dims or formats refused, or n too small.
int p2pt_llama_weight_layout_fmt(const LlamaDims* d, const WeightFormat* fmt, int* index, int* scale_index, int n) {
  if (!dims_ok(*d) || !format_ok(*fmt) || n < R_NROLES * d->n_layers) return -1;
  const WeightTable T{*d, *fmt, nullptr};
  for (int L = 0; L < d->n_layers; L++)
    for (int r = 0; r < R_NROLES; r++) {
      index[L * R_NROLES + r] = T.index(Role(r), L);
      scale_index[L * R_NROLES + r] = T.scale_index(Role(r), L);
    }
  return T.size();
}
// The same for a WeightPlan (bf16 or FP8 throughout; anything else is refused).
int p2pt_llama_weight_layout(const LlamaDims* d, const WeightPlan* wp, int* index, int* scale_index, int n) {
  if (!weights_ok(*wp)) return -1;
  const WeightFormat f{wp->w8, wp->w8};
  return p2pt_llama_weight_layout_fmt(d, &f, index, scale_index, n);
}

// k_attn's span rule: tokens per span slot for a row of `len` tokens.
int p2pt_attn_span(int len, int slots) { return len > 0 && slots > 0 ? attn_span(len, unsigned(slots)) : 0; }

int p2pt_max_rows() { return kMaxM; }

// One decode step over B <= 64 token rows. The grids depend on B alone (the
// context enters through pos), so a captured step serves every position.
//   w: the weight table, in WeightTable's order: embed, final_norm, lm_head, then per layer
//      attn_norm, wqkv [(H+2Hkv)*D, dim], wo [dim, H*D], ffn_norm, w_gate_up [2*ffn, dim], w_down [dim, ffn]
//      where wqkv, w_gate_up and lm_head carry the preceding RMSNorm weight folded
//      into their columns (W[n][k] * g[k]); the norm-weight slots are not read.
//      wqkv rows are interleaved per head (dim i, dim i + D/2, ...) and w_gate_up rows per pair (gate_j, up_j, ...).
//      With dims.qk_norm each layer has 8 entries, q_norm [D] and k_norm [D] appended, and
//      wqkv rows stay in plain order (k_qknorm_rope pairs the RoPE partners itself).
//      With dims.qkv_bias each layer has 7 entries: the six, then bqkv [(H+2Hkv)*D], interleaved like wqkv's rows.
//      With dims.rope_table a fourth global entry follows lm_head, ahead of the layers: inv_freq, fp32 [D/2],
//      8-byte aligned, the RoPE frequencies every layer rotates with (theta is then not read).
//   k_cache/v_cache: [n_layers][max_batch][max_seq][Hkv][D], bf16, or with dims.kv_fp8 one e4m3 byte per element
//   tokens int64 [B <= 64], pos int32 [B] (< max_seq), logits bf16 [B][vocab], ids int64 [B]
//   emit_rows: only rows [0, emit_rows) get logits and ids (the LM head runs on
//     them alone: prefill rows that sample nothing go last); <= 0 means B
//   slots int32 [B] or nullptr: cache slot of each row (< max_batch). Rows of one
//     slot at consecutive positions form a prefill chunk: every row's K/V is
//     appended before attention runs, and each row attends up to its own position.
//   FP8 weights (p2pt_llama_decode_w with WeightPlan::w8): the same table with lm_head, wqkv, wo, w_gate_up and
//      w_down as e4m3 bytes [N][K] (8-byte aligned), quantised after the fold and the interleave, followed by the
//      fp32 row scales: lm_head's [vocab], then per layer wqkv's, wo's, w_gate_up's and w_down's, each [N] in the
//      row order of its weight. Every other entry (embed, norms, inv_freq, bqkv, q_norm, k_norm) is as above.
//   FP8 cache with scales (p2pt_llama_decode_kv with dims.kv_fp8): kv_scales is a device buffer, fp32
//      [4][n_layers][Hkv]: 1 / k_scale, 1 / v_scale, k_scale, v_scale, every entry finite and > 0 (the caller's
//      check). A stored byte is e4m3(clamp(x * (1 / s))) of the head's scale and k_attn undoes it (KvScales).
//      nullptr: scale 1, which is p2pt_llama_decode_w. Refused with a bf16 cache.
//   Sliding windows (p2pt_llama_decode_win): windows is a host array of n_layers ints, read during the call only:
//      0 for a layer with full attention, W >= 1 for one whose rows attend to their last W positions, their own
//      included. Such a layer runs k_attn<D, G, KV8, true> on the slots of a cache of min(max_seq, W) rows; a layer
//      with 0 launches what it did. The cache keeps max_seq rows per slot and appends go to pos as before.
//      nullptr: no windows, which is p2pt_llama_decode_kv. A negative entry is refused.
//   MXFP4 weights (p2pt_llama_decode_fmt with WeightFormat{2, 1}): the FP8 table with each layer's wqkv, wo, w_gate_up
//      and w_down as bytes [N][K / 2] (4-byte aligned), two e2m1 nibbles each with the lower k in the low nibble,
//      quantised after the fold and the interleave, and where the FP8 table has their row scales the e8m0 scale
//      bytes [N][K / 32] of their 32-element blocks. lm_head and its fp32 row scales are the FP8 table's.
//      p2pt_llama_decode_win is this call with {w8, w8}.
int p2pt_llama_decode_fmt(const LlamaDims* dp, const WeightFormat* fmt, const float* kv_scales, const int* windows,
                          const void* const* w, void* k_cache, void* v_cache, const int64_t* tokens, const int* pos,
                          const int* slots, int B, int emit_rows, void* ws, size_t ws_bytes, void* logits,
                          int64_t* ids, void* stream) {
  const LlamaDims d = *dp;
  if (!dims_ok(d) || !rows_ok(B) || (!slots && B > d.max_batch) || !format_ok(*fmt)) return int(hipErrorInvalidValue);
  if (kv_scales && !d.kv_fp8) return int(hipErrorInvalidValue);
  const Windows WN{windows};
  if (!windows_ok(d, WN)) return int(hipErrorInvalidValue);
  const KvScales KS{kv_scales};
  const int w8 = fmt->layers;
  const Workspace W = carve(d, static_cast<uint8_t*>(ws));
  if (ws_bytes < W.bytes) return int(hipErrorInvalidValue);
  const StepPlan P = plan_step(d, B, emit_rows);
  const KvPlan KV = plan_kv(d);
  auto s = static_cast<hipStream_t>(stream);
  const size_t layer_cache = size_t(d.max_batch) * d.max_seq * d.Hkv * d.D * (d.kv_fp8 ? 1 : 2);  // bytes
  hipError_t e;
  auto failed = [&](hipError_t r) { return (e = r) != hipSuccess; };

  const WeightTable T{d, *fmt, w};
  const void* inv_freq = T.get(R_INV_FREQ);
  hipLaunchKernelGGL(k_embed, dim3(B), dim3(256), 0, s, static_cast<const uint16_t*>(T.get(R_EMBED)), tokens, W.resid,
                     W.ss, d.dim, d.vocab);
  if (failed(hipGetLastError())) return int(e);
  for (int L = 0; L < d.n_layers; L++) {
    uint16_t* kc = reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(k_cache) + L * layer_cache);
    uint16_t* vc = reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(v_cache) + L * layer_cache);
    const GemmPlan& qkv = L ? P.qkv : P.qkv_first;
    const GemmArgs qkv_in = gemm(W.resid, T.get(R_WQKV, L), T.scale(R_WQKV, L), w8) + norm(W.ss, qkv.ss_in, d.eps);
    const GemmArgs to_qkv =
        d.qk_norm ? qkv_in + store(W.qkv)
                  : qkv_in + rope(d, pos, slots, W.q, kc, vc, T.get(R_BQKV, L), inv_freq,
                                  KS.at(d, KvScales::K_RECIP, L), KS.at(d, KvScales::V_RECIP, L));
    const GemmArgs to_o = gemm(W.attn, T.get(R_WO, L), T.scale(R_WO, L), w8) + resid(W.resid, W.ss);
    const GemmArgs to_gate_up = gemm(W.resid, T.get(R_W_GATE_UP, L), T.scale(R_W_GATE_UP, L), w8) +
                                norm(W.ss, P.gate_up.ss_in, d.eps) + store(W.h);
    const GemmArgs to_down = gemm(W.h, T.get(R_W_DOWN, L), T.scale(R_W_DOWN, L), w8) + resid(W.resid, W.ss);
    if (failed(launch(qkv, to_qkv, s, w8))) return int(e);
    if (P.qk_norm_grid) {
      const QkNormArgs qn{W.qkv, static_cast<const uint16_t*>(T.get(R_Q_NORM, L)),
                          static_cast<const uint16_t*>(T.get(R_K_NORM, L)), pos, slots, d.max_batch, W.q, kc, vc, d.H,
                          d.Hkv, d.max_seq, d.eps, log2f(d.theta), static_cast<const float*>(inv_freq),
                          KS.at(d, KvScales::K_RECIP, L), KS.at(d, KvScales::V_RECIP, L)};
      if (failed(launch_qknorm(P.qk_norm_grid, B, d.D, P.qk_norm_table != 0, KV.qk_norm_kv8 != 0, qn, s)))
        return int(e);
    }
    const WindowPlan wn = plan_window(d, B, WN.at(L));
    if (failed(launch_attn(P.attn, KV.attn_kv8, W.q, kc, vc, pos, slots, d.max_batch, W.part_o, W.part_ml, W.counters, W.attn, d.H,
                           d.Hkv, d.max_seq, s, KS.at(d, KvScales::K, L), KS.at(d, KvScales::V, L), &wn)))
      return int(e);
    if (failed(launch(P.o, to_o, s, w8))) return int(e);
    if (failed(launch(P.gate_up, to_gate_up, s, w8))) return int(e);
    if (failed(launch(P.down, to_down, s, w8))) return int(e);
  }
  const GemmArgs to_logits =
      gemm(W.resid, T.get(R_LM_HEAD), T.scale(R_LM_HEAD), fmt->lm_head) + norm(W.ss, P.lm_head.ss_in, d.eps) +
      argmax(logits, W.am_val, W.am_idx);
  if (failed(launch(P.lm_head, to_logits, s, fmt->lm_head))) return int(e);
  hipLaunchKernelGGL(k_argmax_merge, dim3(P.emit_rows), dim3(256), 0, s, W.am_val, W.am_idx, P.am_parts, ids);
  return int(hipGetLastError());
}
int p2pt_llama_decode_win(const LlamaDims* dp, const WeightPlan* wp, const float* kv_scales, const int* windows,
                          const void* const* w, void* k_cache, void* v_cache, const int64_t* tokens, const int* pos,
                          const int* slots, int B, int emit_rows, void* ws, size_t ws_bytes, void* logits,
                          int64_t* ids, void* stream) {
  if (!weights_ok(*wp)) return int(hipErrorInvalidValue);
  const WeightFormat f{wp->w8, wp->w8};
  return p2pt_llama_decode_fmt(dp, &f, kv_scales, windows, w, k_cache, v_cache, tokens, pos, slots, B, emit_rows, ws,
                               ws_bytes, logits, ids, stream);
}
int p2pt_llama_decode_kv(const LlamaDims* dp, const WeightPlan* wp, const float* kv_scales, const void* const* w,
                         void* k_cache, void* v_cache, const int64_t* tokens, const int* pos, const int* slots, int B,
                         int emit_rows, void* ws, size_t ws_bytes, void* logits, int64_t* ids, void* stream) {
  return p2pt_llama_decode_win(dp, wp, kv_scales, nullptr, w, k_cache, v_cache, tokens, pos, slots, B, emit_rows, ws,
                               ws_bytes, logits, ids, stream);
}
int p2pt_llama_decode_w(const LlamaDims* dp, const WeightPlan* wp, const void* const* w, void* k_cache, void* v_cache,
                        const int64_t* tokens, const int* pos, const int* slots, int B, int emit_rows, void* ws,
                        size_t ws_bytes, void* logits, int64_t* ids, void* stream) {
  return p2pt_llama_decode_kv(dp, wp, nullptr, w, k_cache, v_cache, tokens, pos, slots, B, emit_rows, ws, ws_bytes,
                              logits, ids, stream);
}
int p2pt_llama_decode(const LlamaDims* dp, const void* const* w, void* k_cache, void* v_cache, const int64_t* tokens,
                      const int* pos, const int* slots, int B, int emit_rows, void* ws, size_t ws_bytes, void* logits,
                      int64_t* ids, void* stream) {
  const WeightPlan bf16{0};
  return p2pt_llama_decode_w(dp, &bf16, w, k_cache, v_cache, tokens, pos, slots, B, emit_rows, ws, ws_bytes, logits,
                             ids, stream);
}

// Standalone skinny GEMM (tests/benchmarks): out[M][N] = bf16(x[M][K] @ w[N][K]^T), M <= 64.
int p2pt_skinny_gemm(const void* x, const void* w, void* out, int M, int N, int K, void* stream) {
  if (!rows_ok(M) || N <= 0 || N % 32 || K <= 0 || K % 32) return int(hipErrorInvalidValue);
  // k_skinny's 32-bit byte offsets and descriptor sizes: both operands below kOob (2 GiB), as dims_ok keeps
  // the step's. A larger one would wrap its descriptor's size and read as zeros, without a fault.
  if (size_t(N) * size_t(K) * 2 >= kOob || size_t(M) * size_t(K) * 2 >= kOob) return int(hipErrorInvalidValue);
  const GemmPlan p = plan_gemm(EPI_STORE, 2, M, N, K);
  return int(launch(p, gemm(x, w) + store(out), static_cast<hipStream_t>(stream)));
}

// Standalone per-head RMSNorm + RoPE + cache append (tests): the kernel the fused step of a QK-norm model
// runs, on caller tensors. qkv [B <= 64][(H + 2 Hkv) * D], q_weight / k_weight [D], q [B][H][D], caches
// [nslots][Smax][Hkv][D]; row b goes to slot slots[b] (nullptr: slot b, B <= nslots) at pos[b]. inv_freq: fp32
// [D / 2], 8-byte aligned, for the table variant (theta is then not read), or nullptr for theta's own frequencies.
int p2pt_qk_norm_rope_cache(const void* qkv, const int* pos, const int* slots, const void* q_weight,
                            const void* k_weight, void* q, void* k_cache, void* v_cache, int B, int H, int Hkv, int D,
                            int Smax, int nslots, float eps, float theta, const float* inv_freq, void* stream) {
  if (!rows_ok(B) || !contains(HeadDims{}, D) || H <= 0 || Hkv <= 0 || Smax <= 0 || nslots <= 0)
    return int(hipErrorInvalidValue);
  if ((!slots && B > nslots) || !(theta > 0.f)) return int(hipErrorInvalidValue);
  const QkNormArgs a{static_cast<const uint16_t*>(qkv), static_cast<const uint16_t*>(q_weight),
                     static_cast<const uint16_t*>(k_weight), pos, slots, nslots, static_cast<uint16_t*>(q),
                     static_cast<uint16_t*>(k_cache), static_cast<uint16_t*>(v_cache), H, Hkv, Smax, eps, log2f(theta),
                     inv_freq, nullptr, nullptr};
  const int per_wg = qknorm_heads_per_wg(D);
  return int(launch_qknorm((H + 2 * Hkv + per_wg - 1) / per_wg, B, D, inv_freq != nullptr, false, a,
                           static_cast<hipStream_t>(stream)));
}

// Microbenchmark hook (scripts/bench_skinny.py --attn): `reps` back-to-back
// launches of the decode attention kernel. part_o / part_ml / counters as in
// the workspace (counters zeroed); q [B][H*D], caches [B][Smax][Hkv][D].
int p2pt_attn_bench(const void* q, const void* kc, const void* vc, const int* pos, int B, int H, int Hkv, int D,
                    int Smax, float* part_o, float* part_ml, unsigned* counters, void* out, int reps, void* stream) {
  if (!rows_ok(B) || Hkv <= 0 || H % Hkv || Smax <= 0 || reps <= 0) return int(hipErrorInvalidValue);
  const AttnPlan p = plan_attn(B, H, Hkv, D, Smax);
  for (int r = 0; r < reps; r++) {
    hipError_t e = launch_attn(p, 0, q, kc, vc, pos, nullptr, B, part_o, part_ml, counters, out, H, Hkv, Smax,
                               static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return int(e);
  }
  return 0;
}

// Microbenchmark hook (scripts/bench_skinny.py): `reps` back-to-back launches
// of the skinny GEMM with an explicit waves-per-block (4 or 8) / subtile
// (1 or 2) choice.
int p2pt_skinny_bench(const void* x, const void* w, void* out, int M, int N, int K, int nw, int tn, int reps,
                      void* stream) {
  if ((nw != 4 && nw != 8) || (tn != 1 && tn != 2)) return int(hipErrorInvalidValue);
  if (!rows_ok(M) || N % (16 * tn) || K <= 0 || K % 32 || reps <= 0) return int(hipErrorInvalidValue);
  const GemmPlan p = plan_gemm(EPI_STORE, tn, M, N, K, false, nw);
  const GemmArgs a = gemm(x, w) + store(out);
  for (int r = 0; r < reps; r++) {
    hipError_t e = launch(p, a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return int(e);
  }
  return 0;
}

}  // extern "C"
