// Host side of the fused Llama decode step for gfx950 (CDNA4 / MI355X): which
// kernel variant runs on which grid (plan_step, a pure function), the
// workspace, the set of kernel instantiations (lists and one predicate), the
// lookups and launches that follow a plan into that set, and the C entry
// points. The kernels and the design notes are in decode_fused_kernels.h.
#include "decode_fused_kernels.h"
#include "decode_f8g.h"
#include "decode_fused_set.h"
#include "decode_lora.h"
#include "decode_moe.h"
#include "decode_w4g.h"

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
// layout is pinned too): the _w entry points take it as an argument of its own. StepPlan does not
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
// 3 (docs/WEIGHT_INT4.md): grouped int4, GPTQ / AWQ style: uint4 nibbles in k-step-quad order with one word (fp16 scale,
// zero point) per group of 128 k, the layers only, with a bf16 LM head. Unlike the others it does change the step: the
// norm weight cannot be folded into a group, so the residual's producers also store xg = bf16(resid * g_next) into a
// workspace buffer of its own and the QKV and gate/up GEMMs read that (plan_step, ws_layout and the table take the
// format for it), and K parts carry whole quads.
// 4 (docs/WEIGHT_FP8G128.md): block-scaled FP8, what block-FP8 checkpoints expand to: e4m3 bytes in k-step-pair order
// with one fp32 scale per output row and group of 128 k, the layers only, with a bf16 LM head. The norm weight cannot
// be folded into a group here either, but the format adds no buffer: the QKV and gate/up kernels read the table's
// attn_norm / ffn_norm entries and multiply their A fragments in registers. It plans K in whole groups as 3 does; the
// workspace is the bf16 one.
bool format_ok(const WeightFormat& f) {
  return (f.layers == 0 && f.lm_head == 0) || (f.layers == 1 && f.lm_head == 1) || (f.layers == 2 && f.lm_head == 1) ||
         (f.layers == kW4g && f.lm_head == 0) || (f.layers == kF8g && f.lm_head == 0);
}
constexpr int kW4gGroup = 128;  // k per group: one quad of k-steps
bool grouped(int w8) { return w8 == kW4g || w8 == kF8g; }  // the formats whose scales change every kW4gGroup k
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

// Chunk attention (docs/CHUNK_ATTN.md), beside the plans as WindowPlan is and for the same reason: an opt-in that is no
// field of LlamaDims or of a plan struct, so a step without it plans, lays out and launches what it did. What
// k_attn_chunk<D, G, KV8> launches for B rows (mirrored with ctypes): (slots, tiles * Hkv) workgroups of `waves` waves.
// The span slots are attn_slots' of the tile count in place of the row count, so within the partials' stride, which
// stays AttnPlan's; the grid depends on (B, dims) alone.
struct ChunkPlan {
  int D, G;
  int tiles;   // 16-row tiles: (B + 15) / 16
  int slots;   // gridDim.x
  int stride;  // partial slots per head in part_o / part_ml (attn_part_stride)
  int grid_y;  // tiles * Hkv: counters[grid_y] are the tickets
  int waves;   // per workgroup: one per query head of the KV head, 4 at least
};
ChunkPlan plan_attn_chunk(int B, int H, int Hkv, int D, int max_seq) {
  const int tiles = (B + 15) >> 4, G = Hkv > 0 ? H / Hkv : 0;
  return {D, G, tiles, attn_slots(tiles, Hkv, max_seq), attn_part_stride(max_seq), tiles * Hkv, chunk_waves(G)};
}
// Which layers of a step run it: the flag is set, the step has more than one row tile and the layer has no window.
bool chunk_layer(int chunk_attn, int B, const WindowPlan& wn) { return chunk_attn && B > 16 && !wn.win; }

// The routed-expert FFN (docs/MOE.md), beside the plans as WeightFormat, KvScales, Windows and ChunkPlan are and for the
// same reason: MoeDims is no field of LlamaDims or of a plan struct, so a dense model (moe == nullptr everywhere below)
// plans, lays out and launches what it did. With it, LlamaDims::ffn is the per-expert intermediate size.
using p2pt_moe::MoeDims;
using p2pt_moe::MoePlan;
using p2pt_moe::ExpertFormat;
// The experts' format beside MoeDims (docs/MOE_FP8.md, docs/MOE_MXFP4.md): bf16, FP8 in k-step-pair order, whose rows
// are whole pairs, or MXFP4 in k-step-quad order, whose rows are whole quads. nullptr everywhere below is bf16, and
// then nothing changes.
bool experts_ok(const LlamaDims& d, const ExpertFormat* f) {
  return !f || f->w8 == 0 || (f->w8 == 1 && d.dim % 64 == 0 && d.ffn % 64 == 0) ||
         (f->w8 == 2 && d.dim % 128 == 0 && d.ffn % 128 == 0);
}
int expert_w8(const ExpertFormat* f) { return f ? f->w8 : 0; }
bool moe_ok(const LlamaDims& d, const MoeDims& m) {
  if (m.n_experts < 1 || m.n_experts > p2pt_moe::kMaxExperts) return false;
  if (m.top_k < 1 || m.top_k > std::min(p2pt_moe::kMaxTopK, m.n_experts)) return false;
  if (m.norm_topk != 0 && m.norm_topk != 1) return false;
  // Per-expert shapes are k_skinny's: whole k-steps of dim and ffn_e, 16-column tiles of [2 ffn_e] and [dim], and
  // each expert's slice below kOob (dims_ok holds d.ffn, the per-expert size, to exactly these).
  return d.dim % 32 == 0 && d.ffn % 32 == 0 && size_t(2) * d.ffn * d.dim * 2 < kOob;
}
// LoRA adapters (docs/LORA.md), beside the plans as MoeDims is and for the same reason: no field of LlamaDims or of a
// plan struct, so a model without adapters (lora == nullptr everywhere below) plans, lays out and launches what it did.
// Mirrored with ctypes. rank: the padded R of wqkv, wo, w_gate_up and w_down (a multiple of 16 up to 192, the same in
// every layer and adapter). tables: per layer eight device pointers, A' then B' of each of the four in that order;
// A' bf16 [n_adapters][R][K] with the preceding norm weight folded into its columns where the base weight has it,
// B' bf16 [n_adapters][N][R] in the row order of the base weight with the PEFT scaling folded in; 16-byte aligned.
struct LoraTable {
  int n_adapters;
  int rank[4];
  const void* const* tables;
};
enum LoraProj : int { LP_QKV, LP_O, LP_GATE_UP, LP_DOWN };
// bf16 dense layers without QK-norm (whose EPI_STORE route has no LORA variant: refused, not served).
bool lora_ok(const LlamaDims& d, const LoraTable& t) {
  if (d.qk_norm) return false;
  const int N[4] = {(d.H + 2 * d.Hkv) * d.D, d.dim, 2 * d.ffn, d.dim}, K[4] = {d.dim, d.H * d.D, d.dim, d.ffn};
  for (int j = 0; j < 4; j++)
    if (!p2pt_lora::shapes_ok(kMaxM, N[j], K[j], t.rank[j], t.n_adapters)) return false;
  return true;
}
// Every option of a step, beside the plans as each of its fields is (mirrored with ctypes): how they travel from the
// entry points to decode_step(), step_kernels(), the workspace and the weight layout. An all-zero struct is the bf16
// dense step without scales, windows, chunk attention or adapters. options_ok() is the one list of what is refused.
struct StepOptions {
  WeightFormat fmt;             // {0, 0}: bf16
  const float* kv_scales;       // device (KvScales), or nullptr
  const int* windows;           // host [n_layers] (Windows), or nullptr
  int chunk_attn;
  const MoeDims* moe;           // or nullptr
  const ExpertFormat* experts;  // or nullptr
  const LoraTable* lora;        // or nullptr
};
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
// quads (grouped int4 and block-scaled FP8 weights): a K part must hold whole quads of k-steps, so where K / 128 does not split into the P
// parts the rule above picks, the next smaller P that does is taken (bf16 gives up K parts there: it never happens
// for a K that is a multiple of 128 * P). The waves then split K / 128 quads, not K / 32 k-steps; nw and um keep
// their rule, so where nw does not divide the quads some waves get fewer or none.
GemmPlan plan_gemm(int epi, int tn, int M, int N, int K, bool k_parts = false, int fixed_nw = 0, bool quads = false) {
  GemmPlan p{};
  p.epi = epi, p.tn = tn, p.M = M, p.N = N, p.K = K;
  if (k_parts && tn == 1 && (N >> 4) < kCUs) {
    int kpl = std::min((N >> 3) >= kCUs ? 1 : 2, kMaxKpl);
    while (quads && kpl > 0 && K % (kW4gGroup << kpl)) kpl--;
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

// What the four kernels launch for B rows: a pure function of (B, dims, moe). Waves and load batch follow plan_gemm's
// rule for the expert's own K; the row tiles held per weight pass cover B pairs, the most one expert gets when a row
// names it once; k_moe_combine's grid is the dense down projection's, so the next norm's readers keep their ss_in.
// FP8 experts (ExpertFormat) run this plan int for int. Their kernels count K in pairs of k-steps, so a load batch um
// means max(um / 2, 1) pairs: 1 -> 2 k-steps in flight, 2 -> 2, 4 -> 4, the bf16 kernel's registers in flight except
// at um = 1; and gu_nw / dn_nw waves split K / 64 pairs, so waves past K / 64 (a K of 64 or 128 with 4 waves) stay idle.
// MXFP4 experts run it int for int too. Their kernels count K in quads of k-steps and a load batch is one quad at every
// um: 1 -> 4 k-steps in flight, 2 -> 4, 4 -> 4; and gu_nw / dn_nw waves split K / 128 quads, wave wv taking quads
// [wv (K / 128) / nw, (wv + 1) (K / 128) / nw): the bf16 kernel's K ranges where nw divides K / 128, otherwise some
// waves get fewer quads or none (a K of 128 or 256 with 4 waves leaves three or two idle).
MoePlan plan_moe(const LlamaDims& d, const MoeDims& m, int B) {
  MoePlan p{};
  const GemmPlan gu = plan_gemm(EPI_SILU, 1, B, 2 * d.ffn, d.dim), dn = plan_gemm(EPI_RESID, 1, B, d.dim, d.ffn);
  const GemmPlan dense_down = plan_gemm(EPI_RESID, kTnResid, B, d.dim, d.ffn, true);
  const int rt = B <= 16 ? 1 : B <= 32 ? 2 : 4;
  p.route_grid = B, p.route_waves = p2pt_moe::kRouteWaves;
  p.gu_grid_x = gu.grid_x, p.gu_grid_y = m.n_experts, p.gu_nw = gu.nw, p.gu_rt = rt, p.gu_um = gu.um;
  p.dn_grid_x = dn.grid_x, p.dn_grid_y = m.n_experts, p.dn_nw = dn.nw, p.dn_rt = rt, p.dn_um = dn.um;
  p.cb_grid = dense_down.grid_x, p.cb_cols = dense_down.grid_x > 0 ? d.dim / dense_down.grid_x : 0;
  p.cb_waves = p2pt_moe::kCombineWaves;
  return p;
}

AttnPlan plan_attn(int B, int H, int Hkv, int D, int max_seq) {
  return {D, Hkv > 0 ? H / Hkv : 0, attn_slots(B, Hkv, max_seq), attn_part_stride(max_seq), B * Hkv};
}

StepPlan plan_step(const LlamaDims& d, int B, int emit_rows, const WeightFormat& f = WeightFormat{0, 0}) {
  const bool quads = grouped(f.layers);
  StepPlan p{};
  p.rows = B;
  p.emit_rows = emit_rows <= 0 || emit_rows > B ? B : emit_rows;
  // QK-norm models: the GEMM stores the raw projection and k_qknorm_rope finishes it.
  // QKV-bias models: the RoPE epilogue with the bias add. No K parts on QKV (launch() refuses them with a bias).
  // Scaled RoPE (rope_table): the table counterpart of whichever kernel rotates; nothing else moves.
  // FP8 cache (kv_fp8): the _KV8 counterpart of whichever kernel appends, and of k_attn; nothing else moves.
  const int qkv_epi = d.qk_norm ? EPI_STORE : rope_epi(d.qkv_bias, d.rope_table, d.kv_fp8);
  p.qkv = plan_gemm(qkv_epi, 1, B, (d.H + 2 * d.Hkv) * d.D, d.dim, false, 0, quads);
  if (d.qk_norm) {
    const int per_wg = qknorm_heads_per_wg(d.D);
    p.qk_norm_grid = (d.H + 2 * d.Hkv + per_wg - 1) / per_wg;
    p.qk_norm_table = d.rope_table;
  }
  p.attn = plan_attn(B, d.H, d.Hkv, d.D, d.max_seq);
  p.o = plan_gemm(EPI_RESID, kTnResid, B, d.dim, d.H * d.D, true, 0, quads);
  p.gate_up = plan_gemm(EPI_SILU, 1, B, 2 * d.ffn, d.dim, false, 0, quads);
  p.down = plan_gemm(EPI_RESID, kTnResid, B, d.dim, d.ffn, true, 0, quads);
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
  uint16_t *resid, *q, *attn, *h, *qkv, *moe_h, *xg;
  float *ss, *part_o, *part_ml, *am_val, *route_w, *route_rs, *moe_part, *delta;
  int *am_idx, *route_id;
  unsigned* counters;  // [kMaxM * H] attention split tickets (self-resetting)
  size_t bytes;
};

// The workspace buffers in layout order (p2pt_llama_step_ws reports all WS_NALL of them in this order).
// The routed-expert FFN's buffers follow WS_QKV and are empty without MoeDims; WS_NDENSE counts the buffers
// p2pt_llama_ws_layout reports, WS_NBUF those of p2pt_llama_ws_layout_moe.
enum WsBuf : int { WS_RESID, WS_Q, WS_ATTN, WS_H, WS_SS, WS_PART_O, WS_PART_ML, WS_AM_VAL, WS_AM_IDX, WS_COUNTERS, WS_QKV,
                   WS_NDENSE, WS_ROUTE_ID = WS_NDENSE, WS_ROUTE_W, WS_ROUTE_RS, WS_MOE_H, WS_MOE_PART, WS_NBUF,
                   WS_XG = WS_NBUF,  // WS_XG: grouped int4 only, after every buffer the other layouts report
                   WS_DELTA, WS_NALL };  // WS_DELTA: LoRA adapters only, after every other buffer

struct WsLayout {
  size_t off[WS_NALL];    // byte offset from the workspace base (256-byte aligned)
  // elements: bf16 resid/q/attn/h/qkv/moe_h, fp32 ss/part_o/part_ml/am_val/route_w/route_rs/moe_part, int32 am_idx/route_id,
  // uint32 counters, fp32 delta
  size_t count[WS_NALL];
  size_t bytes;
};

// The one place that knows the workspace layout. The counts that depend on a
// grid are the plan's own, at their worst case over the row count.
WsLayout ws_layout(const LlamaDims& d, const StepOptions& o) {
  const MoeDims* moe = o.moe;
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
  // The routed-expert FFN: the route of every row, one moe_h row and one moe_part row per (row, choice) pair. Empty
  // without MoeDims, and after everything else, so the offsets and the size of a dense model are unchanged.
  const size_t pairs = moe ? size_t(kMaxM) * moe->top_k : 0;
  take(WS_ROUTE_ID, pairs, 4);
  take(WS_ROUTE_W, pairs, 4);
  take(WS_ROUTE_RS, moe ? kMaxM : 0, 4);
  take(WS_MOE_H, pairs * d.ffn, 2);
  take(WS_MOE_PART, pairs * d.dim, 4);
  // Grouped int4 weights: xg = bf16(resid * g_next), what the QKV and gate/up GEMMs read. Empty otherwise, and last, so
  // the offsets and the size of every other format are unchanged.
  take(WS_XG, o.fmt.layers == kW4g ? size_t(kMaxM) * d.dim : 0, 2);
  // LoRA adapters: delta fp32 [64][the widest projection], what k_lora_delta leaves for the next k_skinny. One buffer
  // serves a layer's four projections in turn (one stream). Empty otherwise, and last, so nothing else moves.
  const size_t widest = std::max(std::max(size_t(d.H + 2 * d.Hkv) * d.D, size_t(d.dim)), size_t(2) * d.ffn);
  take(WS_DELTA, o.lora ? size_t(kMaxM) * widest : 0, 4);
  l.bytes = off;
  return l;
}

Workspace carve(const LlamaDims& d, uint8_t* base, const StepOptions& o) {
  const WsLayout l = ws_layout(d, o);
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
  w.route_id = reinterpret_cast<int*>(at(WS_ROUTE_ID));
  w.route_w = reinterpret_cast<float*>(at(WS_ROUTE_W));
  w.route_rs = reinterpret_cast<float*>(at(WS_ROUTE_RS));
  w.moe_h = reinterpret_cast<uint16_t*>(at(WS_MOE_H));
  w.moe_part = reinterpret_cast<float*>(at(WS_MOE_PART));
  w.xg = reinterpret_cast<uint16_t*>(at(WS_XG));
  w.delta = reinterpret_cast<float*>(at(WS_DELTA));
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
// With FP8 experts (ew8; docs/MOE_FP8.md) w_gate_up and w_down are e4m3 bytes of the same shapes, 16-byte aligned, rows
// in k-step-pair order, and their fp32 row scales [E][2 ffn_e] and [E][dim] follow every other entry, per layer in that
// order; scale(R_W_GATE_UP / R_W_DOWN, L) reaches them, and no role is added.
// With MXFP4 experts (ew8 = 2; docs/MOE_MXFP4.md) w_gate_up and w_down are nibble bytes [E][2 ffn_e][dim / 2] and
// [E][dim][ffn_e / 2], 16-byte aligned, rows in k-step-quad order, and where the FP8-expert table has the row scales it
// has their e8m0 bytes [E][2 ffn_e][dim / 32] and [E][dim][ffn_e / 32], 4-byte aligned: expert_exp() reaches them.
// A grouped int4 table (docs/WEIGHT_INT4.md) has bf16 embed, norms and lm_head (final_norm folded in), each layer GEMM as
// N * K / 2 nibble bytes in k-step-quad order, 16-byte aligned, with no norm weight folded in, and after the table per
// layer the four group-word tensors [N][K / 128] uint32 where the FP8 table has row scales (no lm_head entry ahead of
// them). Its attn_norm and ffn_norm entries are read: they are the g of the xg stores.
// A block-scaled FP8 table (docs/WEIGHT_FP8G128.md) has the same entries as the grouped int4 one: each layer GEMM as
// N * K e4m3 bytes in k-step-pair order, 16-byte aligned, with no norm weight folded in, and after the table per layer
// the four scale tensors [N][K / 128] fp32. Its attn_norm and ffn_norm entries are read by the QKV and gate/up kernels.
// An MoE table (moe set; bf16 apart from the experts) has one more entry per layer, after every other: router, bf16 [E][dim] with the FFN
// norm folded in; its w_gate_up is [E][2 ffn_e][dim], folded and pair-interleaved per expert, and its w_down
// [E][dim][ffn_e]. R_ROUTER follows R_NROLES so that p2pt_llama_weight_layout's 13 roles per layer stay what they are.
enum Role : int { R_EMBED, R_FINAL_NORM, R_LM_HEAD, R_INV_FREQ, R_ATTN_NORM, R_WQKV, R_WO, R_FFN_NORM, R_W_GATE_UP,
                  R_W_DOWN, R_BQKV, R_Q_NORM, R_K_NORM, R_NROLES, R_ROUTER = R_NROLES, R_NROLES_MOE };
struct WeightTable {
  LlamaDims d;
  WeightFormat f;
  const void* const* w;
  int moe = 0;  // the layers carry a router
  int ew8 = 0;  // ExpertFormat::w8 (moe only): FP8 or MXFP4 experts have two scale entries per layer after the table
  int per_layer() const { return (d.qk_norm ? 8 : d.qkv_bias ? 7 : 6) + moe; }
  int scales0() const { return 3 + d.rope_table + per_layer() * d.n_layers; }
  int size() const {
    return scales0() + (f.lm_head ? 1 + 4 * d.n_layers : grouped(f.layers) ? 4 * d.n_layers : 0) + (ew8 ? 2 * d.n_layers : 0);
  }
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
    if (r == R_ROUTER) return moe ? base + per_layer() - 1 : -1;
    if (r == R_BQKV) return d.qkv_bias && !d.qk_norm ? base + 6 : -1;
    return d.qk_norm ? base + 6 + (r - R_Q_NORM) : -1;
  }
  // Index of the scales of a GEMM weight (fp32 row scales, or an MXFP4 weight's e8m0 block scales); -1 for a bf16
  // table (where launch() wants none) or another role.
  int scale_index(Role r, int L = 0) const {
    // FP8 experts: the layers are bf16 (an MoE model's only format), so the experts' scales are all there is.
    if (ew8 && (r == R_W_GATE_UP || r == R_W_DOWN)) return scales0() + 2 * L + (r == R_W_DOWN);
    const int j = r == R_WQKV ? 1 : r == R_WO ? 2 : r == R_W_GATE_UP ? 3 : r == R_W_DOWN ? 4 : 0;
    if (grouped(f.layers)) return j ? scales0() + 4 * L + j - 1 : -1;  // no lm_head scales ahead of the layers'
    return !format(r) ? -1 : scales0() + (j ? 4 * L + j : 0);
  }
  const void* get(Role r, int L = 0) const { return at(index(r, L)); }  // nullptr where the table has none
  const void* scale(Role r, int L = 0) const { return at(scale_index(r, L)); }
  // The experts' scales by their type: fp32 row scales (FP8 experts) or e8m0 block scales (MXFP4 experts), else nullptr.
  const float* expert_scale(Role r, int L) const { return ew8 == 1 ? static_cast<const float*>(scale(r, L)) : nullptr; }
  const uint8_t* expert_exp(Role r, int L) const { return ew8 == 2 ? static_cast<const uint8_t*>(scale(r, L)) : nullptr; }
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
// fp32 row scales of an FP8 weight (fmt 1), the e8m0 block scales of an MXFP4 one (fmt 2), the group words of a
// grouped int4 one (fmt 3) or the fp32 group scales of a block-scaled FP8 one (fmt 4); nullptr: bf16.
GemmArgs gemm(const void* x, const void* w, const void* scale = nullptr, int fmt = 1) {
  GemmArgs a{};
  a.x = static_cast<const uint16_t*>(x), a.w = static_cast<const uint16_t*>(w);
  if (fmt == 2) a.wexp = static_cast<const uint8_t*>(scale);
  else if (fmt == kW4g) a.wgrp = static_cast<const uint32_t*>(scale);
  else a.wscale = static_cast<const float*>(scale);
  return a;
}
// g: block-scaled FP8 only (the norm's weight, which the kernel multiplies into its A fragments).
auto norm(const float* ss, int parts, float eps, const void* g = nullptr) {
  return [=](GemmArgs& a) { a.ss_part = ss, a.ss_parts = parts, a.eps = eps, a.gin = static_cast<const uint16_t*>(g); };
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
// gnext, xg: grouped int4 only (the next norm's weight and the buffer its product with the new residual goes to).
auto resid(uint16_t* r, float* ss_out, const void* gnext = nullptr, uint16_t* xg = nullptr) {
  return [=](GemmArgs& a) { a.out = r, a.ss_out = ss_out, a.gnext = static_cast<const uint16_t*>(gnext), a.xg = xg; };
}
auto argmax(void* logits, float* am_val, int* am_idx) {
  return [=](GemmArgs& a) { a.out = static_cast<uint16_t*>(logits), a.am_val = am_val, a.am_idx = am_idx; };
}

// The kernel a plan names, or nullptr where it is not instantiated.
using SkinnyKernel = void (*)(GemmArgs);
SkinnyKernel skinny_kernel(const GemmPlan& p, int w8 = 0, bool lora = false) {
  // The LoRA-delta variants (bf16 weights only): the same lists and their own predicate, in decode_lora.hip.
  if (lora)
    return w8 ? nullptr
              : reinterpret_cast<SkinnyKernel>(const_cast<void*>(p2pt_lora::skinny_kernel(p.nw, p.tn, p.epi, p.um)));
  // Grouped int4: the same lists and predicate, instantiated in decode_w4g.hip.
  if (w8 == kW4g) return reinterpret_cast<SkinnyKernel>(const_cast<void*>(p2pt_w4g::skinny_kernel(p.nw, p.tn, p.epi, p.um)));
  // Block-scaled FP8: likewise, in decode_f8g.hip.
  if (w8 == kF8g) return reinterpret_cast<SkinnyKernel>(const_cast<void*>(p2pt_f8g::skinny_kernel(p.nw, p.tn, p.epi, p.um)));
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
using ChunkKernel = decltype(&k_attn_chunk<64, 1, false>);
ChunkKernel chunk_kernel(int D, int G, int kv8) {
  ChunkKernel k = nullptr;
  pick([&](auto d, auto g, auto f8) { k = k_attn_chunk<d, g, f8 != 0>; }, D, HeadDims{}, G, GqaRatios{}, kv8, Flags{});
  return k;
}
using QkNormKernel = void (*)(QkNormArgs);
QkNormKernel qknorm_kernel(int D, int table, int kv8) {
  QkNormKernel k = nullptr;
  pick([&](auto d, auto tab, auto f8) { k = k_qknorm_rope<d, tab != 0, f8 != 0>; }, D, HeadDims{}, table, Flags{},
       kv8, Flags{});
  return k;
}

bool rows_ok(int B) { return B > 0 && B <= kMaxM; }

// ------------------------------------------------------------ launches
// Each checks its arguments, looks its kernel up and launches it; a plan that names no kernel is hipErrorInvalidValue.
// w8: the weight's format (WeightFormat): 1, the FP8-weight instantiation, reads a.wscale and is refused without it;
// 2, the MXFP4 one, reads a.wexp likewise; 3, the grouped int4 one, a.wgrp; 4, the block-scaled FP8 one, a.wscale as
// [N][K / 128] and with a normed input a.gin. A scale pointer the format does not read is
// refused too. lora: the LORA instantiation of the plan's kernel, which reads a.delta: refused without it, as is a
// delta without the flag.
hipError_t launch(const GemmPlan& p, GemmArgs a, hipStream_t s, int w8 = 0, bool lora = false) {
  if (lora != (a.delta != nullptr)) return hipErrorInvalidValue;
  if ((w8 == 1 || w8 == kF8g) != (a.wscale != nullptr) || (w8 == 2) != (a.wexp != nullptr)) return hipErrorInvalidValue;
  // Grouped int4: the group words, K parts of whole quads, and for a residual producer the xg store's two pointers.
  if ((w8 == kW4g) != (a.wgrp != nullptr) || (grouped(w8) && p.K % (kW4gGroup << p.kpl))) return hipErrorInvalidValue;
  // Block-scaled FP8: the norm weight with a normed input and never otherwise; the kernels norm every epilogue but
  // RESID, so a plan that differs is refused.
  if ((w8 == kF8g && p.ss_in > 0) != (a.gin != nullptr) || (w8 == kF8g && (p.ss_in > 0) == (p.epi == EPI_RESID)))
    return hipErrorInvalidValue;
  if ((w8 == kW4g && p.epi == EPI_RESID) != (a.gnext != nullptr) || (a.gnext != nullptr) != (a.xg != nullptr))
    return hipErrorInvalidValue;
  if (p.kpl < 0 || p.kpl > kMaxKpl || (p.ss_in > 0) != (a.ss_part != nullptr)) return hipErrorInvalidValue;
  if (p.kpl && (p.tn != 1 || (p.M << p.kpl) > 16 || p.K % (32 << p.kpl))) return hipErrorInvalidValue;
  // The bias is added once, after the K-split reduction: never with K parts, never without a bias.
  if (epi_has_bias(p.epi) && (p.kpl != 0 || a.bias == nullptr)) return hipErrorInvalidValue;
  // A table epilogue reads its table unconditionally: never without one.
  if (epi_has_table(p.epi) && a.inv_freq == nullptr) return hipErrorInvalidValue;
  // Cache scales come in pairs, and only to the epilogues that write an FP8 cache.
  if ((a.k_rscale != nullptr) != (a.v_rscale != nullptr) || (a.k_rscale && !epi_kv8(p.epi))) return hipErrorInvalidValue;
  const SkinnyKernel k = skinny_kernel(p, w8, lora);
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

// (span slot, 16-row tile x KV head) workgroups of k_attn_chunk for B rows; the arguments are launch_attn's. The
// partials' stride must hold the slots, and the counters (kMaxM * H of them) the tickets.
hipError_t launch_attn_chunk(const ChunkPlan& p, int kv8, const void* q, const void* kc, const void* vc, const int* pos,
                             const int* slot, int B, int nslots, float* part_o, float* part_ml, unsigned* counters,
                             void* out, int H, int Hkv, int Smax, hipStream_t s, const float* k_scale = nullptr,
                             const float* v_scale = nullptr) {
  const ChunkKernel k = chunk_kernel(p.D, p.G, kv8);
  if (!k) return hipErrorInvalidValue;
  if ((k_scale != nullptr) != (v_scale != nullptr) || (k_scale && !kv8)) return hipErrorInvalidValue;
  if (!rows_ok(B) || p.tiles != (B + 15) >> 4 || p.grid_y != p.tiles * Hkv || p.G * Hkv != H) return hipErrorInvalidValue;
  if (p.slots < 1 || p.slots > p.stride || p.waves != chunk_waves(p.G)) return hipErrorInvalidValue;
  if ((!slot && B > nslots) || nslots < 1 || Smax < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k, dim3(p.slots, p.grid_y), dim3(p.waves * 64), 0, s, static_cast<const uint16_t*>(q),
                     static_cast<const uint16_t*>(kc), static_cast<const uint16_t*>(vc), pos, slot, B, nslots, part_o,
                     part_ml, counters, static_cast<uint16_t*>(out), H, Hkv, Smax, p.stride, 1.f / sqrtf(float(p.D)),
                     k_scale, v_scale);
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

// Grouped int4 and block-scaled FP8 weights: every K of a layer GEMM (dim, H * D, ffn) in whole groups of 128.
bool format_dims_ok(const LlamaDims& d, const WeightFormat& f) {
  return !grouped(f.layers) || (d.dim % kW4gGroup == 0 && (d.H * d.D) % kW4gGroup == 0 && d.ffn % kW4gGroup == 0);
}

// Every refusal that needs no per-call value, in one place: what the step refuses, the kernel lookup, the workspace
// and the weight layout refuse as well. The row count, slots, adapters, lora->tables and the workspace size are the
// step's own checks.
bool options_ok(const LlamaDims& d, const StepOptions& o) {
  if (!dims_ok(d) || !format_ok(o.fmt) || !format_dims_ok(d, o.fmt)) return false;
  if (!windows_ok(d, Windows{o.windows})) return false;
  if (o.moe && (!moe_ok(d, *o.moe) || o.fmt.layers != 0)) return false;  // an MoE model's layers are bf16
  if (!experts_ok(d, o.experts) || (!o.moe && expert_w8(o.experts))) return false;
  if (o.lora && (o.moe || o.fmt.layers != 0 || o.fmt.lm_head != 0 || !lora_ok(d, *o.lora))) return false;
  return !o.kv_scales || d.kv_fp8;  // a bf16 cache has no scales
}
// The one format of a WeightPlan for the five GEMMs. format_ok passes {w8, w8} for 0 and 1 alone, so every entry point
// that takes a WeightPlan refuses w8 = 2 as weights_ok does.
StepOptions plan_options(const WeightPlan& wp, const float* kv_scales = nullptr, const int* windows = nullptr) {
  return {{wp.w8, wp.w8}, kv_scales, windows};
}
StepOptions moe_options(const MoeDims* moe, const ExpertFormat* experts = nullptr) {
  return {{0, 0}, nullptr, nullptr, 0, moe, experts};
}

size_t ws_bytes(const LlamaDims& d, const StepOptions& o) { return options_ok(d, o) ? ws_layout(d, o).bytes : 0; }
// Offsets and counts of the first `prefix` buffers of WsBuf, then of buffer `extra` where one is named (the kept layout
// exports report such subsets). Returns how many were written; 0: options refused or n too small, nothing written.
int ws_report(const LlamaDims& d, const StepOptions& o, size_t* off, size_t* count, int n, int prefix, int extra = -1) {
  const int total = prefix + (extra >= 0);
  if (!options_ok(d, o) || n < total) return 0;
  const WsLayout l = ws_layout(d, o);
  for (int b = 0; b < total; b++) {
    const int from = b < prefix ? b : extra;
    off[b] = l.off[from], count[b] = l.count[from];
  }
  return total;
}

// The weight table of (dims, options) as the step reads it (host only): its length, and into index[L * roles + r] and,
// where asked for, scale_index[L * roles + r] where role r (enum Role) of layer L and its scales sit, -1 where there is
// none. roles: R_NROLES, or R_NROLES_MOE to include the router's. -1: options refused, or n < roles * n_layers.
int weight_layout(const LlamaDims& d, const StepOptions& o, int roles, int* index, int* scale_index, int n) {
  if (!options_ok(d, o) || n < roles * d.n_layers) return -1;
  const WeightTable T{d, o.fmt, nullptr, o.moe ? 1 : 0, expert_w8(o.experts)};
  for (int L = 0; L < d.n_layers; L++)
    for (int r = 0; r < roles; r++) {
      index[L * roles + r] = T.index(Role(r), L);
      if (scale_index) scale_index[L * roles + r] = T.scale_index(Role(r), L);
    }
  return T.size();
}

}  // namespace

extern "C" {

// The workspace of a step with options o: its bytes (0: refused); it must be zero-filled once before first use (the
// in-kernel arrival counters reset themselves afterwards). Where off and count are given and n >= WS_NALL, also where
// each buffer lies (tests read the step's intermediates through this): byte offsets and element counts of all WS_NALL
// buffers in WsBuf order, those the options do not use with count 0.
size_t p2pt_llama_step_ws(const LlamaDims* d, const StepOptions* o, size_t* off, size_t* count, int n) {
  if (off && count) ws_report(*d, *o, off, count, n, WS_NALL);
  return ws_bytes(*d, *o);
}
// The bf16 dense step's: resid, q, attn, h, ss, part_o, part_ml, am_val, am_idx, counters, qkv (empty unless qk_norm).
// Returns the number of buffers, or 0 for unsupported dims or n too small.
size_t p2pt_llama_ws_bytes(const LlamaDims* d) { return ws_bytes(*d, StepOptions{}); }
int p2pt_llama_ws_layout(const LlamaDims* d, size_t* off, size_t* count, int n) {
  return ws_report(*d, StepOptions{}, off, count, n, WS_NDENSE);
}
// The same for a step with a routed-expert FFN (moe; nullptr: a dense model, whose first eleven buffers and size are
// those above): route_id, route_w, route_rs, moe_h, moe_part follow qkv. Returns the number of buffers (16), or 0.
size_t p2pt_llama_ws_bytes_moe(const LlamaDims* d, const MoeDims* moe) { return ws_bytes(*d, moe_options(moe)); }
int p2pt_llama_ws_layout_moe(const LlamaDims* d, const MoeDims* moe, size_t* off, size_t* count, int n) {
  return ws_report(*d, moe_options(moe), off, count, n, WS_NBUF);
}
// What the routed-expert FFN's four kernels launch for B rows, beside the plans below (host only).
int p2pt_llama_moe_plan(const LlamaDims* d, const MoeDims* moe, int B, MoePlan* out) {
  if (!dims_ok(*d) || !moe_ok(*d, *moe) || !rows_ok(B)) return int(hipErrorInvalidValue);
  *out = plan_moe(*d, *moe, B);
  return 0;
}

// What p2pt_llama_decode launches for B rows (host only: no device is touched).
// Refuses the dims and row counts that the step refuses.
int p2pt_llama_plan(const LlamaDims* d, int B, int emit_rows, StepPlan* out) {
  if (!dims_ok(*d) || !rows_ok(B)) return int(hipErrorInvalidValue);
  *out = plan_step(*d, B, emit_rows);
  return 0;
}

// The same for a step in weight formats fmt (p2pt_llama_decode_fmt): grouped int4 and block-scaled FP8 layers plan
// their K parts in whole quads; every other format is the plan above, int for int.
int p2pt_llama_plan_fmt(const LlamaDims* d, const WeightFormat* fmt, int B, int emit_rows, StepPlan* out) {
  if (!dims_ok(*d) || !rows_ok(B) || !format_ok(*fmt) || !format_dims_ok(*d, *fmt)) return int(hipErrorInvalidValue);
  *out = plan_step(*d, B, emit_rows, *fmt);
  return 0;
}
// The workspace of a step in weight formats fmt: p2pt_llama_ws_bytes' and p2pt_llama_ws_layout's eleven buffers at
// their offsets, and with grouped int4 layers a twelfth, xg bf16 [64][dim], after them (empty otherwise).
size_t p2pt_llama_ws_bytes_fmt(const LlamaDims* d, const WeightFormat* fmt) { return ws_bytes(*d, StepOptions{*fmt}); }
int p2pt_llama_ws_layout_fmt(const LlamaDims* d, const WeightFormat* fmt, size_t* off, size_t* count, int n) {
  return ws_report(*d, StepOptions{*fmt}, off, count, n, WS_NDENSE, WS_XG);
}

// The FP8-cache variants p2pt_llama_decode launches beside the plan above (host only); both 0 for a bf16 cache.
int p2pt_llama_kv_plan(const LlamaDims* d, KvPlan* out) {
  if (!dims_ok(*d)) return int(hipErrorInvalidValue);
  *out = plan_kv(*d);
  return 0;
}

// Whether every stage of the plans above names a kernel that exists, by the launchers' own lookups (host only).
// 0: all do; 1 + n: stage n, counting qkv_first, qkv, qk_norm, attn, o, gate_up, down, lm_head, is the first that
// does not; -1: the options (options_ok) or the row count refused.
// windows: every layer's attention variant must exist, and a windowed layer's slots must fit the partials' stride.
// chunk_attn: the layers chunk_layer names need their k_attn_chunk instead, with its slots inside the stride.
// moe: stages gate_up and down are then the routed-expert FFN's kernels in the experts' format (all four must exist).
// lora: the four layer stages are then their LORA variants.
static int step_kernels(const LlamaDims* d, const StepOptions& o, int B, int emit_rows) {
  if (!options_ok(*d, o) || !rows_ok(B)) return -1;
  const WeightFormat* fmt = &o.fmt;
  const MoeDims* moe = o.moe;
  const bool lr = o.lora != nullptr;
  const bool moe_found =
      !moe || p2pt_moe::moe_kernels_exist(plan_moe(*d, *moe, B), ExpertFormat{expert_w8(o.experts)});
  const StepPlan P = plan_step(*d, B, emit_rows, *fmt);
  const KvPlan KV = plan_kv(*d);
  const int w8 = fmt->layers;
  bool attn = true;
  for (int L = 0; L < d->n_layers; L++) {
    const WindowPlan wn = plan_window(*d, B, Windows{o.windows}.at(L));
    if (chunk_layer(o.chunk_attn, B, wn)) {
      const ChunkPlan cp = plan_attn_chunk(B, d->H, d->Hkv, d->D, d->max_seq);
      attn = attn && chunk_kernel(cp.D, cp.G, KV.attn_kv8) != nullptr && cp.slots >= 1 && cp.slots <= cp.stride;
      continue;
    }
    attn = attn && attn_kernel(P.attn.D, P.attn.G, KV.attn_kv8, wn.win) != nullptr && wn.slots >= 1 &&
           wn.slots <= P.attn.stride;
  }
  const bool found[] = {skinny_kernel(P.qkv_first, w8, lr) != nullptr,
                        skinny_kernel(P.qkv, w8, lr) != nullptr,
                        !P.qk_norm_grid || qknorm_kernel(d->D, P.qk_norm_table, KV.qk_norm_kv8) != nullptr,
                        attn,
                        skinny_kernel(P.o, w8, lr) != nullptr,
                        moe ? moe_found : skinny_kernel(P.gate_up, w8, lr) != nullptr,
                        moe ? moe_found : skinny_kernel(P.down, w8, lr) != nullptr,
                        skinny_kernel(P.lm_head, fmt->lm_head) != nullptr};
  for (int n = 0; n < 8; n++)
    if (!found[n]) return 1 + n;
  return 0;
}
int p2pt_llama_step_kernels(const LlamaDims* d, const StepOptions* o, int B, int emit_rows) {
  return step_kernels(d, *o, B, emit_rows);
}
// The entry points from before StepOptions that tests and scripts call: each is the call above with its arguments as
// options.
int p2pt_llama_plan_kernels_experts(const LlamaDims* d, int B, int emit_rows, const WeightFormat* fmt,
                                    const int* windows, int chunk_attn, const MoeDims* moe,
                                    const ExpertFormat* experts) {
  return step_kernels(d, StepOptions{*fmt, nullptr, windows, chunk_attn, moe, experts}, B, emit_rows);
}
int p2pt_llama_plan_kernels_fmt(const LlamaDims* d, int B, int emit_rows, const WeightFormat* fmt, const int* windows) {
  return step_kernels(d, StepOptions{*fmt, nullptr, windows}, B, emit_rows);
}
// What k_attn_chunk launches for B rows, beside the plans above (host only).
int p2pt_llama_chunk_plan(const LlamaDims* d, int B, ChunkPlan* out) {
  if (!dims_ok(*d) || !rows_ok(B)) return int(hipErrorInvalidValue);
  *out = plan_attn_chunk(B, d->H, d->Hkv, d->D, d->max_seq);
  return 0;
}
// The same with one format for the five GEMMs (WeightPlan: bf16 or FP8; anything else is refused).
int p2pt_llama_plan_kernels_win(const LlamaDims* d, int B, int emit_rows, const WeightPlan* wp, const int* windows) {
  return step_kernels(d, plan_options(*wp, nullptr, windows), B, emit_rows);
}
int p2pt_llama_plan_kernels_w(const LlamaDims* d, int B, int emit_rows, const WeightPlan* wp) {
  return step_kernels(d, plan_options(*wp), B, emit_rows);
}
// What a layer with sliding window `window` (0: none) launches for attention at B rows, beside the plans above
// (host only).
int p2pt_llama_window_plan(const LlamaDims* d, int B, int window, WindowPlan* out) {
  if (!dims_ok(*d) || !rows_ok(B) || window < 0) return int(hipErrorInvalidValue);
  *out = plan_window(*d, B, window);
  return 0;
}
int p2pt_llama_plan_kernels(const LlamaDims* d, int B, int emit_rows) {
  return step_kernels(d, StepOptions{}, B, emit_rows);
}

// The weight format of a step for weight_fp8 in {0, 1} (host only), beside the plans above.
int p2pt_llama_weight_plan(const LlamaDims* d, int weight_fp8, WeightPlan* out) {
  const WeightPlan w{weight_fp8};
  if (!dims_ok(*d) || !weights_ok(w)) return int(hipErrorInvalidValue);
  *out = w;
  return 0;
}

// The weight formats of a step for (layers, lm_head) in {(0, 0), (1, 1), (2, 1), (3, 0), (4, 0)} (host only), beside the
// plans above.
int p2pt_llama_weight_format(const LlamaDims* d, int layers, int lm_head, WeightFormat* out) {
  const WeightFormat f{layers, lm_head};
  if (!dims_ok(*d) || !format_ok(f) || !format_dims_ok(*d, f)) return int(hipErrorInvalidValue);
  *out = f;
  return 0;
}

// The weight table of (dims, weight formats) as the step reads it (host only): its length, and into index[L * 13 + r]
// and scale_index[L * 13 + r] where role r (enum Role) of layer L and its scales (fp32 row scales, or the e8m0 block
// scales of an MXFP4 weight) sit, -1 where there is none.
// n: ints each array holds, at least 13 * n_layers. -1: dims or formats refused, or n too small.
int p2pt_llama_weight_layout_fmt(const LlamaDims* d, const WeightFormat* fmt, int* index, int* scale_index, int n) {
  return weight_layout(*d, StepOptions{*fmt}, R_NROLES, index, scale_index, n);
}
// The same for every option: 14 roles per layer, router (enum Role's R_ROUTER) last and -1 without moe.
int p2pt_llama_step_weights(const LlamaDims* d, const StepOptions* o, int* index, int* scale_index, int n) {
  return weight_layout(*d, *o, R_NROLES_MOE, index, scale_index, n);
}
// The same for an MoE table (bf16 only): 14 roles per layer; no scales.
int p2pt_llama_weight_layout_moe(const LlamaDims* d, const MoeDims* moe, int* index, int n) {
  return weight_layout(*d, moe_options(moe), R_NROLES_MOE, index, nullptr, n);
}
// The same with the experts' format (nullptr: bf16, the call above with no scales): scale_index[L * 14 + r] is where the
// fp32 row scales (FP8) or e8m0 block scales (MXFP4) of role r sit, -1 for every role but w_gate_up and w_down of an
// FP8- or MXFP4-expert table.
int p2pt_llama_weight_layout_experts(const LlamaDims* d, const MoeDims* moe, const ExpertFormat* experts, int* index,
                                     int* scale_index, int n) {
  return weight_layout(*d, moe_options(moe, experts), R_NROLES_MOE, index, scale_index, n);
}
// The same for a WeightPlan (bf16 or FP8 throughout; anything else is refused).
int p2pt_llama_weight_layout(const LlamaDims* d, const WeightPlan* wp, int* index, int* scale_index, int n) {
  return weight_layout(*d, plan_options(*wp), R_NROLES, index, scale_index, n);
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
//   ws, ws_bytes: the workspace, p2pt_llama_step_ws' bytes of the same options at least
//   adapters int32 [B] on the device or nullptr (with o.lora only): the adapter of each row, -1 for none
// The options (StepOptions; options_ok refuses what is not served). The all-zero struct launches the bf16 dense step,
// and each field left zero leaves every launch, the table and the workspace what they are without it.
//   fmt, the weight formats. {1, 1}, FP8: the same table with lm_head, wqkv, wo, w_gate_up and w_down as e4m3 bytes
//      [N][K] (8-byte aligned), quantised after the fold and the interleave, followed by the fp32 row scales: lm_head's
//      [vocab], then per layer wqkv's, wo's, w_gate_up's and w_down's, each [N] in the row order of its weight. Every
//      other entry (embed, norms, inv_freq, bqkv, q_norm, k_norm) is as above. {2, 1}, MXFP4: the FP8 table with each
//      layer's four as bytes [N][K / 2] (4-byte aligned), two e2m1 nibbles each with the lower k in the low nibble,
//      quantised after the fold and the interleave, and where the FP8 table has their row scales the e8m0 scale bytes
//      [N][K / 32] of their 32-element blocks; lm_head and its row scales are the FP8 table's. {3, 0}, grouped int4:
//      the table above WeightTable and docs/WEIGHT_INT4.md describe, and one more workspace buffer, xg. {4, 0},
//      block-scaled FP8: the table above WeightTable and docs/WEIGHT_FP8G128.md describe, on the bf16 workspace.
//   kv_scales (with dims.kv_fp8; refused with a bf16 cache): a device buffer, fp32 [4][n_layers][Hkv]: 1 / k_scale,
//      1 / v_scale, k_scale, v_scale, every entry finite and > 0 (the caller's check). A stored byte is
//      e4m3(clamp(x * (1 / s))) of the head's scale and k_attn undoes it (KvScales). nullptr: scale 1.
//   windows: a host array of n_layers ints, read during the call only: 0 for a layer with full attention, W >= 1 for
//      one whose rows attend to their last W positions, their own included. Such a layer runs k_attn<D, G, KV8, true>
//      on the slots of a cache of min(max_seq, W) rows; a layer with 0 launches what it did. The cache keeps max_seq
//      rows per slot and appends go to pos as before. nullptr: no windows. A negative entry is refused.
//   chunk_attn (docs/CHUNK_ATTN.md): in a step of more than 16 rows, every layer without a window runs k_attn_chunk on
//      ChunkPlan's grid instead of k_attn: one K/V pass per 16-row tile and distinct slot in it. Steps of up to 16 rows
//      and windowed layers launch what they did. The workspace is the same.
//   moe (docs/MOE.md; bf16 layers only): dims.ffn is the per-expert intermediate size, and every layer has a seventh
//      (with q_norm / k_norm or bqkv: last) entry, router, bf16 [E][dim] with the FFN norm folded in; w_gate_up is
//      [E][2 * ffn][dim], folded and pair-interleaved per expert, w_down [E][dim][ffn]. The layer's gate/up and down
//      kernels give way to k_moe_route, k_moe_gate_up, k_moe_down and k_moe_combine on MoePlan's grids; every other
//      launch is the dense step's. The workspace has the five route and expert buffers.
//   experts (with moe only; nullptr or w8 = 0: bf16). w8 = 1, FP8 (docs/MOE_FP8.md): w_gate_up and w_down are e4m3
//      bytes of the same shapes, 16-byte aligned, quantised after the fold and the interleave, every row in
//      k-step-pair order, and after every other entry of the table come, per layer, their fp32 row scales
//      [E][2 * ffn] and [E][dim]; dim and ffn must be multiples of 64. w8 = 2, MXFP4 (docs/MOE_MXFP4.md): nibble bytes
//      of half the element count, 16-byte aligned, every row in k-step-quad order, and where the FP8-expert table has
//      row scales their e8m0 block scales [E][2 * ffn][dim / 32] and [E][dim][ffn / 32], natural order, 4-byte
//      aligned; dim and ffn must be multiples of 128. k_moe_gate_up and k_moe_down are then that format's
//      instantiations on the same MoePlan; every other launch, the router's included, is unchanged.
//   lora (docs/LORA.md; bf16 dense layers without QK-norm): the workspace has one more buffer, delta. Ahead of each of
//      a layer's four projections k_lora_delta writes the rows' low-rank term there, and the projection runs as its
//      LORA variant on the same plan: 9 kernels per layer, one stream. adapters == nullptr launches the base step on
//      the larger workspace, launch for launch.
static int decode_step(const LlamaDims* dp, const StepOptions& o, const void* const* w, void* k_cache, void* v_cache,
                       const int64_t* tokens, const int* pos, const int* slots, int B, int emit_rows, void* ws,
                       size_t ws_bytes, void* logits, int64_t* ids, void* stream, const int* adapters) {
  const LlamaDims d = *dp;
  const WeightFormat* fmt = &o.fmt;
  const MoeDims* moe = o.moe;
  const LoraTable* lora = o.lora;
  if (!options_ok(d, o) || !rows_ok(B) || (!slots && B > d.max_batch)) return int(hipErrorInvalidValue);
  if ((adapters && !lora) || (lora && !lora->tables)) return int(hipErrorInvalidValue);
  const bool lr = lora && adapters;
  const ExpertFormat EF{expert_w8(o.experts)};
  const Windows WN{o.windows};
  const KvScales KS{o.kv_scales};
  const int w8 = fmt->layers;
  const Workspace W = carve(d, static_cast<uint8_t*>(ws), o);
  if (ws_bytes < W.bytes) return int(hipErrorInvalidValue);
  const StepPlan P = plan_step(d, B, emit_rows, *fmt);
  // k_lora_delta for projection j of layer L on the operand its k_skinny reads, and that k_skinny's delta argument.
  auto with_delta = [&](GemmArgs a) {
    a.delta = lr ? W.delta : nullptr;
    return a;
  };
  auto lora_delta = [&](int L, int j, const GemmPlan& p, const void* x) {
    const void* const* t = lora->tables + size_t(L) * 8 + 2 * j;
    return p2pt_lora::launch_delta({static_cast<const uint16_t*>(x), adapters, static_cast<const uint16_t*>(t[0]),
                                    static_cast<const uint16_t*>(t[1]), W.delta, B, p.N, p.K, lora->rank[j],
                                    lora->n_adapters}, static_cast<hipStream_t>(stream));
  };
  // Grouped int4: the normed GEMMs read xg, which the residual's producers store with the next norm's weight.
  const bool w4g = w8 == kW4g;
  const uint16_t* normed_in = w4g ? W.xg : W.resid;
  const MoePlan MP = moe ? plan_moe(d, *moe, B) : MoePlan{};
  const KvPlan KV = plan_kv(d);
  const ChunkPlan CP = plan_attn_chunk(B, d.H, d.Hkv, d.D, d.max_seq);
  auto s = static_cast<hipStream_t>(stream);
  const size_t layer_cache = size_t(d.max_batch) * d.max_seq * d.Hkv * d.D * (d.kv_fp8 ? 1 : 2);  // bytes
  hipError_t e;
  auto failed = [&](hipError_t r) { return (e = r) != hipSuccess; };

  const WeightTable T{d, *fmt, w, moe ? 1 : 0, EF.w8};
  const void* inv_freq = T.get(R_INV_FREQ);
  if (w4g) {
    if (failed(p2pt_w4g::launch_embed_xg(static_cast<const uint16_t*>(T.get(R_EMBED)), tokens, W.resid, W.ss, d.dim,
                                         d.vocab, static_cast<const uint16_t*>(T.get(R_ATTN_NORM, 0)), W.xg, B, s)))
      return int(e);
  } else {
    hipLaunchKernelGGL(k_embed, dim3(B), dim3(256), 0, s, static_cast<const uint16_t*>(T.get(R_EMBED)), tokens,
                       W.resid, W.ss, d.dim, d.vocab);
    if (failed(hipGetLastError())) return int(e);
  }
  for (int L = 0; L < d.n_layers; L++) {
    uint16_t* kc = reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(k_cache) + L * layer_cache);
    uint16_t* vc = reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(v_cache) + L * layer_cache);
    const GemmPlan& qkv = L ? P.qkv : P.qkv_first;
    // Block-scaled FP8: the normed GEMMs read the residual and multiply by the norm weight themselves.
    const bool f8g = w8 == kF8g;
    const GemmArgs qkv_in = gemm(normed_in, T.get(R_WQKV, L), T.scale(R_WQKV, L), w8) +
                            norm(W.ss, qkv.ss_in, d.eps, f8g ? T.get(R_ATTN_NORM, L) : nullptr);
    const GemmArgs to_qkv =
        d.qk_norm ? qkv_in + store(W.qkv)
                  : qkv_in + rope(d, pos, slots, W.q, kc, vc, T.get(R_BQKV, L), inv_freq,
                                  KS.at(d, KvScales::K_RECIP, L), KS.at(d, KvScales::V_RECIP, L));
    // The norm weight the GEMM after each residual producer would have folded: ffn_norm after O, the next layer's
    // attn_norm after down (the last layer's: final_norm, whose xg nothing reads; the LM head keeps its fold).
    const void* g_o = w4g ? T.get(R_FFN_NORM, L) : nullptr;
    const void* g_down = !w4g ? nullptr : L + 1 < d.n_layers ? T.get(R_ATTN_NORM, L + 1) : T.get(R_FINAL_NORM);
    const GemmArgs to_o = gemm(W.attn, T.get(R_WO, L), T.scale(R_WO, L), w8) +
                          resid(W.resid, W.ss, g_o, w4g ? W.xg : nullptr);
    const GemmArgs to_gate_up = gemm(normed_in, T.get(R_W_GATE_UP, L), T.scale(R_W_GATE_UP, L), w8) +
                                norm(W.ss, P.gate_up.ss_in, d.eps, f8g ? T.get(R_FFN_NORM, L) : nullptr) + store(W.h);
    const GemmArgs to_down = gemm(W.h, T.get(R_W_DOWN, L), T.scale(R_W_DOWN, L), w8) +
                             resid(W.resid, W.ss, g_down, w4g ? W.xg : nullptr);
    if (lr && failed(lora_delta(L, LP_QKV, qkv, normed_in))) return int(e);
    if (failed(launch(qkv, with_delta(to_qkv), s, w8, lr))) return int(e);
    if (P.qk_norm_grid) {
      const QkNormArgs qn{W.qkv, static_cast<const uint16_t*>(T.get(R_Q_NORM, L)),
                          static_cast<const uint16_t*>(T.get(R_K_NORM, L)), pos, slots, d.max_batch, W.q, kc, vc, d.H,
                          d.Hkv, d.max_seq, d.eps, log2f(d.theta), static_cast<const float*>(inv_freq),
                          KS.at(d, KvScales::K_RECIP, L), KS.at(d, KvScales::V_RECIP, L)};
      if (failed(launch_qknorm(P.qk_norm_grid, B, d.D, P.qk_norm_table != 0, KV.qk_norm_kv8 != 0, qn, s)))
        return int(e);
    }
    const WindowPlan wn = plan_window(d, B, WN.at(L));
    if (chunk_layer(o.chunk_attn, B, wn)) {
      if (failed(launch_attn_chunk(CP, KV.attn_kv8, W.q, kc, vc, pos, slots, B, d.max_batch, W.part_o, W.part_ml,
                                   W.counters, W.attn, d.H, d.Hkv, d.max_seq, s, KS.at(d, KvScales::K, L),
                                   KS.at(d, KvScales::V, L))))
        return int(e);
    } else if (failed(launch_attn(P.attn, KV.attn_kv8, W.q, kc, vc, pos, slots, d.max_batch, W.part_o, W.part_ml, W.counters, W.attn, d.H,
                                  d.Hkv, d.max_seq, s, KS.at(d, KvScales::K, L), KS.at(d, KvScales::V, L), &wn)))
      return int(e);
    if (lr && failed(lora_delta(L, LP_O, P.o, W.attn))) return int(e);
    if (failed(launch(P.o, with_delta(to_o), s, w8, lr))) return int(e);
    if (moe) {
      // resid and ss as the O projection left them; k_moe_combine leaves them as the down projection would.
      const p2pt_moe::MoeArgs ma{W.resid, W.ss, P.gate_up.ss_in, static_cast<const uint16_t*>(T.get(R_ROUTER, L)),
                                 T.get(R_W_GATE_UP, L), T.get(R_W_DOWN, L), W.route_id, W.route_w, W.route_rs,
                                 W.moe_h, W.moe_part, B, d.dim, d.ffn, moe->n_experts, moe->top_k, moe->norm_topk, d.eps,
                                 T.expert_scale(R_W_GATE_UP, L), T.expert_scale(R_W_DOWN, L),
                                 T.expert_exp(R_W_GATE_UP, L), T.expert_exp(R_W_DOWN, L)};
      if (failed(p2pt_moe::launch_moe(MP, ma, s, EF))) return int(e);
      continue;
    }
    if (lr && failed(lora_delta(L, LP_GATE_UP, P.gate_up, normed_in))) return int(e);
    if (failed(launch(P.gate_up, with_delta(to_gate_up), s, w8, lr))) return int(e);
    if (lr && failed(lora_delta(L, LP_DOWN, P.down, W.h))) return int(e);
    if (failed(launch(P.down, with_delta(to_down), s, w8, lr))) return int(e);
  }
  const GemmArgs to_logits =
      gemm(W.resid, T.get(R_LM_HEAD), T.scale(R_LM_HEAD), fmt->lm_head) + norm(W.ss, P.lm_head.ss_in, d.eps) +
      argmax(logits, W.am_val, W.am_idx);
  if (failed(launch(P.lm_head, to_logits, s, fmt->lm_head))) return int(e);
  hipLaunchKernelGGL(k_argmax_merge, dim3(P.emit_rows), dim3(256), 0, s, W.am_val, W.am_idx, P.am_parts, ids);
  return int(hipGetLastError());
}
int p2pt_llama_step(const LlamaDims* dp, const StepOptions* o, const void* const* w, void* k_cache, void* v_cache,
                    const int64_t* tokens, const int* pos, const int* slots, int B, int emit_rows, void* ws,
                    size_t ws_bytes, void* logits, int64_t* ids, void* stream, const int* adapters) {
  return decode_step(dp, *o, w, k_cache, v_cache, tokens, pos, slots, B, emit_rows, ws, ws_bytes, logits, ids, stream,
                     adapters);
}
// The entry points from before StepOptions that tests and scripts call: each is the step above with its arguments as
// options.
int p2pt_llama_decode_moe(const LlamaDims* dp, const WeightFormat* fmt, const float* kv_scales, const int* windows,
                          const void* const* w, void* k_cache, void* v_cache, const int64_t* tokens, const int* pos,
                          const int* slots, int B, int emit_rows, void* ws, size_t ws_bytes, void* logits,
                          int64_t* ids, void* stream, int chunk_attn, const MoeDims* moe) {
  return decode_step(dp, StepOptions{*fmt, kv_scales, windows, chunk_attn, moe}, w, k_cache, v_cache, tokens, pos, slots,
                     B, emit_rows, ws, ws_bytes, logits, ids, stream, nullptr);
}
int p2pt_llama_decode_chunk(const LlamaDims* dp, const WeightFormat* fmt, const float* kv_scales, const int* windows,
                            const void* const* w, void* k_cache, void* v_cache, const int64_t* tokens, const int* pos,
                            const int* slots, int B, int emit_rows, void* ws, size_t ws_bytes, void* logits,
                            int64_t* ids, void* stream, int chunk_attn) {
  return decode_step(dp, StepOptions{*fmt, kv_scales, windows, chunk_attn}, w, k_cache, v_cache, tokens, pos, slots, B,
                     emit_rows, ws, ws_bytes, logits, ids, stream, nullptr);
}
int p2pt_llama_decode_fmt(const LlamaDims* dp, const WeightFormat* fmt, const float* kv_scales, const int* windows,
                          const void* const* w, void* k_cache, void* v_cache, const int64_t* tokens, const int* pos,
                          const int* slots, int B, int emit_rows, void* ws, size_t ws_bytes, void* logits,
                          int64_t* ids, void* stream) {
  return decode_step(dp, StepOptions{*fmt, kv_scales, windows}, w, k_cache, v_cache, tokens, pos, slots, B, emit_rows,
                     ws, ws_bytes, logits, ids, stream, nullptr);
}
int p2pt_llama_decode_win(const LlamaDims* dp, const WeightPlan* wp, const float* kv_scales, const int* windows,
                          const void* const* w, void* k_cache, void* v_cache, const int64_t* tokens, const int* pos,
                          const int* slots, int B, int emit_rows, void* ws, size_t ws_bytes, void* logits,
                          int64_t* ids, void* stream) {
  return decode_step(dp, plan_options(*wp, kv_scales, windows), w, k_cache, v_cache, tokens, pos, slots, B, emit_rows,
                     ws, ws_bytes, logits, ids, stream, nullptr);
}
int p2pt_llama_decode_w(const LlamaDims* dp, const WeightPlan* wp, const void* const* w, void* k_cache, void* v_cache,
                        const int64_t* tokens, const int* pos, const int* slots, int B, int emit_rows, void* ws,
                        size_t ws_bytes, void* logits, int64_t* ids, void* stream) {
  return decode_step(dp, plan_options(*wp), w, k_cache, v_cache, tokens, pos, slots, B, emit_rows, ws, ws_bytes, logits,
                     ids, stream, nullptr);
}
int p2pt_llama_decode(const LlamaDims* dp, const void* const* w, void* k_cache, void* v_cache, const int64_t* tokens,
                      const int* pos, const int* slots, int B, int emit_rows, void* ws, size_t ws_bytes, void* logits,
                      int64_t* ids, void* stream) {
  return decode_step(dp, StepOptions{}, w, k_cache, v_cache, tokens, pos, slots, B, emit_rows, ws, ws_bytes, logits, ids,
                     stream, nullptr);
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

// Standalone chunk attention (ops.chunk_attention; tests, benchmarks): k_attn_chunk on caller tensors, for any B in
// 1..64. q [B][H*D] bf16, caches [nslots][Smax][Hkv][D] (bf16, or e4m3 bytes with kv8), pos / slots int32 [B] (slots
// nullptr: row b reads slot b, B <= nslots), k_scale / v_scale fp32 [Hkv] or both nullptr. part_o [B * H * stride * D]
// and part_ml [B * H * stride * 2] fp32 with stride = attn_part_stride(Smax), counters [ceil(B / 16) * Hkv] zeroed;
// out [B][H*D] bf16.
int p2pt_chunk_attention(const void* q, const void* kc, const void* vc, const int* pos, const int* slots, int B, int H,
                         int Hkv, int D, int nslots, int Smax, int kv8, const float* k_scale, const float* v_scale,
                         float* part_o, float* part_ml, unsigned* counters, void* out, void* stream) {
  if (!rows_ok(B) || Hkv <= 0 || H <= 0 || H % Hkv || Smax <= 0 || nslots <= 0) return int(hipErrorInvalidValue);
  const ChunkPlan p = plan_attn_chunk(B, H, Hkv, D, Smax);
  return int(launch_attn_chunk(p, kv8, q, kc, vc, pos, slots, B, nslots, part_o, part_ml, counters, out, H, Hkv, Smax,
                               static_cast<hipStream_t>(stream), k_scale, v_scale));
}

// Standalone routed-expert FFN (ops.moe_ffn; tests, benchmarks): the four kernels of one MoE layer on caller
// tensors. resid bf16 [B][dim], updated in place; ss fp32 [>= max(ss_in, cb_grid)][64]: rows [0, ss_in) hold the
// partial sums of squares of resid's rows on entry, rows [0, cb_grid) those of the new rows on return
// (cb_grid: p2pt_llama_moe_plan's); router bf16 [E][dim], w_gate_up bf16 [E][2 * ffn][dim] and w_down bf16
// [E][dim][ffn] as the step's weight table holds them; route_id int32 and route_w fp32 [B][top_k], route_rs fp32 [B],
// moe_h bf16 [B * top_k][ffn], moe_part fp32 [B][top_k][dim]: outputs, every slot a pair owns written.
// FP8 experts (p2pt_moe_ffn_experts with ExpertFormat::w8): w_gate_up and w_down are e4m3 bytes of the same shapes in
// k-step-pair order, gate_up_scale fp32 [E][2 * ffn] and down_scale fp32 [E][dim] their row scales; dim and ffn
// multiples of 64. experts == nullptr (or w8 = 0) wants both scales nullptr and is p2pt_moe_ffn.
// MXFP4 experts (p2pt_moe_ffn_mxfp4; w8 = 2): w_gate_up and w_down are nibble bytes [E][2 * ffn][dim / 2] and
// [E][dim][ffn / 2] in k-step-quad order, gate_up_exp [E][2 * ffn][dim / 32] and down_exp [E][dim][ffn / 32] their e8m0
// block scales in natural order; dim and ffn multiples of 128; no fp32 scales.
int p2pt_moe_ffn_mxfp4(void* resid, float* ss, int ss_in, const void* router, const void* w_gate_up, const void* w_down,
                       int* route_id, float* route_w, float* route_rs, void* moe_h, float* moe_part, int B, int dim,
                       int ffn, int E, int top_k, int norm_topk, float eps, void* stream, const uint8_t* gate_up_exp,
                       const uint8_t* down_exp) {
  if (!rows_ok(B) || dim <= 0 || ffn <= 0) return int(hipErrorInvalidValue);
  LlamaDims d{};
  d.dim = dim, d.ffn = ffn;
  const MoeDims m{E, top_k, norm_topk};
  const ExpertFormat f{2};
  if (!moe_ok(d, m) || !experts_ok(d, &f)) return int(hipErrorInvalidValue);
  const p2pt_moe::MoeArgs a{static_cast<uint16_t*>(resid), ss, ss_in, static_cast<const uint16_t*>(router), w_gate_up,
                            w_down, route_id, route_w, route_rs, static_cast<uint16_t*>(moe_h), moe_part, B, dim, ffn,
                            E, top_k, norm_topk, eps, nullptr, nullptr, gate_up_exp, down_exp};
  return int(p2pt_moe::launch_moe(plan_moe(d, m, B), a, static_cast<hipStream_t>(stream), f));
}
int p2pt_moe_ffn_experts(void* resid, float* ss, int ss_in, const void* router, const void* w_gate_up,
                         const void* w_down, int* route_id, float* route_w, float* route_rs, void* moe_h,
                         float* moe_part, int B, int dim, int ffn, int E, int top_k, int norm_topk, float eps,
                         void* stream, const ExpertFormat* experts, const float* gate_up_scale,
                         const float* down_scale) {
  if (!rows_ok(B) || dim <= 0 || ffn <= 0 || dim % 32 || ffn % 32) return int(hipErrorInvalidValue);
  LlamaDims d{};
  d.dim = dim, d.ffn = ffn;
  const MoeDims m{E, top_k, norm_topk};
  if (!moe_ok(d, m) || !experts_ok(d, experts)) return int(hipErrorInvalidValue);
  const p2pt_moe::MoeArgs a{static_cast<uint16_t*>(resid), ss, ss_in, static_cast<const uint16_t*>(router), w_gate_up,
                            w_down, route_id, route_w, route_rs, static_cast<uint16_t*>(moe_h), moe_part, B, dim, ffn,
                            E, top_k, norm_topk, eps, gate_up_scale, down_scale, nullptr, nullptr};
  return int(p2pt_moe::launch_moe(plan_moe(d, m, B), a, static_cast<hipStream_t>(stream),
                                  ExpertFormat{expert_w8(experts)}));
}
int p2pt_moe_ffn(void* resid, float* ss, int ss_in, const void* router, const void* w_gate_up, const void* w_down,
                 int* route_id, float* route_w, float* route_rs, void* moe_h, float* moe_part, int B, int dim, int ffn,
                 int E, int top_k, int norm_topk, float eps, void* stream) {
  return p2pt_moe_ffn_experts(resid, ss, ss_in, router, w_gate_up, w_down, route_id, route_w, route_rs, moe_h, moe_part,
                              B, dim, ffn, E, top_k, norm_topk, eps, stream, nullptr, nullptr, nullptr);
}
// plan_moe for the standalone op's shapes (host only).
int p2pt_moe_ffn_plan(int B, int dim, int ffn, int E, int top_k, int norm_topk, MoePlan* out) {
  if (!rows_ok(B) || dim <= 0 || ffn <= 0 || dim % 32 || ffn % 32) return int(hipErrorInvalidValue);
  LlamaDims d{};
  d.dim = dim, d.ffn = ffn;
  const MoeDims m{E, top_k, norm_topk};
  if (!moe_ok(d, m)) return int(hipErrorInvalidValue);
  *out = plan_moe(d, m, B);
  return 0;
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
