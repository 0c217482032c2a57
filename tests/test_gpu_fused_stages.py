"""Stage-by-stage fp64 checks of the fused decode step (decode_fused.hip).

Every kernel of the step is checked on its own against an fp64 reference
computed from the exact inputs that kernel read ("teacher forcing"): one-layer
models, one step, and every intermediate read back from the decoder's
workspace (``FusedLlamaDecoder.workspace_views``). The step is deterministic,
so the observed output of one stage is bit for bit the input of the next. The
residual after the O projection, which the down projection overwrites, is
observed by running the same step once with ``w_down`` zeroed in place:
the final residual is then bf(r + bf(0)) = r.

Because the inputs are exact, the allowed error of an element is a few bf16
ulps, not a share of a whole-model maximum. Each bound is derived in the
docstring of its stage helper from these pieces (U = 2^-24, the fp32 unit
roundoff; ulp(x): the bf16 spacing at |x|):

* an output rounded to bf16 once: ulp/2 of the reference (taken at |ref| + E,
  E the error bound of the value before rounding, so a binade edge is safe);
* an inner bf16 rounding (the GEMM result before RoPE / SwiGLU / the residual
  add) mirrors in the reference; it can land on the other neighbour only when
  the fp64 value lies within E of a rounding tie, and then counts one full
  ulp of the inner value (plus E), propagated to the output;
* fp32 accumulation of K products (exact as bf16 x bf16 in fp32) through
  MFMA, the wave split and the K parts: (K + 16) U sum|a_k||w_k|;
* 1/rms from fp32 partial sums of squares: the sum of K non-negative terms
  carries at most K U relative, halved by the inverse square root, plus the
  mean, the eps add and rsqrtf (<= 2 ulp): (K / 2 + 8) U relative.

``ops/build.py`` compiles with -O3 and no fast-math flag, so sincosf, exp2f,
rsqrtf and the division are the precise library versions (<= 2 ulp); the
kernels call the __expf intrinsic explicitly, whose error (the v_exp_f32 ulp
plus the rounding of x * log2(e), so growing with |x|) is used where it occurs.

Two CPU tests keep the bounds honest without the kernel: a plain fp32 torch
emulation with the same rounding points stays inside every bound, and the same
emulation with one arithmetic slip (a dropped k-step, a RoPE sign, a token too
few, a wrong split maximum, a swapped gate/up pair) violates it.

The stage helpers, ``stage_ratios`` and ``emulate`` take any layer of a deeper model (``layer``, default 0, and a
weight table of 6, 7 or 8 entries per layer); tests/test_gpu_fused_layers.py judges layer 1 of two-layer models
with them.
"""
import ctypes
import functools
import itertools
import math
from dataclasses import dataclass, replace

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig, TinyLlama, llama_dims

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")

U = 2.0 ** -24
BF = torch.bfloat16
F64 = torch.float64
VOCAB = 512
SENTINEL_BITS = 0x7B7B  # logits rows that must stay untouched hold this bf16 bit pattern
SENTINEL_ID = -7


# ---------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    name: str
    cfg: LlamaConfig
    pos: tuple
    slots: tuple | None = None  # row -> cache slot (None: row b -> slot b)
    emit_rows: int = 0
    dup_head: bool = False  # LM head = 8 distinct rows repeated over the vocab
    seed: int = 0

    @property
    def rows(self):
        return len(self.pos)

    @property
    def max_batch(self):
        return (max(self.slots) + 1) if self.slots is not None else self.rows


def _cfg(dim, ffn, H, Hkv, D, max_seq):
    return LlamaConfig(vocab=VOCAB, dim=dim, n_layers=1, n_heads=H, n_kv_heads=Hkv, head_dim=D, ffn=ffn,
                       max_seq=max_seq)


def _cases():
    cs = []
    # --- GEMM stages. k_skinny<NW, TN, EPI, UM>; "kp P": P K parts (GemmArgs::kpl).
    # dim 256, ffn 512: QKV <4,1,ROPE,2>, gate/up <4,1,SILU,2>, LM head <4,2,ARGMAX,2> at every row count.
    #   rows 1, 4: O <4,1,RESID,1> kp 4 (2 k-steps per part), down <4,1,RESID,1> kp 4; gate/up and the LM head
    #              read 64 sum-of-squares partials
    #   rows 5, 16, 17, 64: O <4,1,RESID,2>, down <4,1,RESID,4>, no K parts, 16 partials; 5 and 17 end in a
    #              partial row tile, 17 and 64 run 2 and 4 row tiles (blockIdx.y)
    g = _cfg(256, 512, 4, 2, 64, 64)
    for rows in (1, 4, 5, 16, 17, 64):
        cs.append(Case(f"gemm-d256-f512-r{rows}", g, tuple((7 * r + 3) % 61 for r in range(rows))))
    # ffn 352, 3 rows: O kp 4 (64 partials to gate/up), down <4,1,RESID,4> without K parts (352 % 128 != 0):
    # 11 k-steps over 4 waves (2, 3, 3, 3), 16 partials to the LM head.
    cs.append(Case("gemm-d256-f352-r3", _cfg(256, 352, 4, 2, 64, 64), (5, 0, 33)))
    # ffn 2816, 5 rows: down <8,1,RESID,4>, 88 k-steps, 11 per wave in load batches of 4, 4 and 3.
    cs.append(Case("gemm-d256-f2816-r5", _cfg(256, 2816, 4, 2, 64, 64), (1, 9, 17, 40, 63)))
    # dim 1536, ffn 1152, 2 rows: QKV <8,1,ROPE,4>; O kp 4 writes 384 partials; gate/up <8,1,SILU,4> holds
    # 4 * 8 * 8 = 256 of them in registers and reads 256..383 in the late loop; down <4,1,RESID,4> kp 4 with 9
    # k-steps per part; LM head <4,2,ARGMAX,4> reads 384 partials (late loop from 128).
    cs.append(Case("gemm-d1536-f1152-r2", _cfg(1536, 1152, 4, 2, 64, 64), (12, 50)))
    # dim 2048, D 128: O (K 2048) <8,1,RESID,4> and down (K 512) <4,1,RESID,2> in 2 K parts at 8 rows;
    # at 9 rows no K parts (O <8,1,RESID,4>, down <4,1,RESID,4>). k_attn<128,4>.
    w = _cfg(2048, 512, 16, 4, 128, 64)
    cs.append(Case("gemm-d2048-r8", w, tuple(range(8, 64, 7))))
    cs.append(Case("gemm-d2048-r9", w, tuple(range(0, 63, 7))))
    # Ties everywhere: within a 16-column subtile, across a block's two subtiles, across blocks.
    cs.append(Case("ids-dup-head", g, (3, 20, 41, 60, 11), dup_head=True))
    # The LM head and the merge run on the first 3 of 5 rows.
    cs.append(Case("ids-emit3of5", g, (3, 20, 41, 60, 11), emit_rows=3))

    for D in (64, 128):
        # --- Attention, ragged: 4 rows x 2 KV heads -> attn_slots = min(256 / 8, 16) = 16 span slots.
        # k_attn<D,G> for every G. pos 0: length 1, one slot, written directly; pos 64: span 64, a second slot of
        # one token; pos 1000: span 64, 16 slots, the last 41 tokens = pieces of 32 and 9; pos 2047: 16 spans of
        # 128 tokens (4 waves busy).
        for G in (1, 2, 4, 8):
            cs.append(Case(f"attn-ragged-D{D}-G{G}", _cfg(256, 256, 2 * G, 2, D, 2048), (0, 64, 1000, 2047)))
        # --- Attention, several 32-token pieces per wave (the corr rescale). k_attn<D,4> and <D,8>.
        for G in (4, 8):
            # A: 33 rows x 4 KV heads -> attn_slots = 256 / 132 = 1: one workgroup walks ~700 tokens, 3 pieces
            # on waves 0..5 and 2 on waves 6, 7. Rows map onto 3 cache slots at distinct positions.
            cs.append(Case(f"attn-A-D{D}-G{G}", _cfg(256, 256, 4 * G, 4, D, 1024),
                           tuple(650 + 2 * r for r in range(33)), slots=tuple(r % 3 for r in range(33))))
            # B: 24 rows x 4 KV heads -> attn_slots = 256 / 96 = 2: spans of 288..512 tokens, 2 pieces per wave
            # on some or all waves, merged through the arrival ticket.
            cs.append(Case(f"attn-B-D{D}-G{G}", _cfg(256, 256, 4 * G, 4, D, 1024),
                           tuple(520 + 21 * r for r in range(23)) + (1023,)))
            # C: a 32-row prefill chunk on slot 0 at positions 290..321 behind 4 decode rows on slots 1, 2
            # (36 rows x 4 KV heads -> 1 span slot, 10-11 pieces over 8 waves). Row r sees 0..pos[r] only.
            cs.append(Case(f"attn-C-D{D}-G{G}", _cfg(256, 256, 4 * G, 4, D, 512),
                           (400, 37, 401, 300) + tuple(range(290, 322)), slots=(1, 2, 1, 2) + (0,) * 32))
    return [replace(c, seed=i + 1) for i, c in enumerate(cs)]


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


EPI_NAMES = ("STORE", "ROPE", "SILU", "RESID", "ARGMAX", "ROPE_BIAS")  # decode_fused_kernels.h enum Epi
STAGES = ("qkv", "attn", "o", "gate_up", "down", "lm_head")


@functools.lru_cache(maxsize=None)
def step_plan(case):
    """What the library launches for a case: its own plan (host only), never a copy of its rules."""
    c = case.cfg
    dims = ops.LlamaDims(vocab=c.vocab, dim=c.dim, n_layers=c.n_layers, H=c.n_heads, Hkv=c.n_kv_heads, D=c.head_dim,
                         ffn=c.ffn, max_seq=c.max_seq, max_batch=case.max_batch + 1, eps=c.eps, theta=c.rope_theta,
                         qk_norm=int(c.qk_norm), qkv_bias=int(c.qkv_bias))
    return ops.step_plan(dims, case.rows, case.emit_rows)


def fmt(p):
    """A GemmPlan as ``<nw,tn,EPI,um> kpP``, an AttnPlan as ``k_attn<D,G> N slots``."""
    if isinstance(p, ops.AttnPlan):
        return f"k_attn<{p.D},{p.G}> {p.slots} slots"
    return f"<{p.nw},{p.tn},{EPI_NAMES[p.epi]},{p.um}>" + (f" kp{1 << p.kpl}" if p.kpl else "")


def plan_strings(plan):
    return tuple(fmt(getattr(plan, s)) for s in STAGES)


@dataclass
class Inputs:
    model: TinyLlama  # on the CPU: the weights every device copy shares
    weights: list  # the fused weight table (folded, interleaved), CPU
    tokens: torch.Tensor
    pos: torch.Tensor
    slots: torch.Tensor | None
    kc0: torch.Tensor  # [max_batch + 1, max_seq, Hkv, D] cache contents before the step
    vc0: torch.Tensor


def _dup_head(m):
    m.lm_head = m.lm_head[:8].repeat(m.cfg.vocab // 8, 1).contiguous()


@functools.lru_cache(maxsize=None)
def inputs(case: Case) -> Inputs:
    """Seeded inputs of a case, made once and shared (never modified) by every test."""
    m = TinyLlama(case.cfg, device="cpu", max_batch=case.max_batch, seed=case.seed)
    if case.dup_head:
        _dup_head(m)
    g = torch.Generator().manual_seed(1000 + case.seed)
    shape = tuple(m.k_cache.shape[1:])
    # K scaled so that scores spread over several units: a peaked softmax whose running maximum moves.
    kc0 = (torch.randn(shape, generator=g) * 2.5).to(BF)
    vc0 = torch.randn(shape, generator=g).to(BF)
    tokens = torch.randint(0, case.cfg.vocab, (case.rows,), generator=g)
    pos = torch.tensor(case.pos, dtype=torch.int32)
    slots = torch.tensor(case.slots, dtype=torch.int32) if case.slots is not None else None
    return Inputs(m, m.fused_weights(), tokens, pos, slots, kc0, vc0)


# ---------------------------------------------------------------- bf16 arithmetic in fp64
def bf64(x):
    """x (fp64) rounded to bf16, as fp64."""
    return x.to(BF).to(F64)


def ulp(a):
    """bf16 spacing at |a| (fp64)."""
    _, e = torch.frexp(a.abs().clamp_min(2.0 ** -126))  # |a| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(a), e - 8)


def flip(y, E):
    """How far bf16(y') can lie from bf16(y) when |y' - y| <= E: 0 unless y is within E of a rounding tie;
    then |bf(y') - y'| + |y' - y| + |y - bf(y)| <= ulp(|y| + E) + E, one spacing when E is small next to it
    (E exceeds the spacing only for results that cancel to almost nothing)."""
    a = y.abs().contiguous()
    r = a.to(BF)
    bits = r.view(torch.int16).to(torch.int32)
    up = (bits + 1).to(torch.int16).view(BF).to(F64)
    dn = (bits - 1).clamp_min(0).to(torch.int16).view(BF).to(F64)
    rd = r.to(F64)
    dist = torch.minimum(((rd + up) / 2 - a).abs(), ((rd + dn) / 2 - a).abs())
    return torch.where(dist <= E, ulp(a + E) + E, torch.zeros_like(a))


def rounded(ref, E):
    """Bound for an output stored as bf16 whose value before rounding is within E of ref."""
    return E + 0.5 * ulp(ref.abs() + E)


# ---------------------------------------------------------------- fp64 stage references
def gemm_ref(x, w, eps=None):
    """y = (1/rms(x)) x w^T in fp64 and the bound E on the kernel's fp32 value before any bf16 rounding.

    The bf16 products are exact in fp32. Summing K of them through the MFMA chain, the NW-wave split (<= 8
    adds) and the K parts (<= 4) costs at most (K + 16) U sum|x_k||w_k| (the standard recursive-sum bound).
    With a norm, 1/rms comes from fp32 sums of K non-negative squares (relative error <= K U whatever the
    order, halved by the power -1/2), the 1/K multiply, the eps add, rsqrtf (<= 2 ulp) and the final multiply:
    (K / 2 + 8) U relative to |y|.
    """
    xd, wd = x.to(F64), w.to(F64)
    K = x.shape[1]
    y, S = xd @ wd.T, xd.abs() @ wd.abs().T
    if eps is None:
        return y, (K + 16) * U * S
    rs = torch.rsqrt(xd.pow(2).mean(1, keepdim=True) + eps)
    y, S = y * rs, S * rs
    return y, (K + 16) * U * S + (K / 2 + 8) * U * y.abs()


def rope_tables(cfg, pos):
    """cos, sin [M, 1, D/2] in fp64 and the bound on the kernel's fp32 cos/sin.

    The kernel computes inv_freq = exp2f(t), t = -log2f(theta) * (2 i) / D in fp32: log2f, the multiply and the
    divide each round once, so t is off by <= 3 |t| U and inv_freq by ln2 * that relatively, plus exp2f
    (<= 2 ulp) and the rounding of pos * inv_freq: (3 ln2 |t| + 3) U relative to the angle, i.e. pos *
    inv_freq times that in radians. sincosf adds <= 2 ulp of a value <= 1 to each; 4 U covers both.
    """
    half = cfg.head_dim // 2
    t = -math.log2(cfg.rope_theta) * 2.0 * torch.arange(half, dtype=F64) / cfg.head_dim
    inv = torch.exp2(t)
    ang = pos.to(F64)[:, None, None] * inv[None, None, :]
    dsc = ang * ((3 * math.log(2) * t.abs() + 3) * U)[None, None, :] + 4 * U
    return torch.cos(ang), torch.sin(ang), dsc


@functools.lru_cache(maxsize=None)
def table_layout(cfg, weight_fp8=False):
    """The layout of the fused weight table of a model of ``cfg`` (``ops.WeightTable``: the one description)."""
    return ops.WeightTable(llama_dims(cfg, 1), weight_fp8)


def table_stride(cfg):
    """Entries per layer of the fused weight table: the six, + bqkv (Qwen2), or + q_norm, k_norm (Qwen3)."""
    return table_layout(cfg).per_layer


def layer_w(cfg, W, layer, name):
    """Entry ``name`` of ``layer`` in the table W: attn_norm, wqkv, wo, ffn_norm, w_gate_up, w_down (, bqkv | q_norm,
    k_norm)."""
    return W[table_layout(cfg).index(name, layer)]


def stage_qkv(case, W, x0, pos, layer=0):
    """QKV GEMM + RoPE + cache append from the layer's input rows x0 (embed[token] for layer 0): (q, k, v)
    references and bounds, [M, heads, D].

    v = bf(y): bound E + ulp/2 (gemm_ref's E). q and k: the kernel rounds both members of a pair to bf16
    (x1, x2), rotates in fp32 and rounds once more; the reference does the same in fp64. Error before the last
    rounding: the inner flips flip(x1)|cos| + flip(x2)|sin|, the cos/sin error (rope_tables) times |x1| + |x2|,
    and two fp32 products and one add, 3 U (|x1 cos| + |x2 sin|).
    """
    c = case.cfg
    H, Hkv, D, half = c.n_heads, c.n_kv_heads, c.head_dim, c.head_dim // 2
    y, E = gemm_ref(x0, layer_w(c, W, layer, "wqkv"), c.eps)
    M = y.shape[0]
    y, E = y.view(M, H + 2 * Hkv, half, 2), E.view(M, H + 2 * Hkv, half, 2)  # pairs (dim i, dim i + D/2)
    vy, vE = y[:, H + Hkv:], E[:, H + Hkv:]
    v = torch.cat([vy[..., 0], vy[..., 1]], -1)
    vE = torch.cat([vE[..., 0], vE[..., 1]], -1)
    ry, rE = y[:, :H + Hkv], E[:, :H + Hkv]
    x1, x2 = bf64(ry[..., 0]), bf64(ry[..., 1])
    f1, f2 = flip(ry[..., 0], rE[..., 0]), flip(ry[..., 1], rE[..., 1])
    cs, sn, dsc = rope_tables(c, pos)
    o1, o2 = x1 * cs - x2 * sn, x2 * cs + x1 * sn
    common = (x1.abs() + x2.abs()) * dsc
    E1 = f1 * cs.abs() + f2 * sn.abs() + common + 3 * U * ((x1 * cs).abs() + (x2 * sn).abs())
    E2 = f2 * cs.abs() + f1 * sn.abs() + common + 3 * U * ((x2 * cs).abs() + (x1 * sn).abs())
    o, Eo = torch.cat([o1, o2], -1), torch.cat([E1, E2], -1)
    bo = rounded(o, Eo)
    return (o[:, :H], bo[:, :H]), (o[:, H:], bo[:, H:]), (v, rounded(v, vE))


def stage_attn(case, q, kc, vc, pos, slots):
    """Attention of each row over positions 0..pos[row] of its cache slot: reference and bound [M, H*D].

    o = sum_j e_j v_j / sum_j e_j, e_j = exp(s_j - max). What the kernel's e_j can be off by, relatively:
    * the score: D exact bf16 products summed in fp32 (v_dot2 chain, DPP sums) and scaled,
      ds = (D + 8) U scale sum|q||k|, an absolute error of s_j and so a relative one of e_j; the maximum
      carries the same, hence 2 ds;
    * __expf: v_exp_f32 (1 ulp) of x log2(e), whose rounding is worth <= 2 |x| U in the result:
      (2 R + 4) U with R the row's score range; a term passes at most 6 of them (its own weight, the corr
      rescale at up to two later pieces, the wave merge, the slot merge and its rescale);
    * fp32 adds on the way into the sums (<= 8 per piece, 3 pieces, the cross-lane sums, 8 waves, 16
      slots): 64 U.
    With every e_j off by at most eta, numerator and denominator are each off by eta relatively, so
    |o - ref| <= 2 eta sum_j p_j |v_j|; the 1/L and the final multiply add 4 U. All of it is small next
    to the output's own bf16 half ulp unless the output cancels.
    """
    c = case.cfg
    H, Hkv, D = c.n_heads, c.n_kv_heads, c.head_dim
    G = H // Hkv
    scale = 1.0 / math.sqrt(D)
    refs, bounds = [], []
    for b in range(q.shape[0]):
        n = int(pos[b]) + 1
        s_ = int(slots[b]) if slots is not None else b
        K, V = kc[s_, :n].to(F64), vc[s_, :n].to(F64)  # [n, Hkv, D]
        qd = q[b].to(F64).view(Hkv, G, D)
        s = torch.einsum("hgd,lhd->hgl", qd, K) * scale
        ds = (D + 8) * U * scale * torch.einsum("hgd,lhd->hgl", qd.abs(), K.abs()).amax(-1)
        R = s.amax(-1) - s.amin(-1)
        p = torch.softmax(s, -1)
        o = torch.einsum("hgl,lhd->hgd", p, V)
        A = torch.einsum("hgl,lhd->hgd", p, V.abs())
        eta = 2 * ds + 6 * (2 * R + 4) * U + 64 * U
        E = (2 * eta + 4 * U)[..., None] * A
        refs.append(o.reshape(H * D))
        bounds.append(rounded(o, E).reshape(H * D))
    return torch.stack(refs), torch.stack(bounds)


def stage_resid(x, w, prev):
    """Projection + residual add, bf(prev + bf(y)): reference and bound.

    The inner bf(y) can flip within gemm_ref's E; prev + bf(y) is rounded to fp32 by the add (U relative)
    and then to bf16.
    """
    y, E = gemm_ref(x, w)
    r = prev.to(F64) + bf64(y)
    return r, rounded(r, flip(y, E) + U * r.abs())


def silu(z):
    return z / (1 + torch.exp(-z))


def stage_swiglu(case, W, r1, layer=0):
    """RMSNorm + gate/up GEMM + SwiGLU, h = bf(silu(bf(g)) * bf(u)): reference and bound [M, ffn].

    The inner roundings of g and u can flip within gemm_ref's E: the change of silu over that step of g
    (evaluated, not linearised) times |u|, and the step of u times |silu(g)| (plus the cross term). silu in
    fp32: __expf(-g) is off by (2 |g| + 2) U relatively, which 1 / (1 + e) damps to at most as much; the add,
    the divide (correctly rounded: no fast-math flag) and the multiply add 3 U.
    """
    y, E = gemm_ref(r1, layer_w(case.cfg, W, layer, "w_gate_up"), case.cfg.eps)
    M = y.shape[0]
    y, E = y.view(M, -1, 2), E.view(M, -1, 2)  # pairs (gate_j, up_j)
    g, u = bf64(y[..., 0]), bf64(y[..., 1])
    fg, fu = flip(y[..., 0], E[..., 0]), flip(y[..., 1], E[..., 1])
    sg = silu(g)
    dsl = torch.maximum((silu(g + fg) - sg).abs(), (silu(g - fg) - sg).abs())
    h = sg * u
    Eh = dsl * u.abs() + (sg.abs() + dsl) * fu + (2 * g.abs() + 8) * U * h.abs()
    return h, rounded(h, Eh)


def stage_lm_head(case, W, r2):
    """Final RMSNorm + LM head, bf(y): gemm_ref's E plus the output's half ulp."""
    y, E = gemm_ref(r2, W[2], case.cfg.eps)
    return y, rounded(y, E)


def first_argmax(logits):
    """First index of each row's maximum, spelled out (no reliance on a library's tie order)."""
    l = logits.to(torch.float32)
    idx = torch.arange(l.shape[1]).expand_as(l)
    return torch.where(l == l.amax(1, keepdim=True), idx, l.shape[1]).amin(1)


def worst(got, ref_bound):
    """Largest |got - ref| / bound over the elements: 0 where they agree exactly (a bound of 0 asks for that),
    inf where the comparison does not hold, a NaN on either side included."""
    ref, bound = ref_bound
    err = (got.to(F64).reshape(ref.shape) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).max().item()


def stage_ratios(case, W, obs, layer=0, qkv_stage=stage_qkv, inp=None):
    """Largest |observed - reference| / bound of every stage of ``layer``, each reference computed from the
    observed inputs of that stage alone. Layer 0 starts from embed[token]; a later layer from its observed input
    rows ``obs["x0"]``, and ``obs`` then holds that layer's q, attn, r1, h, r2 and its own cache as kc, vc.
    ``qkv_stage(case, W, x0, pos, layer)`` gives the (q, k, v) references of the model's family. ``inp``: the
    tokens, pos and slots of a case whose inputs are not ``inputs(case)``'s (tests/test_gpu_fused_served.py builds
    its wide layers on the device, and runs this under ``torch.device("cuda")`` with every tensor there)."""
    inp = inp if inp is not None else inputs(case)
    c, B = case.cfg, case.rows
    emit = case.emit_rows or B
    rows = torch.arange(B)
    sl = inp.slots.long() if inp.slots is not None else rows
    x0 = W[0][inp.tokens] if layer == 0 else obs["x0"]

    out = {}
    qr, kr, vr = qkv_stage(case, W, x0, inp.pos, layer)
    out["q"] = worst(obs["q"], qr)
    out["k"] = worst(obs["kc"][sl, inp.pos.long()], kr)
    out["v"] = worst(obs["vc"][sl, inp.pos.long()], vr)
    out["attn"] = worst(obs["attn"], stage_attn(case, obs["q"], obs["kc"], obs["vc"], inp.pos, inp.slots))
    out["o"] = worst(obs["r1"], stage_resid(obs["attn"], layer_w(c, W, layer, "wo"), x0))
    out["h"] = worst(obs["h"], stage_swiglu(case, W, obs["r1"], layer))
    out["down"] = worst(obs["r2"], stage_resid(obs["h"], layer_w(c, W, layer, "w_down"), obs["r1"]))
    out["logits"] = worst(obs["logits"][:emit], stage_lm_head(case, W, obs["r2"][:emit]))
    want = first_argmax(obs["logits"][:emit])
    out["ids"] = 0.0 if torch.equal(obs["ids"][:emit], want) else float("inf")
    return out


# ---------------------------------------------------------------- fp32 emulation (CPU)
def bf32(x):
    return x.to(BF).to(torch.float32)


GEMM_STAGES = ("qkv", "o", "gate_up", "down", "lm_head")
MUTATIONS = {  # mutation -> the stage outputs of which at least one must leave its bound
    **{f"drop_kstep:{s}": t for s, t in zip(GEMM_STAGES, (("q", "k", "v"), ("o",), ("h",), ("down",), ("logits",)))},
    "rope_sign": ("q", "k"), "one_token_short": ("attn",), "wrong_split_max": ("attn",), "swap_gate_up": ("h",),
}


# Slips of a layer past the first (``emulate``'s ``slip``): what only a layer L >= 1 can get wrong.
LAYER_SLIPS = (
    "late_loop",  # the QKV GEMM sums only the 32 * nw sum-of-squares partials that fit its registers
    "stale_ss",  # ... or takes 1/rms from the partials the previous layer's O projection left
    "table:wqkv", "table:bias", "table:qk_norm",  # the previous layer's weight-table entry
    "attend_layer0",  # attention over layer 0's cache
    "kv_into_layer0",  # the K and V rows appended to layer 0's cache
    "drop_ss_partial",  # down's epilogue leaves one of its sum-of-squares partials out (every layer)
)


def emulate(case, mut=None, slip=None):
    """The step in plain fp32 torch with the kernels' bf16 rounding points, layer after layer, each layer on a
    cache of its own that starts from the case's kc0 / vc0; ``mut`` names one arithmetic slip (in every layer),
    ``slip`` one of LAYER_SLIPS (in the layers past the first).

    Returns what ``observe_gpu`` returns, for the last layer (kc, vc: its cache), so the same ``stage_ratios``
    judges it, and with it: x0, the last layer's input rows; caches, every layer's (kc, vc); ss2 and ss3 [parts,
    B], the sum-of-squares partials the last layer's down projection writes over the residual before it (r1, as
    when w_down is zero) and after it (r2), one per down.grid_x column tile; qkv, the raw projection of a QK-norm
    model's last layer."""
    inp = inputs(case)
    c, B, W = case.cfg, case.rows, inp.weights
    H, Hkv, D, half = c.n_heads, c.n_kv_heads, c.head_dim, c.head_dim // 2
    G = H // Hkv
    emit = case.emit_rows or B
    sl = inp.slots.long() if inp.slots is not None else torch.arange(B)
    pos = inp.pos.long()
    plan = step_plan(case)

    def sumsq(x):
        return x.float().pow(2).sum(1)

    def partials(x):  # [B, parts]: down's RESID epilogue sums the squares of its own columns
        p = x.float().pow(2).view(B, plan.down.grid_x, -1).sum(-1)
        if slip == "drop_ss_partial":
            p[:, plan.down.grid_x // 2] = 0
        return p

    def gemm(stage, x, w, ss=None):  # ss: the row sums of squares of the folded norm (None: no norm)
        x = x.float()
        rs = torch.rsqrt(ss[:, None] / x.shape[1] + c.eps) if ss is not None else 1.0
        if mut == f"drop_kstep:{stage}":
            x = x.clone()
            x[:, 32:64] = 0
        return (x @ w.float().T) * rs

    inv = torch.exp2(-math.log2(c.rope_theta) * 2 * torch.arange(half, dtype=torch.float32) / D)
    ang = pos.float()[:, None, None] * inv[None, None, :]
    cs, sn = torch.cos(ang), torch.sin(ang)
    sn2 = -sn if mut == "rope_sign" else sn
    caches = [(inp.kc0.clone(), inp.vc0.clone()) for _ in range(c.n_layers)]
    ss_down = ss_o = raw = None
    r2 = W[0][inp.tokens]
    for L in range(c.n_layers):
        late = L > 0

        def entry(name, slipped):  # this layer's table entry, or layer 0's under the slip that names it
            return layer_w(c, W, 0 if late and slip == slipped else L, name)

        x0 = r2
        ss = sumsq(x0)  # layer 0: k_embed's one partial
        if late:  # the previous down projection's partials
            ss = (ss_down[:, :32 * plan.qkv.nw] if slip == "late_loop" else ss_down).sum(1)
            if slip == "stale_ss":
                ss = ss_o
        y = gemm("qkv", x0, entry("wqkv", "table:wqkv"), ss)
        if c.qkv_bias:
            y = y + entry("bqkv", "table:bias").float()[None, :]
        if c.qk_norm:  # STORE, then k_qknorm_rope: plain row order, RoPE partners d and d + D/2
            raw = y.to(BF)
            xh = raw.float().view(B, H + 2 * Hkv, D)
            g = torch.cat([entry("q_norm", "table:qk_norm").float().expand(H, D), entry("k_norm", "table:qk_norm").float().expand(Hkv, D)])
            n = xh[:, :H + Hkv] * torch.rsqrt(xh[:, :H + Hkv].pow(2).sum(-1, keepdim=True) / D + c.eps) * g[None]
            x1, x2 = n[..., :half], n[..., half:]
            v = xh[:, H + Hkv:].to(BF)
        else:
            y = bf32(y).view(B, H + 2 * Hkv, half, 2)
            x1, x2 = y[:, :H + Hkv, :, 0], y[:, :H + Hkv, :, 1]
            v = torch.cat([y[:, H + Hkv:, :, 0], y[:, H + Hkv:, :, 1]], -1).to(BF)
        qk = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn2], -1).to(BF)
        q = qk[:, :H].contiguous()
        kc, vc = caches[0 if late and slip == "kv_into_layer0" else L]
        kc[sl, pos], vc[sl, pos] = qk[:, H:], v
        kc, vc = caches[0 if late and slip == "attend_layer0" else L]
        attn = _emulate_attn(case, q, kc, vc, mut)

        r1 = bf32(x0.float() + bf32(gemm("o", attn, layer_w(c, W, L, "wo")))).to(BF)
        ss_o = sumsq(r1)
        gu = bf32(gemm("gate_up", r1, layer_w(c, W, L, "w_gate_up"), ss_o)).view(B, c.ffn, 2)
        g_, u_ = (gu[..., 1], gu[..., 0]) if mut == "swap_gate_up" else (gu[..., 0], gu[..., 1])
        h = (g_ / (1 + torch.exp(-g_)) * u_).to(BF)
        r2 = bf32(r1.float() + bf32(gemm("down", h, layer_w(c, W, L, "w_down")))).to(BF)
        ss_down = partials(r2)
    logits = gemm("lm_head", r2[:emit], W[2], sumsq(r2[:emit])).to(BF)
    kc, vc = caches[-1]
    return {"q": q, "kc": kc, "vc": vc, "attn": attn, "r1": r1, "h": h, "r2": r2, "logits": logits,
            "ids": first_argmax(logits), "x0": x0, "caches": caches, "ss2": partials(r1).T, "ss3": ss_down.T,
            "qkv": raw}


def _emulate_attn(case, q, kc, vc, mut):
    """``emulate``'s attention: every row over positions 0..pos[row] of its slot, one span slot at a time."""
    inp = inputs(case)
    c, B = case.cfg, case.rows
    H, Hkv, D = c.n_heads, c.n_kv_heads, c.head_dim
    G = H // Hkv
    sl = inp.slots.long() if inp.slots is not None else torch.arange(B)
    pos = inp.pos.long()
    ns = step_plan(case).attn.slots
    scale = torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32)
    attn = torch.empty(B, H * D, dtype=BF)
    for b in range(B):
        n = int(pos[b]) + 1
        if mut == "one_token_short":
            n = max(1, n - 1)
        K, V = kc[sl[b], :n].float(), vc[sl[b], :n].float()
        s = torch.einsum("hgd,lhd->hgl", q[b].float().view(Hkv, G, D), K) * scale
        span = ops.attn_span(n, ns)
        ms, ls, os_ = [], [], []
        for s0 in range(0, n, span):  # one span slot: its own maximum, sum and weighted V
            seg = s[..., s0:s0 + span]
            m = seg.amax(-1, keepdim=True)
            e = torch.exp(seg - m)
            ms.append(m)
            ls.append(e.sum(-1, keepdim=True))
            os_.append(torch.einsum("hgl,lhd->hgd", e, V[s0:s0 + span]))
        m_all = torch.stack(ms).amax(0)
        ww = [torch.exp(m - m_all) for m in ms]
        if mut == "wrong_split_max" and len(ms) > 1:
            ww[1] = torch.exp(ms[0] - m_all)
        L = sum(w_ * l for w_, l in zip(ww, ls))
        o = sum(w_ * o_ for w_, o_ in zip(ww, os_))
        attn[b] = (o / L).reshape(H * D).to(BF)
    return attn


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_fp32_emulation_stays_inside_the_bounds(case):
    # The inputs and the bounds are consistent without the kernel: fp32 arithmetic with the same rounding
    # points, in whatever order torch sums, must pass every stage.
    ratios = stage_ratios(case, inputs(case).weights, emulate(case))
    print("EMU", case.name, {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios


# A GEMM-stage case, a ragged 16-slot attention case and a one-slot case with a row->slot map.
MUT_CASES = [c for c in CASES if c.name in ("gemm-d256-f352-r3", "attn-ragged-D64-G2", "attn-A-D128-G4")]


# A launch with one span slot has no split partials to weight wrongly.
MUT_PARAMS = [pytest.param(c, m, id=f"{c.name}-{m}") for c in MUT_CASES for m in MUTATIONS
              if not (m == "wrong_split_max" and step_plan(c).attn.slots == 1)]


@pytest.mark.parametrize("case,mut", MUT_PARAMS)
def test_perturbed_emulation_violates_the_bounds(case, mut):
    # The bounds bite: one arithmetic slip in the emulation leaves the bound of the stage it hits.
    ratios = stage_ratios(case, inputs(case).weights, emulate(case, mut))
    hit = MUTATIONS[mut]
    assert max(ratios[s] for s in hit) > 1.0, ratios
    # ... and no stage downstream of it: each is judged from its own observed inputs.
    clean = {s: r for s, r in ratios.items() if s not in hit and s != "ids"}
    assert max(clean.values()) <= 1.0, ratios


# ---------------------------------------------------------------- the plan (CPU: the library, no device)
# What each case launches (qkv, attn, o, gate_up, down, lm_head), from the Python copy of the host rules that this
# module held before the library exported its plan (cross-checked against the list in the commit that added the
# cases). A literal: a change to a heuristic that moves a case off its instantiation fails here.
_G = ("<4,1,ROPE,2>", "<4,1,SILU,2>", "<4,2,ARGMAX,2>")
_W = ("<8,1,ROPE,4>", "<8,1,SILU,4>", "<4,2,ARGMAX,4>")


def _row(attn, o, down, three=_G):
    return (three[0], attn, o, three[1], down, three[2])


EXPECTED_PLAN = {
    **{f"gemm-d256-f512-r{r}": _row("k_attn<64,2> 1 slots", "<4,1,RESID,1> kp4", "<4,1,RESID,1> kp4") for r in (1, 4)},
    **{f"gemm-d256-f512-r{r}": _row("k_attn<64,2> 1 slots", "<4,1,RESID,2>", "<4,1,RESID,4>") for r in (5, 16, 17, 64)},
    "gemm-d256-f352-r3": _row("k_attn<64,2> 1 slots", "<4,1,RESID,1> kp4", "<4,1,RESID,4>"),
    "gemm-d256-f2816-r5": _row("k_attn<64,2> 1 slots", "<4,1,RESID,2>", "<8,1,RESID,4>"),
    "gemm-d1536-f1152-r2": _row("k_attn<64,2> 1 slots", "<4,1,RESID,1> kp4", "<4,1,RESID,4> kp4", _W),
    "gemm-d2048-r8": _row("k_attn<128,4> 1 slots", "<8,1,RESID,4> kp2", "<4,1,RESID,2> kp2", _W),
    "gemm-d2048-r9": _row("k_attn<128,4> 1 slots", "<8,1,RESID,4>", "<4,1,RESID,4>", _W),
    "ids-dup-head": _row("k_attn<64,2> 1 slots", "<4,1,RESID,2>", "<4,1,RESID,4>"),
    "ids-emit3of5": _row("k_attn<64,2> 1 slots", "<4,1,RESID,2>", "<4,1,RESID,4>"),
    # ragged: O has K = 2 G D, so its load batch grows with G and D
    **{f"attn-ragged-D{D}-G{G}": _row(f"k_attn<{D},{G}> 16 slots", f"<4,1,RESID,{um}> kp4", "<4,1,RESID,1> kp4")
       for D, G, um in ((64, 1, 1), (64, 2, 1), (64, 4, 1), (64, 8, 2), (128, 1, 1), (128, 2, 1), (128, 4, 2),
                        (128, 8, 4))},
    **{f"attn-{k}-D{D}-G{G}": _row(f"k_attn<{D},{G}> {n} slots", "<8,1,RESID,4>", "<4,1,RESID,2>")
       for k, n in (("A", 1), ("B", 2), ("C", 1)) for D in (64, 128) for G in (4, 8)},
}

# The instantiations the cases launch between them, K parts told apart: 14 k_skinny variants and all 8 k_attn.
EXPECTED_COVERAGE = {
    "<4,1,ROPE,2>", "<8,1,ROPE,4>", "<4,1,SILU,2>", "<8,1,SILU,4>", "<4,2,ARGMAX,2>", "<4,2,ARGMAX,4>",
    "<4,1,RESID,1> kp4", "<4,1,RESID,2>", "<4,1,RESID,2> kp2", "<4,1,RESID,2> kp4", "<4,1,RESID,4>",
    "<4,1,RESID,4> kp4", "<8,1,RESID,4>", "<8,1,RESID,4> kp2",
    *(f"k_attn<{D},{G}>" for D in (64, 128) for G in (1, 2, 4, 8)),
}


def _dims(dim, ffn, H, Hkv, D, max_seq, vocab=VOCAB, max_batch=64):
    return ops.LlamaDims(vocab=vocab, dim=dim, n_layers=2, H=H, Hkv=Hkv, D=D, ffn=ffn, max_seq=max_seq,
                         max_batch=max_batch, eps=1e-5, theta=1e4)


def _shape(p):
    return (p.nw, p.tn, p.um, 1 << p.kpl, p.grid_x, p.grid_y)


def test_plan_of_every_case_is_the_recorded_one():
    assert set(EXPECTED_PLAN) == set(CASE_IDS)
    for case in CASES:
        assert plan_strings(step_plan(case)) == EXPECTED_PLAN[case.name], case.name


def test_plan_of_the_small_config():
    # dim 2048, 16 heads of 128 over 4 KV heads, ffn 5632, vocab 32000: by hand from the rules. 64 k-steps (K 2048)
    # or 176 (K 5632) are above 16, so 8 waves with load batches of 4; the 2048-wide O and down have 128 16-column
    # tiles, below the 256 CUs, and 256 8-column ones: 2 K parts while rows * 2 <= 16.
    small = _dims(2048, 5632, 16, 4, 128, 4096, vocab=32000, max_batch=17)
    p = ops.step_plan(small, 1)
    assert _shape(p.qkv) == _shape(p.qkv_first) == (8, 1, 4, 1, 192, 1)
    assert _shape(p.o) == (8, 1, 4, 2, 256, 1)
    assert _shape(p.gate_up) == (8, 1, 4, 1, 704, 1)
    assert _shape(p.down) == (8, 1, 4, 2, 256, 1)
    assert _shape(p.lm_head) == (4, 2, 4, 1, 1000, 1)
    assert (p.gate_up.ss_in, p.lm_head.ss_in, p.qkv.ss_in, p.qkv_first.ss_in) == (256, 256, 256, 1)
    assert (p.o.ss_in, p.down.ss_in, p.am_parts) == (0, 0, 1000)
    assert (p.attn.D, p.attn.G, p.attn.slots, p.attn.stride, p.attn.grid_y) == (128, 4, 16, 16, 4)
    p = ops.step_plan(small, 9)
    assert _shape(p.o) == _shape(p.down) == (8, 1, 4, 1, 128, 1)
    assert ops.step_plan(small, 16).attn.slots == 4
    assert ops.lib().p2pt_llama_ws_bytes(small) == 10_674_176


def test_cases_cover_the_instantiations_they_claim():
    got = set()
    for case in CASES:
        p = step_plan(case)
        got |= {fmt(getattr(p, s)) for s in STAGES if s != "attn"} | {fmt(p.attn).split(" ")[0]}
    assert got == EXPECTED_COVERAGE


def _ws_counts(dims):
    n = len(ops.FusedLlamaDecoder._WS_BUFFERS)
    off, cnt = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
    assert ops.lib().p2pt_llama_ws_layout(dims, off, cnt, n) == n
    return {name: c for (name, _), c in zip(ops.FusedLlamaDecoder._WS_BUFFERS, cnt)}


def test_plan_invariants_over_a_sweep():
    # Every 3rd of the 640 combinations (3 shares no factor with 5, 4, 2, 4, 4, so each value of each axis and
    # every pair occurs) times 64 row counts times 3 emit_rows: 41,088 plans.
    grid = [(dim, ffn, D, G, S) for dim in (256, 1024, 1536, 2048, 4096) for ffn in (352, 512, 2816, 5632)
            for D in (64, 128) for G in (1, 2, 4, 8) for S in (64, 512, 2048, 4096)][::3]
    M = ops.MAX_ROWS
    for dim, ffn, D, G, S in grid:
        dims = _dims(dim, ffn, 2 * G, 2, D, S)
        count = _ws_counts(dims)
        for B in range(1, M + 1):
            for emit in (0, 1, B):
                p = ops.step_plan(dims, B, emit)
                assert (p.rows, p.emit_rows) == (B, emit or B)
                gemms = {s: getattr(p, s) for s in ("qkv_first", "qkv", "o", "gate_up", "down", "lm_head")}
                for name, g in gemms.items():
                    rows = p.emit_rows if name == "lm_head" else B
                    assert g.M == rows and g.nw in (4, 8) and g.um in (1, 2, 4), (name, B)
                    assert g.grid_x * g.tn * (16 >> g.kpl) == g.N and g.grid_y == -(-g.M // 16), (name, B)
                    if g.kpl:
                        assert g.tn == 1 and (g.M << g.kpl) <= 16 and g.K % (32 << g.kpl) == 0, (name, B)
                    assert g.ss_in * M <= count["ss"]
                assert p.qkv.kpl == p.gate_up.kpl == p.lm_head.kpl == 0  # K parts on O and down only
                # a consumer reads exactly the partials its producer wrote
                assert (p.qkv_first.ss_in, p.o.ss_in, p.down.ss_in) == (1, 0, 0)
                assert p.gate_up.ss_in == p.o.grid_x
                assert p.qkv.ss_in == p.lm_head.ss_in == p.down.grid_x
                assert p.am_parts == p.lm_head.grid_x
                # ... and everything fits its workspace buffer
                assert max(p.o.grid_x, p.down.grid_x) * M <= count["ss"]
                assert p.am_parts * M <= count["am_val"] == count["am_idx"]
                a = p.attn
                assert (a.D, a.G, a.grid_y) == (D, G, B * 2) and 1 <= a.slots <= a.stride
                assert M * dims.H * a.stride * D <= count["part_o"]


# The six model families by their LlamaDims flags (qkv_bias + qk_norm is refused: no family has both).
FAMILIES = {
    "plain": {}, "bias": {"qkv_bias": 1}, "table": {"rope_table": 1}, "bias+table": {"qkv_bias": 1, "rope_table": 1},
    "qk_norm": {"qk_norm": 1}, "qk_norm+table": {"qk_norm": 1, "rope_table": 1},
}
RESTRICTED_PAIRS = {(4, 1), (4, 2), (4, 4), (8, 4)}  # (nw, um) of a table or FP8-cache RoPE epilogue's k_skinny


def _gqa_dims(G, D=64, dim=256, **flags):
    dims = _dims(dim, 512, 2 * G, 2, D, 512)
    for name, value in flags.items():
        setattr(dims, name, value)
    return dims


def test_every_plan_names_an_instantiated_kernel():
    # dim 32 to 8192 is 1 to 256 k-steps on QKV and gate/up, so every (nw, um) branch of plan_gemm: (4, 1) at 1 and
    # 2 k-steps, (4, 2) at 8, (4, 4) at 16, (8, 4) from 17 (dim 544) on. (8, 1) and (8, 2) need 8 waves with at
    # most 2 k-steps each, which the 17-step threshold rules out; the table and FP8-cache epilogues have neither.
    from p2p_llm_tunnel_amd.models.checkpoint import _GQA_RATIOS
    met = set()
    accepted = 0
    for (family, flags), kv_fp8 in itertools.product(FAMILIES.items(), (0, 1)):
        for D, G, dim in itertools.product((64, 128), _GQA_RATIOS, (32, 64, 256, 512, 544, 1024, 2048, 4096, 8192)):
            dims = _gqa_dims(G, D, dim, kv_fp8=kv_fp8, **flags)
            for B in (1, 2, 4, 5, 16, 17, 64):
                for emit in sorted({0, 1, B}):
                    try:
                        p = ops.step_plan(dims, B, emit)
                    except ValueError:
                        continue
                    accepted += 1
                    assert ops.plan_kernels_ok(dims, B, emit), (family, kv_fp8, D, G, dim, B, emit)
                    if "qk_norm" not in flags and (kv_fp8 or "rope_table" in flags):
                        assert p.qkv.epi >= 6, (family, kv_fp8)  # a table or _KV8 RoPE epilogue
                        met |= {(p.qkv.nw, p.qkv.um), (p.qkv_first.nw, p.qkv_first.um)}
    assert accepted == 12 * 2 * len(_GQA_RATIOS) * 9 * (2 + 6 * 3)  # step_plan refused none of them
    assert met == RESTRICTED_PAIRS


def test_gqa_ratios_outside_the_set_are_refused():
    for D in (64, 128):
        for G in (3, *range(9, 17)):
            with pytest.raises(ValueError):
                ops.step_plan(_gqa_dims(G, D), 1)
            with pytest.raises(ValueError):
                ops.plan_kernels_ok(_gqa_dims(G, D), 1)


def test_the_loader_and_the_plan_accept_the_same_gqa_ratios():
    from p2p_llm_tunnel_amd.models.checkpoint import _GQA_RATIOS

    def accepts(G):
        try:
            ops.step_plan(_gqa_dims(G), 1)
        except ValueError:
            return False
        return True

    assert {G for G in range(1, 17) if accepts(G)} == set(_GQA_RATIOS)


def test_plan_refuses_what_the_step_refuses():
    ok = _dims(256, 512, 4, 2, 64, 64)
    bad = [_dims(256, 512, 4, 2, 96, 64), _dims(256, 512, 6, 2, 64, 64), _dims(48, 512, 4, 2, 64, 64),
           _dims(256, 520, 4, 2, 64, 64), _dims(256, 512, 4, 2, 64, 64, vocab=500), _dims(256, 512, 4, 2, 64, 0),
           _dims(256, 512, 4, 2, 64, 64, max_batch=0), _dims(256, 512, 4, 2, 64, 64, vocab=1 << 23)]
    out = ops.StepPlan()
    for dims in [ok] + bad:
        supported = ops.lib().p2pt_llama_ws_bytes(dims) != 0
        assert supported == (dims is ok)
        for B in (-1, 0, 1, 16, ops.MAX_ROWS, ops.MAX_ROWS + 1):
            rc = ops.lib().p2pt_llama_plan(dims, B, 0, out)
            assert (rc == 0) == (supported and 1 <= B <= ops.MAX_ROWS), (B, rc)
            if rc:
                with pytest.raises(ValueError):
                    ops.step_plan(dims, B)


def test_attn_span_rule():
    for slots in range(1, 17):
        for n in range(1, 4097):
            span = ops.attn_span(n, slots)
            assert span == max(64, -(-(-(-n // slots)) // 32) * 32), (n, slots)
            assert -(-n // span) <= slots, (n, slots)  # the slots with tokens never exceed the grid


# ---------------------------------------------------------------- the kernels (GPU)
def observe_gpu(case):
    """Run the step on the device and read every intermediate back (CPU tensors)."""
    inp = inputs(case)
    B = case.rows
    m = TinyLlama(case.cfg, device="cuda", max_batch=case.max_batch, seed=case.seed)
    if case.dup_head:
        _dup_head(m)
    m.k_cache[0].copy_(inp.kc0)
    m.v_cache[0].copy_(inp.vc0)
    dec = m.fused_decoder()
    views = dec.workspace_views()
    tokens, pos = inp.tokens.cuda(), inp.pos.cuda()
    slots = inp.slots.cuda() if inp.slots is not None else None
    logits = torch.empty(B, case.cfg.vocab, dtype=BF, device="cuda")
    ids = torch.empty(B, dtype=torch.int64, device="cuda")

    def run():
        logits.view(torch.int16).fill_(SENTINEL_BITS)
        ids.fill_(SENTINEL_ID)
        dec.step(tokens, pos, logits, ids, slots, case.emit_rows)
        torch.cuda.synchronize()
        return {k: views[k][:B].cpu() for k in ("q", "attn", "h", "resid")}

    # Pass 1 with w_down (passed to the kernel as is) zeroed: the final residual is the post-O residual.
    w_down = dec.weights[dec.table.index("w_down", 0)]
    saved = w_down.clone()
    w_down.zero_()
    first = run()
    w_down.copy_(saved)
    second = run()
    for k in ("q", "attn", "h"):  # the step is deterministic: both passes saw the same inputs
        assert torch.equal(first[k], second[k]), k
    obs = {"q": second["q"], "attn": second["attn"], "h": second["h"], "r1": first["resid"], "r2": second["resid"],
           "kc": m.k_cache[0].cpu(), "vc": m.v_cache[0].cpu(), "logits": logits.cpu(), "ids": ids.cpu()}
    return obs, [w.cpu() for w in dec.weights]


@cuda
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_fused_stages_match_fp64(case):
    inp = inputs(case)
    obs, W = observe_gpu(case)
    for a, b in zip(W, inp.weights):  # the decoder's own table is what the references use
        assert torch.equal(a, b)
    ratios = stage_ratios(case, W, obs)
    print("RATIO", case.name, {k: round(v, 3) for k, v in ratios.items()}, "PLAN", plan_strings(step_plan(case)))
    assert max(ratios.values()) <= 1.0, ratios
    if case.dup_head:  # every maximum ties 64 times over: the first of them is one of the 8 distinct rows
        assert int(obs["ids"].max()) < 8, obs["ids"]

    # The step appended exactly one K and one V row per token row and touched nothing else in the cache.
    sl = inp.slots.long() if inp.slots is not None else torch.arange(case.rows)
    for got, before in ((obs["kc"], inp.kc0), (obs["vc"], inp.vc0)):
        same = got.view(torch.int16) == before.view(torch.int16)
        same[sl, inp.pos.long()] = True
        assert bool(same.all())
    # Rows at or past emit_rows keep what logits and ids held before the step.
    emit = case.emit_rows or case.rows
    assert bool((obs["logits"][emit:].view(torch.int16) == SENTINEL_BITS).all())
    assert bool((obs["ids"][emit:] == SENTINEL_ID).all())
