"""Byte-exact FP8 (e4m3) KV appends at the hidden sizes models are served at, and on layer 1.

tests/test_gpu_kv_fp8.py compares every stored byte with fp64 at hidden size 64 only: ``gemm_ref``'s accumulation
bound (K + 16) U sum|x||w| grows with K until a third of the elements lie within e_pre of an e4m3 rounding boundary
(``test_random_inputs_leave_too_much_undecided``). This module removes the accumulation term instead of widening
anything: the inputs are chosen so that fp32 accumulation is exact in any order, and the value before the one
rounding is then known to 8 U at any K (``gemm_ref_exact``). ``judge``, the rotation and cos / sin terms, the
attention reference and the 1 % cap on undecided elements are the existing modules', unchanged.

Exact inputs. ``embed`` rows are integers in [-3, 3], ``attn_norm`` is all ones (folding it into wqkv is exact) and
wqkv entries are integers in [-3, 3] times 2^-4; ``gemm_ref_exact`` asserts what it relies on from the decoder's own
folded table and the actual rows. A few pair-aligned K and V columns of head 0 carry another power of two (the
grid precondition is per column): 2^b with b = 6 at hidden size 4096 and as much more below it as keeps the value's
spread at 512 or above (2^6 alone leaves a value of spread sqrt(K) / 8 short of 448 from K = 1024 down), 2^-9 and
2^-13. Bias families plant exact values through the bias over zeroed weight rows, as tests/test_gpu_kv_fp8.py does.
Every case then holds decided elements beyond 448, below 2^-6, below 2^-10 (a signed zero) and ordinary ones, and
the bias families one inside (448, 464); NaN is planted in two bias cases, which do not judge attention. A QK-norm
model gets its K classes through the k_norm weight. q is scaled to a spread below 1 and is zero where K head 0 is
scaled up or planted, so the scores stay moderate (``exact_model`` says why).

Cases. One layer and one step at hidden sizes 256 (<4,1,.,2>), 512 (<4,1,.,4>: 16 k-steps, the last 4-wave shape)
and 544, 1536, 2048, 2816, 4096 (<8,1,.,4>: 17 k-steps in shares of 2 and 3; 6 per wave: a load batch of 4 and one
of 2; 8; 11: 4, 4, 3; 16), every _KV8 epilogue at each shape, rows 1, 16, 17, 40 and 64 in ``layout``'s mix; a
QK-norm case per head size at 2048 (EPI_STORE, whose raw projection is held to 8 U too, then ``k_qknorm_rope<D,
TAB, true>``). Two-layer models at hidden size 2048 (plain, bias, QK-norm with and without a table) zero layer 0's
wo and w_down, so layer 1 reads the embedding row again (asserted from the workspace, with the sum-of-squares
partials, after a pass with layer 1's wo and w_down zeroed in place) through the down projection's partials, its
own weight-table entries and the byte offset L * layer_cache; the whole cache tensor is compared byte for byte.

CPU tests hold an fp32 emulation with the kernel's rounding points to the same checks on every case (the cap is
met by the reference alone; a shuffled summation order gives the same bits, which is the precondition at work) and
apply one slip at a time, each of which changes a decided byte or leaves a bound.

Seen on an MI355X (printed by each case as a RATIO kv8-wide line; recorded, not asserted): over the 26 cases no
decided byte differed, K ratios 0.994 .. 1.000 and V ratios 0.986 .. 1.000 (layer 0 of the two-layer cases included;
an element next to a tie sits just under 1), q 0.980 .. 1.000, the raw projection of the QK-norm cases 0.999,
attention 0.832 .. 0.979; undecided K 0 .. 0.69 % and V 0 .. 0.10 % of a case's elements, together at most 0.35 %
of a case (the CPU emulation leaves the same shares: they are the reference's). A case takes 0.1 to 0.3 s.
"""
import functools
import math
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig, TinyLlama, llama_dims
from p2p_llm_tunnel_amd.utils import kv_fp8_ref as ref
from test_gpu_fused_stages import BF, F64, U, bf64, flip, layer_w, rounded, stage_attn, table_layout, worst
from test_gpu_kv_fp8 import (EPS, F8, N_SLOTS, NAN_BYTE, PLANTS, SCALING, angles, appended_reference, decoded,
                             judge_rows, layout, rotate)
from test_gpu_qk_norm import RN
from test_kv_fp8 import SLIPS, rne64, store

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu

F32 = torch.float32
CAP = 0.01  # undecided share of a case's appended K and V elements together, at most
EPI_NAMES = {0: "STORE", 1 + 8: "ROPE_KV8", 5 + 8: "ROPE_BIAS_KV8", 6 + 8: "ROPE_TAB_KV8", 7 + 8: "ROPE_BIAS_TAB_KV8"}
KIND_EPI = {"plain": "ROPE_KV8", "bias": "ROPE_BIAS_KV8", "table": "ROPE_TAB_KV8", "bias_table": "ROPE_BIAS_TAB_KV8",
            "qk_norm": "STORE", "qk_norm_table": "STORE"}


@dataclass(frozen=True)
class Case:
    kind: str
    dim: int
    D: int
    rows: int
    smax: int
    seed: int = 0
    nan: bool = False
    layers: int = 1
    plant = False  # ``layout``: the ordinary mix of single rows and prefill chunks

    @property
    def name(self):
        return (f"{self.kind}-dim{self.dim}-D{self.D}-r{self.rows}-s{self.smax}" + ("-nan" if self.nan else "")
                + ("-layer1" if self.layers == 2 else ""))

    @property
    def heads(self):  # (H, Hkv): H + 2 Hkv small, G = 2
        return (2, 1) if self.D == 128 else (4, 2)

    @property
    def cfg(self):
        H, Hkv = self.heads
        return LlamaConfig(vocab=512, dim=self.dim, n_layers=self.layers, n_heads=H, n_kv_heads=Hkv, head_dim=self.D,
                           ffn=64, max_seq=self.smax, eps=EPS, rope_theta=1e4,
                           rope_scaling=SCALING if "table" in self.kind else None, qkv_bias="bias" in self.kind,
                           qk_norm="qk_norm" in self.kind)


# (kind, hidden size, D, rows, max_seq). Every epilogue gets 256, 512, 544, one of 1536 / 2816 (a ragged last load
# batch) and one of 2048 / 4096; rows 1, 16, 17, 40 and 64 occur at 4-wave and at 8-wave shapes; positions stay
# below 1024 (dsc grows with the angle).
_C = [("plain", 256, 64, 17, 128), ("plain", 512, 128, 1, 1024), ("plain", 544, 64, 64, 64),
      ("plain", 1536, 128, 40, 1024), ("plain", 4096, 64, 16, 128),
      ("bias", 256, 128, 40, 96), ("bias", 512, 64, 16, 1024), ("bias", 544, 128, 17, 128),
      ("bias", 2816, 64, 1, 1024), ("bias", 2048, 128, 64, 64),
      ("table", 256, 64, 16, 64), ("table", 512, 128, 64, 128), ("table", 544, 64, 1, 64),
      ("table", 2816, 128, 17, 96), ("table", 4096, 128, 40, 1024),
      ("bias_table", 256, 128, 1, 1024), ("bias_table", 512, 64, 17, 64), ("bias_table", 544, 128, 16, 1024),
      ("bias_table", 1536, 64, 64, 128), ("bias_table", 2048, 64, 40, 96),
      ("qk_norm", 2048, 128, 40, 128), ("qk_norm_table", 2048, 64, 17, 1024)]
NAN_CASES = {("bias", 544), ("bias_table", 512)}  # NaN through the bias: these two judge the appended rows only
CASES = [Case(*c, seed=i + 1, nan=(c[0], c[1]) in NAN_CASES) for i, c in enumerate(_C)]
# Layer 1 of two-layer models: max_seq 96 and 10 slots, so a layer's cache is 10 * 96 * Hkv * D = 122,880 bytes,
# which is neither a power of two nor the size of any other axis product a mistaken offset could use.
LAYER_CASES = [Case(kind, 2048, D, rows, 96, seed=50 + i, layers=2)
               for i, (kind, D, rows) in enumerate((("plain", 128, 17), ("bias", 64, 40), ("qk_norm_table", 128, 16),
                                                    ("qk_norm", 64, 5)))]
ALL = CASES + LAYER_CASES
IDS = [c.name for c in ALL]


def dims_of(case):
    """The LlamaDims ``TinyLlama.fused_decoder`` builds for the case's model (max_batch = N_SLOTS, an FP8 cache)."""
    return llama_dims(case.cfg, N_SLOTS + 1, kv_fp8=True)


def plan_of(case):
    """(the QKV instantiation, k_attn's, k_qknorm_rope's or None) as the library plans them: never a copy of its rules."""
    d = dims_of(case)
    p, kv = ops.step_plan(d, case.rows), ops.kv_plan(d)
    assert (p.qkv.epi, p.qkv.nw, p.qkv.tn, p.qkv.um) == (p.qkv_first.epi, p.qkv_first.nw, p.qkv_first.tn, p.qkv_first.um)
    assert kv.attn_kv8 == 1 and kv.qk_norm_kv8 == int(case.cfg.qk_norm) and p.qkv.kpl == 0
    qkv = f"<{p.qkv.nw},{p.qkv.tn},{EPI_NAMES[p.qkv.epi]},{p.qkv.um}>"
    attn = f"k_attn<{p.attn.D},{p.attn.G},true> {p.attn.slots} slots"
    qkn = f"k_qknorm_rope<{case.D},{'true' if p.qk_norm_table else 'false'},true>" if p.qk_norm_grid else None
    return qkv, attn, qkn


# What each case launches: a literal, so a heuristic that moves a case off its instantiation fails here.
def _p(nw, um, slots, tab=None):
    return nw, um, slots, tab


EXPECTED_PLAN = {
    "plain-dim256-D64-r17-s128": _p(4, 2, 2), "plain-dim512-D128-r1-s1024": _p(4, 4, 16),
    "plain-dim544-D64-r64-s64": _p(8, 4, 1), "plain-dim1536-D128-r40-s1024": _p(8, 4, 6),
    "plain-dim4096-D64-r16-s128": _p(8, 4, 2),
    "bias-dim256-D128-r40-s96": _p(4, 2, 2), "bias-dim512-D64-r16-s1024": _p(4, 4, 8),
    "bias-dim544-D128-r17-s128-nan": _p(8, 4, 2), "bias-dim2816-D64-r1-s1024": _p(8, 4, 16),
    "bias-dim2048-D128-r64-s64": _p(8, 4, 1),
    "table-dim256-D64-r16-s64": _p(4, 2, 1), "table-dim512-D128-r64-s128": _p(4, 4, 2),
    "table-dim544-D64-r1-s64": _p(8, 4, 1), "table-dim2816-D128-r17-s96": _p(8, 4, 2),
    "table-dim4096-D128-r40-s1024": _p(8, 4, 6),
    "bias_table-dim256-D128-r1-s1024": _p(4, 2, 16), "bias_table-dim512-D64-r17-s64-nan": _p(4, 4, 1),
    "bias_table-dim544-D128-r16-s1024": _p(8, 4, 16), "bias_table-dim1536-D64-r64-s128": _p(8, 4, 2),
    "bias_table-dim2048-D64-r40-s96": _p(8, 4, 2),
    "qk_norm-dim2048-D128-r40-s128": _p(8, 4, 2, "false"), "qk_norm_table-dim2048-D64-r17-s1024": _p(8, 4, 7, "true"),
    "plain-dim2048-D128-r17-s96-layer1": _p(8, 4, 2), "bias-dim2048-D64-r40-s96-layer1": _p(8, 4, 2),
    "qk_norm_table-dim2048-D128-r16-s96-layer1": _p(8, 4, 2, "true"),
    "qk_norm-dim2048-D64-r5-s96-layer1": _p(8, 4, 2, "false"),
}


def test_plan_of_every_case_is_the_recorded_one():
    assert set(EXPECTED_PLAN) == set(IDS)
    for case in ALL:
        nw, um, slots, tab = EXPECTED_PLAN[case.name]
        H, Hkv = case.heads
        want = (f"<{nw},1,{KIND_EPI[case.kind]},{um}>", f"k_attn<{case.D},{H // Hkv},true> {slots} slots",
                f"k_qknorm_rope<{case.D},{tab},true>" if tab else None)
        assert plan_of(case) == want, case.name


def test_cases_cover_the_instantiations_they_claim():
    # All four _KV8 epilogues at each shape plan_gemm can give a QKV projection beyond <4,1,.,1>: 12 instantiations.
    want = {f"<{nw},1,{epi},{um}>" for epi in ("ROPE_KV8", "ROPE_BIAS_KV8", "ROPE_TAB_KV8", "ROPE_BIAS_TAB_KV8")
            for nw, um in ((4, 2), (4, 4), (8, 4))}
    assert len(want) == 12
    assert {plan_of(c)[0] for c in CASES if "qk_norm" not in c.kind} == want
    by = {}
    for c in CASES:
        by.setdefault(c.kind, set()).add(c.dim)
    for kind in ("plain", "bias", "table", "bias_table"):  # the share patterns of the 8-wave shape, per epilogue
        assert {256, 512, 544} <= by[kind] and by[kind] & {1536, 2816} and by[kind] & {2048, 4096}, kind
    assert set().union(*by.values()) >= {256, 512, 544, 1536, 2048, 2816, 4096}
    assert {c.rows for c in CASES} == {1, 16, 17, 40, 64}
    # One wide QK-norm case per head size, and on layer 1 both table states of the FP8 k_qknorm_rope.
    assert {plan_of(c)[2] for c in CASES if "qk_norm" in c.kind} == {"k_qknorm_rope<128,false,true>",
                                                                      "k_qknorm_rope<64,true,true>"}
    assert {plan_of(c)[2] for c in LAYER_CASES} == {None, "k_qknorm_rope<128,true,true>", "k_qknorm_rope<64,false,true>"}
    assert {plan_of(c)[0] for c in LAYER_CASES} == {"<8,1,ROPE_KV8,4>", "<8,1,ROPE_BIAS_KV8,4>", "<8,1,STORE,4>"}
    for c in LAYER_CASES:  # layer 1's QKV reads the down projection's partials
        p = ops.step_plan(dims_of(c), c.rows)
        assert p.qkv.ss_in == p.down.grid_x > 1 and p.qkv_first.ss_in == 1


# ---------------------------------------------------------------- exact inputs
BIG, SMALL, TINY = range(16, 20), range(20, 24), range(24, 28)  # columns d (and d + D/2) of K head 0 and V head 0


def big_exponent(K):
    """b of the module docstring: a value of the scaled columns has spread 2^b sqrt(K) / 8 >= 512."""
    return 6 + max(0, math.ceil(math.log2(64 / math.sqrt(K))))


def q_exponent(K):
    """The q columns' factor: q has spread sqrt(K) / 8 before it, 0.35 to 0.7 after. See ``exact_model``."""
    return -round(math.log2(math.sqrt(K) / 8)) - 1


def column_scale(case):
    """log2 of the extra factor of every wqkv row (output column), plain q | k | v order."""
    c = case.cfg
    H, Hkv, D, half = c.n_heads, c.n_kv_heads, c.head_dim, c.head_dim // 2
    e = torch.zeros((H + 2 * Hkv) * D, dtype=torch.int32)
    e[:H * D] = q_exponent(c.dim)
    for base in ((H + Hkv) * D,) if c.qk_norm else (H * D, (H + Hkv) * D):  # a QK-norm K is normed: see k_norm
        for cols, s in ((BIG, big_exponent(c.dim)), (SMALL, -9), (TINY, -13)):
            for d in cols:
                e[base + d] = e[base + d + half] = s
    return e


@functools.lru_cache(maxsize=None)
def exact_model(case):
    """The CPU model of a case (module docstring), built with ``TinyLlama.from_weights``.

    The scores are kept moderate, as tests/test_gpu_kv_fp8.py's are: q is scaled to a spread below 1 and is zero in
    the dims where K head 0 carries 448, so a score range stays below about 50. Without that (seen on an MI355X with
    q of spread 8 against K rows of 448: ranges of thousands) the softmax is one-hot, and where the winning token's V
    byte is a zero the fp64 output is 1e-40, the sum of the other tokens' subnormal weights: k_attn's __expf flushes
    those to zero and stores 0.0, while ``stage_attn``'s bound presumes gradual underflow (it allows 5e-41 there).
    Every appended byte was right in those runs; only that attention comparison, which decides nothing at one-hot
    weights, left its bound."""
    c = case.cfg
    H, Hkv, D, half = c.n_heads, c.n_kv_heads, c.head_dim, c.head_dim // 2
    N = (H + 2 * Hkv) * D
    g = torch.Generator().manual_seed(case.seed)

    def ints(*shape):
        return torch.randint(-3, 4, shape, generator=g).to(F32)

    def w(*shape, scale):
        return (torch.randn(*shape, generator=g) * scale).to(BF)

    layers = []
    for L in range(c.n_layers):
        wqkv = torch.ldexp(ints(N, c.dim), column_scale(case)[:, None] - 4).to(BF)
        lw = {"attn_norm": torch.ones(c.dim, dtype=BF), "wqkv": wqkv, "wo": w(c.dim, H * D, scale=(H * D) ** -0.5),
              "ffn_norm": (1.0 + 0.1 * torch.randn(c.dim, generator=g)).to(BF),
              "w_gate_up": w(2 * c.ffn, c.dim, scale=c.dim ** -0.5), "w_down": w(c.dim, c.ffn, scale=c.ffn ** -0.5)}
        for h in range(H):  # q is zero where K head 0 is scaled up or planted (with its bias and q_norm weight, below)
            for d in [*BIG, *(range(len(PLANTS)) if c.qkv_bias else ())]:
                lw["wqkv"][h * D + d] = 0
                lw["wqkv"][h * D + d + half] = 0
        if c.n_layers == 2 and L == 0:  # layer 1 then reads the embedding row: bf(r + bf(0)) = r, twice
            lw["wo"].zero_()
            lw["w_down"].zero_()
        if c.qkv_bias:  # ordinary values, and exact plants over zeroed weight rows in columns 0.. of K and V head 0
            lw["bqkv"] = w(N, scale=1.0)
            lw["bqkv"][:H * D] *= 0.25
            for d in [*BIG, *range(len(PLANTS))]:
                lw["bqkv"][:H * D].view(H, D)[:, [d, d + half]] = 0
            for j, val in enumerate(PLANTS if case.nan else PLANTS[:-1]):
                for base in (H * D, (H + Hkv) * D):
                    for d in (j, j + half):
                        lw["wqkv"][base + d] = 0
                        lw["bqkv"][base + d] = val
        if c.qk_norm:
            for n in ("q_norm", "k_norm"):
                lw[n] = (0.5 + torch.rand(D, generator=g)).to(BF)
            for cols, val in ((BIG, 512.0), (SMALL, 2.0 ** -9), (TINY, 2.0 ** -13)):
                for d in cols:
                    lw["k_norm"][d] = lw["k_norm"][d + half] = val
            for d in BIG:
                lw["q_norm"][d] = lw["q_norm"][d + half] = 0
        layers.append(lw)
    weights = dict(embed=ints(c.vocab, c.dim).to(BF), final_norm=(1.0 + 0.1 * torch.randn(c.dim, generator=g)).to(BF),
                   lm_head=w(c.vocab, c.dim, scale=c.dim ** -0.5), layers=layers)
    return TinyLlama.from_weights(c, weights, device="cpu", max_batch=N_SLOTS, kv_dtype="fp8")


@dataclass
class Inputs:
    model: TinyLlama  # on the CPU
    weights: list  # its fused weight table
    tokens: torch.Tensor
    pos: torch.Tensor
    slots: torch.Tensor
    kc0: torch.Tensor  # uint8 [n_layers, N_SLOTS + 1, smax, Hkv, D]: the caches before the step
    vc0: torch.Tensor


@functools.lru_cache(maxsize=None)
def inputs(case) -> Inputs:
    """Seeded inputs of a case, made once and shared (never modified). The caches hold e4m3 bytes of N(0, 2.5) K and
    N(0, 1) V values up to each slot's length and NaN bytes (0x7f) beyond it and in unused slots, in every layer."""
    m = exact_model(case)
    g = torch.Generator().manual_seed(1000 + case.seed)
    shape = tuple(m.k_cache.shape)
    kc0 = (torch.randn(shape, generator=g) * 2.5).to(F8).view(torch.uint8)
    vc0 = torch.randn(shape, generator=g).to(F8).view(torch.uint8)
    pos, slots = layout(case)
    length = [0] * shape[1]
    for p, s in zip(pos, slots):
        length[s] = max(length[s], p + 1)
    for s, n in enumerate(length):
        kc0[:, s, n:] = NAN_BYTE
        vc0[:, s, n:] = NAN_BYTE
    tokens = torch.randint(0, case.cfg.vocab, (case.rows,), generator=g)
    return Inputs(m, m.fused_weights(), tokens, torch.tensor(pos, dtype=torch.int32),
                  torch.tensor(slots, dtype=torch.int32), kc0, vc0)


# ---------------------------------------------------------------- the exact reference
def granule(wd):
    """[N]: the largest power of two of which every entry of the column's weight row (fp64 holding bf16 values) is an
    integer multiple; 1 for an all-zero row."""
    m, e = torch.frexp(wd.abs())  # |w| = m 2^e, m in [0.5, 1): m 2^8 is an integer for a bf16 value
    mi = (m * 256).to(torch.int64)
    assert bool((mi.to(F64) == m * 256).all()), "precondition: the weights are bf16 values"
    low = (mi & -mi).to(F64)  # the lowest set bit
    ex = torch.where(mi > 0, e.to(F64) - 8 + torch.log2(low.clamp_min(1)), torch.full_like(low, 1e9)).amin(1)
    return torch.exp2(torch.where(ex > 1e8, torch.zeros_like(ex), ex))


def gemm_ref_exact(x, w, eps):
    """y = (1/rms(x)) x w^T in fp64 and the bound E on the kernel's fp32 value, for inputs whose fp32 accumulation is
    exact. Asserted on the actual tensors (a violated precondition is an error of the test, never a skip):

    * every x[m][k] is an integer, every w[n][k] an integer multiple of its column's granule g_n = 2^-s_n;
    * sum_k |x||w| / g_n < 2^24 for every output element: every partial sum of any subset of the products, in any
      order, is then an integer multiple of g_n below 2^24 g_n, so exactly an fp32 value: the MFMA chain, the sum
      over the waves through LDS and ``gemm_ref``'s (K + 16) U sum|x||w| term are exact;
    * sum_k x^2 < 2^24 for every row: the sum-of-squares partials and their sums are exact integers, and
      ``gemm_ref``'s K / 2 U |y| goes too.

    What is left is the ``if (norm)`` block of k_skinny on exact sums: 1.f / float(K) rounds once (U) and its
    product with ssum once more (U); the eps add rounds once (U), and eps as an fp32 value is off by U eps at most,
    less than U of the sum: 4 U on the argument, which the power -1/2 halves to 2 U; rsqrtf is within 2 ulp = 4 U;
    the one multiply of the exact accumulator adds U. 7 U in all: E = 8 U |y|, the non-accumulation part of
    ``gemm_ref``'s norm term. (The caller adds U |y + b| for a bias add, as ``appended_reference`` does.)"""
    xd, wd = x.to(F64), w.to(F64)
    K = x.shape[1]
    assert bool((xd == xd.round()).all()), "precondition: integer activations"
    g = granule(wd)
    wq = wd / g[:, None]
    assert bool((wq == wq.round()).all()), "precondition: weights on their column's grid"
    assert float((xd.abs() @ wq.abs().T).max()) < 2.0 ** 24, "precondition: sum |x||w| / granule < 2^24"
    ss = xd.pow(2).sum(1, keepdim=True)
    assert float(ss.max()) < 2.0 ** 24, "precondition: sum x^2 < 2^24"
    y = (xd @ wd.T) * torch.rsqrt(ss / K + eps)
    return y, 8 * U * y.abs()


def rope_table_of(cfg, W):
    """The RoPE frequency table in the weight table W of a scaled model, or None."""
    return W[table_layout(cfg).index("inv_freq")] if cfg.rope_scaling is not None else None


def reference(case, W, layer, x0, pos, raw=None):
    """{"q": (q, bound), "k": (x, e_pre), "v": (x, e_pre)} of ``layer``'s appended rows [M, heads, D], as
    tests/test_gpu_kv_fp8.py's ``appended_reference`` gives them but from ``gemm_ref_exact`` and the layer's own
    weight-table entries. ``raw``: the observed bf16 projection of a QK-norm model, which is held to the exact
    reference here as "qkv": (y, bound)."""
    c = case.cfg
    H, Hkv, D, half = c.n_heads, c.n_kv_heads, c.head_dim, c.head_dim // 2
    table = rope_table_of(c, W)
    cs, sn, dsc = angles(c, pos, table)
    y, E = gemm_ref_exact(x0, layer_w(c, W, layer, "wqkv"), c.eps)
    if c.qk_norm:
        if raw is None:
            return {"qkv": (y, rounded(y, E))}
        x = raw.view(-1, H + 2 * Hkv, D)
        xd = x[:, :H + Hkv].to(F64)
        g = torch.cat([layer_w(c, W, layer, "q_norm").to(F64).expand(H, D), layer_w(c, W, layer, "k_norm").to(F64).expand(Hkv, D)])[None]
        n = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + c.eps) * g
        zero = torch.zeros_like(n[..., :half])
        o, Eo = rotate(n[..., :half], n[..., half:], zero, zero, RN + 3 * U, cs, sn, dsc)
        v = x[:, H + Hkv:].to(F64)
        return {"q": (o[:, :H], rounded(o, Eo)[:, :H]), "k": (o[:, H:], Eo[:, H:]), "v": (v, torch.zeros_like(v)),
                "qkv": (y, rounded(y, E))}
    if c.qkv_bias:
        y = y + layer_w(c, W, layer, "bqkv").to(F64)[None, :]
        E = E + U * y.abs()
    M = y.shape[0]
    y, E = y.view(M, H + 2 * Hkv, half, 2), E.view(M, H + 2 * Hkv, half, 2)  # pairs (dim i, dim i + D/2)
    v = torch.cat([y[:, H + Hkv:, :, 0], y[:, H + Hkv:, :, 1]], -1)
    vE = torch.cat([E[:, H + Hkv:, :, 0], E[:, H + Hkv:, :, 1]], -1)
    ry, rE = y[:, :H + Hkv], E[:, :H + Hkv]
    o, Eo = rotate(bf64(ry[..., 0]), bf64(ry[..., 1]), flip(ry[..., 0], rE[..., 0]), flip(ry[..., 1], rE[..., 1]),
                   3 * U, cs, sn, dsc)
    return {"q": (o[:, :H], rounded(o, Eo)[:, :H]), "k": (o[:, H:], Eo[:, H:]), "v": (v, vE)}


def decided_values(r):
    """The reference values of the elements ``judge`` calls decided (NaN references included)."""
    x, e = (t.numpy().ravel() for t in r)
    e = np.where(np.isnan(x) | np.isnan(e), 0.0, e)
    return x[np.isnan(x) | (ref.boundary_distance(np.where(np.isnan(x), 0.0, x)) > e) | (e == 0)]


def measure(case, obs):
    """What a step left, against the references: {"k" | "v" | "k0" | "v0": (ratio, wrong decided bytes, undecided
    share), "q": ratio, "qkv": ratio (QK-norm), "open": the last layer's undecided share of K and V together,
    "cache": what is wrong with the cache tensors (``cache_problems``), "classes": the value classes missing among
    the last layer's decided elements}. ``obs``: q, raw and, as uint8 [n_layers, slots, smax, Hkv, D], kc and vc.
    A two-layer case has its layer-0 rows judged as k0, v0 (the same input rows, layer 0's weights)."""
    inp = inputs(case)
    c, W = case.cfg, inp.weights
    sl, ps = inp.slots.long(), inp.pos.long()
    x0 = W[0][inp.tokens]
    out, last = {}, c.n_layers - 1
    for L in range(c.n_layers):
        r = reference(case, W, L, x0, inp.pos, obs["raw"] if L == last else None)
        if L == last:
            out["q"] = worst(obs["q"], r["q"])
            if c.qk_norm:
                out["qkv"] = worst(obs["raw"], r["qkv"])
        elif c.qk_norm:
            continue  # k_qknorm_rope's references need the raw projection, which only the last layer leaves behind
        for n, cache in (("k", obs["kc"]), ("v", obs["vc"])):
            ratio, wrong, undecided = judge_rows(r[n], cache[L][sl, ps])
            out[n if L == last else n + "0"] = (ratio, wrong, undecided)
        if L == last:
            out["open"] = (out["k"][2] + out["v"][2]) / 2  # K and V have the same number of elements
            x = np.concatenate([decided_values(r["k"]), decided_values(r["v"])])
            a = np.abs(x)
            have = {"beyond 448": (a > 464).any(), "subnormal": ((a > 0) & (a < 2.0 ** -6)).any(),
                    "signed zero": ((a > 0) & (a < 2.0 ** -10)).any(), "ordinary": ((a > 0.125) & (a < 400)).any(),
                    "(448, 464)": ((a > 448) & (a < 464)).any() or not c.qkv_bias, "NaN": np.isnan(x).any() == case.nan}
            out["classes"] = sorted(k for k, v in have.items() if not v)
    out["cache"] = cache_problems(case, obs["kc"], obs["vc"], obs.get("past", ()))
    return out


def show(out):
    r = lambda v: tuple(round(x, 5) for x in v) if isinstance(v, tuple) else round(v, 5) if isinstance(v, float) else v
    return {k: r(v) for k, v in out.items() if v != []}


def failures(out):
    """What of ``measure``'s result breaks a check (empty: the step passes)."""
    bad = [k for k in ("k", "v", "k0", "v0") if k in out and (out[k][0] > 1.0 or out[k][1] > 0)]
    bad += [k for k in ("q", "qkv") if k in out and not out[k] <= 1.0]
    return bad + (["open"] if out["open"] > CAP else []) + out["cache"] + out["classes"]


def cache_problems(case, kc, vc, past=()):
    """What is wrong with the whole cache tensors [n_layers, slots, smax, Hkv, D] after the step (empty: nothing):
    every layer changed in exactly the token rows, every other byte is unchanged (the NaN bytes past every length,
    the last slot of a layer and the first slot of the next on either side of L * layer_cache included), and
    layer 1's appended bytes are not layer 0's."""
    inp = inputs(case)
    sl, ps = inp.slots.long(), inp.pos.long()
    bad = [f"{name}: bytes past the cache were written" for name in past]
    for name, got, before in (("K", kc, inp.kc0), ("V", vc, inp.vc0)):
        for L in range(got.shape[0]):
            same = got[L] == before[L]
            if bool(same[sl, ps].flatten(1).all(1).any()):
                bad.append(f"layer {L} {name}: a token row's cache row was not written")
            same[sl, ps] = True
            if not bool(same.all()):
                bad.append(f"layer {L} {name}: changed outside the token rows")
            if not (bool(same[0].all()) and bool(same[-1].all())):  # named, though the line above covers them
                bad.append(f"layer {L} {name}: a slot next to the layer offset changed outside the token rows")
        if got.shape[0] == 2 and bool((got[0][sl, ps] == got[1][sl, ps]).flatten(1).all(1).any()):
            bad.append(f"{name}: layer 0 and layer 1 hold the same row")
    return bad


# ---------------------------------------------------------------- fp32 emulation (CPU)
def bf32(x):
    return x.to(BF).to(F32)


# Slips of the emulation; the names of test_kv_fp8.SLIPS where they apply (there to a store, here to the step).
WIDE_SLIPS = ("drop_last_kstep",  # wave 1 leaves out the last k-step of its share
              "oob_step_as_data",  # wave 0's last load batch reads the k-steps past its share as data, not zeros
              "drop_ss_partial",  # layer 1 sums the down projection's partials but one
              "through_bf16",  # V converted from its bf16 rounding
              "truncation", "clamp_after",
              "partner_swapped",  # the packed 2-byte store takes lane c ^ 1 for lane c + 2: dim d + D/2 lands in byte d + 1
              "kv_into_layer0",  # layer 1 appended at layer 0's offset
              "offset_in_bf16")  # ... or at L * layer_cache counted for 2-byte elements
assert {"through_bf16", "truncation", "clamp_after"} <= set(SLIPS)


def emulate_rows(case, W, layer, x0, pos, slip=None, order=None):
    """One layer's QKV projection and append in plain fp32 torch with the kernels' rounding points: q (bf16), the K
    and V bytes [M, Hkv, D] and the raw bf16 projection of a QK-norm model. ``order``: a permutation of the K axis
    the products are summed in."""
    c = case.cfg
    H, Hkv, D, half, K = c.n_heads, c.n_kv_heads, c.head_dim, c.head_dim // 2, c.dim
    table = rope_table_of(c, W)
    x, w = x0.to(F32), layer_w(c, W, layer, "wqkv").to(F32)
    M = x.shape[0]
    p = ops.step_plan(dims_of(case), case.rows).qkv
    S = K // 32

    def steps(a, b):  # the contribution of k-steps [a, b)
        return x[:, 32 * a:32 * b] @ w[:, 32 * a:32 * b].T

    acc = x @ w.T if order is None else x[:, order] @ w[:, order].T
    if slip == "drop_last_kstep":
        s1 = 2 * S // p.nw
        acc = acc - steps(s1 - 1, s1)
    if slip == "oob_step_as_data":
        s1 = S // p.nw  # wave 0's share is [0, s1); its last batch runs to the next multiple of um
        assert s1 % p.um, "every k-step of the last batch is in range: nothing to misread"
        acc = acc + steps(s1, -(-s1 // p.um) * p.um)
    if layer == 0:
        ss = x.pow(2).sum(1)  # k_embed's one partial
    else:  # the previous down projection's partials, one per column tile
        parts = x.pow(2).view(M, ops.step_plan(dims_of(case), case.rows).down.grid_x, -1).sum(-1)
        if slip == "drop_ss_partial":
            parts[:, parts.shape[1] // 2] = 0
        ss = parts.sum(1)
    rs = torch.rsqrt(ss * (torch.tensor(1.0, dtype=F32) / K) + torch.tensor(c.eps, dtype=F32))
    y = acc * rs[:, None]
    if c.qkv_bias:
        y = y + layer_w(c, W, layer, "bqkv").to(F32)[None, :]
    inv = table if table is not None else torch.exp2(-math.log2(c.rope_theta) * 2 * torch.arange(half, dtype=F32) / D)
    ang = pos.to(F32)[:, None, None] * inv.to(F32)[None, None, :]
    cs, sn = torch.cos(ang), torch.sin(ang)
    raw = None
    if c.qk_norm:  # STORE, then k_qknorm_rope: plain row order, RoPE partners d and d + D/2
        raw = y.to(BF)
        xh = raw.to(F32).view(M, H + 2 * Hkv, D)
        g = torch.cat([layer_w(c, W, layer, "q_norm").to(F32).expand(H, D), layer_w(c, W, layer, "k_norm").to(F32).expand(Hkv, D)])
        n = xh[:, :H + Hkv] * torch.rsqrt(xh[:, :H + Hkv].pow(2).sum(-1, keepdim=True) / D + c.eps) * g[None]
        x1, x2 = n[..., :half], n[..., half:]
        vf = xh[:, H + Hkv:]
    else:
        y = y.view(M, H + 2 * Hkv, half, 2)
        r = bf32(y)
        x1, x2 = r[:, :H + Hkv, :, 0], r[:, :H + Hkv, :, 1]
        vf = torch.cat([y[:, H + Hkv:, :, 0], y[:, H + Hkv:, :, 1]], -1)  # the fp32 value, not its bf16 rounding
    rot = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1)
    at_store = slip if slip in ("truncation", "clamp_after") else None
    kb = store(rot[:, H:].contiguous().numpy(), at_store)
    vb = store(vf.contiguous().numpy(), "through_bf16" if slip == "through_bf16" else at_store)
    if slip == "partner_swapped":
        for b in (kb, vb):
            good = b.copy()
            b[..., 1::2] = np.roll(good, -half, axis=-1)[..., 0::2]
    return rot[:, :H].to(BF), torch.from_numpy(kb), torch.from_numpy(vb), raw


def emulate(case, slip=None, order=None):
    """The step's appends, layer after layer, on flat copies of the case's caches: what ``measure`` takes."""
    inp = inputs(case)
    c, W = case.cfg, inp.weights
    sl, ps = inp.slots.long(), inp.pos.long()
    x0 = W[0][inp.tokens]  # every layer's input: a two-layer case zeroes layer 0's wo and w_down
    shape = inp.kc0.shape
    layer_cache = inp.kc0[0].numel()  # bytes
    # one layer's worth of room behind the caches, so that a slipped offset shows instead of raising
    flat = [torch.cat([t.flatten(), torch.full((layer_cache,), NAN_BYTE, dtype=torch.uint8)]) for t in (inp.kc0, inp.vc0)]
    row = ((sl * shape[2] + ps) * shape[3] * shape[4])[:, None] + torch.arange(shape[3] * shape[4])[None, :]
    for L in range(c.n_layers):
        q, kb, vb, raw = emulate_rows(case, W, L, x0, inp.pos, slip if L == c.n_layers - 1 else None, order)
        off = L * layer_cache * (0 if slip == "kv_into_layer0" else 2 if slip == "offset_in_bf16" else 1)
        for f, b in zip(flat, (kb, vb)):
            f[off + row] = b.flatten(1)
    past = [n for n, f in zip("KV", flat) if bool((f[-layer_cache:] != NAN_BYTE).any())]
    kc, vc = (f[:-layer_cache].view(shape) for f in flat)
    return {"q": q, "raw": raw, "kc": kc, "vc": vc, "past": past}


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_fp32_emulation_passes_and_the_cap_holds_by_the_reference_alone(case):
    out = measure(case, emulate(case))
    print("EMU kv8-wide", case.name, show(out))
    assert failures(out) == [], out
    # The precondition at work: summed in another order over K, the fp32 accumulator, and with it every byte, is
    # the same bit for bit. Inputs that are not exact fail here.
    a = emulate(case)
    b = emulate(case, order=torch.randperm(case.dim, generator=torch.Generator().manual_seed(7)))
    assert all(torch.equal(a[k], b[k]) for k in ("kc", "vc")) and torch.equal(a["q"].view(torch.int16), b["q"].view(torch.int16))
    inp = inputs(case)
    x, w = inp.weights[0][inp.tokens].to(F32), layer_w(case.cfg, inp.weights, 0, "wqkv").to(F32)
    order = torch.randperm(case.dim, generator=torch.Generator().manual_seed(8))
    assert torch.equal(x @ w.T, x[:, order] @ w[:, order].T) and torch.equal((x @ w.T).to(F64), x.to(F64) @ w.to(F64).T)


SLIP_CASES = {"dim544": next(c for c in CASES if c.dim == 544 and c.nan),
              "layer1": next(c for c in LAYER_CASES if c.kind == "plain")}
# A slip runs where it can show: the layer slips on the two-layer case; an out-of-range k-step only where a load
# batch has one (at 2048 a wave's 8 k-steps are two whole batches); a clamp after the conversion differs from the
# clamp before it on NaN alone (both saturate beyond 464), and NaN is planted in cases that do not judge attention.
ONLY = {"drop_ss_partial": ("layer1",), "kv_into_layer0": ("layer1",), "offset_in_bf16": ("layer1",),
        "oob_step_as_data": ("dim544",), "clamp_after": ("dim544",)}
SLIP_PARAMS = [pytest.param(SLIP_CASES[k], s, id=f"{k}-{s}") for s in WIDE_SLIPS for k in ONLY.get(s, tuple(SLIP_CASES))]


@pytest.mark.parametrize("case,slip", SLIP_PARAMS)
def test_every_slip_changes_a_decided_byte_or_leaves_a_bound(case, slip):
    assert SLIP_CASES["dim544"].dim == 544 and SLIP_CASES["layer1"].dim == 2048
    out = measure(case, emulate(case, slip))
    print("SLIP kv8-wide", case.name, slip, show(out))
    bad = set(failures(out)) - {"open"}  # the cap is a condition on the reference, not a catch
    assert bad, out
    if slip in ("kv_into_layer0", "offset_in_bf16"):
        assert out["cache"] and {"k", "v"} <= bad, out
    elif slip == "through_bf16":
        assert bad == {"v"}, out
    else:
        assert out["cache"] == [], out


def test_random_inputs_leave_too_much_undecided():
    # Why the exact inputs exist: with ordinary random bf16 weights at hidden size 2048, gemm_ref's accumulation bound
    # leaves far more than the cap undecided (23 % of V, 41 % of K measured), so a byte-exact check decides too little.
    case = Case("plain", 2048, 128, 40, 1024, seed=3)
    m = TinyLlama(case.cfg, device="cpu", max_batch=N_SLOTS, seed=3, kv_dtype="fp8")
    W = m.fused_weights()
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(0, case.cfg.vocab, (case.rows,), generator=g)
    pos = torch.tensor(layout(case)[0], dtype=torch.int32)
    with pytest.raises(AssertionError, match="precondition"):
        gemm_ref_exact(W[0][tokens], W[4], case.cfg.eps)
    _, kr, vr = appended_reference(case, W, W[0][tokens], pos, None)
    for r in (kr, vr):
        _, wrong, undecided = judge_rows(r, torch.from_numpy(rne64(r[0].numpy())))
        assert wrong == 0 and undecided > 10 * CAP, undecided


# ---------------------------------------------------------------- the kernels (GPU)
def observe_gpu(case):
    """One step on the device from the case's caches: q, attn, raw, the whole caches as bytes (CPU tensors); for a
    two-layer case also x1 and ss, the final residual and the sum-of-squares partials of a first pass with layer
    1's wo and w_down zeroed in place (the residual is then layer 1's input, bit for bit)."""
    inp = inputs(case)
    c, B, src = case.cfg, case.rows, inp.model
    w = dict(embed=src.embed.cuda(), final_norm=src.final_norm.cuda(), lm_head=src.lm_head.cuda(),
             layers=[{k: v.cuda() for k, v in L.items()} for L in src.layers])
    m = TinyLlama.from_weights(c, w, device="cuda", max_batch=N_SLOTS, kv_dtype="fp8")
    assert m.k_cache.dtype == F8 and m.k_cache.element_size() == 1 and tuple(m.k_cache.shape) == tuple(inp.kc0.shape)
    dec = m.fused_decoder()
    assert len(dec.weights) == len(inp.weights)
    for a, b in zip(dec.weights, inp.weights):  # the decoder's own table is what the references use
        # (a planted NaN bias may carry another payload on the device: NaN against NaN is a match)
        assert torch.equal(a.cpu().float().nan_to_num(nan=4096.0), b.float().nan_to_num(nan=4096.0))
    tokens, pos, slots = inp.tokens.cuda(), inp.pos.cuda(), inp.slots.cuda()
    kc0, vc0 = inp.kc0.cuda(), inp.vc0.cuda()
    lo, hi = int(inp.pos.min()), int(inp.pos.max())
    views = dec.workspace_views()

    def step():
        m.k_cache.view(torch.uint8).copy_(kc0)
        m.v_cache.view(torch.uint8).copy_(vc0)
        m.decode_step(tokens, pos, (lo, hi), slots=slots)
        torch.cuda.synchronize()

    obs = {}
    if c.n_layers == 2:
        zeroed = [layer_w(c, dec.weights, 1, "wo"), layer_w(c, dec.weights, 1, "w_down")]
        saved = [t.clone() for t in zeroed]
        for t in zeroed:
            t.zero_()
        step()
        obs["x1"], obs["ss"] = views["resid"][:B].cpu(), views["ss"].cpu()
        for t, s in zip(zeroed, saved):
            t.copy_(s)
    step()
    obs.update(q=views["q"][:B].cpu(), attn=views["attn"][:B].cpu(), raw=views["qkv"][:B].cpu() if c.qk_norm else None,
               kc=m.k_cache.view(torch.uint8).cpu(), vc=m.v_cache.view(torch.uint8).cpu())
    return obs


@cuda
@gpu
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_wide_appends_match_fp64_byte_for_byte(case):
    inp = inputs(case)
    c = case.cfg
    obs = observe_gpu(case)
    if c.n_layers == 2:
        # Layer 1 read the embedding rows, bit for bit, and exact integer sums of their squares.
        x0 = inp.weights[0][inp.tokens]
        assert torch.equal(obs["x1"].view(torch.int16), x0.view(torch.int16))
        parts = ops.step_plan(dims_of(case), case.rows).down.grid_x
        assert torch.equal(obs["ss"][:parts, :case.rows].to(F64).sum(0), x0.to(F64).pow(2).sum(1))
    out = measure(case, obs)
    last = c.n_layers - 1
    if not case.nan:
        ar = stage_attn(SimpleNamespace(cfg=c), obs["q"], decoded(obs["kc"][last]), decoded(obs["vc"][last]), inp.pos,
                        inp.slots)
        out["attn"] = worst(obs["attn"], ar)
    print("RATIO kv8-wide", case.name, show(out), "PLAN", plan_of(case))
    assert failures(out) == [], out
    assert out.get("attn", 0.0) <= 1.0, out
