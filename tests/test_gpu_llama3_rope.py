"""llama3 / linear RoPE scaling on the device: the kernels that read their frequencies from an fp32 table
(``k_skinny<.., EPI_ROPE_TAB | EPI_ROPE_BIAS_TAB, ..>``, ``k_qknorm_rope<D, true>``, the standalone
``k_rope_qkv_cache<true>``), element by element against fp64, then the model, the engine and a loaded
llama3-scaled checkpoint behind the endpoint.

Fused stage checks: one-layer models, one step over poisoned caches, every element of q and of the appended K and V
rows against fp64 computed from the exact inputs the kernel read (embed[token], the folded and interleaved wqkv,
the bias, the table: an exact fp32 input). The bound of an element is ``stage_qkv`` of test_gpu_fused_stages with
the angle term of the table path (tests/test_llama3_rope.py's module docstring, ``rotation``):

* E = gemm_ref's bound on acc * rs (+ U |y + bias| with a bias): (K + 16) U sum|x||w| rs + (K / 2 + 8) U |y|;
* v = bf(y): E + ulp(|y| + E) / 2;
* q, k: the inner rounding flips only within E of a tie (``flip``); cos and sin are off by
  dsc = |p f| 2^-24 (the one fp32 product p * f; f is exact) + 4 U (sincosf, 2 ulp of a value <= 1);
  the rotation's two products and one add 3 U (|x1 cos| + |x2 sin|); the store half a bf16 ulp.

Nothing is scaled by a global maximum and no element is left out; both caches are compared whole against the
poison pattern. The QK-norm variant takes test_gpu_qk_norm's bound (RN = 11 U for the norm) with the same dsc;
the standalone kernel rotates exact bf16 inputs, so its bound is the rotation's alone.

The largest error / bound seen on an MI355X is printed by each test as a RATIO line and recorded in
docs/LLAMA3.md; it is not asserted beyond <= 1.
"""
import functools
import http.client
import json
import math
import random
from dataclasses import dataclass, replace

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models import rope
from p2p_llm_tunnel_amd.models.rope import RopeScaling
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, LlamaConfig, TinyLlama
from test_gpu_fused_stages import BF, F64, U, bf64, flip, gemm_ref, rounded
from test_gpu_qk_norm import RN, ulp

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu

POISON_BITS = 0x7B7B
EPS = 1e-5
EPI_STORE, EPI_ROPE, EPI_ROPE_BIAS, EPI_ROPE_TAB, EPI_ROPE_BIAS_TAB = 0, 1, 5, 6, 7
N_SLOTS = 5  # cache slots 0..4, and the scratch slot 5

L32 = RopeScaling("llama3", 32.0, 1.0, 4.0, 8192)  # Llama 3.2's, at theta 500000 on a 4096-row cache
SHORT = RopeScaling("llama3", 8.0, 1.0, 4.0, 64)  # original length 64 at theta 10000 on a 512-row cache
PARAMS = {"l32": (L32, 500000.0, 4096), "short": (SHORT, 10000.0, 512)}


def _rules():  # imported lazily by name from the CPU module to keep one copy of the bound
    from test_llama3_rope import rotation, table_angles
    return rotation, table_angles


# ---------------------------------------------------------------- cases of the fused stage
@dataclass(frozen=True)
class Case:
    H: int
    Hkv: int
    D: int
    rows: int
    params: str
    kind: str = "llama"  # "llama", "bias" (Qwen2-shaped) or "qk_norm" (Qwen3-shaped)
    seed: int = 0

    @property
    def name(self):
        return f"{self.kind}-H{self.H}of{self.Hkv}-D{self.D}-r{self.rows}-{self.params}"

    @property
    def cfg(self):
        s, theta, smax = PARAMS[self.params]
        return LlamaConfig(vocab=512, dim=256, n_layers=1, n_heads=self.H, n_kv_heads=self.Hkv, head_dim=self.D,
                           ffn=256, max_seq=smax, eps=EPS, rope_theta=theta, rope_scaling=s,
                           qkv_bias=self.kind == "bias", qk_norm=self.kind == "qk_norm")


# Head layouts on a hidden size of 256: D 64 with G 4 (Llama-3.2-1B's 32 / 8 of 64), D 128 with G 4 (Llama-3.1-8B's
# 32 / 8 of 128) and G 8 (Llama-3.1-70B's 64 / 8).
HEADS = ((8, 2, 64), (8, 1, 128), (4, 1, 128))
CASES = [Case(H, Hkv, D, rows, ("l32", "short")[(i + j) % 2], seed=10 * i + j)
         for i, (H, Hkv, D) in enumerate(HEADS) for j, rows in enumerate((1, 16, 17, 40))]
CASES += [Case(8, 2, 64, 17, "short", seed=41), Case(8, 1, 128, 40, "short", seed=42),  # the other parameter set
          Case(14, 2, 64, 17, "short", kind="bias", seed=50), Case(4, 2, 128, 17, "l32", kind="qk_norm", seed=51)]
CASE_IDS = [c.name for c in CASES]


def seam_position(case):
    """A position that puts p * f next to pi / 2 at the first interpolated frequency (a neighbour's entry, or the
    unscaled one, turns the pair visibly), inside the cache with room for a prefill chunk after it."""
    from test_llama3_rope import bands
    s, theta, smax = PARAMS[case.params]
    table = rope.inv_freq(theta, case.D, s)
    i = bands(theta, case.D, s)[1][0]
    return min(smax - 10, max(2, int(round(0.5 * math.pi / float(table[i])))))


def layout(case):
    """(pos, slots): decode rows at position 0, the cache's last row and 1 on slots 4, 1 and 3 (rows and slots in
    different orders), a prefill chunk of up to 8 consecutive positions from the seam position on slot 2, the rest
    as a second chunk on slot 0. One row alone sits at the seam position of slot 3."""
    smax, rows, seam = PARAMS[case.params][2], case.rows, seam_position(case)
    if rows == 1:
        return (seam,), (3,)
    pos, slots = [0, smax - 1, 1][:min(rows, 3)], [4, 1, 3][:min(rows, 3)]
    a = min(8, rows - len(pos))
    pos += list(range(seam, seam + a))
    slots += [2] * a
    b = rows - len(pos)
    pos += list(range(3, 3 + b))
    slots += [0] * b
    assert len(set(zip(slots, pos))) == rows and max(pos) < smax
    return tuple(pos), tuple(slots)


@dataclass
class Inputs:
    model: TinyLlama  # on the CPU
    weights: list  # its fused weight table: embed, final_norm, lm_head, inv_freq, then the layer
    tokens: torch.Tensor
    pos: torch.Tensor
    slots: torch.Tensor


@functools.lru_cache(maxsize=None)
def case_inputs(case) -> Inputs:
    """Seeded inputs of a case, made once and shared (never modified)."""
    m = TinyLlama(case.cfg, device="cpu", max_batch=N_SLOTS, seed=case.seed)
    if case.kind == "bias":  # magnitude 2
        g = torch.Generator().manual_seed(900 + case.seed)
        m.layers[0]["bqkv"] = (torch.randn(m.layers[0]["bqkv"].shape, generator=g) * 2.0).to(BF)
    g = torch.Generator().manual_seed(700 + case.seed)
    tokens = torch.randint(0, case.cfg.vocab, (case.rows,), generator=g)
    pos, slots = layout(case)
    return Inputs(m, m.fused_weights(), tokens, torch.tensor(pos, dtype=torch.int32),
                  torch.tensor(slots, dtype=torch.int32))


# ---------------------------------------------------------------- fp64 references and bounds
def stage_qkv_table(cfg, wqkv, bias, x0, pos, table):
    """(q, k, v) references and bounds [M, heads, D] of the table epilogues from the residual rows x0, the folded
    and interleaved wqkv, the interleaved bias (or None) and the table: module docstring."""
    rotation, table_angles = _rules()
    H, Hkv, half = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim // 2
    y, E = gemm_ref(x0, wqkv, cfg.eps)
    if bias is not None:
        y = y + bias.to(F64)[None, :]
        E = E + U * y.abs()
    M = y.shape[0]
    y, E = y.view(M, H + 2 * Hkv, half, 2), E.view(M, H + 2 * Hkv, half, 2)  # pairs (dim i, dim i + D/2)
    vy, vE = y[:, H + Hkv:], E[:, H + Hkv:]
    v = torch.cat([vy[..., 0], vy[..., 1]], -1)
    vE = torch.cat([vE[..., 0], vE[..., 1]], -1)
    ry, rE = y[:, :H + Hkv], E[:, :H + Hkv]
    x1, x2 = bf64(ry[..., 0]), bf64(ry[..., 1])
    f1, f2 = flip(ry[..., 0], rE[..., 0]), flip(ry[..., 1], rE[..., 1])
    cs, sn, dsc = table_angles(pos, table)
    o, bo = rotation(x1, x2, f1, f2, cs, sn, dsc)
    return (o[:, :H], bo[:, :H]), (o[:, H:], bo[:, H:]), (v, rounded(v, vE))


def qknorm_table_reference(qkv, gq, gk, pos, H, Hkv, D, eps, table):
    """test_gpu_qk_norm.reference with the angles of the table: (q, bound), (k, bound), (v, 0: bit for bit)."""
    _, table_angles = _rules()
    R, half = qkv.shape[0], D // 2
    x = qkv.view(R, H + 2 * Hkv, D)
    xd = x[:, :H + Hkv].to(F64)
    g = torch.cat([gq.to(F64).expand(H, D), gk.to(F64).expand(Hkv, D)])[None]
    n = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps) * g
    cs, sn, dsc = table_angles(pos, table)
    n1, n2 = n[..., :half], n[..., half:]
    o = torch.cat([n1 * cs - n2 * sn, n2 * cs + n1 * sn], -1)
    common = (n1.abs() + n2.abs()) * dsc
    E = torch.cat([(RN + 3 * U) * ((n1 * cs).abs() + (n2 * sn).abs()) + common,
                   (RN + 3 * U) * ((n2 * cs).abs() + (n1 * sn).abs()) + common], -1)
    bound = E + 0.5 * ulp(o.abs() + E)
    v = x[:, H + Hkv:].to(F64)
    return (o[:, :H], bound[:, :H]), (o[:, H:], bound[:, H:]), (v, torch.zeros_like(v))


def worst(got, ref_bound):
    ref, bound = ref_bound
    err = (got.to(F64).reshape(ref.shape) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).max().item()


def on_gpu(inp, cfg):
    """A device copy of the case's CPU model (the same weights, bit for bit), as ``cfg``."""
    src = inp.model
    w = dict(embed=src.embed.cuda(), final_norm=src.final_norm.cuda(), lm_head=src.lm_head.cuda(),
             layers=[{k: v.cuda() for k, v in L.items()} for L in src.layers])
    return TinyLlama.from_weights(cfg, w, device="cuda", max_batch=N_SLOTS)


def run_step(m, inp, rows):
    m.k_cache.view(torch.int16).fill_(POISON_BITS)
    m.v_cache.view(torch.int16).fill_(POISON_BITS)
    pos = inp.pos.tolist()
    m.decode_step(inp.tokens.cuda(), inp.pos.cuda(), (min(pos), max(pos)), slots=inp.slots.cuda())
    torch.cuda.synchronize()
    views = m.fused_decoder().workspace_views()
    return views["q"][:rows].cpu(), m.k_cache[0].cpu(), m.v_cache[0].cpu(), views["qkv"][:rows].cpu()


@cuda
@gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_table_stage_matches_fp64(case):
    inp = case_inputs(case)
    cfg, rows = case.cfg, case.rows
    m = on_gpu(inp, cfg)
    dec = m.fused_decoder()
    per = {"llama": 6, "bias": 7, "qk_norm": 8}[case.kind]
    assert len(dec.weights) == 4 + per and dec.dims.rope_table == 1
    for a, b in zip(dec.weights, inp.weights):  # the decoder's own table is what the reference used
        assert torch.equal(a.cpu(), b)
    table = inp.weights[3]
    assert table.dtype == torch.float32 and torch.equal(table, rope.inv_freq(cfg.rope_theta, cfg.head_dim,
                                                                             cfg.rope_scaling))
    plan = ops.step_plan(dec.dims, rows)
    want_epi = {"llama": EPI_ROPE_TAB, "bias": EPI_ROPE_BIAS_TAB, "qk_norm": EPI_STORE}[case.kind]
    assert plan.qkv.epi == plan.qkv_first.epi == want_epi and plan.qk_norm_table == int(case.kind == "qk_norm")
    assert plan.qkv.grid_y == (rows + 15) // 16
    if rows == 1:
        assert plan.o.kpl > 0 and plan.down.kpl > 0  # batch 1 keeps its K parts
    q, kc, vc, raw = run_step(m, inp, rows)
    W = inp.weights
    if case.kind == "qk_norm":
        L = inp.model.layers[0]
        refs = qknorm_table_reference(raw, L["q_norm"], L["k_norm"], inp.pos, cfg.n_heads, cfg.n_kv_heads,
                                      cfg.head_dim, cfg.eps, table)
    else:
        refs = stage_qkv_table(cfg, W[5], W[10] if case.kind == "bias" else None, W[0][inp.tokens], inp.pos, table)
    sl, ps = inp.slots.long(), inp.pos.long()
    ratios = {n: worst(got, r) for n, got, r in zip("qkv", (q, kc[sl, ps], vc[sl, ps]), refs)}
    print("RATIO table", case.name, {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    # one K and one V row per token row, nothing else in either cache
    for got in (kc, vc):
        same = got.view(torch.int16) == POISON_BITS
        same[sl, ps] = True
        assert bool(same.all())
    assert not bool((kc[sl, ps].view(torch.int16) == POISON_BITS).all(-1).any())
    # The scaling is in the result: default RoPE on the same weights stores other K rows (position 0 aside).
    if rows == 17:
        plain = on_gpu(inp, replace(cfg, rope_scaling=None))
        assert plain.fused_decoder().dims.rope_table == 0 and len(plain.fused_decoder().weights) == 3 + per
        _, kc0, vc0, _ = run_step(plain, inp, rows)
        assert not torch.equal(kc0.view(torch.int16), kc.view(torch.int16))
        assert torch.equal(vc0.view(torch.int16), vc.view(torch.int16))
        assert worst(kc0[sl, ps], refs[1]) > 1.0


# ---------------------------------------------------------------- the standalone kernels
@functools.lru_cache(maxsize=None)
def standalone_inputs(D, H, Hkv, B, smax, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B, (H + 2 * Hkv) * D, generator=g) * 1.5).to(BF)
    pos = torch.tensor(([0, 1, smax - 1] + list(range(7, 7 + B)))[:B], dtype=torch.int32)
    return qkv, pos


def standalone_reference(qkv, pos, table, H, Hkv, D, extra_rel=0.0):
    """(q, bound), (k, bound) of the standalone kernel (exact bf16 inputs: the rotation's own bound) and v.
    ``extra_rel``: a relative error of the frequency itself, for a kernel that computes its own."""
    rotation, table_angles = _rules()
    B, half = qkv.shape[0], D // 2
    x = qkv.view(B, H + 2 * Hkv, D)
    r = x[:, :H + Hkv].to(F64)
    cs, sn, dsc = table_angles(pos, table)
    dsc = dsc + (dsc - 4 * U) / U * extra_rel  # |p f| * extra_rel
    zero = torch.zeros_like(r[..., :half])
    o, bound = rotation(r[..., :half], r[..., half:], zero, zero, cs, sn, dsc)
    return (o[:, :H], bound[:, :H]), (o[:, H:], bound[:, H:]), x[:, H + Hkv:]


@cuda
@gpu
@pytest.mark.parametrize("D,H,Hkv,B,params", [(64, 8, 2, 5, "l32"), (128, 8, 1, 3, "l32"), (64, 4, 2, 9, "short")])
def test_standalone_rope_with_a_table(D, H, Hkv, B, params):
    s, theta, smax = PARAMS[params]
    qkv, pos = standalone_inputs(D, H, Hkv, B, smax, 5 + D + B)
    table = rope.inv_freq(theta, D, s)

    def run(**kw):
        kc = torch.full((B, smax, Hkv, D), POISON_BITS, dtype=torch.int16, device="cuda").view(BF)
        vc = kc.clone()
        q = ops.rope_qkv_cache(qkv.cuda(), pos.cuda(), kc, vc, H, Hkv, D, theta=theta, **kw)
        torch.cuda.synchronize()
        return q.cpu(), kc.cpu(), vc.cpu()

    def judge(out, refs):
        q, kc, vc = out
        rows, ps = torch.arange(B), pos.long()
        ratios = {"q": worst(q, refs[0]), "k": worst(kc[rows, ps], refs[1])}
        assert torch.equal(vc[rows, ps].reshape(B, -1).view(torch.int16), refs[2].reshape(B, -1).view(torch.int16))
        for c in (kc, vc):
            same = c.view(torch.int16) == POISON_BITS
            same[rows, ps] = True
            assert bool(same.all())
        return ratios

    with_table = run(inv_freq=table.cuda())
    ratios = judge(with_table, standalone_reference(qkv, pos, table, H, Hkv, D))
    print("RATIO standalone table", D, params, {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    # A table of the default frequencies, computed on the host in fp32 the way the kernel computes its own: the
    # table path is held to it exactly as above, and the inline path within the same bound widened by what two
    # evaluations of theta^(-2i/D) in fp32 can differ by, 2 (3 ln2 |t| + 3) U relative (rope_tables). Bits may differ.
    t = -math.log2(theta) * 2.0 * torch.arange(D // 2, dtype=torch.float32) / D
    default = torch.exp2(t)
    refs = standalone_reference(qkv, pos, default, H, Hkv, D)
    r_tab = judge(run(inv_freq=default.cuda()), refs)
    wide = standalone_reference(qkv, pos, default, H, Hkv, D,
                                extra_rel=(2 * (3 * math.log(2) * t.abs().to(F64) + 3) * U)[None, None, :])
    r_inline = judge(run(), wide)
    print("RATIO standalone default", D, params, r_tab, r_inline)
    assert max(r_tab.values()) <= 1.0 and max(r_inline.values()) <= 1.0, (r_tab, r_inline)
    assert not torch.equal(with_table[1].view(torch.int16), run()[1].view(torch.int16))  # the scaling shows


@cuda
@gpu
def test_table_validation_raises_before_launching():
    H, Hkv, D, B, S = 4, 2, 64, 3, 16
    dev = "cuda"
    poisoned = lambda *shape: torch.full(shape, POISON_BITS, dtype=torch.int16, device=dev).view(BF)
    good = torch.full((D // 2,), 0.5, device=dev)
    pad = torch.full((D // 2 + 1,), 0.5, device=dev)

    def entry(i, v):
        t = good.clone()
        t[i] = v
        return t
    bad = [(TypeError, good.double()), (TypeError, good.to(BF)), (TypeError, [0.5] * (D // 2)),
           (ValueError, good.cpu()), (ValueError, pad), (ValueError, good[:-1]), (ValueError, good.view(1, -1)),
           (ValueError, torch.full((D,), 0.5, device=dev)[::2]),  # not contiguous
           (ValueError, pad[1:]),  # the right length, 4-byte aligned only
           (ValueError, entry(0, 0.0)), (ValueError, entry(5, -1e-3)), (ValueError, entry(D // 2 - 1, float("inf"))),
           (ValueError, entry(7, float("nan")))]
    kc, vc = poisoned(B, S, Hkv, D), poisoned(B, S, Hkv, D)
    nk, nv = poisoned(B, S, Hkv, D), poisoned(B, S, Hkv, D)
    qkv = torch.zeros(B, (H + 2 * Hkv) * D, dtype=BF, device=dev)
    pos = torch.tensor([0, 5, S - 1], dtype=torch.int32, device=dev)
    w = torch.ones(D, dtype=BF, device=dev)
    for exc, t in bad:
        with pytest.raises(exc):
            ops.rope_qkv_cache(qkv, pos, kc, vc, H, Hkv, D, theta=1e4, inv_freq=t)
        with pytest.raises(exc):
            ops.qk_norm_rope_cache(qkv, pos, nk, nv, w, w, H, Hkv, D, 1e-6, 1e4, inv_freq=t)
    torch.cuda.synchronize()
    for c in (kc, vc, nk, nv):  # nothing was launched
        assert bool((c.view(torch.int16) == POISON_BITS).all())
    ops.rope_qkv_cache(qkv, pos, kc, vc, H, Hkv, D, theta=1e4, inv_freq=good)
    ops.qk_norm_rope_cache(qkv, pos, nk, nv, w, w, H, Hkv, D, 1e-6, 1e4, inv_freq=good)
    torch.cuda.synchronize()
    # the decoder checks its table entry the same way, and the table's place in the weight list
    cfg = LlamaConfig(vocab=64, dim=64, n_layers=1, n_heads=2, n_kv_heads=1, head_dim=64, ffn=64, max_seq=8,
                      rope_scaling=SHORT)
    m = TinyLlama(cfg, device="cuda", max_batch=1, seed=0)
    tab = m.fused_weights()
    dims = ops.LlamaDims(vocab=64, dim=64, n_layers=1, H=2, Hkv=1, D=64, ffn=64, max_seq=8, max_batch=2, eps=1e-5,
                         theta=1e4, rope_table=1)
    with pytest.raises((TypeError, ValueError), match="inv_freq"):  # a bf16 layer weight where the table belongs
        ops.FusedLlamaDecoder(dims, tab[:3] + tab[4:], m.k_cache, m.v_cache)
    with pytest.raises(ValueError, match="inv_freq"):
        ops.FusedLlamaDecoder(dims, tab[:3] + [tab[3][:-2].contiguous()] + tab[4:], m.k_cache, m.v_cache)
    with pytest.raises((TypeError, ValueError)):  # a table where the unscaled step expects a layer's first weight
        ops.FusedLlamaDecoder(replace_dims(dims, rope_table=0), tab, m.k_cache, m.v_cache)
    ops.FusedLlamaDecoder(dims, tab, m.k_cache, m.v_cache)


def replace_dims(d, **kw):
    return ops.LlamaDims(**{**{n: getattr(d, n) for n, _ in ops.LlamaDims._fields_}, **kw})


# ---------------------------------------------------------------- model, engine, checkpoint
M3 = replace(CONFIGS["micro"], rope_scaling=SHORT)  # micro: 2 layers, 4 / 2 heads of 64, max_seq 512
MODEL_SEED, MODEL_NEW = 0, 6


def _ids(seed, n, vocab=4096):
    rng = random.Random(seed)
    return [rng.randrange(vocab) for _ in range(n)]


# Prompts of the engine test: (prompt, greedy continuation under the fp32 reference of the scaled model (seed 0),
# the same weights' continuation with default RoPE or None where it is not compared). Searched on the CPU for a
# top-2 gap of at least 3 % of the largest logit at every generated index, under both models where both are given,
# and for continuations that differ: tests/test_llama3_rope.py::test_model_tokens_depend_on_the_scaling re-checks.
# 37 tokens (chunked prefill next to nothing), one token, 71 tokens (more than one 64-row step)
ENGINE_PROMPTS = [(_ids(550, 37), [1409, 1845, 538, 2427, 7, 1268], [1409, 1845, 538, 2427, 7, 2021]),
                  (_ids(95, 1), [873, 3583, 4034, 325, 1152, 816], None),
                  (_ids(170, 71), [3658, 2483, 4009, 1389, 1890, 3251], [3658, 67, 3210, 77, 1315, 547])]


@cuda
@gpu
def test_scaled_model_fused_unfused_and_reference():
    # tests/test_gpu_qwen2.py's tolerances and confident-argmax rule, on the scaled micro model.
    B, T = 3, 70  # crosses a 64-token attention split; beyond the original length of 64
    mf = TinyLlama(M3, device="cuda", max_batch=B, seed=4, fused=True)
    mu = TinyLlama(M3, device="cuda", max_batch=B, seed=4, fused=False)
    assert len(mf.fused_weights()) == 4 + 6 * M3.n_layers
    torch.manual_seed(1)
    seqs = torch.randint(0, M3.vocab, (B, T), device="cuda")
    for p in range(T):
        pos = torch.full((B,), p, dtype=torch.int32, device="cuda")
        idf, lf = mf.decode_step(seqs[:, p], pos, (p, p), return_logits=True)
        idu, lu = mu.decode_step(seqs[:, p], pos, (p, p), return_logits=True)
    scale = lu.float().abs().max().item()
    assert (lf.float() - lu.float()).abs().max().item() < 0.03 * scale
    top2 = lu.float().topk(2, -1).values
    confident = (top2[:, 0] - top2[:, 1]) > 0.03 * scale
    assert torch.equal(idf[confident], idu[confident])
    kdiff = (mf.k_cache[:, :B, :T].float() - mu.k_cache[:, :B, :T].float()).abs().max().item()
    assert kdiff < 0.05 * mu.k_cache[:, :B, :T].float().abs().max().item()

    ref = mf.reference_logits(seqs)
    for logits in (lf, lu):
        scale = ref.abs().max().item()
        assert (logits.float() - ref).abs().max().item() < 0.05 * scale
        top2 = ref.topk(2, -1).values
        confident = (top2[:, 0] - top2[:, 1]) > 0.05 * scale
        assert torch.equal(logits.float().argmax(-1)[confident], ref.argmax(-1)[confident])
    # The scaling is in the result: the same weights with default RoPE give other logits.
    plain = TinyLlama.from_weights(replace(M3, rope_scaling=None),
                                   dict(embed=mf.embed, final_norm=mf.final_norm, lm_head=mf.lm_head, layers=mf.layers),
                                   device="cuda", max_batch=B)
    assert (plain.reference_logits(seqs) - ref).abs().max().item() > 0.05 * scale


@cuda
@gpu
def test_scaled_model_graph_replay_matches_eager():
    torch.manual_seed(3)
    m = TinyLlama(M3, device="cuda", max_batch=4, seed=2)
    m.k_cache.normal_()
    m.v_cache.normal_()
    m.capture_graph(rows=4)
    toks = torch.randint(0, M3.vocab, (4,), device="cuda")
    pos = torch.tensor([5, 130, 0, 300], dtype=torch.int32, device="cuda")
    kc, vc = m.k_cache.clone(), m.v_cache.clone()
    ids_g, logits_g = m.graph_step(toks, pos, return_logits=True)
    logits_g, kg = logits_g.clone(), m.k_cache.clone()
    m.k_cache.copy_(kc)
    m.v_cache.copy_(vc)
    ids_e, logits_e = m.decode_step(toks, pos, (0, 300), return_logits=True)
    assert torch.equal(ids_g, ids_e)
    assert (logits_g.float() - logits_e.float()).abs().max().item() < 1e-2
    assert torch.equal(kg.view(torch.int16), m.k_cache.view(torch.int16))


@cuda
@gpu
def test_scaled_model_unfused_graph_replay_matches_eager():
    """The unfused step of a scaled model syncs nothing and captures: the table is checked once, where it is made,
    and ``rope_qkv_cache`` is told so (``inv_freq_checked``), as ``pos_range`` tells it the positions."""
    torch.manual_seed(6)
    B = 4
    m = TinyLlama(M3, device="cuda", max_batch=B, seed=2, fused=False)
    m.k_cache.normal_()
    m.v_cache.normal_()
    m.capture_graph()  # a device-to-host copy during capture would raise here
    assert B in m._graphs and m._fused is None
    toks = torch.randint(0, M3.vocab, (B,), device="cuda")
    pos = torch.tensor([5, 130, 0, 300], dtype=torch.int32, device="cuda")
    kc, vc = m.k_cache.clone(), m.v_cache.clone()
    ids_g, logits_g = m.graph_step(toks, pos, return_logits=True)
    ids_g, logits_g, kg = ids_g.clone(), logits_g.clone(), m.k_cache.clone()
    m.k_cache.copy_(kc)
    m.v_cache.copy_(vc)
    ids_e, logits_e = m.decode_step(toks, pos, (0, 300), return_logits=True)
    assert torch.equal(ids_g, ids_e)
    assert (logits_g.float() - logits_e.float()).abs().max().item() < 1e-2
    assert torch.equal(kg.view(torch.int16), m.k_cache.view(torch.int16))
    # the rows the step appended are the table's, not theta's own: default RoPE on the same weights differs
    plain = TinyLlama.from_weights(replace(M3, rope_scaling=None),
                                   dict(embed=m.embed, final_norm=m.final_norm, lm_head=m.lm_head, layers=m.layers),
                                   device="cuda", max_batch=B, fused=False)
    plain.k_cache.copy_(kc)
    plain.v_cache.copy_(vc)
    plain.decode_step(toks, pos, (0, 300))
    assert not torch.equal(plain.k_cache[0, 1, 130].view(torch.int16), kg[0, 1, 130].view(torch.int16))
    # ... and the op itself, told that the table is checked, reads nothing back: an unchecked call still refuses
    bad = m.rope_inv_freq().clone()
    bad[3] = 0.0
    c = M3
    qkv = torch.zeros(B, (c.n_heads + 2 * c.n_kv_heads) * c.head_dim, dtype=BF, device="cuda")
    with pytest.raises(ValueError, match="finite"):
        ops.rope_qkv_cache(qkv, pos, m.k_cache[0, :B], m.v_cache[0, :B], c.n_heads, c.n_kv_heads, c.head_dim,
                           c.rope_theta, pos_range=(0, 300), inv_freq=bad)
    with pytest.raises(ValueError, match="shape"):  # the host-side checks stay with the flag
        ops.rope_qkv_cache(qkv, pos, m.k_cache[0, :B], m.v_cache[0, :B], c.n_heads, c.n_kv_heads, c.head_dim,
                           c.rope_theta, pos_range=(0, 300), inv_freq=bad[:-2].contiguous(), inv_freq_checked=True)


@cuda
@gpu
def test_engine_serves_a_scaled_model():
    from p2p_llm_tunnel_amd.models.server import Engine, Request
    model = TinyLlama(M3, device="cuda:0", max_batch=4, seed=MODEL_SEED)
    twin = TinyLlama(M3, device="cuda:0", max_batch=1, seed=MODEL_SEED)
    plain = TinyLlama(replace(M3, rope_scaling=None), device="cuda:0", max_batch=1, seed=MODEL_SEED)
    eng = Engine(model=model)
    try:
        assert len(eng._graphs) == 12
        # all at once (batched, chunked prefill next to decode rows), then one by one: the same greedy tokens
        reqs = [eng.submit(Request(list(prompt), len(want))) for prompt, want, _ in ENGINE_PROMPTS]
        for r, (prompt, want, _) in zip(reqs, ENGINE_PROMPTS):
            got = []
            while (t := r.out.get(timeout=60)) is not None:
                got.append(t)
            assert got == list(want), len(prompt)
        for prompt, want, without in ENGINE_PROMPTS:
            r = eng.submit(Request(list(prompt), len(want)))
            got = []
            while (t := r.out.get(timeout=60)) is not None:
                got.append(t)
            assert got == twin.generate(list(prompt), len(want)) == list(want)
            if without is not None:  # ... and they are the scaling's: default RoPE continues differently
                assert plain.generate(list(prompt), len(want)) == list(without) != list(want)
    finally:
        eng.stop()


@cuda
@gpu
def test_fused_decode_on_a_loaded_llama3_checkpoint(tmp_path):
    from test_checkpoint import _hf_logits, _tokenizer_dir
    from test_llama3_rope import scaled_checkpoint
    from p2p_llm_tunnel_amd.models.checkpoint import load_llama
    from p2p_llm_tunnel_amd.models.server import start_server
    hf = scaled_checkpoint(str(tmp_path), SHORT, tie=True, spelling="rope_scaling")
    _tokenizer_dir(str(tmp_path))
    ours = load_llama(str(tmp_path), device="cuda", max_batch=2, max_seq=256)
    assert ours.cfg.rope_scaling == SHORT and ours.fused and ours.fused_decoder().dims.rope_table == 1
    torch.manual_seed(5)
    T = 33
    seqs = torch.randint(0, ours.cfg.vocab, (2, T))
    d = seqs.cuda()
    for p in range(T):
        _, logits = ours.decode_step(d[:, p], torch.full((2,), p, dtype=torch.int32, device="cuda"), (p, p),
                                     return_logits=True)
    want = _hf_logits(hf, seqs)
    scale = want.abs().max().item()
    assert (logits.float().cpu() - want).abs().max().item() < 0.05 * scale
    assert torch.nn.functional.cosine_similarity(logits.float().cpu(), want, dim=-1).min().item() > 0.995
    # ... and the endpoint serves it (hipGraph path) with a tokenizer next to it
    srv, port, eng = start_server(port=0, device="cuda:0", max_batch=2, checkpoint=str(tmp_path), max_seq=256)
    try:
        assert eng.use_graph and srv.tok is not None and eng.model.cfg.rope_scaling == SHORT
        assert len(eng._graphs) == 12
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        c.request("POST", "/v1/chat/completions", body=json.dumps(
            {"stream": True, "max_tokens": 8, "messages": [{"role": "user", "content": "hello world"}]}))
        r = c.getresponse()
        data = r.read()
        assert r.status == 200 and data.rstrip().endswith(b"data: [DONE]")
    finally:
        srv.shutdown()
        eng.stop()
