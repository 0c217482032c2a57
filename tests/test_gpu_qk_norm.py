"""Per-head QK RMSNorm + RoPE + cache append (``k_qknorm_rope``, decode_fused_kernels.h): the kernel on its
own (``ops.qk_norm_rope_cache``) and inside the fused step of a QK-norm model (Qwen3), element by element
against fp64, then the model, the engine and a loaded Qwen3 checkpoint.

The reference is computed in fp64 from the exact bf16 inputs the kernel read. For a q or k head x[0..D) with
weight g, position p and i < D/2:

    n[d] = x[d] * rsqrt(mean(x^2) + eps) * g[d]
    o[i] = n[i] cos(a_i) - n[i + D/2] sin(a_i),  o[i + D/2] = n[i + D/2] cos(a_i) + n[i] sin(a_i),
    a_i = p * theta^(-2i/D)

and the kernel's result is bf16(o). The bound of one element, with U = 2^-24 (the fp32 unit roundoff) and
ulp(y) the bf16 spacing at |y|, is built from what the kernel does in fp32 on the way to that element alone;
nothing is scaled by a maximum over the head, the row or the tensor:

* The sum of squares. Each x^2 is rounded once; a lane adds its 4 squares (3 adds) and the lanes of the head are
  summed in log2(D / 4) <= 5 steps: at most 9 roundings on the way of any term, all terms non-negative, so the
  sum is off by at most 9 U relatively. Times 1/D is exact (a power of two); + eps rounds once (U of the
  sum); rsqrtf is good to 2 ulp = 4 U (ops/build.py compiles without fast-math); the power -1/2 halves what
  came before it: r = rsqrt(...) is off by (9 + 1) / 2 + 4 = 9 U relatively.
* n = (x * r) * g: two more roundings; n is off by RN = 11 U relatively. x and g are exact (bf16 in fp32).
* The angle, exactly as in the QKV epilogue of the models without QK-norm (test_gpu_fused_stages.rope_tables):
  t = -log2f(theta) * (2 i) / D rounds three times, exp2f is good to 2 ulp, p * inv_freq rounds once:
  a_i is off by a_i (3 ln2 |t| + 3) U, and sincosf adds 2 ulp of a value <= 1: each of cos and sin is off by
  dsc = a_i (3 ln2 |t| + 3) U + 4 U.
* The rotation: two products and one add (or an fma and a product): 3 U (|n1 cos| + |n2 sin|).

    E = (RN + 3 U) (|n1 cos| + |n2 sin|) + (|n1| + |n2|) dsc        (the error before the last rounding)
    bound = E + ulp(|o| + E) / 2                                     (the one bf16 store)

An all-zero head gives exactly 0 (0 * rsqrt(eps)); v is copied, so its bound is 0: bit equality.

Largest |error| / bound seen on an MI355X (printed by each test as RATIO lines, recorded here, not asserted):
standalone kernel, 12 cases: q 0.983 .. 1.000, k 0.990 .. 1.000 (three decimals; E is ~1e-6 of |o| and the half
ulp of the store ~4e-3, so an element that lands next to a rounding tie sits just under 1); inside the fused
step, 6 cases: q 0.998 .. 1.000, k 0.991 .. 0.999. v bit-exact and the rest of both caches untouched in all 18.
"""
import functools
import math
import random
from dataclasses import dataclass, replace

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig, TinyLlama

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu

U = 2.0 ** -24
RN = 11 * U
BF = torch.bfloat16
F64 = torch.float64
POISON_BITS = 0x7B7B  # cache contents before the kernel runs; rows it must not touch keep this pattern
EPS = 1e-6


# ---------------------------------------------------------------- cases of the standalone kernel
@dataclass(frozen=True)
class Case:
    D: int
    H: int
    Hkv: int
    rows: int
    theta: float
    max_seq: int = 96
    n_slots: int = 6  # slot 5 plays the scratch slot, slot 4 is never addressed
    no_slots: bool = False  # slots=None: row b -> slot b
    seed: int = 0

    @property
    def name(self):
        return f"D{self.D}-H{self.H}of{self.Hkv}-r{self.rows}-theta{self.theta:g}" + ("-noslots" if self.no_slots else "")

    @property
    def mid(self):
        return self.max_seq // 2 - 5


def _cases():
    cs = []
    for D in (64, 128):
        # every G with every D; 6, 8, 18, 10, 6, 8 heads in all: whole and partial waves and workgroups
        # (a workgroup covers 16 heads at D 64, 8 at D 128)
        for idx, (rows, G, Hkv) in enumerate(((1, 1, 2), (3, 2, 2), (16, 4, 3), (17, 8, 1), (40, 1, 2), (64, 2, 2))):
            theta = (1e4, 1e6)[(idx + (D == 128)) % 2]
            cs.append(Case(D, G * Hkv, Hkv, rows, theta, no_slots=rows == 3, seed=len(cs) + 1))
    return cs


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


def layout(case):
    """(pos, slots) of a case's rows. Row 0 sits at position 0, row 1 at max_seq - 1, row 2 in the middle, each
    on a slot of its own; rows 3..10 are a prefill chunk: one slot, consecutive positions; the rest are padding
    rows on the scratch slot (at distinct positions, so that what lands there is defined). One row alone takes
    the case's turn of the three positions."""
    S, R = case.max_seq, case.rows
    if R == 1:
        return [(0, case.mid, S - 1)[(case.seed + (case.D == 128)) % 3]], [3]
    pos, slots = [0, S - 1, case.mid][:R], [0, 1, 3][:R]
    for r in range(3, R):
        if r < 11:
            pos.append(case.mid + r - 3)
            slots.append(2)
        else:
            pos.append(r - 10)
            slots.append(case.n_slots - 1)
    if case.no_slots:
        slots = list(range(R))
    return pos, slots


@dataclass
class Inputs:
    qkv: torch.Tensor  # bf16 [rows, (H + 2 Hkv) D]
    gq: torch.Tensor
    gk: torch.Tensor
    pos: torch.Tensor
    slots: torch.Tensor


@functools.lru_cache(maxsize=None)
def inputs(case) -> Inputs:
    """Seeded inputs of a case, made once and shared (never modified)."""
    g = torch.Generator().manual_seed(500 + case.seed)
    H, Hkv, D, R = case.H, case.Hkv, case.D, case.rows
    x = (torch.randn(R, H + 2 * Hkv, D, generator=g) * 1.5).to(BF)
    big, zero = min(2, R - 1), min(1, R - 1)
    x[big, H - 1] = (x[big, H - 1].float() * 2.0 ** 40).to(BF)  # a q and a k head scaled by 2^40: eps plays no part
    x[big, H + Hkv - 1] = (x[big, H + Hkv - 1].float() * 2.0 ** 40).to(BF)
    if H > 1:
        x[0, 1] = (x[0, 1].float() * 2.0 ** -12).to(BF)  # mean(x^2) ~ 1e-7 next to eps = 1e-6: eps dominates
    x[0, H] = (x[0, H].float() * 2.0 ** -12).to(BF)
    x[zero, 0] = 0  # all-zero q and k heads: eps alone
    x[zero, H] = 0
    gq = (0.5 + torch.rand(D, generator=g)).to(BF)
    gk = (0.5 + torch.rand(D, generator=g)).to(BF)
    pos, slots = layout(case)
    return Inputs(x.view(R, -1).contiguous(), gq, gk, torch.tensor(pos, dtype=torch.int32),
                  torch.tensor(slots, dtype=torch.int32))


# ---------------------------------------------------------------- fp64 reference and bound
def ulp(a):
    """bf16 spacing at |a| (fp64)."""
    _, e = torch.frexp(a.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(a), e - 8)


def reference(qkv, gq, gk, pos, H, Hkv, D, eps, theta):
    """(q, bound) [R, H, D], (k, bound) [R, Hkv, D] in fp64 and v [R, Hkv, D] (bf16, to be matched bit for bit)
    from the bf16 inputs: the module docstring's formulas, term by term."""
    R, half = qkv.shape[0], D // 2
    x = qkv.view(R, H + 2 * Hkv, D)
    xd = x[:, :H + Hkv].to(F64)
    g = torch.cat([gq.to(F64).expand(H, D), gk.to(F64).expand(Hkv, D)])[None]
    n = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps) * g
    t = -math.log2(theta) * 2.0 * torch.arange(half, dtype=F64) / D
    ang = pos.to(F64)[:, None, None] * torch.exp2(t)[None, None, :]
    dsc = ang * ((3 * math.log(2) * t.abs() + 3) * U)[None, None, :] + 4 * U
    cs, sn = torch.cos(ang), torch.sin(ang)
    n1, n2 = n[..., :half], n[..., half:]
    o = torch.cat([n1 * cs - n2 * sn, n2 * cs + n1 * sn], -1)
    common = (n1.abs() + n2.abs()) * dsc
    E = torch.cat([(RN + 3 * U) * ((n1 * cs).abs() + (n2 * sn).abs()) + common,
                   (RN + 3 * U) * ((n2 * cs).abs() + (n1 * sn).abs()) + common], -1)
    bound = E + 0.5 * ulp(o.abs() + E)
    return (o[:, :H], bound[:, :H]), (o[:, H:], bound[:, H:]), x[:, H + Hkv:]


@functools.lru_cache(maxsize=None)
def case_reference(case):
    inp = inputs(case)
    return reference(inp.qkv, inp.gq, inp.gk, inp.pos, case.H, case.Hkv, case.D, EPS, case.theta)


def worst(got, ref_bound):
    """Largest |got - ref| / bound; inf where the comparison does not hold (a NaN included)."""
    ref, bound = ref_bound
    err = (got.to(F64).reshape(ref.shape) - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio).max().item()


def poisoned(shape, device="cpu"):
    return torch.full(shape, POISON_BITS, dtype=torch.int16, device=device).view(BF)


def check_outputs(q, kc, vc, refs, pos, slots):
    """Error / bound ratios of q and of the K rows the step appended; "v": 0 when the V rows are bit-exact, "rest":
    0 when both caches, compared whole, are untouched outside the addressed rows; inf otherwise."""
    qr, kr, v = refs
    p, s = pos.long(), slots.long()
    ratios = {"q": worst(q, qr), "k": worst(kc[s, p], kr)}
    exact = torch.equal(vc[s, p].view(torch.int16), v.contiguous().view(torch.int16))
    ratios["v"] = 0.0 if exact else float("inf")
    untouched = True
    for c in (kc, vc):
        same = c.view(torch.int16) == POISON_BITS
        same[s, p] = True
        untouched = untouched and bool(same.all())
    ratios["rest"] = 0.0 if untouched else float("inf")
    return ratios


# ---------------------------------------------------------------- the standalone kernel (GPU)
def run_kernel(case):
    inp = inputs(case)
    shape = (case.n_slots, case.max_seq, case.Hkv, case.D)
    kc, vc = poisoned(shape, "cuda"), poisoned(shape, "cuda")
    slots = None if case.no_slots else inp.slots.cuda()
    q = ops.qk_norm_rope_cache(inp.qkv.cuda(), inp.pos.cuda(), kc, vc, inp.gq.cuda(), inp.gk.cuda(), case.H, case.Hkv,
                               case.D, EPS, case.theta, slots=slots)
    torch.cuda.synchronize()
    return q.cpu(), kc.cpu(), vc.cpu()


@cuda
@gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_qk_norm_rope_cache_matches_fp64(case):
    inp = inputs(case)
    q, kc, vc = run_kernel(case)
    assert q.shape == (case.rows, case.H, case.D) and q.dtype == BF
    ratios = check_outputs(q, kc, vc, case_reference(case), inp.pos, inp.slots)
    print("RATIO", case.name, {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    zero = min(1, case.rows - 1)  # the all-zero heads come out as exact zeros (of either sign)
    assert bool((q[zero, 0].float() == 0).all())
    assert bool((kc[inp.slots[zero], inp.pos[zero], 0].float() == 0).all())


@cuda
@gpu
def test_qk_norm_rope_cache_validates_before_launching():
    H, Hkv, D, R, S, N = 4, 2, 64, 3, 16, 4
    dev = "cuda"
    ok = dict(qkv=torch.zeros(R, (H + 2 * Hkv) * D, dtype=BF, device=dev),
              pos=torch.tensor([0, 5, S - 1], dtype=torch.int32, device=dev), k_cache=poisoned((N, S, Hkv, D), dev),
              v_cache=poisoned((N, S, Hkv, D), dev), q_weight=torch.ones(D, dtype=BF, device=dev),
              k_weight=torch.ones(D, dtype=BF, device=dev), n_heads=H, n_kv_heads=Hkv, head_dim=D, eps=EPS, theta=1e4)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)
    bad = [
        (TypeError, dict(qkv=ok["qkv"].float())), (TypeError, dict(pos=ok["pos"].long())),
        (TypeError, dict(k_cache=ok["k_cache"].float())), (TypeError, dict(q_weight=ok["q_weight"].float())),
        (TypeError, dict(slots=torch.zeros(R, dtype=torch.int64, device=dev))),
        (ValueError, dict(qkv=ok["qkv"].cpu())), (ValueError, dict(k_weight=ok["k_weight"].cpu())),
        (ValueError, dict(qkv=torch.zeros(R, 2 * (H + 2 * Hkv) * D, dtype=BF, device=dev)[:, ::2])),  # not contiguous
        (ValueError, dict(qkv=ok["qkv"][:, :-D].contiguous())), (ValueError, dict(pos=i32(0, 1))),
        (ValueError, dict(v_cache=poisoned((N, S + 1, Hkv, D), dev))),
        (ValueError, dict(k_cache=poisoned((N, S, Hkv + 1, D), dev), v_cache=poisoned((N, S, Hkv + 1, D), dev))),
        (ValueError, dict(head_dim=32, qkv=torch.zeros(R, (H + 2 * Hkv) * 32, dtype=BF, device=dev))),
        (ValueError, dict(head_dim=96)), (ValueError, dict(n_heads=3)),
        (ValueError, dict(pos=i32(0, 5, S))), (ValueError, dict(pos=i32(-1, 5, 6))),
        (ValueError, dict(pos_range=(0, S))),
        (ValueError, dict(slots=i32(0, 1, N))), (ValueError, dict(slots=i32(-1, 1, 2))), (ValueError, dict(slots=i32(0, 1))),
        (ValueError, dict(q_weight=torch.ones(D + 8, dtype=BF, device=dev))),
        (ValueError, dict(k_weight=torch.ones(1, D, dtype=BF, device=dev))),
        (ValueError, dict(qkv=torch.zeros(N + 1, (H + 2 * Hkv) * D, dtype=BF, device=dev),  # more rows than slots
                          pos=torch.zeros(N + 1, dtype=torch.int32, device=dev))),
        (ValueError, dict(qkv=torch.zeros(ops.MAX_ROWS + 1, (H + 2 * Hkv) * D, dtype=BF, device=dev),
                          pos=torch.zeros(ops.MAX_ROWS + 1, dtype=torch.int32, device=dev),
                          slots=torch.zeros(ops.MAX_ROWS + 1, dtype=torch.int32, device=dev))),
        (ValueError, dict(eps=float("nan"))), (ValueError, dict(theta=0.0)),
    ]
    for exc, change in bad:
        with pytest.raises(exc):
            ops.qk_norm_rope_cache(**{**ok, **change})
    torch.cuda.synchronize()
    for c in (ok["k_cache"], ok["v_cache"]):  # nothing was launched
        assert bool((c.view(torch.int16) == POISON_BITS).all())
    ops.qk_norm_rope_cache(**ok)  # and the arguments they were derived from are fine
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the kernel inside the fused step (GPU)
# One layer; D 128 with H * D = 512 != dim = 256 (Qwen3's shape), and D 64.
STAGE_CFGS = {
    "D128": LlamaConfig(vocab=512, dim=256, n_layers=1, n_heads=4, n_kv_heads=2, head_dim=128, ffn=256, max_seq=96,
                        eps=EPS, rope_theta=1e6, qk_norm=True),
    "D64": LlamaConfig(vocab=512, dim=256, n_layers=1, n_heads=4, n_kv_heads=1, head_dim=64, ffn=256, max_seq=96,
                       eps=EPS, rope_theta=1e4, qk_norm=True),
}


@cuda
@gpu
@pytest.mark.parametrize("rows", [1, 16, 40])
@pytest.mark.parametrize("name", list(STAGE_CFGS))
def test_fused_step_norm_stage_matches_fp64(name, rows):
    cfg = STAGE_CFGS[name]
    m = TinyLlama(cfg, device="cuda", max_batch=5, seed=11)  # slots 0..4 and the scratch slot 5
    pos, slots = layout(Case(cfg.head_dim, cfg.n_heads, cfg.n_kv_heads, rows, cfg.rope_theta, seed=rows))
    m.k_cache.view(torch.int16).fill_(POISON_BITS)
    m.v_cache.view(torch.int16).fill_(POISON_BITS)
    g = torch.Generator().manual_seed(rows)
    tokens = torch.randint(0, cfg.vocab, (rows,), generator=g).cuda()
    d_pos, d_slots = torch.tensor(pos, dtype=torch.int32).cuda(), torch.tensor(slots, dtype=torch.int32).cuda()
    dec = m.fused_decoder()
    plan = ops.step_plan(dec.dims, rows)
    assert plan.qk_norm_grid > 0 and plan.qkv.epi == 0 and plan.qkv_first.epi == 0
    m.decode_step(tokens, d_pos, (min(pos), max(pos)), slots=d_slots)
    torch.cuda.synchronize()
    views = dec.workspace_views()
    qkv = views["qkv"][:rows].cpu()  # what the kernel read
    assert qkv.shape == (rows, (cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim)
    assert bool(qkv.float().abs().sum() > 0)
    L = m.layers[0]
    refs = reference(qkv, L["q_norm"].cpu(), L["k_norm"].cpu(), torch.tensor(pos), cfg.n_heads, cfg.n_kv_heads,
                     cfg.head_dim, cfg.eps, cfg.rope_theta)
    ratios = check_outputs(views["q"][:rows].cpu(), m.k_cache[0].cpu(), m.v_cache[0].cpu(), refs,
                           torch.tensor(pos), torch.tensor(slots))
    print("RATIO fused", name, rows, {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios


# ---------------------------------------------------------------- model, engine, checkpoint (GPU)
# Prompts of the engine test with their greedy continuations under the fp32 reference (seed 0), each chosen with a
# comfortable top-2 margin: tests/test_qwen3_checkpoint.py::test_engine_prompts_are_confident checks them on the CPU.
def _ids(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(4096) for _ in range(n)]


# 37 tokens (chunked prefill next to nothing), one token, 71 tokens (more than one 64-row step)
ENGINE_PROMPTS = [(_ids(262, 37), [411, 3533, 1190, 3843, 1525, 3778]), (_ids(466, 1), [3410, 2569, 3896, 3999, 590, 2724]),
                  (_ids(909, 71), [616, 366, 3075, 2932, 73, 3473])]

QK2 = LlamaConfig(vocab=4096, dim=256, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, ffn=512, max_seq=512,
                  eps=EPS, rope_theta=1e6, qk_norm=True)


@cuda
@gpu
def test_qk_norm_model_fused_unfused_and_reference():
    # tests/test_gpu_model.py's tolerances and its confident-argmax rule, on a 2-layer QK-norm model.
    B, T = 3, 70  # crosses a 64-token attention split
    mf = TinyLlama(QK2, device="cuda", max_batch=B, seed=4, fused=True)
    mu = TinyLlama(QK2, device="cuda", max_batch=B, seed=4, fused=False)
    assert len(mf.fused_weights()) == 3 + 8 * QK2.n_layers
    torch.manual_seed(1)
    seqs = torch.randint(0, QK2.vocab, (B, T), device="cuda")
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
    # The norm is in the result: the same weights without it give other logits.
    plain = TinyLlama.from_weights(replace(QK2, qk_norm=False),
                                   dict(embed=mf.embed, final_norm=mf.final_norm, lm_head=mf.lm_head, layers=mf.layers),
                                   device="cuda", max_batch=B)
    assert (plain.reference_logits(seqs) - ref).abs().max().item() > 0.05 * scale


@cuda
@gpu
def test_qk_norm_graph_replay_matches_eager():
    torch.manual_seed(3)
    m = TinyLlama(QK2, device="cuda", max_batch=4, seed=2)
    m.k_cache.normal_()
    m.v_cache.normal_()
    m.capture_graph(rows=4)
    toks = torch.randint(0, QK2.vocab, (4,), device="cuda")
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
def test_engine_serves_a_qk_norm_model():
    from p2p_llm_tunnel_amd.models.server import Engine, Request
    model = TinyLlama(QK2, device="cuda:0", max_batch=4, seed=0)
    twin = TinyLlama(QK2, device="cuda:0", max_batch=1, seed=0)
    eng = Engine(model=model)
    try:
        assert len(eng._graphs) == 12
        assert ENGINE_PROMPTS
        for prompt, want in ENGINE_PROMPTS:
            r = eng.submit(Request(list(prompt), len(want)))
            got = []
            while (t := r.out.get(timeout=60)) is not None:
                got.append(t)
            assert got == twin.generate(list(prompt), len(want)) == list(want)
    finally:
        eng.stop()


@cuda
@gpu
def test_fused_decode_on_a_loaded_qwen3_checkpoint(tmp_path):
    from test_qwen3_checkpoint import hf_logits, qwen3_checkpoint
    from p2p_llm_tunnel_amd.models.checkpoint import load_llama
    hf = qwen3_checkpoint(str(tmp_path))
    ours = load_llama(str(tmp_path), device="cuda", max_batch=2, max_seq=256)
    assert ours.cfg.qk_norm and ours.fused
    torch.manual_seed(5)
    T = 33
    seqs = torch.randint(0, ours.cfg.vocab, (2, T))
    d = seqs.cuda()
    for p in range(T):
        _, logits = ours.decode_step(d[:, p], torch.full((2,), p, dtype=torch.int32, device="cuda"), (p, p),
                                     return_logits=True)
    want = hf_logits(hf, seqs)
    scale = want.abs().max().item()
    assert (logits.float().cpu() - want).abs().max().item() < 0.05 * scale
    assert torch.nn.functional.cosine_similarity(logits.float().cpu(), want, dim=-1).min().item() > 0.995

    # ... and the endpoint serves it (hipGraph path) with a tokenizer next to it, template variables included.
    import http.client
    import json
    from test_checkpoint import _tokenizer_dir
    from p2p_llm_tunnel_amd.models.server import start_server
    _tokenizer_dir(str(tmp_path))
    srv, port, eng = start_server(port=0, device="cuda:0", max_batch=2, checkpoint=str(tmp_path), max_seq=256)
    try:
        assert eng.use_graph and srv.tok is not None and eng.model.cfg.qk_norm and len(eng._graphs) == 12
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        c.request("POST", "/v1/chat/completions", body=json.dumps(
            {"stream": True, "max_tokens": 8, "messages": [{"role": "user", "content": "hello world"}],
             "chat_template_kwargs": {"enable_thinking": False}}))
        r = c.getresponse()
        data = r.read()
        assert r.status == 200 and data.rstrip().endswith(b"data: [DONE]")
    finally:
        srv.shutdown()
        eng.stop()
