"""Block-scaled FP8 GEMM weights (``weight_dtype="fp8g128"``; docs/WEIGHT_FP8G128.md) in the fused decode step, on the GPU.

Every stage of the last layer of one fused step (q after RoPE, the appended K / V rows, the residual after O, the SwiGLU
output, the final residual; for QK-norm also the raw projection), and layer 0's K / V rows of a two-layer RoPE model, are
held to the fp64 stage references of tests/test_gpu_fused_stages.py, test_gpu_qwen2.py (bias), test_gpu_llama3_rope.py
(table) and test_gpu_qk_norm.py, computed from the exact dequantised weights ``e4m3(q) * s[n][k // 128]`` and the exact
inputs each kernel read, with their ``gemm_ref`` replaced by this format's (``hook``). Its bound is derived, not measured:
``k_skinny<.., W8 = 4>`` computes, per wave, ``acc = fma(s_G, sum_{k in G} a_k q_k, acc)`` group by group. The decoded
q_k and the A values are exact bf16 numbers, so the group sums, scaled by s_G, stay inside gemm_ref's own
(K + 16) U sum|a_k||w_k| with w = q s (the reference's w_k = fl(q_k s) is off by U relatively, once: inside the slack of
16). Each FMA rounds once, U |acc| <= U sum|a_k||w_k|, K / 128 of them per row: E = (K + 16 + K / 128) U sum|a_k||w_k|
before 1/rms (``grouped``). The A operand of QKV and gate/up, ``bf16(x * g)``, is one definite bf16 number (the fp32
product of two bf16 values is exact): part of the reference, no term; 1/rms is taken from x (``normed``). An e4m3 cache
stores the fp32 value with one rounding: half a step, 2^-4 relative or 2^-10, on top of the stage's bound.

Two checks need no tolerance: a power-of-two scale commutes with every rounding of a group's sum, so bytes with scales
2^e per (row, group, layer) must give, bit for bit, what the same bytes pre-shifted by 2^e give with scale 1; and caches
that start from a poison pattern must keep it everywhere but in the appended rows.
"""
import functools
from dataclasses import replace

import pytest
import torch

import test_gpu_fused_stages as stages
import test_gpu_llama3_rope as llama3
import test_gpu_qk_norm as qkn
import test_gpu_qwen2 as qwen2
from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, GEMM_WEIGHTS, TinyLlama, fused_row_perm, llama_dims
from test_gpu_fused_stages import BF, F64, U, _cfg, bf64, inputs, rounded, table_layout, worst
from test_gpu_kv_fp8 import LOGIT_BOUND, N_NEW, _ids, collect, reference_generation
from test_gpu_weight_fp8 import FAMILY_FLAGS, _case, as_bytes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]
F8, F8G = torch.float8_e4m3fn, "fp8g128"

# (dim, ffn, H, Hkv, D): K of QKV and gate/up is dim, of O H * D, of down ffn; in groups of 128: 1, 2, 5 and 17.
# Up to 16 k-steps run 4 waves, more run 8: one group leaves three waves idle, 2 two, 5 over 8 waves three, 17 over 8
# gives two or three each. One row plans K parts where whole groups allow (down of S1 and S5B: 2 parts of one group).
S1, S2, S5, S17, S5B = (128, 256, 2, 1, 64), (256, 640, 4, 2, 64), (640, 2176, 5, 1, 128), (256, 2176, 2, 2, 128), (640, 256, 10, 2, 64)
GRID = [(S1, 1, "plain", 0, 1), (S2, 16, "bias", 1, 2), (S5, 17, "table", 0, 1), (S17, 40, "qk_norm", 1, 1),
        (S5B, 1, "plain", 1, 2), (S2, 17, "qk_norm", 0, 2), (S17, 16, "table", 1, 2), (S5B, 40, "bias", 0, 1)]
CASES = [(_case(f"d{s[0]}-f{s[1]}-D{s[4]}-r{rows}-{fam}-kv{8 if kv8 else 16}-L{L}",
                replace(_cfg(*s, 64), n_layers=L, **FAMILY_FLAGS[fam]), rows, 900 + i), kv8)
         for i, (s, rows, fam, kv8, L) in enumerate(GRID)]
IDS = [c.name for c, _ in CASES]
one_weight = lambda cfg, name, w: {table_layout(cfg).index(name, 0): w}  # all stage_qkv / stage_swiglu read of a table


@functools.lru_cache(maxsize=None)
def model(case, kind):
    """An fp8g128 CPU model of the case and {(layer, name): W_deq fp32 in table row order}. ``kind``: "general" (random
    bytes, scales, norm weights); "pow2" (norm weights 1, scales 2^-2 .. 2^2 distinct for neighbouring rows, groups and
    layers, bytes of magnitude 2^-3 .. 2^-1); "shifted" (pow2's bytes times its scales, exact in e4m3, scale 1)."""
    cfg, m = case.cfg, inputs(case).model
    g = torch.Generator().manual_seed(case.seed)
    norm = lambda: (0.5 + torch.rand(cfg.dim, generator=g)).to(BF) if kind == "general" else torch.ones(cfg.dim, dtype=BF)
    layers, deq = [], {}
    for i, src in enumerate(m.layers):
        L = dict({k: v for k, v in src.items() if k not in GEMM_WEIGHTS}, attn_norm=norm(), ffn_norm=norm())
        for j, name in enumerate(GEMM_WEIGHTS):
            N, K = src[name].shape
            r = torch.randn(N, K, generator=g)
            if kind == "general":
                q, s = (r * 100).clamp(-448, 448).to(F8), (0.5 + torch.rand(N, K // 128, generator=g)) * 0.01 / K ** 0.5
            else:
                q = (r.sign() * r.abs().clamp(2.0 ** -3, 2.0 ** -1)).to(F8)
                e = ((7 * torch.arange(N)[:, None] + 3 * torch.arange(K // 128)[None, :] + 4 * i + j) % 5 - 2).to(torch.int32)
                s = torch.ldexp(torch.ones(N, K // 128), e)
                if kind == "shifted":
                    q, s = (q.float() * s.repeat_interleave(128, 1)).to(F8), torch.ones(N, K // 128)
            L[name + "_q"], L[name + "_s"] = ops.pack_weight_fp8g128(q), s.contiguous()
            deq[i, name] = ops.dequantize_weight_fp8g128(q, s)
        layers.append(L)
    w = dict(embed=m.embed, lm_head=m.lm_head, final_norm=norm(), layers=layers)
    return TinyLlama.from_weights(cfg, w, device="cpu", max_batch=case.max_batch, weight_dtype=F8G), deq


def run_step(case, m, kv8, graph=False, zero=()):
    """One step of a fresh decoder on caches that start from the case's kc0 / vc0 in every layer (``graph``: the third
    replay's results; ``zero``: (name, layer) weights zeroed): views, caches before (k0, v0) and after, logits, ids."""
    inp, B, cfg = inputs(case), case.rows, case.cfg
    cache = lambda t: (t.float().clamp(-448, 448).to(F8) if kv8 else t)[None].expand(cfg.n_layers, *t.shape).contiguous().cuda()
    kc, vc = cache(inp.kc0), cache(inp.vc0)
    table = [t.cuda() for t in m.fused_weights()]
    dec = ops.FusedLlamaDecoder(llama_dims(cfg, case.max_batch + 1, kv8), table, kc, vc, weight_format=F8G)
    for name, layer in zero:
        table[dec.table.index(name, layer)].view(torch.uint8).zero_()
    logits = torch.zeros(B, cfg.vocab, dtype=BF, device="cuda")
    ids = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    args = (inp.tokens.cuda(), inp.pos.cuda(), logits, ids, inp.slots.cuda() if inp.slots is not None else None, case.emit_rows)
    if graph:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dec.step(*args)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                dec.step(*args)
        for _ in range(3):  # the step appends the same rows at the same positions: every replay must agree
            g.replay()
    else:
        dec.step(*args)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in dec.workspace_views().items()}
    out.update(k_cache=kc.cpu(), v_cache=vc.cpu(), k0=cache(inp.kc0).cpu(), v0=cache(inp.vc0).cpu(), logits=logits.cpu(), ids=ids.cpu())
    return out


def grouped(a, w):
    """sum_k a_k w_k in fp64 and the module docstring's bound on the kernel's fp32 value."""
    ad, wd, K = a.to(F64), w.to(F64), a.shape[1]
    return ad @ wd.T, (K + 16 + K // 128) * U * (ad.abs() @ wd.abs().T)


def normed(x, g, w, eps):
    """(1 / rms(x)) sum_k bf16(x_k g_k) w_k, with gemm_ref's (K / 2 + 8) U |y| for 1 / rms."""
    y, E = grouped(bf64(x.to(F64) * g.to(F64)[None, :]), w)
    rs = torch.rsqrt(x.to(F64).pow(2).mean(1, keepdim=True) + eps)
    return y * rs, E * rs + (x.shape[1] / 2 + 8) * U * (y * rs).abs()


def hook(mp, g):
    """The stage references' ``gemm_ref`` becomes this format's, with norm weight ``g``. It leans on those modules looking
    ``gemm_ref`` up in their own globals; with a general g an unhooked reference is wrong and the stage test fails."""
    f = lambda x, w, eps=None: grouped(x, w) if eps is None else normed(x, g, w, eps)
    for mod in (stages, qwen2, llama3):
        mp.setattr(mod, "gemm_ref", f)


def qkv_refs(mp, case, m, deq, L, x, raw):
    """((q, k, v) references and bounds of layer L from its input rows x, the raw projection's or None). QK-norm: q and
    k from ``raw``, the projection k_qknorm_rope read, v bit for bit."""
    cfg, pos, lay = case.cfg, inputs(case).pos, m.layers[L]
    H, Hkv, D = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
    hook(mp, lay["attn_norm"])
    w, perm = deq[L, "wqkv"], fused_row_perm(cfg, "wqkv", "cpu")
    bias = lay["bqkv"][perm] if cfg.qkv_bias else None
    if cfg.qk_norm:
        y, E = normed(x, lay["attn_norm"], w, cfg.eps)
        q, k, v = qkn.reference(raw, lay["q_norm"], lay["k_norm"], pos, H, Hkv, D, cfg.eps, cfg.rope_theta)
        return (q, k, (v.to(F64), torch.zeros(v.shape, dtype=F64))), (y, rounded(y, E))
    if cfg.rope_scaling is not None:
        return llama3.stage_qkv_table(cfg, w, bias, x, pos, m.rope_inv_freq()), None
    if bias is not None:
        return qwen2.stage_qkv_bias(cfg, w, bias, x, pos), None
    return stages.stage_qkv(case, one_weight(cfg, "wqkv", w), x, pos), None


@pytest.mark.parametrize("case,kv8", CASES, ids=IDS)
def test_every_stage_stays_inside_its_fp64_bound(case, kv8, monkeypatch):
    cfg, inp, B, Z = case.cfg, inputs(case), case.rows, case.cfg.n_layers - 1
    m, deq = model(case, "general")
    a = run_step(case, m, kv8)
    x0, r1 = m.embed[inp.tokens], run_step(case, m, kv8, zero=[("w_down", Z)])["resid"][:B]  # r1: the last residual after O
    x = x0 if Z == 0 else run_step(case, m, kv8, zero=[("wo", Z), ("w_down", Z)])["resid"][:B]  # the last layer's input
    rows = lambda c, L: c[L].view(F8 if kv8 else BF)[inp.slots.long(), inp.pos.long()].float()  # layer L's appended rows
    stored = lambda rb: rb if not kv8 else (rb[0], rb[1] + rb[0].abs() * 2.0 ** -4 + 2.0 ** -10)
    (q, k, v), raw = qkv_refs(monkeypatch, case, m, deq, Z, x, a["qkv"][:B] if cfg.qk_norm else None)
    ratios = dict(q=worst(a["q"][:B], q), k=worst(rows(a["k_cache"], Z), stored(k)), v=worst(rows(a["v_cache"], Z), stored(v)))
    if raw is not None:
        ratios["raw"] = worst(a["qkv"][:B], raw)
    if Z and not cfg.qk_norm:  # layer 0 of a two-layer model, through its cache rows (the rest of it is overwritten)
        (_, k, v), _ = qkv_refs(monkeypatch, case, m, deq, 0, x0, None)
        ratios.update(k0=worst(rows(a["k_cache"], 0), stored(k)), v0=worst(rows(a["v_cache"], 0), stored(v)))
    hook(monkeypatch, m.layers[Z]["ffn_norm"])
    ratios["o"] = worst(r1, stages.stage_resid(a["attn"][:B], deq[Z, "wo"], x))
    ratios["h"] = worst(a["h"][:B], stages.stage_swiglu(case, one_weight(cfg, "w_gate_up", deq[Z, "w_gate_up"]), r1))
    ratios["down"] = worst(a["resid"][:B], stages.stage_resid(a["h"][:B], deq[Z, "w_down"], r1))
    print(case.name, {k: round(v, 4) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0 and not torch.equal(a["resid"][:B], r1), ratios


@pytest.mark.parametrize("case,kv8", CASES, ids=IDS)
def test_planted_scales_equal_pre_shifted_bytes_and_scale_one_appends_its_rows_alone(case, kv8):
    (planted, _), (shifted, _), inp = model(case, "pow2"), model(case, "shifted"), inputs(case)
    got, want = run_step(case, planted, kv8), run_step(case, shifted, kv8)
    assert not [n for n in got if not torch.equal(as_bytes(got[n]), as_bytes(want[n]))]
    assert bool(torch.isfinite(got["logits"].float()).all()) and bool((got["ids"] >= 0).all())
    if case.rows in (16, 40):  # three graph replays of the scale-1 step equal its eager run
        replay = run_step(case, shifted, kv8, graph=True)
        assert not [n for n in want if not torch.equal(as_bytes(want[n]), as_bytes(replay[n]))]
    for after, before in ((want["k_cache"], want["k0"]), (want["v_cache"], want["v0"])):  # scale 1, g = 1: the poison, whole
        diff = (as_bytes(after) != as_bytes(before)).view(case.cfg.n_layers, case.max_batch + 1, case.cfg.max_seq, -1).any(-1)
        assert bool(diff[:, inp.slots.long(), inp.pos.long()].all())
        diff[:, inp.slots.long(), inp.pos.long()] = False
        assert not bool(diff.any())


# ---------------------------------------------------------------- engine and endpoint
# Prompts (2, 71 and 1 tokens) and a checkpoint seed searched on the CPU for decided tokens; both tests re-check the margins.
ENGINE_PROMPTS, SERVED_SEED, SERVED_NEW = ((478, 2), (267, 71), (466, 1)), 41, 4


def test_engine_serves_fp8g128_weights_on_twelve_graphs():
    from p2p_llm_tunnel_amd.models.server import Engine, Request
    cpu = TinyLlama(CONFIGS["micro"], device="cpu", max_batch=1, seed=0, weight_dtype=F8G)
    eng = Engine(device="cuda:0", config="micro", max_batch=4, seed=0, weight_dtype=F8G)
    try:
        assert len(eng._graphs) == 12 and eng.model.weight_dtype == F8G and eng.model.lm_head.dtype == BF
        for seed, n in ENGINE_PROMPTS:  # a prefill chunk and six decode steps each, token for token against fp32
            want, margin = reference_generation(cpu, _ids(seed, n), N_NEW)
            assert margin > LOGIT_BOUND, (seed, margin)  # every compared token is decided
            assert collect(eng.submit(Request(_ids(seed, n), N_NEW))) == want
    finally:
        eng.stop()


def test_endpoint_serves_a_block_fp8_qwen3_checkpoint_with_no_flag(tmp_path):
    from test_checkpoint import _tokenizer_dir
    from test_gpu_weight_mxfp4 import _chat
    from test_weight_fp8g128 import fp8_checkpoint
    from p2p_llm_tunnel_amd.models.checkpoint import Tokenizer, load_llama
    from p2p_llm_tunnel_amd.models.server import start_server
    fp8_checkpoint(str(tmp_path), "Qwen3ForCausalLM", seed=SERVED_SEED)
    _tokenizer_dir(str(tmp_path))
    tok, messages = Tokenizer(str(tmp_path)), [{"role": "user", "content": "hello world"}]
    new, margin = reference_generation(load_llama(str(tmp_path), device="cpu", max_batch=1), tok.chat(messages), SERVED_NEW)
    assert margin > LOGIT_BOUND and not set(new) & tok.eos_ids, (new, margin)
    srv, port, eng = start_server(port=0, device="cuda:0", max_batch=2, checkpoint=str(tmp_path))
    try:
        assert eng.use_graph and len(eng._graphs) == 12 and eng.model.cfg.qk_norm and eng.model.weight_dtype == F8G
        assert _chat(port, messages, SERVED_NEW) == tok.decode(new).rstrip("�")
    finally:
        srv.shutdown()
        eng.stop()
