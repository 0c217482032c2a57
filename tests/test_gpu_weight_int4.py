"""Grouped int4 GEMM weights (``weight_dtype="int4g128"``) in the fused decode step, on the device (docs/WEIGHT_INT4.md).

The oracle needs no tolerance. ``W_deq = bf16((q - z) * s)`` is a bf16 number by definition, and with norm weights g
that are powers of two both ``bf16(x * g)`` (what the int4 step's normed GEMMs read) and the fold ``W_deq * g`` (what
the bf16 step's table holds) are exact, so every MFMA product is the same real number on both sides. Where the two
plans split K alike (the same waves, load batch and K parts, and a wave count that divides the quads of a K part:
read from ``ops.step_plan``, asserted below) the int4 step must therefore equal the bf16 step on the dequantised
weights bit for bit: every workspace buffer the two share, both caches whole, the logits and the ids.
"""
import functools
from dataclasses import replace

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.tiny_llm import GEMM_WEIGHTS, TinyLlama, fused_row_perm, llama_dims
from test_gpu_fused_stages import BF, SENTINEL_BITS, SENTINEL_ID, _cfg, inputs
from test_gpu_weight_fp8 import _case, as_bytes

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu
F8 = torch.float8_e4m3fn
W4 = "int4g128"

# (dim, ffn, H, Hkv, D): K of QKV and gate/up is dim, of O H * D, of down ffn. One row plans 4 K parts on O and down
# (N = 512), so their K is 2048 there: 4 quads per part for 4 waves; 17 and 40 rows plan none, and K = 512 is 4 quads.
WIDE128, WIDE64, FLAT64 = (512, 2048, 16, 4, 128), (512, 2048, 32, 4, 64), (512, 512, 8, 2, 64)
CASES = [(_case(f"d{s[0]}-f{s[1]}-D{s[4]}-r{rows}-L{L}-kv{8 if kv8 else 16}", replace(_cfg(*s, 64), n_layers=L), rows,
                700 + i), kv8)
         for i, (s, rows, L, kv8) in enumerate([(WIDE128, 1, 1, 0), (WIDE64, 1, 2, 1), (WIDE128, 17, 2, 1),
                                                (FLAT64, 17, 1, 0), (FLAT64, 40, 2, 1), (WIDE128, 40, 1, 0)])]
IDS = [c.name for c, _ in CASES]


def pow2_norm(n, salt):
    """2^-2 .. 2^2, a step of 3 (mod 5) from one k to the next: it varies inside every group of 128."""
    return torch.ldexp(torch.ones(n), ((3 * torch.arange(n) + salt) % 5 - 2).to(torch.int32)).to(BF)


def planted(N, K, salt):
    """(q, z, s) of an [N, K] weight: q over 0..15, z over 0..16 and s over 2^-14 .. 2^3, each cycling with a stride
    coprime to its range, so that every value of each occurs in every row of 256 k or more."""
    g = torch.Generator().manual_seed(salt)
    q = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    q[:, 0], q[:, 1] = 0, 15
    grp = torch.arange(N * (K // 128)).reshape(N, K // 128) + salt
    z = (grp * 5 % 17).to(torch.uint8)
    s = torch.ldexp(torch.ones(N, K // 128), (grp * 7 % 18 - 14).to(torch.int32)).to(torch.float16)
    return q, z, s


@functools.lru_cache(maxsize=None)
def models(case):
    """(int4 model, its bf16 twin on W_deq), CPU, with power-of-two norm weights."""
    cfg, m = case.cfg, inputs(case).model
    norms = lambda L, i: {n: pow2_norm(cfg.dim, 2 * i + j) for j, n in enumerate(("attn_norm", "ffn_norm"))}
    top = dict(embed=m.embed, lm_head=m.lm_head, final_norm=pow2_norm(cfg.dim, 99))
    w4, bf = [], []
    for i, L in enumerate(m.layers):
        a, b = norms(L, i), norms(L, i)
        for j, name in enumerate(GEMM_WEIGHTS):
            N, K = L[name].shape
            q, z, s = planted(N, K, 10 * i + j)
            assert {0, 15} <= set(q.flatten().tolist()) and {0, 16} <= set(z.flatten().tolist())
            assert {2.0 ** -14, 8.0} <= set(s.flatten().tolist())
            a[name + "_q"], a[name + "_s"] = ops.pack_weight_w4g(q, z, s)  # q, z, s are in the table's row order
            perm = fused_row_perm(cfg, name, "cpu")
            deq = ops.dequantize_weight_w4g(q, z, s)
            b[name] = deq[torch.argsort(perm)] if perm is not None else deq
        w4.append(a), bf.append(b)
    return (TinyLlama.from_weights(cfg, dict(top, layers=w4), device="cpu", max_batch=case.max_batch, weight_dtype=W4),
            TinyLlama.from_weights(cfg, dict(top, layers=bf), device="cpu", max_batch=case.max_batch))


def run_step(case, model, kv8, graph=False):
    """One step of a fresh decoder over ``model``'s table on caches that start from the case's kc0 / vc0; with
    ``graph`` the step is captured and the third replay's results are returned. Everything as bytes."""
    inp, B, cfg = inputs(case), case.rows, case.cfg
    cache = lambda t: (t.float().clamp(-448, 448).to(F8) if kv8 else t)[None].expand(
        cfg.n_layers, *t.shape).contiguous().cuda()
    kc, vc = cache(inp.kc0), cache(inp.vc0)
    dec = ops.FusedLlamaDecoder(llama_dims(cfg, case.max_batch + 1, kv8), [t.cuda() for t in model.fused_weights()],
                                kc, vc, weight_format=model.weight_dtype)
    logits = torch.empty(B, cfg.vocab, dtype=BF, device="cuda")
    logits.view(torch.int16).fill_(SENTINEL_BITS)
    ids = torch.full((B,), SENTINEL_ID, dtype=torch.int64, device="cuda")
    args = (inp.tokens.cuda(), inp.pos.cuda(), logits, ids, inp.slots.cuda() if inp.slots is not None else None,
            case.emit_rows)
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
    out = {name: as_bytes(v).cpu() for name, v in dec.workspace_views().items()}
    out.update(k_cache=as_bytes(kc).cpu(), v_cache=as_bytes(vc).cpu(), logits=as_bytes(logits).cpu(), ids=ids.cpu())
    return out


def plans(case, kv8):
    d = llama_dims(case.cfg, case.max_batch + 1, kv8)
    return ops.step_plan(d, case.rows, weight_format=W4), ops.step_plan(d, case.rows)


@pytest.mark.parametrize("case,kv8", CASES, ids=IDS)
def test_the_cases_split_k_as_the_bf16_plan_does(case, kv8):
    p4, p16 = plans(case, kv8)
    for stage in ("qkv_first", "qkv", "o", "gate_up", "down"):
        a, b = getattr(p4, stage), getattr(p16, stage)
        assert (a.nw, a.um, a.kpl, a.grid_x, a.grid_y) == (b.nw, b.um, b.kpl, b.grid_x, b.grid_y), stage
        assert ((a.K >> a.kpl) // 128) % a.nw == 0, (stage, a.K, a.kpl, a.nw)
    assert ops.plan_kernels_ok(llama_dims(case.cfg, case.max_batch + 1, kv8), case.rows, weight_format=W4)


@cuda
@gpu
@pytest.mark.parametrize("case,kv8", CASES, ids=IDS)
def test_int4_step_equals_the_bf16_step_on_the_dequantised_weights(case, kv8):
    w4, bf = models(case)
    got, want = run_step(case, w4, kv8), run_step(case, bf, kv8)
    assert set(got) == set(want) | {"xg"}
    for name in want:
        assert torch.equal(got[name], want[name]), (case.name, name, int((got[name] != want[name]).sum()))
    assert bool((got["ids"] != SENTINEL_ID).all())
    # xg is the last residual times the norm weight its producer was given (the final norm's: exact here).
    resid = got["resid"].view(BF).view(64, -1)[:case.rows].float()
    xg = got["xg"].view(BF).view(64, -1)[:case.rows].float()
    assert torch.equal(xg, resid * w4.final_norm.float()[None, :]) and bool(torch.isfinite(resid).all())


@cuda
@gpu
@pytest.mark.parametrize("case,kv8", [CASES[1], CASES[4]], ids=[IDS[1], IDS[4]])
def test_graph_replay_equals_the_eager_step(case, kv8):
    w4, _ = models(case)
    eager, replay = run_step(case, w4, kv8), run_step(case, w4, kv8, graph=True)
    for name in eager:
        assert torch.equal(eager[name], replay[name]), (case.name, name)


# ---------------------------------------------------------------- the general case, against fp64
from test_gpu_fused_stages import F64, U, bf64, flip, gemm_ref, rounded, silu, stage_resid, worst  # noqa: E402

# dim 384: 3 quads over 4 waves (one idle) on QKV, O and gate/up, 5 quads over 8 waves on down (ffn 640); dim 128: one
# quad, three waves idle. 3 rows and 17 rows (two row tiles). Read from the plan below, not assumed.
GENERAL = [_case(f"g-d{s[0]}-f{s[1]}-r{rows}", _cfg(*s, 64), rows, 800 + i)
           for i, (s, rows) in enumerate([((384, 640, 6, 1, 64), 3), ((384, 640, 6, 1, 64), 17), ((128, 384, 2, 1, 64), 3)])]


def normed_gemm_ref(x, g, w, eps):
    """The int4 step's normed GEMM, y = (1 / rms(x)) * sum_k bf16(x_k g_k) w_k, in fp64, and gemm_ref's bound on the
    kernel's fp32 value. The one rounding the format adds on the A side, bf16(x * g) (2^-9 relative), needs no term of
    its own: the product of two bf16 values is exact in fp32, so the rounded operand is one definite bf16 number, and
    it is part of this reference. What remains is gemm_ref's: (K + 16) U sum|a_k||w_k| / rms for the fp32 sum and
    (K / 2 + 8) U |y| for 1 / rms, which is taken from x, not from the product."""
    a, K = bf64(x.to(F64) * g.to(F64)[None, :]), x.shape[1]
    y, E = gemm_ref(a, w)
    rs = torch.rsqrt(x.to(F64).pow(2).mean(1, keepdim=True) + eps)
    return y * rs, E * rs + (K / 2 + 8) * U * (y * rs).abs()


@functools.lru_cache(maxsize=None)
def general_model(case, zero_down):
    """An int4 model with general norm weights and fp16 scales; ``zero_down``: w_down dequantises to zero (q = z), so
    that the final residual is the residual after O. Returns (model, {name: W_deq in the table's row order})."""
    cfg, m = case.cfg, inputs(case).model
    g = torch.Generator().manual_seed(case.seed)
    norm = lambda: (0.5 + torch.rand(cfg.dim, generator=g)).to(BF)
    L, deq = {"attn_norm": norm(), "ffn_norm": norm()}, {}
    for name in GEMM_WEIGHTS:
        N, K = m.layers[0][name].shape
        q = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
        z = torch.randint(0, 17, (N, K // 128), generator=g, dtype=torch.uint8)
        s = ((0.5 + torch.rand(N, K // 128, generator=g)) * 0.3 / K ** 0.5).to(torch.float16)
        if zero_down and name == "w_down":
            z = z.clamp(max=15)
            q = z.repeat_interleave(128, 1)
        L[name + "_q"], L[name + "_s"] = ops.pack_weight_w4g(q, z, s)
        deq[name] = ops.dequantize_weight_w4g(q, z, s)
    w = dict(embed=m.embed, lm_head=m.lm_head, final_norm=norm(), layers=[L])
    return TinyLlama.from_weights(cfg, w, device="cpu", max_batch=case.max_batch, weight_dtype=W4), deq


def observe(case, model):
    inp, B, cfg = inputs(case), case.rows, case.cfg
    kc, vc = inp.kc0[None].contiguous().cuda(), inp.vc0[None].contiguous().cuda()
    dec = ops.FusedLlamaDecoder(llama_dims(cfg, case.max_batch + 1), [t.cuda() for t in model.fused_weights()], kc, vc,
                                weight_format=W4)
    logits = torch.empty(B, cfg.vocab, dtype=BF, device="cuda")
    ids = torch.empty(B, dtype=torch.int64, device="cuda")
    dec.step(inp.tokens.cuda(), inp.pos.cuda(), logits, ids, inp.slots.cuda() if inp.slots is not None else None, 0)
    torch.cuda.synchronize()
    out = {k: v[:B].cpu() for k, v in dec.workspace_views().items() if k in ("attn", "resid", "h", "xg")}
    sl = inp.slots.long() if inp.slots is not None else torch.arange(B)
    out.update(v=vc[0].cpu()[sl, inp.pos.long()].reshape(B, -1), logits=logits.cpu())
    return out


@cuda
@gpu
@pytest.mark.parametrize("case", GENERAL, ids=[c.name for c in GENERAL])
def test_uneven_quad_splits_and_general_norm_weights_stay_inside_the_fp64_bounds(case):
    """Each stage's reference is computed in fp64 from the observed inputs of that stage alone, with the bounds of
    tests/test_gpu_fused_stages.py (``normed_gemm_ref`` derives why bf16(x * g) adds no term). ``xg`` is exact."""
    cfg, inp = case.cfg, inputs(case)
    p = ops.step_plan(llama_dims(cfg, case.max_batch + 1), case.rows, weight_format=W4)
    assert any(((g.K >> g.kpl) // 128) % g.nw for g in (p.qkv, p.o, p.gate_up, p.down))
    (full, deq), (cut, _) = general_model(case, False), general_model(case, True)
    a, b = observe(case, full), observe(case, cut)  # b: w_down = 0, so its resid is the residual after O
    x0, L, r1 = full.embed[inp.tokens], full.layers[0], b["resid"]
    assert torch.equal(a["attn"], b["attn"]) and torch.equal(a["h"], b["h"]) and not torch.equal(a["resid"], r1)
    ratios = {}
    nv = cfg.n_kv_heads * cfg.head_dim  # V: the last rows of plain wqkv, that is of the table's rows un-interleaved
    wv = deq["wqkv"][torch.argsort(fused_row_perm(cfg, "wqkv", "cpu"))][-nv:]
    y, E = normed_gemm_ref(x0, L["attn_norm"], wv, cfg.eps)
    ratios["v"] = worst(a["v"], (y, rounded(y, E)))
    ratios["o"] = worst(r1, stage_resid(a["attn"], deq["wo"], x0))
    y, E = normed_gemm_ref(r1, L["ffn_norm"], deq["w_gate_up"], cfg.eps)
    y, E = y.view(case.rows, -1, 2), E.view(case.rows, -1, 2)  # stage_swiglu's bound, on this reference
    gt, up, fg, fu = bf64(y[..., 0]), bf64(y[..., 1]), flip(y[..., 0], E[..., 0]), flip(y[..., 1], E[..., 1])
    dsl = torch.maximum((silu(gt + fg) - silu(gt)).abs(), (silu(gt - fg) - silu(gt)).abs())
    h = silu(gt) * up
    ratios["h"] = worst(a["h"], (h, rounded(h, dsl * up.abs() + (silu(gt).abs() + dsl) * fu + (2 * gt.abs() + 8) * U * h.abs())))
    ratios["down"] = worst(a["resid"], stage_resid(a["h"], deq["w_down"], r1))
    print(case.name, ratios)
    assert max(ratios.values()) <= 1.0, ratios
    for obs in (a, b):  # the xg store with a general g: the exact product, rounded once
        assert torch.equal(obs["xg"], (obs["resid"].double() * full.final_norm.double()[None, :]).to(BF))


# ---------------------------------------------------------------- engine and endpoint
@cuda
@gpu
@pytest.mark.parametrize("config", ("micro", "tiny"))
def test_engine_serves_int4_weights_with_as_many_graphs_as_bf16(config):
    from p2p_llm_tunnel_amd.models.server import Engine, Request
    from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS
    from test_gpu_kv_fp8 import LOGIT_BOUND, N_NEW, _ids, collect, reference_generation
    ref = Engine(device="cuda:0", config=config, max_batch=4, seed=0)
    n_graphs = len(ref._graphs)
    ref.stop()
    eng = Engine(device="cuda:0", config=config, max_batch=4, seed=0, weight_dtype=W4)
    try:
        m = eng.model
        assert len(eng._graphs) == n_graphs > 0 and m.weight_dtype == W4 and m.lm_head.dtype == BF
        assert all(L[n + "_q"].dtype == torch.uint8 and L[n + "_s"].dtype == torch.int32 and n not in L
                   for L in m.layers for n in GEMM_WEIGHTS)
        prompt = _ids(245, 20, CONFIGS[config].vocab)  # micro: found on the CPU, margin 0.082
        toks = collect(eng.submit(Request(list(prompt), N_NEW)))
        assert len(toks) == N_NEW and all(0 <= t < m.cfg.vocab for t in toks)
        assert toks == collect(eng.submit(Request(list(prompt), N_NEW)))
        if config == "micro":  # a 20-token prefill chunk and six decode steps, token for token against fp32
            cpu = TinyLlama(CONFIGS[config], device="cpu", max_batch=1, seed=0, weight_dtype=W4)
            want, margin = reference_generation(cpu, prompt, N_NEW)
            assert margin > LOGIT_BOUND and toks == want, (margin, toks, want)
    finally:
        eng.stop()


@cuda
@gpu
def test_endpoint_serves_a_checkpoint_with_the_flag(tmp_path):
    from test_checkpoint import _tokenizer_dir
    from test_gpu_qwen2 import SERVED_MESSAGES, SERVED_NEW
    from test_gpu_weight_mxfp4 import _chat
    from test_qwen2_checkpoint import qwen2_checkpoint
    from p2p_llm_tunnel_amd.models.checkpoint import Tokenizer
    from p2p_llm_tunnel_amd.models.server import Request, start_server, weights_line
    from test_gpu_kv_fp8 import collect
    qwen2_checkpoint(str(tmp_path), tie=True, seed=2)
    _tokenizer_dir(str(tmp_path))
    srv, port, eng = start_server(port=0, device="cuda:0", max_batch=2, checkpoint=str(tmp_path), max_seq=256,
                                  weight_dtype=W4)
    try:
        m = eng.model
        assert eng.use_graph and m.cfg.qkv_bias and m.weight_dtype == W4 and m.lm_head.dtype == BF
        assert f"{W4} GEMM weights {m.weight_bytes()['gemm']}" in weights_line(m, W4)
        # the endpoint's text is the engine's own greedy continuation of the chat prompt (a random model: it may be
        # all special tokens, so the tokens are compared through the tokenizer, not the text for being non-empty)
        tok = Tokenizer(str(tmp_path))
        toks = collect(eng.submit(Request(tok.chat(SERVED_MESSAGES), SERVED_NEW)))
        assert 1 <= len(toks) <= SERVED_NEW
        assert _chat(port, SERVED_MESSAGES, SERVED_NEW) == tok.decode([t for t in toks if t not in tok.eos_ids]).rstrip("\ufffd")
    finally:
        srv.shutdown()
        eng.stop()
