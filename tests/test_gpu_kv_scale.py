"""Per-layer, per-KV-head scales of the FP8 KV cache on the GPU: the bytes the scaled writers append, ``k_attn<D, G,
true>`` with its two scalars, saturation with and without calibrated scales, the whole model, the engine and a
served checkpoint. The host side is tests/test_kv_scale.py.

Appended bytes. The inputs are tests/test_gpu_kv_fp8_wide.py's exact ones (integer embedding rows, an all-ones norm,
weights on a power-of-two grid: fp32 accumulation is exact), in two-layer models of hidden size 256 and 512 with two
KV heads. The scales are powers of two from 2^-3 to 2^4 that differ per head, per layer and between K and V, so
x * fp32(1 / s) is exact and the reference of a scaled row is that module's (x, e_pre), both divided by s. Every
appended byte is judged against it with ``judge`` (the 1 % cap on undecided elements included), both caches are
compared whole against their poison pattern, and the same bytes must equal, by ``torch.equal``, those of an unscaled
FP8 model whose K and V rows of wqkv (and bias) were multiplied by 1 / s: a power of two moves through the
accumulation, the 1/rms scale, the bias add, the bf16 rounding and the rotation unchanged. A QK-norm model's K is
normed per head, so no weight carries a per-head factor into it: there the equality covers V in both layers, and K is
held to fp64 in the last layer (whose raw projection the workspace keeps), as the wide module does.

Attention. ``k_attn<D, G, true>`` is held to ``stage_attn``'s fp64 reference and bound, computed from the observed q
and the decoded bytes times the scales. The scales are powers of two, so scale * k_scale and v_scale / L round as
scale and 1 / L do and the unscaled stage's bound holds as it stands. One head's scales are 64 times the other's.
"""
import functools
import http.client
import importlib.util
import json
import os
from types import SimpleNamespace

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models import kv_scales as kvs
from p2p_llm_tunnel_amd.models.kv_scales import KvScales
from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig, TinyLlama
from test_gpu_fused_stages import BF, F64, stage_attn, worst
from test_gpu_kv_fp8 import (F8, LOGIT_BOUND, MICRO, N_NEW, N_SLOTS, PROMPT_SEEDS, _ids, collect, decoded, judge_rows,
                             reference_generation)
from test_gpu_kv_fp8_wide import CAP, Case, cache_problems, exact_model, inputs, reference

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu


# ---------------------------------------------------------------- 1. appended bytes
class ScaledCase(Case):
    """A two-layer wide case with two KV heads at either head size (G = 2)."""

    @property
    def heads(self):
        return 4, 2


# (kind, hidden size, D, rows, max_seq): every _KV8 epilogue and both k_qknorm_rope<D, TAB, true>, D 64 and 128,
# hidden 256 (<4,1,.,2>) and 512 (<4,1,.,4>), rows 1, 16, 17 and 40 in ``layout``'s mix of single rows and prefill
# chunks on permuted slots.
BYTE_CASES = [ScaledCase(*c, seed=70 + i, layers=2) for i, c in enumerate((
    ("plain", 256, 64, 17, 128), ("bias", 512, 128, 40, 128), ("table", 256, 128, 1, 128),
    ("bias_table", 512, 64, 16, 128), ("qk_norm", 512, 128, 17, 128), ("qk_norm_table", 256, 64, 40, 128)))]
# Head 0 of K and of V carries the bias families' exact plants (2^-8, -3 * 2^-11, +-2^-12 among them). A scale of
# 2^-2, 2^-1 or 2^2 would put one of them exactly on a rounding tie of the subnormal range (2^-10 or 3 * 2^-10),
# where the reference's own error bound decides nothing: head 0 takes none of those three.
BYTE_SCALES = KvScales([[2.0 ** -3, 2.0 ** 2], [2.0 ** 4, 2.0 ** -1]], [[2.0 ** 0, 2.0 ** 3], [2.0 ** 1, 2.0 ** -2]])


def test_byte_cases_and_scales_are_what_the_module_says():
    assert {c.kind for c in BYTE_CASES} == {"plain", "bias", "table", "bias_table", "qk_norm", "qk_norm_table"}
    assert {c.rows for c in BYTE_CASES} == {1, 16, 17, 40} and {c.D for c in BYTE_CASES} == {64, 128}
    assert {(c.kind, c.D) for c in BYTE_CASES if "qk_norm" in c.kind} == {("qk_norm", 128), ("qk_norm_table", 64)}
    s = BYTE_SCALES
    every = torch.cat([s.k.flatten(), s.v.flatten()])
    assert len(set(every.tolist())) == 8 and kvs.is_power_of_two(every)
    assert every.min().item() == 2.0 ** -3 and every.max().item() == 2.0 ** 4
    assert not {2.0 ** -2, 2.0 ** -1, 2.0 ** 2} & {*s.k[:, 0].tolist(), *s.v[:, 0].tolist()}
    for c in BYTE_CASES:
        assert c.cfg.n_layers == 2 and c.cfg.n_kv_heads == 2 and c.cfg.dim in (256, 512)
        p = ops.step_plan(exact_model(c).dims(), c.rows)
        assert (p.qkv.nw, p.qkv.um) == ((4, 2) if c.dim == 256 else (4, 4))


def rescaled_weights(case, scales):
    """The case's weights with the K and V rows of wqkv (and bias) of layer L, head h times 1 / s[L][h] (V alone for
    a QK-norm model): what an unscaled FP8 model must hold to store the scaled model's bytes."""
    src, c = exact_model(case), case.cfg
    H, Hkv, D = c.n_heads, c.n_kv_heads, c.head_dim
    layers = []
    for L, lw in enumerate(src.layers):
        lw = {k: v.clone() for k, v in lw.items()}
        for which, base, s in (("k", H * D, scales.k), ("v", (H + Hkv) * D, scales.v)):
            if which == "k" and c.qk_norm:
                continue
            for h in range(Hkv):
                rows = slice(base + h * D, base + (h + 1) * D)
                for name in ("wqkv", "bqkv") if c.qkv_bias else ("wqkv",):
                    lw[name][rows] = (lw[name][rows].float() / s[L, h]).to(BF)
        layers.append(lw)
    return dict(embed=src.embed, final_norm=src.final_norm, lm_head=src.lm_head, layers=layers)


def run_step(case, weights, scales):
    """One step of the case's rows from its poisoned caches on the device: q, attn, raw and the caches as bytes."""
    inp, c = inputs(case), case.cfg
    w = dict(embed=weights["embed"].cuda(), final_norm=weights["final_norm"].cuda(), lm_head=weights["lm_head"].cuda(),
             layers=[{k: v.cuda() for k, v in L.items()} for L in weights["layers"]])
    m = TinyLlama.from_weights(c, w, device="cuda", max_batch=N_SLOTS, kv_dtype="fp8", kv_scales=scales)
    assert tuple(m.k_cache.shape) == tuple(inp.kc0.shape) and m.k_cache.dtype == F8
    m.k_cache.view(torch.uint8).copy_(inp.kc0.cuda())
    m.v_cache.view(torch.uint8).copy_(inp.vc0.cuda())
    m.decode_step(inp.tokens.cuda(), inp.pos.cuda(), (int(inp.pos.min()), int(inp.pos.max())), slots=inp.slots.cuda())
    torch.cuda.synchronize()
    views = m.fused_decoder().workspace_views()
    B = case.rows
    return dict(q=views["q"][:B].cpu(), attn=views["attn"][:B].cpu(), raw=views["qkv"][:B].cpu() if c.qk_norm else None,
                kc=m.k_cache.view(torch.uint8).cpu(), vc=m.v_cache.view(torch.uint8).cpu())


@cuda
@gpu
@pytest.mark.parametrize("case", BYTE_CASES, ids=[c.name for c in BYTE_CASES])
def test_scaled_appends_match_fp64_and_the_rescaled_model_byte_for_byte(case):
    inp, c, s = inputs(case), case.cfg, BYTE_SCALES
    src = exact_model(case)
    plain = dict(embed=src.embed, final_norm=src.final_norm, lm_head=src.lm_head, layers=src.layers)
    obs = run_step(case, plain, s)
    sl, ps = inp.slots.long(), inp.pos.long()
    x0 = inp.weights[0][inp.tokens]
    last = c.n_layers - 1
    out = {}
    for L in range(c.n_layers):
        if c.qk_norm and L != last:
            continue  # k_qknorm_rope's reference needs the raw projection, which only the last layer leaves behind
        r = reference(case, inp.weights, L, x0, inp.pos, obs["raw"] if L == last else None)
        for n, cache, sc in (("k", obs["kc"], s.k), ("v", obs["vc"], s.v)):
            div = sc[L].to(F64)[None, :, None]
            out[f"{n}{L}"] = judge_rows((r[n][0] / div, r[n][1] / div), cache[L][sl, ps])
    # both caches whole, against the poison pattern
    out["cache"] = cache_problems(case, obs["kc"], obs["vc"])
    print("RATIO kv-scale", case.name, {k: tuple(round(x, 5) for x in v) if isinstance(v, tuple) else v
                                         for k, v in out.items()})
    for key, v in out.items():
        if key != "cache":
            assert v[0] <= 1.0 and v[1] == 0, (key, out)
    assert (out[f"k{last}"][2] + out[f"v{last}"][2]) / 2 <= CAP, out
    assert out["cache"] == [], out
    # the scales are in use: the same step without them stores other bytes in K and in V
    bare = run_step(case, plain, None)
    assert not torch.equal(bare["kc"], obs["kc"]) and not torch.equal(bare["vc"], obs["vc"])
    # an unscaled FP8 model with the scales in its weights stores the same bytes
    twin = run_step(case, rescaled_weights(case, s), None)
    assert torch.equal(twin["vc"], obs["vc"])
    if not c.qk_norm:
        assert torch.equal(twin["kc"], obs["kc"])


# ---------------------------------------------------------------- 2. attention
# (D, H): G = 2, 4 and 6 over two KV heads. Rows: a 40-token context (one span slot: the single-slot exit) and a
# 401-token one (7 of 8 span slots: the cross-slot merge).
ATTN_CASES = ((64, 4), (128, 8), (64, 12))
ATTN_POS = (39, 400)
# layer 1 (the one observed): head 1's scales are 64 times head 0's; layer 0's are neither
ATTN_SCALES = KvScales([[2.0, 0.5], [2.0 ** -4, 2.0 ** 2]], [[0.25, 4.0], [2.0 ** -3, 2.0 ** 3]])


@cuda
@gpu
@pytest.mark.parametrize("D,H", ATTN_CASES, ids=[f"D{D}-G{H // 2}" for D, H in ATTN_CASES])
def test_attention_with_scales_matches_fp64(D, H):
    cfg = LlamaConfig(vocab=512, dim=256, n_layers=2, n_heads=H, n_kv_heads=2, head_dim=D, ffn=256, max_seq=512)
    s = ATTN_SCALES
    assert float(s.k[1, 1] / s.k[1, 0]) == 64.0 == float(s.v[1, 1] / s.v[1, 0])
    m = TinyLlama(cfg, device="cuda", max_batch=2, seed=9, kv_dtype="fp8", kv_scales=s)
    plan = ops.step_plan(m.dims(), 2)
    assert (plan.attn.D, plan.attn.G, plan.attn.slots) == (D, H // 2, 8) and ops.kv_plan(m.dims()).attn_kv8 == 1
    span = [ops.attn_span(p + 1, plan.attn.slots) for p in ATTN_POS]
    assert [-(-(p + 1) // sp) for p, sp in zip(ATTN_POS, span)] == [1, 7]  # span slots with tokens
    g = torch.Generator().manual_seed(D + H)
    m.k_cache.copy_((torch.randn(m.k_cache.shape, generator=g) * 2.5).to(F8))
    m.v_cache.copy_(torch.randn(m.v_cache.shape, generator=g).to(F8))
    tokens = torch.randint(0, cfg.vocab, (2,), generator=g).cuda()
    pos = torch.tensor(ATTN_POS, dtype=torch.int32)
    m.decode_step(tokens, pos.cuda(), (min(ATTN_POS), max(ATTN_POS)))
    torch.cuda.synchronize()
    views = m.fused_decoder().workspace_views()
    q, attn = views["q"][:2].cpu(), views["attn"][:2].cpu()
    kd = decoded(m.k_cache[1].view(torch.uint8).cpu()).to(F64) * s.k[1].to(F64)[None, None, :, None]
    vd = decoded(m.v_cache[1].view(torch.uint8).cpu()).to(F64) * s.v[1].to(F64)[None, None, :, None]
    ratio = worst(attn, stage_attn(SimpleNamespace(cfg=cfg), q, kd, vd, pos, None))
    # the same comparison with the heads' scales swapped, or without them, is far outside the bound
    swapped = worst(attn, stage_attn(SimpleNamespace(cfg=cfg), q, kd.flip(2), vd.flip(2), pos, None))
    print("RATIO kv-scale attn", D, H // 2, round(ratio, 4), "swapped heads", round(swapped, 1))
    assert ratio <= 1.0, ratio
    assert swapped > 10.0


# ---------------------------------------------------------------- 3. saturation
SAT_CFG = LlamaConfig(vocab=512, dim=256, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, ffn=256, max_seq=256,
                      qkv_bias=True)
SATURATED = 0x7E  # | sign: the byte of +-448


def big_k_weights(device):
    """A bias model whose K of KV head 1 reaches a few thousand (the bias and the rows times 1024)."""
    base = TinyLlama(SAT_CFG, device="cpu", max_batch=1, seed=5)
    for L in base.layers:
        for name in ("wqkv", "bqkv"):
            L[name][(4 + 1) * 64:(4 + 2) * 64] = (L[name][(4 + 1) * 64:(4 + 2) * 64].float() * 1024).to(BF)
    return dict(embed=base.embed.to(device), final_norm=base.final_norm.to(device), lm_head=base.lm_head.to(device),
                layers=[{k: v.to(device) for k, v in L.items()} for L in base.layers])


def calibrate_module():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scripts", "calibrate_kv.py")
    spec = importlib.util.spec_from_file_location("calibrate_kv", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@cuda
@gpu
def test_calibrated_scales_end_saturation():
    cal = calibrate_module()
    prompts = [_ids(11, 70, SAT_CFG.vocab), _ids(12, 33, SAT_CFG.vocab)]
    w = big_k_weights("cuda")
    mk = lambda **kw: TinyLlama.from_weights(SAT_CFG, w, device="cuda", max_batch=2, **kw)
    wide = mk()
    scales = cal.calibrate(wide, prompts)
    assert kvs.is_power_of_two(scales.k) and kvs.is_power_of_two(scales.v)
    ka, _ = kvs.absmax(wide.k_cache, wide.v_cache, [70, 33])
    assert float(ka[:, 1].min()) > 2000 and float(ka[:, 0].max()) < 448  # head 1 is the one that needs a scale
    assert float(scales.k[:, 1].min()) >= 8 and bool((scales.k.double() * 448 >= ka.double()).all())

    def saturated(m, layer):
        rows = torch.cat([m.k_cache[layer, s, :len(p)].view(torch.uint8) for s, p in enumerate(prompts)]).cpu()
        return (rows & 0x7F) == SATURATED

    counts, bare0 = {}, None
    for name, sc in (("scale 1", None), ("calibrated", scales)):
        m = mk(kv_dtype="fp8", kv_scales=sc)
        lengths = cal.prefill(m, prompts)
        assert lengths == [70, 33]
        counts[name] = [int(saturated(m, L).sum()) for L in range(2)]
        if sc is None:
            bare0 = saturated(m, 0)
            continue
        # Layer 0's K rows depend on the embedding rows alone, so the bf16 model's rows are the fp64 values to 2^-9
        # relatively. Below the format's last rounding boundary, 432, by more than that (424), no value over s may
        # have become +-448.
        proxy = torch.cat([wide.k_cache[0, s, :len(p)] for s, p in enumerate(prompts)]).double().cpu()
        below = (proxy.abs() / sc.k[0].double()[None, :, None]) < 424.0
        assert int((bare0 & below).sum()) > 0  # elements that saturate at scale 1 are among them
        assert int((saturated(m, 0) & below).sum()) == 0
    print("SATURATED kv-scale", counts)
    assert min(counts["scale 1"]) > 0


# ---------------------------------------------------------------- 4. the whole model, graphs, the engine
# powers of two at or below 1: K after RoPE and V of micro are a few units, so x / s stays far below 448
MODEL_SCALES = KvScales([[2.0 ** -2, 2.0 ** -1], [2.0 ** -3, 2.0 ** -2]], [[2.0 ** -1, 2.0 ** -3], [2.0 ** -2, 2.0 ** -1]])


@functools.lru_cache(maxsize=None)
def scaled_prompts():
    """The existing FP8 prompts, their margins re-checked on the CPU under the reference with MODEL_SCALES."""
    ref = TinyLlama(MICRO, device="cpu", max_batch=1, seed=0, kv_dtype="fp8", kv_scales=MODEL_SCALES)
    out = []
    for seed, n in PROMPT_SEEDS:
        prompt = _ids(seed, n)
        want, margin = reference_generation(ref, prompt, N_NEW)
        assert margin > LOGIT_BOUND, (seed, margin)
        out.append((prompt, want))
    return out


@cuda
@gpu
def test_scaled_model_graph_replay_logits_and_tokens():
    torch.manual_seed(3)
    m = TinyLlama(MICRO, device="cuda", max_batch=4, seed=2, kv_dtype="fp8", kv_scales=MODEL_SCALES)
    for c in (m.k_cache, m.v_cache):
        c.copy_(torch.randn(c.shape, device="cuda").to(F8))
    m.capture_graph(rows=4)
    toks = torch.randint(0, MICRO.vocab, (4,), device="cuda")
    pos = torch.tensor([5, 130, 0, 300], dtype=torch.int32, device="cuda")
    kc, vc = m.k_cache.clone(), m.v_cache.clone()
    ids_g, logits_g = m.graph_step(toks, pos, return_logits=True)
    ids_g, logits_g, kg, vg = ids_g.clone(), logits_g.clone(), m.k_cache.clone(), m.v_cache.clone()
    m.k_cache.copy_(kc)
    m.v_cache.copy_(vc)
    ids_e, logits_e = m.decode_step(toks, pos, (0, 300), return_logits=True)
    assert torch.equal(ids_g, ids_e) and torch.equal(logits_g.view(torch.int16), logits_e.view(torch.int16))
    assert torch.equal(kg.view(torch.uint8), m.k_cache.view(torch.uint8))
    assert torch.equal(vg.view(torch.uint8), m.v_cache.view(torch.uint8))
    assert not torch.equal(kg.view(torch.uint8), kc.view(torch.uint8))
    # the logits of a prompt's last position against the fp32 reference with the same scales
    g = TinyLlama(MICRO, device="cuda", max_batch=1, seed=0, kv_dtype="fp8", kv_scales=MODEL_SCALES)
    ref = TinyLlama(MICRO, device="cpu", max_batch=1, seed=0, kv_dtype="fp8", kv_scales=MODEL_SCALES)
    prompt = scaled_prompts()[0][0]
    n = len(prompt)
    _, logits = g.decode_step(torch.tensor(prompt, device="cuda"), torch.arange(n, dtype=torch.int32, device="cuda"),
                              (0, n - 1), return_logits=True, slots=torch.zeros(n, dtype=torch.int32, device="cuda"))
    want = ref.reference_logits(torch.tensor([prompt]))[0]
    err = (logits[-1].float().cpu() - want).abs().max().item()
    print("LOGITS kv-scale", round(err, 4), "of", round(want.abs().max().item(), 3))
    assert err <= LOGIT_BOUND * want.abs().max().item()
    for prompt, want in scaled_prompts():
        assert g.generate(list(prompt), N_NEW) == want, len(prompt)


@cuda
@gpu
def test_engine_serves_a_scaled_model():
    from p2p_llm_tunnel_amd.models.server import Engine, Request
    eng = Engine(device="cuda:0", config="micro", max_batch=4, seed=0, prefix_cache=True, kv_dtype="fp8",
                 kv_scales=MODEL_SCALES)
    try:
        m = eng.model
        assert len(eng._graphs) == 12 and m.kv_scales == MODEL_SCALES and m.fused_decoder().kv_scales is not None
        prompts = scaled_prompts()
        # one by one (the prefix cache reuses a slot in place where prompts share a start), then all at once
        for prompt, want in prompts:
            assert collect(eng.submit(Request(list(prompt), N_NEW))) == want
        hits = eng.prefix_hits
        r = eng.submit(Request(list(prompts[2][0]), N_NEW))  # resident in a free slot: an in-place hit
        assert collect(r) == prompts[2][1] and r.cached_tokens > 0 and eng.prefix_hits == hits + 1
        reqs = [eng.submit(Request(list(prompt), N_NEW)) for prompt, want in prompts]
        assert [collect(r) for r in reqs] == [want for _, want in prompts]
        # a shared prefix copied from a slot that is still generating: scales belong to (layer, head), not to a
        # slot, so the copied bytes serve the new slot as they are
        long, want = prompts[2]
        copies = eng.kv_copies
        bg = eng.submit(Request(list(long) + [5, 6, 7], 200))
        bg.out.get(timeout=60)
        r = eng.submit(Request(list(long), N_NEW))
        assert collect(r) == want and r.cached_tokens >= 64 and eng.kv_copies == copies + 1
        bg.cancelled = True
    finally:
        eng.stop()


# ---------------------------------------------------------------- 5. a served checkpoint
@cuda
@gpu
def test_endpoint_serves_a_checkpoint_with_its_scales(tmp_path):
    from safetensors.torch import load_file, save_file
    from test_checkpoint import _tokenizer_dir
    from test_gpu_qwen2 import SERVED_MESSAGES, SERVED_NEW, SERVED_SEED
    from test_qwen2_checkpoint import qwen2_checkpoint
    from p2p_llm_tunnel_amd.models.checkpoint import Tokenizer, load_llama
    from p2p_llm_tunnel_amd.models.server import kv_cache_line, start_server
    qwen2_checkpoint(str(tmp_path), tie=True, seed=SERVED_SEED)
    _tokenizer_dir(str(tmp_path))
    f = os.path.join(str(tmp_path), "model.safetensors")
    ts = load_file(f)
    for i in range(2):  # one KV head: a scalar k_scale and a [1] v_scale per layer
        ts[f"model.layers.{i}.self_attn.k_scale"] = torch.tensor(2.0 ** (-1 - i))
        ts[f"model.layers.{i}.self_attn.v_scale"] = torch.tensor([2.0 ** (-3 + i)])
    save_file(ts, f, metadata={"format": "pt"})
    tok = Tokenizer(str(tmp_path))
    ref = load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=256, kv_dtype="fp8", kv_scales="checkpoint")
    assert ref.kv_scales.k.tolist() == [[0.5], [0.25]] and ref.kv_scales.v.tolist() == [[0.125], [0.25]]
    prompt = tok.chat(SERVED_MESSAGES)
    new, margin = reference_generation(ref, prompt, SERVED_NEW)
    assert margin > LOGIT_BOUND and not set(new) & tok.eos_ids, (new, margin)
    srv, port, eng = start_server(port=0, device="cuda:0", max_batch=2, checkpoint=str(tmp_path), max_seq=256,
                                  kv_dtype="fp8", kv_scales="checkpoint")
    try:
        assert eng.use_graph and len(eng._graphs) == 12 and eng.model.kv_scales == ref.kv_scales
        assert "scales in use: k_scale 0.25 .. 0.5, v_scale 0.125 .. 0.25" in kv_cache_line(eng.model, "fp8")
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        c.request("POST", "/v1/chat/completions", body=json.dumps(
            {"stream": True, "max_tokens": SERVED_NEW, "messages": SERVED_MESSAGES}))
        r = c.getresponse()
        data = r.read()
        assert r.status == 200 and data.rstrip().endswith(b"data: [DONE]")
        objs = [json.loads(l[6:]) for l in data.split(b"\n") if l.startswith(b"data: {")]
        text = "".join(o["choices"][0]["delta"].get("content", "") for o in objs)
        assert text == tok.decode(new).rstrip("�"), (text, new)
    finally:
        srv.shutdown()
        eng.stop()
