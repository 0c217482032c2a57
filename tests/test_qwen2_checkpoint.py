"""Qwen2 / Qwen2.5 checkpoints (models/checkpoint.py: ``Qwen2ForCausalLM``, a bias on q, k and v; GQA ratios 5, 6
and 7) without a GPU: the name mapping against transformers' own Qwen2 on a synthetic checkpoint written here,
the loader and its refusals, what the fused step plans for a bias model and for the new ratios, and an fp32 NumPy
emulation of the bias epilogue held to the fp64 bound of tests/test_gpu_qwen2.py (and six one-line slips that each
leave it)."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.checkpoint import Tokenizer, load_llama, read_config
from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig, TinyLlama
from test_checkpoint import _tokenizer_dir
from test_gpu_fused_stages import emulate as emulate_step, inputs as step_inputs, stage_ratios
from test_gpu_qwen2 import (ATTN_CASES, ATTN_IDS, BF, BIAS_CASES, BIAS_IDS, ENGINE_PROMPTS, EPI_ROPE, EPI_ROPE_BIAS, Q2,
                            SERVED_SEED, bias_inputs, bias_ratios, bias_reference, served_reference)

# 6 / 1 heads of 64 on hidden size 128: ratio 6, H * D = 384 != hidden_size
QWEN2 = dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=6,
             num_key_value_heads=1, head_dim=64, max_position_embeddings=512, rms_norm_eps=1e-6, rope_theta=1e6)


def qwen2_checkpoint(path, tie=True, seed=0):
    """A random transformers Qwen2 saved as safetensors, weights rounded to bf16 so both sides compute with
    identical weights; the q / k / v biases drawn with magnitude about 2 (a lost one changes the logits)."""
    transformers = pytest.importorskip("transformers")
    cfg = transformers.Qwen2Config(**QWEN2, tie_word_embeddings=tie)
    torch.manual_seed(seed)
    m = transformers.Qwen2ForCausalLM(cfg).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() > 1:
                p.normal_(0, 0.05)
            elif name.endswith("_proj.bias"):
                p.normal_(0, 2.0)
            else:
                p.uniform_(0.8, 1.2)
            p.copy_(p.to(torch.bfloat16).float())
    m.save_pretrained(path, safe_serialization=True)
    return m


def hf_logits(m, seqs):
    with torch.no_grad():
        return m(seqs).logits[:, -1].float()


@pytest.mark.parametrize("tie", [False, True])
def test_loader_matches_transformers_qwen2(tmp_path, tie):
    m = qwen2_checkpoint(str(tmp_path), tie=tie)
    ours = load_llama(str(tmp_path), device="cpu", max_batch=2)
    c = ours.cfg
    assert (c.vocab, c.dim, c.n_layers, c.n_heads, c.n_kv_heads, c.head_dim, c.ffn) == (512, 128, 2, 6, 1, 64, 256)
    assert c.qkv_bias and not c.qk_norm and c.n_heads * c.head_dim != c.dim and c.rope_theta == 1e6 and c.eps == 1e-6
    assert c.max_seq == 512  # use_sliding_window is false in what transformers writes
    assert (ours.lm_head is ours.embed) == tie
    sd = m.state_dict()
    for i, L in enumerate(ours.layers):
        p = f"model.layers.{i}.self_attn."
        want = torch.cat([sd[p + "q_proj.bias"], sd[p + "k_proj.bias"], sd[p + "v_proj.bias"]])
        assert L["bqkv"].shape == (8 * 64,) and torch.equal(L["bqkv"].float(), want)
        assert float(L["bqkv"].float().abs().mean()) > 1.0
    torch.manual_seed(3)
    seqs = torch.randint(0, c.vocab, (2, 29))
    ref = ours.reference_logits(seqs)
    hf = hf_logits(m, seqs)
    scale = hf.abs().max().item()
    # the criterion of tests/test_checkpoint.py for Llama: agreement to bf16 accuracy
    assert (ref - hf).abs().max().item() < 0.03 * scale
    assert torch.nn.functional.cosine_similarity(ref, hf, dim=-1).min().item() > 0.999
    # ... which the biases decide: without them the logits are another model's
    saved = [L["bqkv"] for L in ours.layers]
    for L in ours.layers:
        L["bqkv"] = torch.zeros_like(L["bqkv"])
    assert (ours.reference_logits(seqs) - hf).abs().max().item() > 0.03 * scale
    for L, b in zip(ours.layers, saved):
        L["bqkv"] = b
    # the fused weight table: 7 entries per layer, the bias interleaved like wqkv's rows
    table = ours.fused_weights()
    assert len(table) == 3 + 7 * c.n_layers
    heads, half = c.n_heads + 2 * c.n_kv_heads, c.head_dim // 2
    perm = (torch.arange(heads)[:, None, None] * c.head_dim + torch.arange(half)[None, :, None]
            + torch.tensor([0, half])[None, None, :]).flatten()  # head h: dims 0, D/2, 1, D/2 + 1, ...
    for i, L in enumerate(ours.layers):
        assert torch.equal(table[3 + 7 * i + 6], L["bqkv"][perm])
        folded = (L["wqkv"].float() * L["attn_norm"].float()[None]).to(torch.bfloat16)
        assert torch.equal(table[3 + 7 * i + 1], folded[perm])
    assert not torch.equal(table[3 + 6], ours.layers[0]["bqkv"])


# ---------------------------------------------------------------- loader, refusals and neutrality
H, HKV, D, DIM, FFN, V, NL = 14, 2, 64, 128, 256, 512, 2
CONF = {"architectures": ["Qwen2ForCausalLM"], "vocab_size": V, "hidden_size": DIM, "intermediate_size": FFN,
        "num_hidden_layers": NL, "num_attention_heads": H, "num_key_value_heads": HKV, "head_dim": D,
        "max_position_embeddings": 4096, "rms_norm_eps": 1e-6, "rope_theta": 1e6, "tie_word_embeddings": True,
        "use_sliding_window": False, "sliding_window": 256, "max_window_layers": 1}


def _tensors(bias=True):
    g = torch.Generator().manual_seed(0)

    def r(*s):
        return torch.randn(*s, generator=g).to(torch.bfloat16)
    ts = {"model.embed_tokens.weight": r(V, DIM), "model.norm.weight": r(DIM)}
    for i in range(NL):
        p = f"model.layers.{i}."
        ts.update({p + "input_layernorm.weight": r(DIM), p + "post_attention_layernorm.weight": r(DIM),
                   p + "self_attn.q_proj.weight": r(H * D, DIM), p + "self_attn.k_proj.weight": r(HKV * D, DIM),
                   p + "self_attn.v_proj.weight": r(HKV * D, DIM), p + "self_attn.o_proj.weight": r(DIM, H * D),
                   p + "mlp.gate_proj.weight": r(FFN, DIM), p + "mlp.up_proj.weight": r(FFN, DIM),
                   p + "mlp.down_proj.weight": r(DIM, FFN)})
        if bias:
            ts.update({p + "self_attn.q_proj.bias": r(H * D), p + "self_attn.k_proj.bias": r(HKV * D),
                       p + "self_attn.v_proj.bias": r(HKV * D)})
    return ts


def _write(path, tensors, **conf):
    save_file(tensors, str(path / "model.safetensors"))
    (path / "config.json").write_text(json.dumps(dict(CONF, **conf)))


def test_loader_refusals_and_neutrality(tmp_path):
    ts = _tensors()
    _write(tmp_path, ts)
    m = load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64)
    assert m.cfg.qkv_bias and m.cfg.head_dim == D and m.cfg.n_heads // m.cfg.n_kv_heads == 7
    p = "model.layers.1.self_attn."
    assert torch.equal(m.layers[1]["bqkv"], torch.cat([ts[p + "q_proj.bias"], ts[p + "k_proj.bias"],
                                                       ts[p + "v_proj.bias"]]))
    assert len(m.fused_weights()) == 3 + 7 * NL
    # head_dim defaults to hidden_size / num_attention_heads
    conf = {k: v for k, v in CONF.items() if k != "head_dim"}
    (tmp_path / "config.json").write_text(json.dumps(dict(conf, hidden_size=H * D)))
    assert read_config(str(tmp_path))[0].head_dim == D
    # use_sliding_window: false ignores sliding_window and max_window_layers; true caps the context
    (tmp_path / "config.json").write_text(json.dumps(CONF))
    assert read_config(str(tmp_path))[0].max_seq == 4096
    (tmp_path / "config.json").write_text(json.dumps(dict(CONF, use_sliding_window=True)))
    assert read_config(str(tmp_path))[0].max_seq == 256

    # a missing bias is the reader's KeyError naming the tensor; a wrong shape is refused
    for n in ("q", "k", "v"):
        name = f"model.layers.1.self_attn.{n}_proj.bias"
        _write(tmp_path, {k: v for k, v in ts.items() if k != name})
        with pytest.raises(KeyError, match=name.replace(".", r"\.")):
            load_llama(str(tmp_path), device="cpu", max_seq=64)
    _write(tmp_path, dict(ts, **{"model.layers.0.self_attn.k_proj.bias": torch.ones(H * D, dtype=torch.bfloat16)}))
    with pytest.raises(ValueError, match="k_proj.bias.*shape"):
        load_llama(str(tmp_path), device="cpu", max_seq=64)
    # o_proj or MLP biases: refused for every architecture
    for n, shape in (("self_attn.o_proj", DIM), ("mlp.gate_proj", FFN), ("mlp.up_proj", FFN), ("mlp.down_proj", DIM)):
        for arch, tensors in (("Qwen2ForCausalLM", ts), ("LlamaForCausalLM", _tensors(bias=False))):
            _write(tmp_path, dict(tensors, **{f"model.layers.1.{n}.bias": torch.ones(shape, dtype=torch.bfloat16)}),
                   architectures=[arch])
            with pytest.raises(ValueError, match=n.replace(".", r"\.") + r"\.bias.*only q, k and v"):
                load_llama(str(tmp_path), device="cpu", max_seq=64)

    _write(tmp_path, ts)
    for bad, msg in ((dict(architectures=["Qwen2MoeForCausalLM"]), "Qwen2MoeForCausalLM.*mixture-of-experts"),
                     (dict(mlp_bias=True), "bias"),
                     (dict(rope_scaling={"rope_type": "yarn", "factor": 4.0}), "rope"),
                     (dict(layer_types=["full_attention", "sliding_attention"]), "layer_types.*sliding_attention"),
                     (dict(num_attention_heads=6, num_key_value_heads=2), r"GQA ratio 6/2 = 3 "),
                     (dict(num_attention_heads=18, num_key_value_heads=2), r"GQA ratio 18/2 = 9 "),
                     (dict(num_attention_heads=7, num_key_value_heads=2), r"GQA ratio 7/2 ")):
        (tmp_path / "config.json").write_text(json.dumps(dict(CONF, **bad)))
        with pytest.raises(ValueError, match=msg):
            read_config(str(tmp_path))
    for arch in ("LlamaForCausalLM", "MistralForCausalLM", "Qwen3ForCausalLM"):
        for flag in ("attention_bias", "mlp_bias"):
            (tmp_path / "config.json").write_text(json.dumps(dict(CONF, architectures=[arch], **{flag: True})))
            with pytest.raises(ValueError, match="bias"):
                read_config(str(tmp_path))
    for ratio, (h, hkv) in {1: (4, 4), 2: (4, 2), 4: (8, 2), 5: (40, 8), 6: (12, 2), 7: (28, 4), 8: (16, 2)}.items():
        (tmp_path / "config.json").write_text(json.dumps(dict(CONF, num_attention_heads=h, num_key_value_heads=hkv)))
        c = read_config(str(tmp_path))[0]
        assert c.n_heads // c.n_kv_heads == ratio

    # A Llama, Mistral or Qwen3 checkpoint carrying q_proj.bias is refused, not loaded without it ...
    for arch in ("LlamaForCausalLM", "MistralForCausalLM", "Qwen3ForCausalLM"):
        extra = {}
        if arch == "Qwen3ForCausalLM":
            for i in range(NL):
                extra.update({f"model.layers.{i}.self_attn.{n}.weight": torch.ones(D, dtype=torch.bfloat16)
                              for n in ("q_norm", "k_norm")})
        _write(tmp_path, dict(ts, **extra), architectures=[arch])
        with pytest.raises(ValueError, match="projection biases"):
            load_llama(str(tmp_path), device="cpu", max_seq=64)
    # ... and a plain one loads as before, with six entries per layer.
    _write(tmp_path, _tensors(bias=False), architectures=["LlamaForCausalLM"])
    m = load_llama(str(tmp_path), device="cpu", max_seq=64)
    assert m.cfg.qkv_bias is False and "bqkv" not in m.layers[0] and len(m.fused_weights()) == 3 + 6 * NL


def test_model_config_rules():
    with pytest.raises(ValueError, match="qkv_bias"):
        TinyLlama(LlamaConfig(vocab=64, dim=64, n_layers=1, n_heads=1, n_kv_heads=1, head_dim=64, ffn=64, max_seq=8,
                              qkv_bias=True, qk_norm=True), device="cpu", max_batch=1)
    cfg = LlamaConfig(vocab=64, dim=64, n_layers=2, n_heads=2, n_kv_heads=1, head_dim=64, ffn=64, max_seq=8,
                      qkv_bias=True)
    m = TinyLlama(cfg, device="cpu", max_batch=1, seed=0)
    b = m.layers[1]["bqkv"].float()
    assert b.shape == (4 * 64,) and 0.5 < float(b.abs().mean()) and 2.0 < float(b.abs().max()) < 8.0
    # the same seed without the bias draws the same layer-0 projection: the flag adds a tensor, nothing else
    plain = TinyLlama(LlamaConfig(**{**cfg.__dict__, "qkv_bias": False}), device="cpu", max_batch=1, seed=0)
    assert torch.equal(plain.layers[0]["wqkv"], m.layers[0]["wqkv"]) and "bqkv" not in plain.layers[0]
    layers = [{k: v for k, v in L.items() if k != "bqkv"} for L in m.layers]
    with pytest.raises(ValueError, match="bqkv"):
        TinyLlama.from_weights(cfg, dict(embed=m.embed, final_norm=m.final_norm, lm_head=m.lm_head, layers=layers),
                               device="cpu", max_batch=1)


# ---------------------------------------------------------------- planning (the library, no device)
def _lib_or_skip():
    try:
        return ops.lib()
    except (OSError, RuntimeError) as e:  # no hipcc and no prebuilt library on this host
        pytest.skip(f"the HIP library is not available: {e}")


def _dims(qkv_bias=0, qk_norm=0, H=14, Hkv=2, D=64, dim=896, ffn=4864, vocab=151936):
    return ops.LlamaDims(vocab=vocab, dim=dim, n_layers=2, H=H, Hkv=Hkv, D=D, ffn=ffn, max_seq=2048, max_batch=9,
                         eps=1e-6, theta=1e6, qk_norm=qk_norm, qkv_bias=qkv_bias)


def _layout(lib, d):
    n = len(ops.FusedLlamaDecoder._WS_BUFFERS)
    off, cnt = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
    assert lib.p2pt_llama_ws_layout(ctypes.byref(d), off, cnt, n) == n
    return list(off), list(cnt), lib.p2pt_llama_ws_bytes(ctypes.byref(d))


def test_plan_of_a_bias_model():
    lib = _lib_or_skip()
    assert ops.LlamaDims(vocab=1).qkv_bias == 0  # every construction without the keyword keeps the old step
    assert ops.LlamaDims._fields_[-1][0] == "qkv_bias"
    for shape in (dict(), dict(H=12, Hkv=2, D=128, dim=1536, ffn=8960), dict(H=4, Hkv=2, D=64, dim=256, ffn=256, vocab=512)):
        for B in (1, 16, 17, 64):
            on, off = ops.step_plan(_dims(1, **shape), B), ops.step_plan(_dims(0, **shape), B)
            assert on.qkv.epi == on.qkv_first.epi == EPI_ROPE_BIAS == 5
            assert off.qkv.epi == off.qkv_first.epi == EPI_ROPE == 1
            assert on.qkv.kpl == on.qkv_first.kpl == 0 and on.qk_norm_grid == 0
            for name, _ in ops.StepPlan._fields_:  # nothing else moves
                a, b = getattr(on, name), getattr(off, name)
                if name in ("qkv", "qkv_first"):
                    for f, _ in ops.GemmPlan._fields_:
                        if f != "epi":
                            assert getattr(a, f) == getattr(b, f), (B, name, f)
                    continue
                if isinstance(a, ctypes.Structure):
                    a, b = bytes(a), bytes(b)
                assert a == b, (B, name)
        assert _layout(lib, _dims(1, **shape)) == _layout(lib, _dims(0, **shape))
    for bad in (_dims(2), _dims(-1), _dims(1, qk_norm=1)):
        assert lib.p2pt_llama_ws_bytes(ctypes.byref(bad)) == 0
        with pytest.raises(ValueError):
            ops.step_plan(bad, 1)
    assert lib.p2pt_llama_ws_bytes(ctypes.byref(_dims(0, qk_norm=1))) != 0


def test_plan_of_the_new_gqa_ratios():
    lib = _lib_or_skip()
    for Dd in (64, 128):
        for G in (5, 6, 7):
            for Hkv in (1, 2, 8):
                d = _dims(H=G * Hkv, Hkv=Hkv, D=Dd, dim=1024, ffn=1024, vocab=512)
                for B in (1, 16, 17, 64):
                    a = ops.step_plan(d, B).attn
                    assert (a.D, a.G, a.grid_y) == (Dd, G, B * Hkv) and 1 <= a.slots <= a.stride
        # ratio 3 stays refused (test_gpu_fused_stages pins it too), as does 9
        for Hh, Hkv in ((6, 2), (3, 1), (18, 2), (7, 2)):
            assert lib.p2pt_llama_ws_bytes(ctypes.byref(_dims(H=Hh, Hkv=Hkv, D=Dd, dim=1024, ffn=1024, vocab=512))) == 0
    for c in ATTN_CASES:  # the GPU cases launch what they claim
        assert c.cfg.n_heads // c.cfg.n_kv_heads in (5, 6, 7)
    assert {(c.cfg.head_dim, c.cfg.n_heads // c.cfg.n_kv_heads) for c in ATTN_CASES} == {(Dd, G) for Dd in (64, 128)
                                                                                         for G in (5, 6, 7)}


# ---------------------------------------------------------------- fp32 emulation of the bias epilogue (NumPy)
MUTATIONS = {  # slip -> the outputs it touches: at least one of them must leave its bound, the others must stay inside
    "bias_dropped": ("q", "k", "v"), "bias_before_scale": ("q", "k", "v"), "bias_after_rope": ("q", "k"),
    "bias_not_interleaved": ("q", "k", "v"), "v_without_bias": ("v",), "q_bias_for_k": ("k",),
}


def _bf(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(BF).float().numpy()


def emulate(case, mut=None):
    """The QKV stage of a bias model in fp32 NumPy with the kernel's rounding points: 1/rms scale, bias add, bf16
    round, rotate-half RoPE, bf16 round; ``mut`` names one slip. Returns (q [M, H, D], k rows, v rows) as bf16."""
    f32 = np.float32
    inp = bias_inputs(case)
    c = case.cfg
    Hh, Hkv, Dd, half = c.n_heads, c.n_kv_heads, c.head_dim, c.head_dim // 2
    W = inp.weights
    x = W[0][inp.tokens].float().numpy()
    w = W[4].float().numpy()
    bias = (inp.model.layers[0]["bqkv"] if mut == "bias_not_interleaved" else W[9]).float().numpy().copy()
    nq, nk = Hh * Dd, Hkv * Dd
    if mut == "q_bias_for_k":
        bias[nq:nq + nk] = bias[:nk]
    if mut == "v_without_bias":
        bias[nq + nk:] = 0
    acc = x @ w.T
    rs = (f32(1.0) / np.sqrt((x * x).sum(1, keepdims=True, dtype=f32) * f32(1.0 / c.dim) + f32(c.eps))).astype(f32)
    if mut in ("bias_dropped", "bias_after_rope"):
        t = acc * rs
    elif mut == "bias_before_scale":
        t = (acc + bias[None]) * rs
    else:
        t = acc * rs + bias[None]
    assert t.dtype == f32
    M = t.shape[0]
    t = _bf(t).reshape(M, Hh + 2 * Hkv, half, 2)  # pairs (dim i, dim i + D/2)
    i = np.arange(half, dtype=f32)
    inv = np.exp2(-f32(math.log2(c.rope_theta)) * (f32(2.0) * i) / f32(Dd)).astype(f32)
    ang = (inp.pos.numpy().astype(f32)[:, None, None] * inv[None, None, :]).astype(f32)
    cs, sn = np.cos(ang), np.sin(ang)
    x1, x2 = t[:, :Hh + Hkv, :, 0], t[:, :Hh + Hkv, :, 1]
    o = np.concatenate([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1)
    if mut == "bias_after_rope":
        b = bias[:nq + nk].reshape(1, Hh + Hkv, half, 2)
        o = o + np.concatenate([b[..., 0], b[..., 1]], -1)
        vb = bias[nq + nk:].reshape(1, Hkv, half, 2)  # v has no rotation: its bias is where it belongs
        t = t.copy()
        t[:, Hh + Hkv:] = _bf((acc * rs).reshape(M, -1, half, 2)[:, Hh + Hkv:] + vb)
    v = np.concatenate([t[:, Hh + Hkv:, :, 0], t[:, Hh + Hkv:, :, 1]], -1)
    to_bf = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(f32))).to(BF)
    return to_bf(o[:, :Hh]), to_bf(o[:, Hh:]), to_bf(v)


@pytest.mark.parametrize("case", BIAS_CASES, ids=BIAS_IDS)
def test_fp32_emulation_stays_inside_the_bound(case):
    ratios = bias_ratios(*emulate(case), bias_reference(case))
    print("EMU", case.name, {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("mut", list(MUTATIONS))
@pytest.mark.parametrize("case", [c for c in BIAS_CASES if c.bias != "zero"], ids=[c.name for c in BIAS_CASES
                                                                                   if c.bias != "zero"])
def test_one_line_slips_leave_the_bound(case, mut):
    ratios = bias_ratios(*emulate(case, mut), bias_reference(case))
    hit = MUTATIONS[mut]
    for s in hit:
        assert ratios[s] > 1.0, ratios
    assert max([r for s, r in ratios.items() if s not in hit] + [0.0]) <= 1.0, ratios


def test_the_bias_cases_cover_what_the_issue_asks():
    assert {(c.H, c.Hkv, c.D) for c in BIAS_CASES} == {(4, 2, 64), (14, 2, 64), (6, 1, 128)}
    for shape in {(c.H, c.Hkv, c.D) for c in BIAS_CASES}:
        assert {c.rows for c in BIAS_CASES if (c.H, c.Hkv, c.D) == shape} >= {1, 16, 17, 40}
    assert {c.bias for c in BIAS_CASES} == {"random", "big", "zero"}
    for c in BIAS_CASES:
        inp = bias_inputs(c)
        b = inp.model.layers[0]["bqkv"].float().abs()
        assert {"random": 2.0 < float(b.max()) < 8.0, "big": float(b.max()) == 64.0, "zero": float(b.max()) == 0.0}[c.bias]
        pos, slots = inp.pos.tolist(), inp.slots.tolist()
        assert len(set(zip(slots, pos))) == c.rows and max(slots) < 5
        if c.rows > 11:  # two prefill chunks next to the decode rows
            chunk = [p for p, s in zip(pos, slots) if s == 2]
            assert chunk == list(range(20, 28)) and slots.count(4) == c.rows - 11


@pytest.mark.parametrize("case", ATTN_CASES, ids=ATTN_IDS)
def test_fp32_emulation_of_the_new_ratio_cases_stays_inside_the_bounds(case):
    # The attention cases of the GPU module, judged by test_gpu_fused_stages' own emulation and bounds.
    ratios = stage_ratios(case, step_inputs(case).weights, emulate_step(case))
    print("EMU", case.name, {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios


# ---------------------------------------------------------------- the GPU tests' fixed inputs (see test_gpu_qwen2)
def test_engine_prompts_are_confident():
    # The greedy continuations the GPU test expects, from the fp32 reference, each with a top-2 gap of at least
    # 3 % of the largest logit: bf16-level differences between a 1-row step and a 16-row graph cannot flip them.
    assert [len(p) for p, _ in ENGINE_PROMPTS] == [37, 1, 71]
    m = TinyLlama(Q2, device="cpu", max_batch=1, seed=0)
    for prompt, want in ENGINE_PROMPTS:
        seq = list(prompt)
        for k in range(len(want)):
            lg = m.reference_logits(torch.tensor([seq]))[0]
            top = lg.topk(2).values
            assert float(top[0] - top[1]) >= 0.03 * float(lg.abs().max()), (len(prompt), k)
            assert int(lg.argmax()) == want[k]
            seq.append(want[k])


def test_served_checkpoint_is_confident(tmp_path):
    qwen2_checkpoint(str(tmp_path), tie=True, seed=SERVED_SEED)
    _tokenizer_dir(str(tmp_path))
    tok = Tokenizer(str(tmp_path))
    _, new, margin = served_reference(str(tmp_path), tok)
    assert margin >= 0.03 and max(new) < tok.tok.get_vocab_size() and not set(new) & tok.eos_ids, (new, margin)
    assert len(tok.decode(new).strip()) >= len(new)
