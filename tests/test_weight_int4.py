"""Grouped int4 weights (``weight_dtype="int4g128"``; docs/WEIGHT_INT4.md) on the host: the byte order, the quantiser, the
definition of the dequantised weight, the weight table against the library's, the plans and the refusals."""
import ctypes
from dataclasses import replace

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models import server
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, LlamaConfig, TinyLlama, llama_dims

W4 = "int4g128"
LLAMA8B = LlamaConfig(vocab=128256, dim=4096, n_layers=2, n_heads=32, n_kv_heads=8, head_dim=128, ffn=14336, max_seq=2048)


def random_qzs(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    z = torch.randint(0, 17, (N, K // 128), generator=g, dtype=torch.uint8)
    s = (torch.rand(N, K // 128, generator=g) + 0.01).to(torch.float16)
    return q, z, s


@pytest.mark.parametrize("K", (128, 384))
def test_pack_is_the_documented_order_and_unpack_its_inverse(K):
    q, z, s = random_qzs(3, K, K)
    nib, grp = ops.pack_weight_w4g(q, z, s)
    assert nib.shape == (3, K // 2) and nib.dtype == torch.uint8 and grp.shape == (3, K // 128) and grp.dtype == torch.int32
    for n in range(3):
        for Q in range(K // 128):
            word = int(grp[n, Q])
            assert word & 0xffff == int(s[n, Q].view(torch.int16)) & 0xffff and word >> 16 == int(z[n, Q])
            for kq in range(4):
                for u in range(4):
                    for j in range(8):
                        byte = int(nib[n, 64 * Q + 16 * kq + 4 * u + j // 2])
                        assert (byte >> 4 if j % 2 else byte & 15) == int(q[n, 128 * Q + 32 * u + 8 * kq + j])
    back = ops.unpack_weight_w4g(nib, grp)
    assert all(torch.equal(a, b) for a, b in zip(back, (q, z, s)))


def test_dequantise_is_the_definition():
    q, z, s = random_qzs(4, 256, 1)
    z[0, 0], z[1, 1] = 16, 0
    want = torch.empty(4, 256)
    for n in range(4):
        for k in range(256):  # fp32(q - z) * fp32(s) is exact; one rounding, to bf16
            want[n, k] = (float(q[n, k]) - float(z[n, k // 128])) * float(s[n, k // 128])
    assert torch.equal(ops.dequantize_weight_w4g(q, z, s), want.to(torch.bfloat16))


def test_the_quantiser_stays_within_half_a_step():
    """|w - W_deq| <= s / 2 (round to nearest) + 16 * 2^-11 * s (s is rounded to fp16, relative error 2^-11, which can
    push the group's largest element that far past step 15, where q is clamped) + 2^-8 |W_deq| (bf16's own rounding
    of the dequantised value, a full ulp). Groups: random, all positive (z = 0), all negative (z = 15), constant,
    all zero."""
    torch.manual_seed(2)
    w = torch.randn(6, 256)
    w[1] = w[1].abs() + 0.5
    w[2] = -w[2].abs() - 0.5
    w[3] = 0.37
    w[4] = 0.0
    q, z, s = ops.quantize_weight_w4g(w)
    assert bool((z[1] == 0).all()) and bool((z[2] == 15).all()) and int(q.max()) == 15 and int(z.max()) <= 15
    assert bool((s[4] == 2.0 ** -14).all()) and bool((q[4] == 0).all()) and bool((z[4] == 0).all())
    deq, sf = ops.dequantize_weight_w4g(q, z, s).float(), s.float().repeat_interleave(128, 1)
    assert bool(((w - deq).abs() <= sf / 2 + 16 * 2.0 ** -11 * sf + 2.0 ** -8 * deq.abs()).all())
    assert torch.equal(deq[4], torch.zeros(256)) and bool(((deq[3] - 0.37).abs() <= 0.37 * 2.0 ** -8).all())
    for bad in (w.to(torch.bfloat16), w[:, :100], torch.full((1, 128), float("nan"))):
        with pytest.raises((TypeError, ValueError)):
            ops.quantize_weight_w4g(bad)


@pytest.mark.parametrize("family", ({}, {"qk_norm": True}, {"qkv_bias": True}))
def test_the_weight_table_is_the_librarys(family):
    cfg = LlamaConfig(vocab=512, dim=256, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, ffn=384, max_seq=64, **family)
    d, f = llama_dims(cfg, 3), ops.as_weight_format(weight_format=W4)
    T, n = ops.WeightTable(d, weight_format=W4), 13 * cfg.n_layers
    idx, sidx = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    assert ops.lib().p2pt_llama_weight_layout_fmt(ctypes.byref(d), ctypes.byref(f), idx, sidx, n) == len(T)
    roles = (None, None, None, None, "attn_norm", "wqkv", "wo", "ffn_norm", "w_gate_up", "w_down", "bqkv", "q_norm", "k_norm")
    for L in range(cfg.n_layers):
        for r, name in enumerate(roles):
            if name is None:
                continue
            has = (name, L) in T._at
            assert idx[13 * L + r] == (T.index(name, L) if has else -1), (L, name)
            assert sidx[13 * L + r] == (T.scale_index(name, L) if name in ops.LAYER_GEMMS else -1), (L, name)
    e = T[T.index("w_down", 1)], T[T.scale_index("w_down", 1)], T[T.index("lm_head")]
    assert e[0][2:] == ((torch.uint8,), (256, 192), 16) and e[1][2:] == ((torch.int32,), (256, 3), 4)
    assert e[2].dtypes == (torch.bfloat16,) and (f.layers, f.lm_head) == (3, 0)
    out = ops.weight_plan(d, weight_format=W4)
    assert (out.layers, out.lm_head) == (3, 0)


@pytest.mark.parametrize("cfg", (CONFIGS["tiny"], LLAMA8B), ids=("tiny", "llama-3.1-8b"))
def test_every_row_count_plans_kernels_that_exist(cfg):
    d = llama_dims(cfg, 65)
    for B in range(1, 65):
        assert ops.plan_kernels_ok(d, B, weight_format=W4), B
        p = ops.step_plan(d, B, weight_format=W4)
        for stage in ("qkv", "o", "gate_up", "down"):
            g = getattr(p, stage)
            assert g.K % (128 << g.kpl) == 0, (B, stage)


def test_the_other_formats_plan_and_allocate_what_they_did():
    d = llama_dims(CONFIGS["tiny"], 5)
    ws = ops.lib().p2pt_llama_ws_bytes(ctypes.byref(d))
    for name in ("bf16", "fp8", "mxfp4"):
        f = ops.as_weight_format(weight_format=name)
        assert ops.lib().p2pt_llama_ws_bytes_fmt(ctypes.byref(d), ctypes.byref(f)) == ws
        for B in (1, 3, 16, 17, 64):
            assert bytes(ops.step_plan(d, B, weight_format=name)) == bytes(ops.step_plan(d, B))
    f = ops.as_weight_format(weight_format=W4)
    assert ops.lib().p2pt_llama_ws_bytes_fmt(ctypes.byref(d), ctypes.byref(f)) == ws + 64 * d.dim * 2
    off, cnt = (ctypes.c_size_t * 12)(), (ctypes.c_size_t * 12)()
    off0, cnt0 = (ctypes.c_size_t * 11)(), (ctypes.c_size_t * 11)()
    assert ops.lib().p2pt_llama_ws_layout_fmt(ctypes.byref(d), ctypes.byref(f), off, cnt, 12) == 12
    assert ops.lib().p2pt_llama_ws_layout(ctypes.byref(d), off0, cnt0, 11) == 11
    assert list(off)[:11] == list(off0) and list(cnt)[:11] == list(cnt0) and (off[11], cnt[11]) == (ws, 64 * d.dim)


def test_the_cpu_model_and_the_refusals():
    cfg = LlamaConfig(vocab=512, dim=128, n_layers=2, n_heads=2, n_kv_heads=1, head_dim=64, ffn=256, max_seq=32)
    m = TinyLlama(cfg, device="cpu", max_batch=2, weight_dtype=W4)
    assert m.lm_head.dtype == torch.bfloat16 and m.layers[0]["wo_s"].dtype == torch.int32 and "wo" not in m.layers[0]
    b = m.weight_bytes()
    assert b["gemm"] == sum(t.numel() * t.element_size() for L in m.layers for k, t in L.items() if k[-2:] in ("_q", "_s")) \
        + m.lm_head.numel() * 2
    seqs = torch.randint(0, 512, (2, 6), generator=torch.Generator().manual_seed(3))
    ref = TinyLlama.from_weights(cfg, dict(embed=m.embed, final_norm=m.final_norm, lm_head=m.lm_head, layers=[
        {k: (m.reference_weight(k, i).to(torch.bfloat16) if k + "_q" in L else L[k]) for k in
         ("attn_norm", "wqkv", "wo", "ffn_norm", "w_gate_up", "w_down")} for i, L in enumerate(m.layers)]), device="cpu")
    # the bf16 model of W_deq differs by the bf16(x * g) rounding alone: 2^-9 relative on A, a few bf16 ulps of a logit
    got, want = m.reference_logits(seqs), ref.reference_logits(seqs)
    assert not torch.equal(got, want) and float((got - want).abs().max()) < 0.05 * float(want.abs().max())
    assert server.parse_weight_dtype(W4) == W4
    assert server.arg_parser().parse_args(["--weight-dtype", W4]).weight_dtype == W4
    cmd = server.replica_cmd(server.arg_parser().parse_args(["--gpus", "2", "--weight-dtype", W4, "--port", "9000"]), 1)
    assert cmd[cmd.index("--weight-dtype") + 1] == W4
    with pytest.raises(ValueError, match="fused step only"):
        TinyLlama(cfg, device="cpu", weight_dtype=W4, fused=False)
    with pytest.raises(ValueError, match="multiples of 128"):
        TinyLlama(LlamaConfig(vocab=512, dim=128, n_layers=1, n_heads=2, n_kv_heads=1, head_dim=64, ffn=192, max_seq=32),
                  device="cpu", weight_dtype=W4)
    with pytest.raises(ValueError, match="multiples of 128"):
        ops.WeightTable(llama_dims(LlamaConfig(vocab=512, dim=192, n_layers=1, n_heads=2, n_kv_heads=1, head_dim=64,
                                               ffn=256, max_seq=32), 2), weight_format=W4)
    with pytest.raises(ValueError, match="bf16 only"):
        TinyLlama(CONFIGS["tiny-moe"], device="cpu", weight_dtype=W4)
    with pytest.raises(ValueError, match="weights need the graph-captured HIP step"):
        server.Engine(model=m)
    with pytest.raises(ValueError, match="weight_dtype='int4g128'"):
        TinyLlama.from_weights(cfg, dict(embed=m.embed, final_norm=m.final_norm, lm_head=m.lm_head, layers=m.layers),
                               device="cpu")
    for bad in (ops.WeightFormat(3, 1), ops.WeightFormat(3, 3)):
        with pytest.raises(ValueError, match="weight_format"):
            ops.as_weight_format(weight_format=bad)


# ---------------------------------------------------------------- GPTQ / AWQ checkpoints
CK = LlamaConfig(vocab=512, dim=128, n_layers=2, n_heads=2, n_kv_heads=1, head_dim=64, ffn=256, max_seq=64)
AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)
QCONF = {"gptq": dict(quant_method="gptq", bits=4, group_size=128, desc_act=False),
         "gptq_v2": dict(quant_method="gptq", bits=4, group_size=128, desc_act=False, checkpoint_format="gptq_v2"),
         "awq": dict(quant_method="awq", bits=4, group_size=128, version="gemm", zero_point=True)}


def pack_words(rows):
    """Lists of 8 nibbles to int32 words, nibble i in bits 4 i .. 4 i + 3 (two's complement above 2^31)."""
    out = []
    for nibs in rows:
        v = sum(int(x) << (4 * i) for i, x in enumerate(nibs))
        out.append(v - (1 << 32) if v >= 1 << 31 else v)
    return torch.tensor(out, dtype=torch.int32)


def packed_linear(kind, q, z, s):
    """(q, z, s) of one linear layer as the format's qweight / qzeros / scales, by the published layouts, in loops."""
    N, K = q.shape
    G = K // 128
    if kind == "awq":
        qw = pack_words([[q[8 * c + AWQ_ORDER[i], k] for i in range(8)] for k in range(K) for c in range(N // 8)]).view(K, N // 8)
        qz = pack_words([[z[8 * c + AWQ_ORDER[i], g] for i in range(8)] for g in range(G) for c in range(N // 8)])
    else:
        off = 1 if kind == "gptq" else 0  # v1 stores z - 1 (mod 16: z = 16 cannot occur there, z = 0 wraps to 15)
        qw = pack_words([[q[n, 8 * r + i] for i in range(8)] for r in range(K // 8) for n in range(N)]).view(K // 8, N)
        qz = pack_words([[(int(z[8 * c + j, g]) - off) & 15 for j in range(8)] for g in range(G) for c in range(N // 8)])
    return {"qweight": qw, "qzeros": qz.view(G, N // 8), "scales": s.T.contiguous()}


def int4_checkpoint(path, kind, bias=False, **conf):
    """A two-layer synthetic checkpoint in format ``kind`` and the TinyLlama built from the same (q, z, s) directly."""
    import json
    from safetensors.torch import save_file
    from p2p_llm_tunnel_amd.models.tiny_llm import fused_row_perm
    c = replace(CK, qkv_bias=bias)
    g = torch.Generator().manual_seed(len(kind))
    bf = lambda *shape: (torch.randn(*shape, generator=g) * 0.5).to(torch.bfloat16)
    T = {"model.embed_tokens.weight": bf(c.vocab, c.dim), "model.norm.weight": bf(c.dim), "lm_head.weight": bf(c.vocab, c.dim)}
    layers = []
    for i in range(c.n_layers):
        p, L, qzs = f"model.layers.{i}.", {}, {}
        for n, N, K in (("self_attn.q_proj", 128, 128), ("self_attn.k_proj", 64, 128), ("self_attn.v_proj", 64, 128),
                        ("self_attn.o_proj", 128, 128), ("mlp.gate_proj", 256, 128), ("mlp.up_proj", 256, 128),
                        ("mlp.down_proj", 128, 256)):
            q, z, s = random_qzs(N, K, 100 * i + N + K + len(n))
            z = z.clamp(1 if kind == "gptq" else 0, 16 if kind == "gptq" else 15)  # what the format can store
            s = (s * 0.05).to(torch.float16)
            qzs[n] = (q, z, s)
            T.update({p + n + "." + k: v for k, v in packed_linear(kind, q, z, s).items()})
            if bias and n[-6:] in ("q_proj", "k_proj", "v_proj"):
                T[p + n + ".bias"] = bf(N)
        for name, srcs in (("wqkv", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")), ("wo", ("self_attn.o_proj",)),
                           ("w_gate_up", ("mlp.gate_proj", "mlp.up_proj")), ("w_down", ("mlp.down_proj",))):
            q, z, s = (torch.cat([qzs[n][j] for n in srcs]) for j in range(3))
            perm = fused_row_perm(c, name, "cpu")
            q, z, s = (q[perm], z[perm], s[perm]) if perm is not None else (q, z, s)
            L[name + "_q"], L[name + "_s"] = ops.pack_weight_w4g(q.contiguous(), z.contiguous(), s.contiguous())
        L["attn_norm"] = T[p + "input_layernorm.weight"] = bf(c.dim)
        L["ffn_norm"] = T[p + "post_attention_layernorm.weight"] = bf(c.dim)
        if bias:
            L["bqkv"] = torch.cat([T[p + f"self_attn.{n}_proj.bias"] for n in "qkv"])
        layers.append(L)
    if kind == "gptq":
        T["model.layers.0.mlp.down_proj.g_idx"] = (torch.arange(256) // 128).to(torch.int32)
    save_file(T, f"{path}/model.safetensors")
    conf = dict(architectures=["Qwen2ForCausalLM" if bias else "LlamaForCausalLM"], vocab_size=c.vocab, hidden_size=c.dim,
                intermediate_size=c.ffn, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=64,
                max_position_embeddings=64, rms_norm_eps=c.eps, rope_theta=c.rope_theta, tie_word_embeddings=False,
                quantization_config=QCONF[kind], **conf)
    with open(f"{path}/config.json", "w") as f:
        json.dump(conf, f)
    direct = TinyLlama.from_weights(replace(c, eps=c.eps), dict(embed=T["model.embed_tokens.weight"], final_norm=T["model.norm.weight"],
                                            lm_head=T["lm_head.weight"], layers=layers), device="cpu", max_batch=2, weight_dtype=W4)
    return direct, T, conf


@pytest.mark.parametrize("kind", ("gptq", "gptq_v2", "awq"))
def test_gptq_and_awq_checkpoints_load_to_the_same_model(tmp_path, kind):
    from p2p_llm_tunnel_amd.models.checkpoint import load_llama
    direct, _, _ = int4_checkpoint(str(tmp_path), kind, bias=kind == "awq")
    m = load_llama(str(tmp_path), device="cpu", max_batch=2)  # no flag
    assert m.weight_dtype == W4 and m.cfg.qkv_bias == (kind == "awq")
    for La, Lb in zip(direct.layers, m.layers):
        assert set(La) == set(Lb) and all(torch.equal(La[k], Lb[k]) for k in La)
    seqs = torch.randint(0, 512, (2, 5), generator=torch.Generator().manual_seed(5))
    assert torch.equal(m.reference_logits(seqs), direct.reference_logits(seqs))


def test_a_bf16_checkpoint_is_quantised_round_to_nearest(tmp_path):
    from test_qwen2_checkpoint import qwen2_checkpoint
    from p2p_llm_tunnel_amd.models.checkpoint import load_llama
    from p2p_llm_tunnel_amd.models.tiny_llm import quantize_layer_
    qwen2_checkpoint(str(tmp_path), tie=False, seed=6)  # dim 128, ffn 256, but 6 heads of 64: H * D = 384
    a = load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64)
    b = load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64, weight_dtype=W4)
    want = TinyLlama.from_weights(a.cfg, dict(embed=a.embed, final_norm=a.final_norm, lm_head=a.lm_head, layers=[
        quantize_layer_(a.cfg, dict(L), W4) for L in a.layers]), device="cpu", max_batch=1, weight_dtype=W4)
    seqs = torch.randint(0, 512, (1, 5), generator=torch.Generator().manual_seed(7))
    assert b.weight_dtype == W4 and torch.equal(b.reference_logits(seqs), want.reference_logits(seqs))


REFUSALS = [(dict(bits=8), "bits"), (dict(group_size=64), "group_size"), (dict(desc_act=True), "desc_act"),
            (dict(quant_method="bitsandbytes"), "quant_method"), (dict(checkpoint_format="marlin"), "checkpoint_format")]


@pytest.mark.parametrize("change,match", REFUSALS, ids=[m for _, m in REFUSALS])
def test_gptq_configs_the_kernels_do_not_run_are_refused(change, match):
    from p2p_llm_tunnel_amd.models.checkpoint import read_quantization
    with pytest.raises(ValueError, match=match):
        read_quantization(dict(quantization_config=dict(QCONF["gptq"], **change)))
    assert read_quantization({}) is None


def test_awq_configs_and_tensors_the_kernels_do_not_run_are_refused(tmp_path):
    import json
    from safetensors.torch import save_file
    from p2p_llm_tunnel_amd.models.checkpoint import load_llama, read_quantization
    for change, match in ((dict(version="gemv"), "version"), (dict(zero_point=False), "zero_point")):
        with pytest.raises(ValueError, match=match):
            read_quantization(dict(quantization_config=dict(QCONF["awq"], **change)))
    with pytest.raises(ValueError, match="MoE"):
        read_quantization(dict(quantization_config=QCONF["awq"], num_local_experts=8))
    _, T, conf = int4_checkpoint(str(tmp_path), "gptq")
    for dt in ("fp8", "mxfp4"):
        with pytest.raises(ValueError, match="on a gptq checkpoint"):
            load_llama(str(tmp_path), device="cpu", weight_dtype=dt)
    with pytest.raises(ValueError, match="fused step only"):
        load_llama(str(tmp_path), device="cpu", fused=False)
    perm = dict(T)
    perm["model.layers.0.mlp.down_proj.g_idx"] = T["model.layers.0.mlp.down_proj.g_idx"].flip(0).contiguous()
    save_file(perm, f"{tmp_path}/model.safetensors")
    with pytest.raises(ValueError, match="g_idx is permuted"):
        load_llama(str(tmp_path), device="cpu")
    save_file(dict(T, **{"lm_head.qweight": torch.zeros(16, 512, dtype=torch.int32)}), f"{tmp_path}/model.safetensors")
    with pytest.raises(ValueError, match="quantised lm_head"):
        load_llama(str(tmp_path), device="cpu")
