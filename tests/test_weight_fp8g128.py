"""Block-scaled FP8 weights (``weight_dtype="fp8g128"``; docs/WEIGHT_FP8G128.md) on the host: the quantiser against NumPy,
the byte order, the weight table against the library's, the flag, the block-FP8 checkpoint loader, the refusals."""
import copy
import ctypes
import json

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models import server
from p2p_llm_tunnel_amd.models.checkpoint import load_llama, read_quantization
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, GEMM_WEIGHTS, LlamaConfig, TinyLlama, fused_row_perm, llama_dims
from p2p_llm_tunnel_amd.utils import kv_fp8_ref

F8G, F8 = "fp8g128", torch.float8_e4m3fn
ROLES13 = (None, None, None, None, "attn_norm", "wqkv", "wo", "ffn_norm", "w_gate_up", "w_down", "bqkv", "q_norm", "k_norm")


def test_the_quantiser_is_absmax_over_448_per_group_in_numpy():
    w = torch.randn(24, 384, generator=torch.Generator().manual_seed(1)) * torch.logspace(-3, 2, 24)[:, None]
    w[3, 128:256] = 0.0  # a zero group: scale 1, zero bytes
    q, s = ops.quantize_weight_fp8g128(w)
    g = w.numpy().reshape(24, 3, 128)
    amax = np.abs(g).max(2)
    want_s = np.where(amax > 0, amax / np.float32(448.0), np.float32(1.0)).astype(np.float32)
    want_q = kv_fp8_ref.encode((g / want_s[:, :, None]).astype(np.float32)).reshape(24, 384)
    assert q.dtype == F8 and np.array_equal(s.numpy(), want_s) and np.array_equal(q.view(torch.uint8).numpy(), want_q)
    deq = ops.dequantize_weight_fp8g128(q, s).numpy().reshape(24, 3, 128)
    assert np.array_equal(deq, kv_fp8_ref.decode(want_q).reshape(24, 3, 128) * want_s[:, :, None])


@pytest.mark.parametrize("K", (128, 384))
def test_pack_is_the_documented_order_and_unpack_its_inverse(K):
    q = torch.randint(0, 256, (5, K), generator=torch.Generator().manual_seed(K), dtype=torch.uint8)
    p = ops.pack_weight_fp8g128(q)
    assert torch.equal(ops.unpack_weight_fp8g128(p), q) and torch.equal(ops.pack_weight_fp8g128(q.view(F8)).view(torch.uint8), p)
    # One planted byte per lane position: lane group g, k-step h of the pair P and byte j of the lane's eight sit at
    # 64 P + 16 g + 8 h + j and hold k = 64 P + 32 h + 8 g + j.
    for P, g, h, j in ((P, g, h, j) for P in range(K // 64) for g in range(4) for h in range(2) for j in range(8)):
        one = torch.zeros(1, K, dtype=torch.uint8)
        one[0, 64 * P + 32 * h + 8 * g + j] = 0x5A
        assert ops.pack_weight_fp8g128(one)[0].nonzero().flatten().tolist() == [64 * P + 16 * g + 8 * h + j]


@pytest.mark.parametrize("family", ({}, {"qk_norm": True}, {"qkv_bias": True}), ids=("plain", "qk_norm", "bias"))
def test_the_weight_table_is_the_librarys(family):
    cfg = LlamaConfig(vocab=512, dim=256, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, ffn=384, max_seq=64, **family)
    d, f = llama_dims(cfg, 3), ops.as_weight_format(weight_format=F8G)
    T, n = ops.WeightTable(d, weight_format=F8G), 13 * cfg.n_layers
    idx, sidx = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    assert ops.lib().p2pt_llama_weight_layout_fmt(ctypes.byref(d), ctypes.byref(f), idx, sidx, n) == len(T)
    for L, (r, name) in ((L, rn) for L in range(cfg.n_layers) for rn in enumerate(ROLES13) if rn[1]):
        assert idx[13 * L + r] == (T.index(name, L) if (name, L) in T._at else -1), (L, name)
        assert sidx[13 * L + r] == (T.scale_index(name, L) if name in ops.LAYER_GEMMS else -1), (L, name)
    e = T[T.index("w_down", 1)], T[T.scale_index("w_down", 1)], T[T.index("lm_head")], T[T.index("ffn_norm", 0)]
    assert e[0][2:] == (ops.WEIGHT_FP8_DTYPES, (256, 384), 16) and e[1][2:] == ((torch.float32,), (256, 3), 4)
    assert e[2].dtypes == (torch.bfloat16,) and e[3].align == 16 and T[-1][:2] == ("w_down scale", 1)


def test_the_cpu_model_the_flag_and_the_refusals():
    cfg = LlamaConfig(vocab=512, dim=128, n_layers=2, n_heads=2, n_kv_heads=1, head_dim=64, ffn=256, max_seq=32)
    m = TinyLlama(cfg, device="cpu", max_batch=2, weight_dtype=F8G)
    L0, perm = m.layers[0], fused_row_perm(cfg, "wqkv", "cpu")
    assert m.lm_head.dtype == torch.bfloat16 and m.lm_head_q is None and "wo" not in L0 and L0["w_down_s"].shape == (128, 2)
    # quantised per 1 x 128 group with no norm fold, in the table's row order, bytes in the kernel's order
    q, s = ops.quantize_weight_fp8g128(TinyLlama(cfg, device="cpu", max_batch=2).layers[0]["wqkv"].float()[perm].contiguous())
    assert torch.equal(L0["wqkv_q"].view(torch.uint8), ops.pack_weight_fp8g128(q).view(torch.uint8)) and torch.equal(L0["wqkv_s"], s)
    assert torch.equal(m.reference_weight("wqkv", 0)[perm], ops.dequantize_weight_fp8g128(q, s))
    cmd = server.replica_cmd(server.arg_parser().parse_args(["--gpus", "2", "--weight-dtype", F8G, "--port", "9000"]), 1)
    assert cmd[cmd.index("--weight-dtype") + 1] == F8G == server.parse_weight_dtype(F8G)
    for match, call in [("fp8g128 weights run the fused step only", lambda: TinyLlama(cfg, device="cpu", weight_dtype=F8G, fused=False)),
                        ("bf16 only", lambda: TinyLlama(CONFIGS["tiny-moe"], device="cpu", weight_dtype=F8G)),
                        ("lora: adapters need a dense bf16 model", lambda: TinyLlama(cfg, device="cpu", weight_dtype=F8G, loras={"a": 0})),
                        ("fp8g128 weights need the graph-captured HIP step", lambda: server.Engine(model=m))]:
        with pytest.raises(ValueError, match=match):
            call()


# ---------------------------------------------------------------- block-FP8 checkpoints
QCONF = dict(quant_method="fp8", fmt="e4m3", activation_scheme="dynamic", weight_block_size=[128, 128],
             modules_to_not_convert=["lm_head", "model.norm", "input_layernorm", "post_attention_layernorm"])
LINEARS = {"wqkv": {"self_attn.q_proj": (256, 128), "self_attn.k_proj": (64, 128), "self_attn.v_proj": (64, 128)},  # (N, K)
           "wo": {"self_attn.o_proj": (128, 256)}, "w_gate_up": {"mlp.gate_proj": (384, 128), "mlp.up_proj": (384, 128)},
           "w_down": {"mlp.down_proj": (128, 384)}}


def fp8_checkpoint(path, arch, scale_dtype=torch.float32, seed=0, change=None):
    """A two-layer synthetic block-FP8 checkpoint (e4m3 ``weight`` + ``weight_scale_inv`` per 128 x 128 block, written
    with torch; K / V projections have 64 rows, half a block), with the tensors of ``change`` put over its own. Returns
    per layer the hand-dequantised fp32 GEMM weights in plain row order."""
    from safetensors.torch import save_file
    g = torch.Generator().manual_seed(len(arch) + seed)
    bf = lambda *shape: (torch.randn(*shape, generator=g) * 0.5).to(torch.bfloat16)
    T = {"model.embed_tokens.weight": bf(512, 128), "model.norm.weight": bf(128), "lm_head.weight": bf(512, 128)}
    layers = []
    for p in ("model.layers.0.", "model.layers.1."):
        deq = {}
        for n, (N, K) in ((n, nk) for srcs in LINEARS.values() for n, nk in srcs.items()):
            w = torch.randn(N, K, generator=g).clamp(-3, 3).mul(100).to(F8)
            s = (torch.rand(-(-N // 128), K // 128, generator=g) * 1e-3 + 1e-4).to(scale_dtype)
            T[p + n + ".weight"], T[p + n + ".weight_scale_inv"] = w, s
            deq[n] = w.float() * s.float()[torch.arange(N) // 128][:, torch.arange(K) // 128]  # by hand, in fp32
        layers.append({name: torch.cat([deq[n] for n in srcs]) for name, srcs in LINEARS.items()})
        names = ["input_layernorm", "post_attention_layernorm"] + ["self_attn.q_norm", "self_attn.k_norm"] * (arch == "Qwen3ForCausalLM")
        T.update({p + n + ".weight": bf(64 if "self_attn" in n else 128) for n in names})
    save_file(dict(T, **(change or {})), f"{path}/model.safetensors")
    conf = dict(architectures=[arch], vocab_size=512, hidden_size=128, intermediate_size=384, num_hidden_layers=2,
                num_attention_heads=4, num_key_value_heads=1, head_dim=64, max_position_embeddings=64, rms_norm_eps=1e-5,
                rope_theta=10000.0, tie_word_embeddings=False, quantization_config=QCONF)
    with open(f"{path}/config.json", "w") as fh:
        json.dump(conf, fh)
    return layers


@pytest.mark.parametrize("arch,scale_dtype", [("Qwen3ForCausalLM", torch.float32), ("LlamaForCausalLM", torch.bfloat16)])
def test_a_block_fp8_checkpoint_loads_with_no_flag_to_the_hand_dequantised_model(tmp_path, arch, scale_dtype):
    layers = fp8_checkpoint(str(tmp_path), arch, scale_dtype)
    m = load_llama(str(tmp_path), device="cpu", max_batch=2)  # no flag
    assert m.weight_dtype == F8G and m.cfg.qk_norm == (arch == "Qwen3ForCausalLM") and m.lm_head.dtype == torch.bfloat16
    for i, name in ((i, name) for i in range(2) for name in GEMM_WEIGHTS):
        L = m.layers[i]
        assert L[name + "_q"].dtype == F8 and L[name + "_s"].dtype == torch.float32 and name not in L
        assert torch.equal(m.reference_weight(name, i), layers[i][name]), (i, name)
    by_hand = copy.copy(m)  # the same model computing with the hand-dequantised weights
    by_hand.reference_weight = lambda name, layer=None: m.reference_weight(name) if layer is None else layers[layer][name]
    seqs = torch.randint(0, 512, (2, 5), generator=torch.Generator().manual_seed(5))
    got = m.reference_logits(seqs)
    assert torch.equal(got, by_hand.reference_logits(seqs)) and bool(torch.isfinite(got).all())


# What the issue lists as refused: (quantization_config change, config.json change, tensor change, message).
REFUSALS = {"block": (dict(weight_block_size=[64, 64]), {}, {}, r"weight_block_size \[64, 64\] is not supported"),
            "per-tensor": (dict(weight_block_size=None), {}, {}, "without weight_block_size"),
            "moe": ({}, dict(num_experts=8), {}, "a quantised MoE checkpoint is not supported"),
            "lm_head": ({}, {}, {"lm_head.weight_scale_inv": torch.ones(4, 1)}, "a quantised lm_head or embedding is not supported"),
            "scale shape": ({}, {}, {"model.layers.1.mlp.down_proj.weight_scale_inv": torch.ones(1, 2)},
                            r"weight_scale_inv: shape \(1, 2\) != expected \(1, 3\)")}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_what_the_kernels_do_not_run_is_refused(tmp_path, what):
    qc, top, change, match = REFUSALS[what]
    with pytest.raises(ValueError, match=match):
        if not change:
            read_quantization(dict(quantization_config=dict(QCONF, **qc), **top))
        fp8_checkpoint(str(tmp_path), "LlamaForCausalLM", change=change)
        load_llama(str(tmp_path), device="cpu")
    assert read_quantization(dict(quantization_config=dict(QCONF, activation_scheme="static"))) == \
        {"method": "fp8", "skip": tuple(QCONF["modules_to_not_convert"])}
