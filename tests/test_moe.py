"""The routed-expert FFN without a GPU (docs/MOE.md): the Mixtral loader against transformers, the plans, the weight
table in Python and in C, and the refusals."""
import ctypes
import json

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.checkpoint import load_llama, read_config
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, LlamaConfig, TinyLlama, llama_dims

MIXTRAL = dict(vocab_size=512, hidden_size=128, intermediate_size=96, num_hidden_layers=2, num_attention_heads=4,
               num_key_value_heads=2, head_dim=64, max_position_embeddings=256, rms_norm_eps=1e-5, rope_theta=10000.0,
               num_local_experts=4, num_experts_per_tok=2, sliding_window=None)


def _lib():
    try:
        return ops.lib()
    except OSError as e:  # no hipcc and no prebuilt library on this host; a failed compile is an error, not a skip
        pytest.skip(f"HIP library unavailable: {e}")


def mixtral_checkpoint(path, tie):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.MixtralConfig(**MIXTRAL, tie_word_embeddings=tie)
    torch.manual_seed(0)
    m = transformers.MixtralForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in m.parameters():
            p.normal_(0, 0.05) if p.dim() > 1 else p.uniform_(0.8, 1.2)
            p.copy_(p.to(torch.bfloat16).float())
    m.save_pretrained(path, safe_serialization=True)
    return m


@pytest.mark.parametrize("tie", [False, True])
def test_loader_matches_transformers_mixtral(tmp_path, tie):
    m = mixtral_checkpoint(str(tmp_path), tie)
    ours = load_llama(str(tmp_path), device="cpu", max_batch=2)
    c = ours.cfg
    assert (c.dim, c.n_layers, c.ffn, c.n_experts, c.top_k, c.norm_topk) == (128, 2, 96, 4, 2, True)
    assert tuple(ours.layers[0]["w_gate_up"].shape) == (4, 192, 128) and tuple(ours.layers[1]["router"].shape) == (4, 128)
    torch.manual_seed(3)
    seqs = torch.randint(0, c.vocab, (2, 29))
    ref = ours.reference_logits(seqs)
    with torch.no_grad():
        hf = m(seqs).logits[:, -1].float()
    # the Llama loader's tolerance (test_checkpoint.py)
    assert (ref - hf).abs().max().item() < 0.03 * hf.abs().max().item()
    assert torch.nn.functional.cosine_similarity(ref, hf, dim=-1).min().item() > 0.999


def test_moe_plan_depends_on_rows_and_dims_alone():
    _lib()
    cfg = CONFIGS["tiny-moe"]
    d = llama_dims(cfg, 9)
    fields = [n for n, _ in ops.MoePlan._fields_]
    for B, rt in ((1, 1), (16, 1), (17, 2), (64, 4)):
        p, again = ops.moe_plan(d, cfg.moe, B), ops.moe_plan(llama_dims(cfg, 9), cfg.moe, B)
        assert [getattr(p, n) for n in fields] == [getattr(again, n) for n in fields]
        assert (p.route_grid, p.gu_grid_x, p.gu_grid_y, p.dn_grid_x, p.dn_grid_y) == (B, 2 * 1408 // 16, 8, 1024 // 16, 8)
        assert p.gu_rt == p.dn_rt == rt
        assert p.cb_grid == ops.step_plan(d, B).qkv.ss_in == ops.step_plan(d, B).lm_head.ss_in
        assert p.cb_grid * p.cb_cols == cfg.dim
        assert ops.plan_kernels_ok(d, B, moe=cfg.moe)


def test_a_dense_model_is_untouched_by_the_new_path():
    lib = _lib()
    d = llama_dims(CONFIGS["tiny"], 9)
    off, cnt, off2, cnt2 = ((ctypes.c_size_t * 16)() for _ in range(4))
    assert lib.p2pt_llama_ws_layout(ctypes.byref(d), off, cnt, 16) == 11
    assert lib.p2pt_llama_ws_layout_moe(ctypes.byref(d), None, off2, cnt2, 16) == 16
    assert list(off[:11]) == list(off2[:11]) and list(cnt[:11]) == list(cnt2[:11]) and not any(cnt2[11:])
    assert lib.p2pt_llama_ws_bytes(ctypes.byref(d)) == lib.p2pt_llama_ws_bytes_moe(ctypes.byref(d), None)
    assert ops.plan_kernels_ok(d, 17, moe=None) and list(ops.WeightTable(d)) == list(ops.WeightTable(d, moe=None))


# tiny-moe (seed 0) prompts and the fp32 reference's greedy continuation, searched on the CPU for a top-2 gap of at
# least 0.03 x max|logit| at every generated index (test_gpu_prefix_cache.py's "confident" margin).
def _ids(seed, n):
    return [int(t) for t in torch.randint(1, 32000, (n,), generator=torch.Generator().manual_seed(seed))]


CONFIDENT = [(_ids(14, 6), [12286, 29819, 9305, 26661, 29033]), (_ids(26, 11), [28755, 24380, 8550, 2788, 17035]),
             (_ids(53, 10), [14027, 28570, 26140, 8765, 26917])]


def test_the_confident_prompts_are_confident():
    m = TinyLlama("tiny-moe", device="cpu", max_batch=1, seed=0)
    for prompt, ref in CONFIDENT:
        seq = list(prompt)
        for want in ref:
            lg = m.reference_logits(torch.tensor([seq]))[0]
            top = lg.topk(2)
            assert int(top.indices[0]) == want and float(top.values[0] - top.values[1]) >= 0.03 * float(lg.abs().max())
            seq.append(want)


ROLES = ("embed", "final_norm", "lm_head", "inv_freq", "attn_norm", "wqkv", "wo", "ffn_norm", "w_gate_up", "w_down",
         "bqkv", "q_norm", "k_norm", "router")  # decode_fused.hip's enum Role, R_ROUTER last


@pytest.mark.parametrize("family", [{}, {"qkv_bias": True}, {"qk_norm": True}])
def test_the_moe_weight_table_is_the_c_one(family):
    lib = _lib()
    cfg = LlamaConfig(vocab=512, dim=128, n_layers=3, n_heads=4, n_kv_heads=2, head_dim=64, ffn=96, max_seq=64,
                      n_experts=4, top_k=2, **family)
    d = llama_dims(cfg, 2)
    table = ops.WeightTable(d, moe=cfg.moe)
    n = len(ROLES) * d.n_layers
    at = (ctypes.c_int * n)()
    assert lib.p2pt_llama_weight_layout_moe(ctypes.byref(d), ctypes.byref(cfg.moe), at, n) == len(table)
    R = len(ROLES)  # a global role (the first four) is reported once per layer, every time the same
    assert {(ROLES[j % R], None if j % R < 4 else j // R): at[j] for j in range(n) if at[j] >= 0} == \
        {(e.name, e.layer): i for i, e in enumerate(table)}
    assert table[table.index("w_gate_up", 1)].shape == (4, 192, 128) and table[-1].name == "router"
    assert table[table.index("w_down", 2)].shape == (4, 128, 96) and table[table.index("router", 0)].shape == (4, 128)


def test_refusals_carry_their_reason(tmp_path):
    moe = CONFIGS["tiny-moe"].moe
    for make, message in (
            (lambda: LlamaConfig(n_experts=4, top_k=5), "top_k must be 1..min"),
            (lambda: LlamaConfig(n_experts=129, top_k=2), "n_experts must be 1..128"),
            (lambda: LlamaConfig(ffn=1000, n_experts=4, top_k=2), "multiples of 32"),
            (lambda: LlamaConfig(dim=16384, ffn=32768, n_experts=2, top_k=1), "must stay below 2 GiB"),
            (lambda: TinyLlama("tiny-moe", device="cpu", weight_dtype="fp8"), "bf16 only"),
            (lambda: ops.WeightTable(llama_dims(CONFIGS["tiny-moe"], 2), weight_format="mxfp4", moe=moe), "bf16 only"),
            (lambda: TinyLlama("tiny-moe", device="cpu", fused=False), "fused step only")):
        with pytest.raises(ValueError, match=message):
            make()
    base = dict(MIXTRAL, architectures=["MixtralForCausalLM"])
    for change, message in (({"num_experts_per_tok": 9, "num_local_experts": 16}, "num_experts_per_tok 9"),
                            ({"num_local_experts": 256}, "num_local_experts 256"),
                            ({"num_local_experts": None}, "num_local_experts None")):
        (tmp_path / "config.json").write_text(json.dumps(dict(base, **change)))
        with pytest.raises(ValueError, match=message):
            read_config(str(tmp_path))


def test_a_missing_expert_a_wrong_shape_and_an_expert_bias_are_refused(tmp_path):
    from safetensors.torch import load_file, save_file
    mixtral_checkpoint(str(tmp_path), tie=False)
    f = str(tmp_path / "model.safetensors")
    good = load_file(f)
    name = "model.layers.1.block_sparse_moe.experts.3.w2.weight"
    extra = {name.replace("experts.3", "experts.4").replace("w2", "w1"): torch.zeros(96, 128)}
    for change, err, message in ((lambda t: t.pop(name), KeyError, "expert 3 of 4 is missing"),
                                 (lambda t: t.update(extra), ValueError, "more experts than num_local_experts"),
                                 (lambda t: t.update({name: t[name][:, :64].contiguous()}), ValueError, "shape"),
                                 (lambda t: t.update({name[:-6] + "bias": torch.zeros(128)}), ValueError, "expert biases")):
        tensors = dict(good)
        change(tensors)
        save_file(tensors, f)
        with pytest.raises(err, match=message):
            load_llama(str(tmp_path), device="cpu", max_batch=2)
