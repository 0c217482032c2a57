"""FP8 expert weights without a GPU (docs/MOE_FP8.md): the byte order, the weight table in Python and in C, the plan,
the loader, the sizes and the refusals."""
import ctypes

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.checkpoint import load_llama
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, LlamaConfig, TinyLlama, llama_dims, quantize_experts_
from test_moe import CONFIDENT, MIXTRAL, ROLES, _lib, mixtral_checkpoint

CFG = dict(vocab=512, dim=128, n_layers=3, n_heads=4, n_kv_heads=2, head_dim=64, ffn=192, max_seq=64, n_experts=4, top_k=2)
FP8_CONFIDENT = CONFIDENT  # tiny-moe with FP8 experts continues test_moe.py's prompts alike; the margins are held below


def test_the_confident_prompts_are_confident_with_fp8_experts():
    m = TinyLlama("tiny-moe", device="cpu", max_batch=1, seed=0, expert_dtype="fp8")
    for prompt, ref in FP8_CONFIDENT:  # the fp32 reference on the dequantised experts, as test_moe.py checks CONFIDENT
        seq = list(prompt)
        for want in ref:
            lg = m.reference_logits(torch.tensor([seq]))[0]
            top = lg.topk(2)
            assert int(top.indices[0]) == want and float(top.values[0] - top.values[1]) >= 0.03 * float(lg.abs().max())
            seq.append(want)


@pytest.mark.parametrize("K", [64, 192, 1408])
def test_the_byte_order_is_the_stated_rule_and_its_inverse_restores_it(K):
    nat = (torch.arange(2 * 3 * K) % 251).to(torch.uint8).view(2, 3, K)
    dev = ops.block_expert_fp8(nat)
    for blk, g in ((b, g) for b in range(K // 64) for g in range(4)):
        at = 64 * blk + 16 * g
        assert torch.equal(dev[..., at:at + 8], nat[..., 64 * blk + 8 * g:64 * blk + 8 * g + 8])
        assert torch.equal(dev[..., at + 8:at + 16], nat[..., 64 * blk + 32 + 8 * g:64 * blk + 40 + 8 * g])
    assert torch.equal(ops.unblock_expert_fp8(dev), nat) and dev.is_contiguous()


@pytest.mark.parametrize("family", [{}, {"qkv_bias": True}, {"qk_norm": True}])
def test_the_fp8_expert_table_is_the_c_one_and_the_plan_is_the_bf16_plan(family):
    lib, cfg = _lib(), LlamaConfig(**CFG, **family)
    d, ef, R = llama_dims(cfg, 2), ops.ExpertFormat(1), len(ROLES)
    table, bf16 = ops.WeightTable(d, moe=cfg.moe, expert_format="fp8"), ops.WeightTable(d, moe=cfg.moe)
    n = R * d.n_layers
    at, sc = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    assert lib.p2pt_llama_weight_layout_experts(ctypes.byref(d), ctypes.byref(cfg.moe), ctypes.byref(ef), at, sc, n) \
        == len(table) == len(bf16) + 2 * d.n_layers
    want = {(e.name, e.layer): i for i, e in enumerate(table)}
    assert {(ROLES[j % R], None if j % R < 4 else j // R): at[j] for j in range(n) if at[j] >= 0} | \
        {(ROLES[j % R] + " scale", j // R): sc[j] for j in range(n) if sc[j] >= 0} == want
    e = table[table.scale_index("w_down", 2)]
    assert (e.dtypes, e.shape) == ((torch.float32,), (4, 128)) and table[-2].shape == (4, 384)
    assert table[table.index("w_gate_up", 1)] == ("w_gate_up", 1, ops.WEIGHT_FP8_DTYPES, (4, 384, 128), 16)
    # bf16 experts: the table and the C layout of the parent commit, through the old and the new entry point
    old = (ctypes.c_int * n)()
    assert lib.p2pt_llama_weight_layout_moe(ctypes.byref(d), ctypes.byref(cfg.moe), old, n) == len(bf16)
    assert lib.p2pt_llama_weight_layout_experts(ctypes.byref(d), ctypes.byref(cfg.moe), None, at, sc, n) == len(bf16)
    assert list(old) == list(at) and set(sc) == {-1}
    assert [(e.name, e.layer, e.shape) for e in bf16] == [(e.name, e.layer, e.shape) for e in table[:len(bf16)]]
    assert all(t.dtypes == (torch.bfloat16,) for t in ops.WeightTable(d, moe=cfg.moe, expert_format="bf16"))
    for B in (1, 16, 17, 64):  # MoePlan has no format argument: one plan, whose kernels exist in both formats
        assert ops.plan_kernels_ok(d, B, moe=cfg.moe, expert_format="fp8") and ops.plan_kernels_ok(d, B, moe=cfg.moe)


def test_the_loader_quantises_what_quantising_the_bf16_load_gives_and_the_expert_bytes_halve(tmp_path, monkeypatch):
    monkeypatch.setitem(MIXTRAL, "intermediate_size", 128)  # the checkpoint of test_moe.py at a size that blocks
    mixtral_checkpoint(str(tmp_path), tie=False)
    bf16 = load_llama(str(tmp_path), device="cpu", max_batch=2)
    fp8 = load_llama(str(tmp_path), device="cpu", max_batch=2, expert_dtype="fp8")
    c, nb = fp8.cfg, lambda t: t.numel() * t.element_size()
    for L, ref in zip(fp8.layers, bf16.layers):
        want = quantize_experts_(c, dict(ref))
        for name in ("w_gate_up_q", "w_gate_up_s", "w_down_q", "w_down_s"):
            assert torch.equal(L[name].view(torch.uint8), want[name].view(torch.uint8)), name
        assert "w_gate_up" not in L and torch.equal(L["wqkv"], ref["wqkv"]) and L["router"].dtype == torch.bfloat16
        s = ops.quantize_weight_fp8((ref["w_down"][1].float()).contiguous())[1]
        assert torch.equal(L["w_down_s"][1], s)
    experts = c.n_layers * c.n_experts * 3 * c.ffn * c.dim
    scales = c.n_layers * c.n_experts * (2 * c.ffn + c.dim) * 4
    assert bf16.weight_bytes()["gemm"] - fp8.weight_bytes()["gemm"] == experts - scales
    table = fp8.fused_weights()  # device order from here on; the dequantised experts do not move
    i = ops.WeightTable(fp8.dims(), moe=c.moe, expert_format="fp8").index("w_down", 1)
    assert torch.equal(ops.unblock_expert_fp8(table[i]).view(torch.uint8), want["w_down_q"].view(torch.uint8))
    assert torch.equal(fp8.expert_weight("w_down", 1), want["w_down_q"].float() * want["w_down_s"][..., None])
    again = TinyLlama(c, device="cpu", max_batch=2, weights={**vars(bf16), "layers": [want, want]}, expert_dtype="fp8")
    assert again.layers[0]["w_down_q"] is want["w_down_q"]


def test_refusals_carry_their_reason(tmp_path):
    cfg = LlamaConfig(**CFG)
    d, moe, odd = llama_dims(cfg, 2), cfg.moe, LlamaConfig(**{**CFG, "ffn": 96})
    x, ss = torch.zeros(1, 128, dtype=torch.bfloat16), torch.zeros(32, 64)
    q = lambda *s: torch.zeros(*s, dtype=torch.uint8)  # noqa: E731
    ffn = lambda **kw: ops.moe_ffn(x, ss, x.new_zeros(4, 128), q(4, 384, 128), q(4, 128, 192), 2, **kw)  # noqa: E731
    s_gu, s_dn = torch.ones(4, 384), torch.ones(4, 128)
    bad = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in quantize_experts_(cfg, dict(
        TinyLlama(cfg, device="cpu", max_batch=1).layers[0])).items()}
    bad["w_down_s"][2, 5] = float("inf")
    weights = {"embed": None, "final_norm": None, "lm_head": None, "layers": [bad] * 3}
    (tmp_path / "ckpt").mkdir()
    mixtral_checkpoint(str(tmp_path / "ckpt"), tie=False)  # per-expert ffn 96
    for make, err, message in (
            (lambda: TinyLlama("tiny", device="cpu", expert_dtype="fp8"), ValueError, "a dense model has no experts"),
            (lambda: TinyLlama(cfg, device="cpu", expert_dtype="fp8", fused=False), ValueError, "fused step only"),
            (lambda: TinyLlama(odd, device="cpu", expert_dtype="fp8"), ValueError, "multiples of 64"),
            (lambda: load_llama(str(tmp_path / "ckpt"), device="cpu", expert_dtype="fp8"), ValueError, "multiples of 64"),
            (lambda: ops.WeightTable(llama_dims(odd, 2), moe=moe, expert_format="fp8"), ValueError, "multiples of 64"),
            (lambda: TinyLlama(cfg, device="cpu", expert_dtype="int8"), ValueError, "expert_dtype must be one of"),
            (lambda: ops.WeightTable(d, moe=moe, expert_format="int8"), ValueError, "expert_dtype must be one of"),
            (lambda: ops.WeightTable(d, expert_format="fp8"), ValueError, "a dense model has no experts"),
            (lambda: TinyLlama(cfg, device="cpu", weight_dtype="fp8", expert_dtype="fp8"), ValueError, "bf16 only"),
            (lambda: TinyLlama(cfg, device="cpu", weights=weights, expert_dtype="fp8"), ValueError, "finite and > 0"),
            (lambda: TinyLlama(cfg, device="cpu", weights=weights), ValueError, "pass expert_dtype='fp8'"),
            (lambda: ffn(gate_up_scale=s_gu), ValueError, "both gate_up_scale and down_scale"),
            (lambda: ffn(gate_up_scale=s_gu, down_scale=s_dn[:3]), ValueError, r"down_scale must be fp32 \(4, 128\)"),
            (lambda: ffn(gate_up_scale=s_gu.double(), down_scale=s_dn), ValueError, "gate_up_scale must be fp32")):
        with pytest.raises(err, match=message):
            make()
    from p2p_llm_tunnel_amd.models.engine import Engine
    from p2p_llm_tunnel_amd.models.server import arg_parser, parse_expert_dtype, replica_cmd
    with pytest.raises(ValueError, match="fp8 experts need the graph-captured HIP step"):
        Engine(model=TinyLlama(cfg, device="cpu", max_batch=2, expert_dtype="fp8"), max_batch=2)
    with pytest.raises(ValueError, match="expert_dtype must be one of"):
        parse_expert_dtype("int8")
    a = arg_parser().parse_args(["--expert-dtype", "fp8", "--gpus", "2"])
    assert replica_cmd(a, 1)[-2:] == ["--expert-dtype", "fp8"] and "--expert-dtype" not in replica_cmd(
        arg_parser().parse_args([]), 0)
    lib, wf, ef = _lib(), ops.WeightFormat(1, 1), ops.ExpertFormat(1)  # --weight-dtype on MoE stays refused in C
    assert lib.p2pt_llama_plan_kernels_experts(ctypes.byref(d), 1, 0, ctypes.byref(wf), None, 0, ctypes.byref(moe),
                                               ctypes.byref(ef)) == -1
    dense = llama_dims(CONFIGS["micro"], 2)
    assert lib.p2pt_llama_plan_kernels_experts(ctypes.byref(dense), 1, 0, ctypes.byref(ops.WeightFormat(0, 0)), None, 0,
                                               None, ctypes.byref(ef)) == -1
