"""MXFP4 expert weights without a GPU (docs/MOE_MXFP4.md): the byte order, the weight table in Python and in C, the
plans, the model against the bf16 model of its dequantised experts, the engine test's prompts, and the refusals."""
import ctypes
import functools

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.checkpoint import load_llama
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, LlamaConfig, TinyLlama, fused_row_perm, llama_dims
from test_moe import ROLES, _ids, _lib, mixtral_checkpoint

CFG = dict(vocab=512, dim=128, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, ffn=256, max_seq=64, n_experts=4, top_k=2)
MIXTRAL_8X7B = LlamaConfig(vocab=32000, dim=4096, n_layers=4, n_heads=32, n_kv_heads=8, head_dim=128, ffn=14336,
                           max_seq=2048, n_experts=8, top_k=2)
# The engine test's prompts: the pool's seeds (those of 0..39 that a search on the CPU kept; most prompts of this random
# model meet a narrow margin within three tokens), prompt tokens, greedy tokens. The rule is re-checked at every run.
POOL, PROMPT, STEPS = (3, 7, 23, 25, 32, 33), 8, 3


@functools.lru_cache(maxsize=None)
def confident_prompts():
    """``[(prompt, the fp32 reference's greedy tokens)]`` of the pool's prompts on ``tiny-moe`` with MXFP4 experts (the
    reference runs on the dequantised experts) whose top-2 margin is at least test_moe_fp8.py's 0.03 max|logit| at
    every step."""
    m, kept = TinyLlama("tiny-moe", device="cpu", max_batch=1, seed=0, expert_dtype="mxfp4"), []
    for seed in POOL:
        seq, ref = _ids(seed, PROMPT), []
        for _ in range(STEPS):
            lg = m.reference_logits(torch.tensor([seq]))[0]
            top = lg.topk(2)
            if float(top.values[0] - top.values[1]) < 0.03 * float(lg.abs().max()):
                break
            ref.append(int(top.indices[0]))
            seq.append(ref[-1])
        if len(ref) == STEPS:
            kept.append((_ids(seed, PROMPT), ref))
    return kept


def test_at_least_four_prompts_of_the_pool_are_confident_with_mxfp4_experts():
    assert len(confident_prompts()) >= 4


@pytest.mark.parametrize("K", [128, 384])
def test_the_byte_order_is_the_stated_rule_and_its_inverse_restores_it(K):
    nat = (torch.arange(2 * 3 * (K // 2)) % 251).to(torch.uint8).view(2, 3, K // 2)
    dev = ops.block_expert_mxfp4(nat)
    for blk, g, h, b in ((blk, g, h, b) for blk in range(K // 128) for g in range(4) for h in range(4) for b in range(4)):
        assert torch.equal(dev[..., 64 * blk + 16 * g + 4 * h + b], nat[..., 64 * blk + 16 * h + 4 * g + b])
    assert torch.equal(ops.unblock_expert_mxfp4(dev), nat) and dev.is_contiguous()
    if K == 384:  # the worked example: k = 275 is block 2, k-step 0, group 2, element 3: natural byte 137, device 161
        codes = torch.zeros(1, 384, dtype=torch.uint8)
        codes[0, 275] = 0xB
        packed = ops.pack_weight_mxfp4(codes)[None]
        assert packed[0, 0, 137] == 0xB0 and packed.count_nonzero() == 1
        assert ops.block_expert_mxfp4(packed)[0, 0, 161] == 0xB0


@pytest.mark.parametrize("family", [{}, {"qkv_bias": True}, {"qk_norm": True}])
def test_the_mxfp4_expert_table_is_the_c_one(family):
    lib, cfg = _lib(), LlamaConfig(**CFG, **family)
    d, ef, R = llama_dims(cfg, 2), ops.ExpertFormat(2), len(ROLES)
    table, bf16 = ops.WeightTable(d, moe=cfg.moe, expert_format="mxfp4"), ops.WeightTable(d, moe=cfg.moe)
    n = R * d.n_layers
    at, sc = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    assert lib.p2pt_llama_weight_layout_experts(ctypes.byref(d), ctypes.byref(cfg.moe), ctypes.byref(ef), at, sc, n) \
        == len(table) == len(bf16) + 2 * d.n_layers
    want = {(e.name, e.layer): i for i, e in enumerate(table)}
    assert {(ROLES[j % R], None if j % R < 4 else j // R): at[j] for j in range(n) if at[j] >= 0} | \
        {(ROLES[j % R] + " scale", j // R): sc[j] for j in range(n) if sc[j] >= 0} == want
    u8 = (torch.uint8,)
    assert table[table.index("w_gate_up", 1)] == ("w_gate_up", 1, u8, (4, 512, 64), 16)
    assert table[table.index("w_down", 0)] == ("w_down", 0, u8, (4, 128, 128), 16)
    assert table[table.scale_index("w_gate_up", 0)] == ("w_gate_up scale", 0, u8, (4, 512, 4), 4)
    assert table[table.scale_index("w_down", 1)] == ("w_down scale", 1, u8, (4, 128, 8), 4)
    assert [(e.name, e.layer) for e in bf16] == [(e.name, e.layer) for e in table[:len(bf16)]]
    m = TinyLlama(cfg, device="cpu", max_batch=1, expert_dtype="mxfp4")  # the model fills the table as described
    natural = m.layers[1]["w_down_q"]
    for e, t in zip(table, m.fused_weights()):
        assert t.dtype in e.dtypes and tuple(t.shape) == e.shape and t.data_ptr() % e.align == 0, e
    assert torch.equal(ops.unblock_expert_mxfp4(m.fused_weights()[table.index("w_down", 1)]), natural)


@pytest.mark.parametrize("cfg", [CONFIGS["tiny-moe"], MIXTRAL_8X7B], ids=["tiny-moe", "mixtral"])
def test_every_row_count_runs_the_bf16_plan_and_its_mxfp4_kernels_exist(cfg):
    _lib()
    d = llama_dims(cfg, 8)
    for B in range(1, 65):  # MoePlan has no format argument: one plan, int for int, whose kernels exist in format 2
        assert ops.plan_kernels_ok(d, B, moe=cfg.moe, expert_format="mxfp4") and ops.plan_kernels_ok(d, B, moe=cfg.moe)
        p = ops.moe_ffn_plan(B, cfg.dim, cfg.ffn, cfg.moe)
        assert bytes(p) == bytes(ops.moe_plan(d, cfg.moe, B)) and p.gu_um in (1, 2, 4) and p.gu_nw in (4, 8)


def test_the_mxfp4_model_is_the_bf16_model_of_its_dequantised_experts():
    cfg = LlamaConfig(**CFG)
    base = TinyLlama(cfg, device="cpu", max_batch=1, seed=5)
    layers = [L | {"ffn_norm": torch.ones(128).bfloat16()} for L in base.layers]  # a norm of one: the fold is exact
    top = {k: getattr(base, k) for k in ("embed", "final_norm", "lm_head")}
    q = TinyLlama(cfg, device="cpu", max_batch=1, weights={**top, "layers": layers}, expert_dtype="mxfp4")
    back = torch.argsort(fused_row_perm(cfg, "w_gate_up", "cpu"))
    deq = [{k: t for k, t in L.items() if k[:-2] not in ("w_gate_up", "w_down")} |
           {"w_gate_up": q.expert_weight("w_gate_up", i)[:, back].bfloat16().contiguous(),
            "w_down": q.expert_weight("w_down", i).bfloat16()} for i, L in enumerate(q.layers)]
    assert torch.equal(deq[0]["w_down"].float(), q.expert_weight("w_down", 0))  # every decoded value is a bf16 number
    ref = TinyLlama(cfg, device="cpu", max_batch=1, weights={**top, "layers": deq})
    seqs = torch.randint(0, 512, (2, 9), generator=torch.Generator().manual_seed(1))
    assert torch.equal(q.reference_logits(seqs), ref.reference_logits(seqs))
    c = cfg
    experts = c.n_layers * c.n_experts * 3 * c.ffn * c.dim
    assert ref.weight_bytes()["gemm"] - q.weight_bytes()["gemm"] == 2 * experts - experts // 2 - experts // 32
    again = TinyLlama(cfg, device="cpu", max_batch=1, weights={**top, "layers": q.layers}, expert_dtype="mxfp4")
    assert again.layers[0]["w_down_q"] is q.layers[0]["w_down_q"]  # layers that are MXFP4 already are taken as they are


def test_refusals_carry_their_reason(tmp_path):
    from p2p_llm_tunnel_amd.models.engine import Engine
    from p2p_llm_tunnel_amd.models.server import arg_parser, parse_expert_dtype, replica_cmd, start_server, weights_line
    cfg = LlamaConfig(**CFG)
    d, moe, odd = llama_dims(cfg, 2), cfg.moe, LlamaConfig(**{**CFG, "ffn": 192})
    x, ss = torch.zeros(1, 128, dtype=torch.bfloat16), torch.zeros(32, 64)
    q = lambda *s: torch.zeros(*s, dtype=torch.uint8)  # noqa: E731
    ffn = lambda **kw: ops.moe_ffn(x, ss, x.new_zeros(4, 128), q(4, 512, 64), q(4, 128, 128), 2, **kw)  # noqa: E731
    e_gu, e_dn = q(4, 512, 4), q(4, 128, 8)
    mx = TinyLlama(cfg, device="cpu", max_batch=2, expert_dtype="mxfp4")
    fp8 = TinyLlama(cfg, device="cpu", max_batch=2, expert_dtype="fp8")
    held = {"embed": mx.embed, "final_norm": mx.final_norm, "lm_head": mx.lm_head, "layers": mx.layers}
    engine = type("E", (), {"model": fp8})()
    (tmp_path / "ckpt").mkdir()
    mixtral_checkpoint(str(tmp_path / "ckpt"), tie=False)  # per-expert ffn 96
    for make, err, message in (
            (lambda: TinyLlama("tiny", device="cpu", expert_dtype="mxfp4"), ValueError, "a dense model has no experts"),
            (lambda: TinyLlama(cfg, device="cpu", expert_dtype="mxfp4", fused=False), ValueError, "fused step only"),
            (lambda: TinyLlama(odd, device="cpu", expert_dtype="mxfp4"), ValueError,
             "multiples of 128, got dim 128, ffn 192"),
            (lambda: load_llama(str(tmp_path / "ckpt"), device="cpu", expert_dtype="mxfp4"), ValueError,
             "multiples of 128, got dim 128, ffn 96"),
            (lambda: ops.WeightTable(llama_dims(odd, 2), moe=moe, expert_format="mxfp4"), ValueError, "multiples of 128"),
            (lambda: ops.WeightTable(d, expert_format="mxfp4"), ValueError, "a dense model has no experts"),
            (lambda: ops.as_expert_format(ops.ExpertFormat(3), moe, 128, 128), ValueError, "w8 0, 1 or 2"),
            (lambda: TinyLlama(cfg, device="cpu", weight_dtype="mxfp4", expert_dtype="mxfp4"), ValueError, "bf16 only"),
            (lambda: TinyLlama(cfg, device="cpu", weights=held), ValueError, "pass expert_dtype='mxfp4'"),
            (lambda: TinyLlama(cfg, device="cpu", weights=held, expert_dtype="fp8"), ValueError, "pass expert_dtype='mxfp4'"),
            (lambda: Engine(model=mx, max_batch=2), ValueError, "mxfp4 experts need the graph-captured HIP step"),
            (lambda: Engine(model=fp8, max_batch=2, expert_dtype="mxfp4"), ValueError, "was built with 'fp8' experts"),
            (lambda: start_server(engine=engine, expert_dtype="mxfp4"), ValueError, "model has 'fp8' experts"),
            (lambda: ffn(gate_up_exp=e_gu), ValueError, "both gate_up_exp and down_exp"),
            (lambda: ffn(gate_up_exp=e_gu, down_exp=e_dn, gate_up_scale=torch.ones(4, 512), down_scale=torch.ones(4, 128)),
             ValueError, "take no fp32 row scales"),
            (lambda: ffn(gate_up_exp=e_gu, down_exp=e_dn[:, :, :4]), ValueError, r"down_exp must be uint8 \(4, 128, 8\)"),
            (lambda: ffn(gate_up_exp=e_gu.float(), down_exp=e_dn), ValueError, "gate_up_exp must be uint8")):
        with pytest.raises(err, match=message):
            make()
    assert parse_expert_dtype("mxfp4") == "mxfp4" and "mxfp4 experts 417792 bytes" in weights_line(mx, "bf16")
    a = arg_parser().parse_args(["--expert-dtype", "mxfp4", "--gpus", "2"])
    assert replica_cmd(a, 1)[-2:] == ["--expert-dtype", "mxfp4"]
    lib, ef = _lib(), ops.ExpertFormat(2)  # in C: --weight-dtype on MoE, a dense model, and a size that does not block
    for dims, wf, m in ((d, ops.WeightFormat(2, 1), moe), (llama_dims(CONFIGS["micro"], 2), ops.WeightFormat(0, 0), None),
                        (llama_dims(odd, 2), ops.WeightFormat(0, 0), moe)):
        assert lib.p2pt_llama_plan_kernels_experts(ctypes.byref(dims), 1, 0, ctypes.byref(wf), None, 0,
                                                   ctypes.byref(m) if m else None, ctypes.byref(ef)) == -1
