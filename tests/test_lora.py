"""LoRA adapters without a GPU (docs/LORA.md): a synthetic PEFT directory through ``load_lora`` and ``ops.pack_lora``
exactly in fp64, what the loader refuses, which adapter a request's "model" selects, and the kernels' plans."""
import json
import math

import pytest
import torch
from safetensors.torch import save_file

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models import checkpoint, params, server
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, LlamaConfig, fused_row_perm, llama_dims

CFG = LlamaConfig(vocab=512, dim=256, n_layers=1, n_heads=4, n_kv_heads=2, head_dim=64, ffn=352, max_seq=64)
ALL = tuple(checkpoint.LORA_MODULES)


def _pow2(shape, g):
    """Signed powers of two: products and sums of a few of them are exact in bf16 and fp32."""
    return torch.ldexp(torch.randint(0, 2, shape, generator=g) * 2.0 - 1.0, torch.randint(-2, 2, shape, generator=g))


def write_adapter(path, cfg, r=8, modules=ALL, seed=0, b_scale=1.0, exact=False, **config):
    """A PEFT adapter directory for ``cfg``. ``exact``: lora_A with one power of two per row and lora_B of powers of
    two, so that every product is exact; otherwise Gaussian."""
    g = torch.Generator().manual_seed(seed)
    q, kv = cfg.n_heads * cfg.head_dim, cfg.n_kv_heads * cfg.head_dim
    n_k = {"q_proj": (q, cfg.dim), "k_proj": (kv, cfg.dim), "v_proj": (kv, cfg.dim), "o_proj": (cfg.dim, q),
           "gate_proj": (cfg.ffn, cfg.dim), "up_proj": (cfg.ffn, cfg.dim), "down_proj": (cfg.dim, cfg.ffn)}
    t = {}
    for i in range(cfg.n_layers):
        for m in modules:
            n, K = n_k.get(m, (cfg.dim, cfg.dim))
            p = f"base_model.model.model.layers.{i}.{checkpoint.LORA_MODULES.get(m, 'mlp')}.{m}."
            t[p + "lora_A.weight"] = (torch.zeros(r, K).scatter_(1, torch.randint(0, K, (r, 1), generator=g),
                                                                 _pow2((r, 1), g)) if exact
                                      else torch.randn(r, K, generator=g) * K ** -0.5)
            t[p + "lora_B.weight"] = _pow2((n, r), g) if exact else torch.randn(n, r, generator=g) * b_scale
    save_file(t, str(path / "adapter_model.safetensors"))
    (path / "adapter_config.json").write_text(json.dumps(
        {"peft_type": "LORA", "r": r, "lora_alpha": 2 * r, "target_modules": list(modules), "bias": "none", **config}))
    return t


@pytest.mark.parametrize("r,modules,rslora", [(1, ALL, False), (8, ALL, False), (64, ALL, False),
                                              (8, ("q_proj", "v_proj"), False), (4, ALL, True)],
                         ids=["r1", "r8", "r64", "q-and-v-only", "rslora"])
def test_loaded_adapter_packs_to_the_scaled_product_exactly(tmp_path, r, modules, rslora):
    """unpack(B') @ unpack(A') == scaling * lora_B @ lora_A per module, block-structured for a fused projection, with
    power-of-two norm weights folded into A''s columns and B''s rows in ``fused_row_perm`` order."""
    t = write_adapter(tmp_path, CFG, r, modules, exact=True, use_rslora=rslora)
    ad = checkpoint.load_lora(str(tmp_path), CFG)
    assert ad.scaling == (2 * r / math.sqrt(r) if rslora else 2.0) and ad.modules == tuple(sorted(modules))
    g = torch.Generator().manual_seed(1)
    for name, parts in ops.LORA_PARTS.items():
        sizes, K = ops.lora_shapes(CFG)[name]
        norm = _pow2((K,), g).abs() if name in ("wqkv", "w_gate_up") else None
        ab = [ad.layers[0].get(m, (None, None)) for m in parts]
        Ap, Bp = ops.pack_lora(CFG, name, [x[0] for x in ab], [x[1] for x in ab], ad.scaling, norm)
        assert Ap.shape == (ops.lora_rank(*[r * (m in modules) for m in parts]), K) and Ap.shape[0] % 16 == 0
        pre = "base_model.model.model.layers.0."
        want = torch.cat([ad.scaling * t[f"{pre}{checkpoint.LORA_MODULES[m]}.{m}.lora_B.weight"].double()
                          @ t[f"{pre}{checkpoint.LORA_MODULES[m]}.{m}.lora_A.weight"].double() if m in modules
                          else torch.zeros(n, K, dtype=torch.float64) for m, n in zip(parts, sizes)])
        A64, B64 = ops.unpack_lora(CFG, name, Ap, Bp, norm)
        assert torch.equal(B64 @ A64, want)
        perm = fused_row_perm(CFG, name, "cpu")
        folded = want * norm.double()[None, :] if norm is not None else want
        assert torch.equal(Bp.double() @ Ap.double(), folded[perm] if perm is not None else folded)
        if name == "wqkv" and "k_proj" not in modules:  # the k block of a q-and-v-only adapter
            assert not bool(B64[sizes[0]:sizes[0] + sizes[1]].any())


@pytest.mark.parametrize("kw,msg", [
    (dict(use_dora=True), "use_dora"), (dict(bias="all"), "bias"), (dict(modules_to_save=["lm_head"]), "modules_to_save"),
    (dict(rank_pattern={"q_proj": 4}), "rank_pattern"), (dict(alpha_pattern={"q_proj": 4}), "alpha_pattern"),
    (dict(fan_in_fan_out=True), "fan_in_fan_out"), (dict(modules=("q_proj", "lm_head")), "target module 'lm_head'"),
    (dict(modules=("embed_tokens",)), "target module 'embed_tokens'"), (dict(r=65), "r must be an int in 1..64"),
    (dict(cfg=LlamaConfig(dim=512)), "does not match the base model"),
    (dict(cfg=CONFIGS["tiny-moe"]), "MoE"), (dict(weight_dtype="fp8"), "weight_dtype 'fp8'"),
    (dict(fused=False), "eager or unfused"),
])
def test_load_lora_refusals(tmp_path, kw, msg):
    kw = dict(kw)
    cfg, wd, fused = kw.pop("cfg", CFG), kw.pop("weight_dtype", "bf16"), kw.pop("fused", True)
    write_adapter(tmp_path, CFG, kw.pop("r", 8), kw.pop("modules", ALL), **kw)
    with pytest.raises(ValueError, match=msg):
        checkpoint.load_lora(str(tmp_path), cfg, wd, fused)


def test_model_selects_the_adapter():
    """The request-parsing layer, which ``_dispatch`` calls once ahead of the four routes (tests/test_gpu_lora.py
    drives each): ``model`` equal to a configured name runs under it, any other value is the base as before."""
    names = ("sql", "legal")
    assert params.adapter_param({"model": "legal", "messages": [], "prompt": "x"}, names) == "legal"
    for other in ("p2pt-tiny", "LEGAL", None, 7):
        assert params.adapter_param({"model": other}, names) is None
    assert params.adapter_param({}, names) is None and params.adapter_param({"model": "sql"}, ()) is None
    assert params.model_names("p2pt-tiny", names) == ["p2pt-tiny", "sql", "legal"]
    assert server.check_loras(["sql=/a", "legal=/b"]) == {"sql": "/a", "legal": "/b"}
    for bad in (["sql"], ["sql=/a", "sql=/b"], [f"a{i}=/d" for i in range(9)]):
        with pytest.raises(ValueError, match="--lora"):
            server.check_loras(bad)
    a = server.arg_parser().parse_args(["--lora", "sql=/a", "--lora", "legal=/b", "--gpus", "2"])
    assert server.replica_cmd(a, 1)[-4:] == ["--lora", "sql=/a", "--lora", "legal=/b"]


@pytest.mark.parametrize("rows", (1, 17, 40))
@pytest.mark.parametrize("config", ("tiny", "small"))
def test_lora_plans(config, rows):
    cfg = CONFIGS[config]
    dims, ranks = llama_dims(cfg, 64), (48, 16, 32, 16)
    assert ops.plan_kernels_ok(dims, rows, lora=ranks)
    assert ops.plan_kernels_ok(llama_dims(cfg, 64, kv_fp8=True), rows, lora=(192, 64, 128, 64))
    # The LoRA variants run on the base step's plan, (nw, um, kpl, grid) and all; k_lora_delta launches ahead of each.
    plan = ops.step_plan(dims, rows)
    for (name, (sizes, K)), R, stage in zip(ops.lora_shapes(cfg).items(), ranks, ("qkv", "o", "gate_up", "down")):
        p, g = ops.lora_plan(rows, sum(sizes), K, R), getattr(plan, stage)
        assert (g.N, g.K, g.grid_y) == (sum(sizes), K, p.grid_y)
        assert (p.grid_x, p.grid_y, p.waves, p.passes) == (-(-sum(sizes) // p.cols), -(-rows // 16), 4, -(-R // 64))
    with pytest.raises(ValueError, match="QK-norm"):
        ops.plan_kernels_ok(llama_dims(LlamaConfig(qk_norm=True), 8), rows, lora=ranks)
    for bad in (dict(R=8), dict(R=208), dict(K=48), dict(n=9)):
        with pytest.raises(ValueError):
            ops.lora_plan(rows, 512, bad.get("K", 256), bad.get("R", 16), bad.get("n", 1))
