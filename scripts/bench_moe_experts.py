"""One timing window of an MoE model's fused decode step in one expert format (docs/MOE_MXFP4.md, docs/MOE_FP8.md).

    python scripts/bench_moe_experts.py --model mixtral --experts mxfp4 --batch 1 16 [--out FILE]

One process is one window per batch: the model is built with random weights drawn on the device (``mixtral`` is
Mixtral-8x7B's shape with 4 of its 32 layers), the experts quantised, the step captured in a hipGraph, replayed
``--warmup`` times and then timed over ``--steps`` replays at context ``--ctx``; rows = batch. A caller alternates
processes of the formats it compares. Prints one JSON line per batch with the ms per step, the experts the last layer
touched and ``weight_bytes()``.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, LlamaConfig, TinyLlama, quantize_experts_  # noqa: E402

SHAPES = {
    "tiny": CONFIGS["tiny"],
    "tiny-moe": CONFIGS["tiny-moe"],
    "mixtral": LlamaConfig(vocab=32000, dim=4096, n_layers=4, n_heads=32, n_kv_heads=8, head_dim=128, ffn=14336,
                           max_seq=2048, eps=1e-5, rope_theta=1e6, n_experts=8, top_k=2),
}


def random_weights(c: LlamaConfig, experts: str, seed=0) -> dict:
    """TinyLlama's initialisation drawn on the device, each layer's experts quantised as soon as they are drawn."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = lambda *shape, scale: (torch.randn(*shape, generator=g, device="cuda") * scale).to(torch.bfloat16)  # noqa: E731
    norm_w = lambda n: (1.0 + 0.1 * torch.randn(n, generator=g, device="cuda")).to(torch.bfloat16)  # noqa: E731
    stack = (c.n_experts,) if c.n_experts else ()
    layers = []
    for _ in range(c.n_layers):
        L = {"attn_norm": norm_w(c.dim),
             "wqkv": w((c.n_heads + 2 * c.n_kv_heads) * c.head_dim, c.dim, scale=1 / math.sqrt(c.dim)),
             "wo": w(c.dim, c.n_heads * c.head_dim, scale=1 / math.sqrt(c.n_heads * c.head_dim)),
             "ffn_norm": norm_w(c.dim), "w_gate_up": w(*stack, 2 * c.ffn, c.dim, scale=1 / math.sqrt(c.dim)),
             "w_down": w(*stack, c.dim, c.ffn, scale=1 / math.sqrt(c.ffn))}
        if c.n_experts:
            L["router"] = w(c.n_experts, c.dim, scale=1 / math.sqrt(c.dim))
        layers.append(quantize_experts_(c, L, experts) if experts != "bf16" else L)
    return {"embed": w(c.vocab, c.dim, scale=1.0), "final_norm": norm_w(c.dim),
            "lm_head": w(c.vocab, c.dim, scale=1 / math.sqrt(c.dim)), "layers": layers}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=sorted(SHAPES), default="mixtral")
    ap.add_argument("--experts", choices=("bf16", "fp8", "mxfp4"), default="bf16")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--tag", default="", help="copied into the result line (which tree, which window)")
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file as well")
    a = ap.parse_args()
    cfg = dataclasses.replace(SHAPES[a.model], max_seq=a.ctx + a.warmup + a.steps + 8)
    m = TinyLlama.from_weights(cfg, random_weights(cfg, a.experts), device="cuda", max_batch=max(a.batch),
                               **({"expert_dtype": a.experts} if a.experts != "bf16" else {}))
    for cache in (m.k_cache, m.v_cache):
        for layer in cache:
            layer.copy_(torch.randn(layer.shape, device="cuda", dtype=torch.bfloat16).to(layer.dtype))
    for B in a.batch:
        m.capture_graph(rows=B)
        tok = torch.randint(0, cfg.vocab, (B,), device="cuda")
        pos = [torch.full((B,), a.ctx + i, dtype=torch.int32, device="cuda") for i in range(a.warmup + a.steps)]
        for p in pos[:a.warmup]:
            m.graph_step(tok, p)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for p in pos[a.warmup:]:
            m.graph_step(tok, p)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        line = {"model": a.model, "experts": a.experts, "batch": B, "rows": B, "ctx": a.ctx, "warmup": a.warmup,
                "steps": a.steps, "ms": round(ms, 4), "weight_bytes": m.weight_bytes(), "tag": a.tag}
        if cfg.n_experts:
            ids = m.fused_decoder().workspace_views()["route_id"][:B]
            line["experts_touched_last_layer"] = int(ids.unique().numel())
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
