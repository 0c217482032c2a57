"""bf16 against FP8 (e4m3) KV cache: the fused decode step replayed from a hipGraph, both caches in ONE process.

    python scripts/bench_kv_fp8.py --model small --ctx 1024 8192 32768 --batch 1 16 [--out FILE]

Two models share one set of random weights and differ in ``kv_dtype`` alone. For every (ctx, batch) the two are
timed in alternating windows (bf16, fp8, bf16, ...), ``--rounds`` windows of ``--steps`` replays each, every
window ending in a device synchronise; the result line carries each window's ms per step and the medians. Caches
are filled with N(0, 1) values up to ctx. ``llama1b`` is Llama-3.2-1B's shape with random weights.

``--scales`` adds a third model to the alternation, "fp8+scales": the FP8 cache with per-layer, per-KV-head scales
(powers of two between 1/4 and 4, all different within a layer: the kernels take the same path whatever the values).
``--no-bf16`` leaves the bf16 model out. The parent commit's own FP8 path is timed by running the parent's copy of
this script in a process of its own, alternating with this one (profiles/kv_scale.json says how).
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from p2p_llm_tunnel_amd.models.rope import RopeScaling  # noqa: E402
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, LlamaConfig, TinyLlama  # noqa: E402

SHAPES = {
    "small": CONFIGS["small"],
    "tiny": CONFIGS["tiny"],
    "llama1b": LlamaConfig(vocab=128256, dim=2048, n_layers=16, n_heads=32, n_kv_heads=8, head_dim=64, ffn=8192,
                           max_seq=131072, eps=1e-5, rope_theta=500000.0,
                           rope_scaling=RopeScaling("llama3", 32.0, 1.0, 4.0, 8192)),
}


def fill(cache):
    """N(0, 1) in the cache's own format, a layer at a time (normal_ has no float8 kernel)."""
    for layer in cache:
        layer.copy_(torch.randn(layer.shape, device=layer.device, dtype=torch.bfloat16).to(layer.dtype))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=sorted(SHAPES), default="small")
    ap.add_argument("--ctx", type=int, nargs="+", default=[1024])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scales", action="store_true", help="also time the FP8 cache with per-head scales")
    ap.add_argument("--no-bf16", action="store_true", help="leave the bf16-cache model out of the alternation")
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file as well")
    a = ap.parse_args()
    max_batch = max(a.batch)
    cfg = dataclasses.replace(SHAPES[a.model], max_seq=max(a.ctx) + a.steps * (2 * a.rounds + 2) + 8)
    models = {"bf16": TinyLlama(cfg, device="cuda", max_batch=max_batch, seed=0)}
    w = dict(embed=models["bf16"].embed, final_norm=models["bf16"].final_norm, lm_head=models["bf16"].lm_head,
             layers=models["bf16"].layers)
    models["fp8"] = TinyLlama.from_weights(cfg, w, device="cuda", max_batch=max_batch, kv_dtype="fp8")
    if a.scales:
        from p2p_llm_tunnel_amd.models.kv_scales import KvScales
        exps = torch.arange(cfg.n_layers * cfg.n_kv_heads).view(cfg.n_layers, cfg.n_kv_heads) % 5 - 2
        models["fp8+scales"] = TinyLlama.from_weights(cfg, w, device="cuda", max_batch=max_batch, kv_dtype="fp8",
                                                      kv_scales=KvScales(torch.exp2(exps.float()),
                                                                         torch.exp2(-exps.float())))
    if a.no_bf16:
        del models["bf16"]
    for m in models.values():
        fill(m.k_cache)
        fill(m.v_cache)
        for B in a.batch:
            m.capture_graph(rows=B)
    for ctx in a.ctx:
        for B in a.batch:
            tok = torch.randint(0, cfg.vocab, (B,), device="cuda")
            ms = {name: [] for name in models}
            q = ctx

            def window(m, q0, n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(n):
                    m.graph_step(tok, torch.full((B,), q0 + i, dtype=torch.int32, device="cuda"))
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / n

            for m in models.values():  # warm-up of this shape
                window(m, q, a.steps)
            for _ in range(a.rounds):
                for name, m in models.items():
                    ms[name].append(window(m, q, a.steps))
                q += a.steps
            line = {"model": a.model, "batch": B, "ctx": ctx, "steps": a.steps, "graph": True, "fused": True,
                    "kv_bytes": {n: m.kv_cache_bytes() for n, m in models.items()},
                    "ms_per_step": ms, "median_ms": {n: statistics.median(v) for n, v in ms.items()}}
            print(json.dumps(line), flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
