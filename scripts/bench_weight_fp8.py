"""bf16 against FP8 (e4m3, per-row scales) GEMM weights: the fused decode step replayed from a hipGraph, both
models in ONE process (docs/WEIGHT_FP8.md).

    python scripts/bench_weight_fp8.py --model small --batch 1 16 [--ctx 1024] [--out FILE]
    python scripts/bench_weight_fp8.py --model tiny --batch 1 16 --against _hip_ops_parent.so [--out FILE]

Two models share one set of random weights (drawn on the device) and differ in ``weight_dtype`` alone. For every
batch the two are timed in alternating windows (bf16, fp8, bf16, ...), ``--rounds`` windows of ``--steps`` replays
each, every window ending in a device synchronise; the result line carries each window's ms per step, the medians
and the weight bytes of both. ``--quality`` adds the quality record: over a fixed set of 8 random prompts of 16
tokens and 16 generated ones (the bf16 model's greedy tokens, fed to both), the share of steps whose greedy token
agrees and the largest logit difference.

``--against LIB`` compares the default bf16 path of this build with another build of the kernel library in
``p2p_llm_tunnel_amd/ops/`` (the parent commit's), again in alternating windows: the second model's decoder is
built and captured through that library. The line carries the difference of the medians and the other build's own
window-to-window spread (max - min).

``tinyllama1b``, ``llama1b`` and ``llama8b`` are the shapes of TinyLlama-1.1B, Llama-3.2-1B and Llama-3.1-8B with
random weights.
"""
from __future__ import annotations

import argparse
import ctypes
import dataclasses
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from p2p_llm_tunnel_amd import ops  # noqa: E402
from p2p_llm_tunnel_amd.models.rope import RopeScaling  # noqa: E402
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, LlamaConfig, TinyLlama  # noqa: E402

_L3 = RopeScaling("llama3", 32.0, 1.0, 4.0, 8192)
SHAPES = {
    "tiny": CONFIGS["tiny"],
    "small": CONFIGS["small"],
    "tinyllama1b": LlamaConfig(vocab=32000, dim=2048, n_layers=22, n_heads=32, n_kv_heads=4, head_dim=64, ffn=5632,
                               max_seq=2048, eps=1e-5, rope_theta=10000.0),
    "llama1b": LlamaConfig(vocab=128256, dim=2048, n_layers=16, n_heads=32, n_kv_heads=8, head_dim=64, ffn=8192,
                           max_seq=131072, eps=1e-5, rope_theta=500000.0, rope_scaling=_L3),
    "llama8b": LlamaConfig(vocab=128256, dim=4096, n_layers=32, n_heads=32, n_kv_heads=8, head_dim=128, ffn=14336,
                           max_seq=131072, eps=1e-5, rope_theta=500000.0,
                           rope_scaling=dataclasses.replace(_L3, factor=8.0)),
}


def random_weights(c: LlamaConfig, seed=0) -> dict:
    """TinyLlama's initialisation, drawn on the device (a CPU draw of 8e9 values takes minutes)."""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def w(*shape, scale):
        return (torch.randn(*shape, generator=g, device="cuda") * scale).to(torch.bfloat16)

    def norm_w(n):
        return (1.0 + 0.1 * torch.randn(n, generator=g, device="cuda")).to(torch.bfloat16)

    qkv_out = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim
    layers = [{"attn_norm": norm_w(c.dim), "wqkv": w(qkv_out, c.dim, scale=1 / math.sqrt(c.dim)),
               "wo": w(c.dim, c.n_heads * c.head_dim, scale=1 / math.sqrt(c.n_heads * c.head_dim)),
               "ffn_norm": norm_w(c.dim), "w_gate_up": w(2 * c.ffn, c.dim, scale=1 / math.sqrt(c.dim)),
               "w_down": w(c.dim, c.ffn, scale=1 / math.sqrt(c.ffn))} for _ in range(c.n_layers)]
    return {"embed": w(c.vocab, c.dim, scale=1.0), "final_norm": norm_w(c.dim),
            "lm_head": w(c.vocab, c.dim, scale=1 / math.sqrt(c.dim)), "layers": layers}


def fill(cache):
    for layer in cache:
        layer.copy_(torch.randn(layer.shape, device=layer.device, dtype=torch.bfloat16).to(layer.dtype))


def other_library(name):
    """Another build of the kernels, with the signatures of the entry points a bf16 decoder calls."""
    new, other = ops.lib(), ctypes.CDLL(os.path.join(ops.HERE, name))
    for fn in ("p2pt_llama_ws_bytes", "p2pt_llama_ws_layout", "p2pt_llama_decode"):
        getattr(other, fn).argtypes = getattr(new, fn).argtypes
        getattr(other, fn).restype = getattr(new, fn).restype
    return other


def quality(models, cfg, n_prompts=8, n_prompt=16, n_new=16):
    """Teacher-forced on the bf16 model's greedy tokens: top-1 agreement and the largest logit difference."""
    g = torch.Generator(device="cuda").manual_seed(1234)
    toks = torch.randint(0, cfg.vocab, (n_prompts, n_prompt), generator=g, device="cuda")
    agree = steps = 0
    worst = top = 0.0
    cur = toks[:, 0]
    for p in range(n_prompt + n_new - 1):
        pos = torch.full((n_prompts,), p, dtype=torch.int32, device="cuda")
        out = {n: m.decode_step(cur, pos, (p, p), return_logits=True) for n, m in models.items()}
        (ia, la), (ib, lb) = out["bf16"], out["fp8"]
        if p >= n_prompt - 1:
            agree += int((ia == ib).sum())
            steps += n_prompts
            worst = max(worst, float((la.float() - lb.float()).abs().max()))
            top = max(top, float(la.float().abs().max()))
        cur = toks[:, p + 1] if p + 1 < n_prompt else ia
    return {"prompts": n_prompts, "prompt_tokens": n_prompt, "new_tokens": n_new, "top1_agreement": agree / steps,
            "max_logit_diff": worst, "max_abs_logit_bf16": top}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=sorted(SHAPES), default="small")
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--against", default=None, metavar="LIB")
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file as well")
    a = ap.parse_args()
    max_batch = max(a.batch + [8])
    cfg = dataclasses.replace(SHAPES[a.model], max_seq=a.ctx + a.steps * (2 * a.rounds + 2) + 8)
    w = random_weights(cfg)
    layers = lambda: [dict(L) for L in w["layers"]]
    first, second = ("this", "other") if a.against else ("bf16", "fp8")
    models = {first: TinyLlama.from_weights(cfg, dict(w, layers=layers()), device="cuda", max_batch=max_batch)}
    if a.against:
        models[second] = TinyLlama.from_weights(cfg, dict(w, layers=layers()), device="cuda", max_batch=max_batch)
    else:
        models[second] = TinyLlama.from_weights(cfg, dict(w, layers=layers()), device="cuda", max_batch=max_batch,
                                                weight_dtype="fp8")
    for name, m in models.items():
        fill(m.k_cache)
        fill(m.v_cache)
        saved = ops._LIB
        if name == "other":
            ops._LIB = other_library(a.against)
        try:
            for B in a.batch:
                m.capture_graph(rows=B)
        finally:
            ops._LIB = saved

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")

    for B in a.batch:
        tok = torch.randint(0, cfg.vocab, (B,), device="cuda")
        ms = {n: [] for n in models}
        q = a.ctx

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
        med = {n: statistics.median(v) for n, v in ms.items()}
        line = {"model": a.model, "batch": B, "ctx": a.ctx, "steps": a.steps, "rounds": a.rounds, "graph": True,
                "fused": True, "ms_per_step": ms, "median_ms": med,
                "weight_bytes": {n: m.weight_bytes() for n, m in models.items()}}
        if a.against:
            line["against"] = a.against
            line["median_diff_ms"] = med["this"] - med["other"]
            line["other_spread_ms"] = max(ms["other"]) - min(ms["other"])
        else:
            line["speedup"] = med["bf16"] / med["fp8"]
        emit(line)
    if a.quality and not a.against:
        emit({"model": a.model, "quality": quality(models, cfg)})


if __name__ == "__main__":
    main()
