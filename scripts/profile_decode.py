"""Decode-step microbenchmark of the on-node inference upstream (for rocprofv3).

    python scripts/profile_decode.py --config tiny --batch 8 --ctx 1024 --steps 50 [--eager]

Fills the KV cache with random values up to `ctx`, then times `steps`
batched decode steps through the HIP kernels — replayed from a captured
hipGraph by default, or launched eagerly with --eager; the fused step
(decode_fused.hip) by default, the unfused kernels + hipBLASLt with
--unfused — and prints tokens/s.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from p2p_llm_tunnel_amd.models.rope import RopeScaling  # noqa: E402
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, LlamaConfig, TinyLlama, capture  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="tiny")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--unfused", action="store_true", help="kernels.hip + hipBLASLt path instead of decode_fused.hip")
    ap.add_argument("--set", action="append", default=[], metavar="FIELD=INT",
                    help="override a field of --config (e.g. --set n_layers=2 --set vocab=8000)")
    ap.add_argument("--cfg", default=None, metavar="JSON",
                    help="an explicit LlamaConfig as a JSON object of its fields, instead of --config, e.g. a "
                         "Qwen3-0.6B-shaped model: '{\"vocab\": 151936, \"dim\": 1024, \"n_layers\": 28, "
                         "\"n_heads\": 16, \"n_kv_heads\": 8, \"head_dim\": 128, \"ffn\": 3072, \"max_seq\": 2048, "
                         "\"eps\": 1e-6, \"rope_theta\": 1e6, \"qk_norm\": true}'. \"rope_scaling\" takes an "
                         "object of RopeScaling's fields, e.g. {\"kind\": \"llama3\", \"factor\": 32, "
                         "\"low_freq_factor\": 1, \"high_freq_factor\": 4, \"original_max_seq\": 8192}")
    ap.add_argument("--name", default=None, help="label of a --cfg model in the result line")
    ap.add_argument("--checkpoint", default=None, help="load this HF Llama checkpoint instead of a random --config")
    ap.add_argument("--weight-dtype", choices=("bf16", "fp8", "mxfp4"), default="bf16",
                    help="format of the GEMM weights: bf16, fp8 (e4m3 with per-row scales, docs/WEIGHT_FP8.md) or "
                         "mxfp4 (block-scaled FP4 layers with an fp8 LM head, docs/WEIGHT_MXFP4.md); the fused step "
                         "only")
    ap.add_argument("--compare", default=None, metavar="DTYPES",
                    help="weight formats to compare in this one process, e.g. bf16,fp8,mxfp4: one model per format "
                         "from the same bf16 weights, then --windows alternating windows of --steps graph replays "
                         "for every format and every batch of --batches; one JSON line per (format, batch) with the "
                         "windows and their median, and the share of rows whose greedy token is the bf16 model's")
    ap.add_argument("--windows", type=int, default=5, help="windows per format and batch (with --compare)")
    ap.add_argument("--batches", default="1,16", help="comma-separated batch sizes (with --compare)")
    ap.add_argument("--loop", action="store_true",
                    help="device-side autoregression: one graph = the fused step (ids feed the next step's "
                         "tokens in place) + pos += 1, no host copies per step")
    a = ap.parse_args()
    if a.compare:
        return compare(a)
    if a.checkpoint:
        from p2p_llm_tunnel_amd.models.checkpoint import load_llama
        m = load_llama(a.checkpoint, device="cuda", max_batch=a.batch, fused=not a.unfused,
                       weight_dtype=a.weight_dtype)
        a.config = os.path.basename(os.path.normpath(a.checkpoint))
    else:
        if a.cfg:
            fields = json.loads(a.cfg)
            if fields.get("rope_scaling") is not None:
                fields["rope_scaling"] = RopeScaling(**fields["rope_scaling"])
            cfg = LlamaConfig(**fields)
            a.config = a.name or "custom"
        else:
            cfg = CONFIGS[a.config]
        if a.set:
            cfg = dataclasses.replace(cfg, **{k: int(v) for k, v in (x.split("=", 1) for x in a.set)})
            a.config += "[" + ",".join(a.set) + "]"
        m = TinyLlama(cfg, device="cuda", max_batch=a.batch, fused=not a.unfused, weight_dtype=a.weight_dtype)
    m.k_cache.normal_()
    m.v_cache.normal_()
    if a.loop:
        return loop(m, a)
    if not a.eager:
        m.capture_graph(rows=a.batch)
    B = a.batch
    tok = torch.randint(0, m.cfg.vocab, (B,), device="cuda")

    def step(q):
        p = torch.full((B,), q, dtype=torch.int32, device="cuda")
        return m.decode_step(tok, p, (q, q)) if a.eager else m.graph_step(tok, p)

    for i in range(a.warmup):
        tok = step(a.ctx + i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        tok = step(a.ctx + a.warmup + i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"config": a.config, "batch": B, "ctx": a.ctx, "steps": a.steps, "graph": not a.eager, "fused": not a.unfused,
                      "weight_dtype": a.weight_dtype, "weight_bytes": m.weight_bytes()["total"],
                      "ms_per_step": dt * 1e3 / a.steps, "tokens_per_s": B * a.steps / dt}))


def compare(a):
    """--compare: every format on the same weights in one process, the windows alternating between the formats so
    that clock and temperature drift fall on all of them alike."""
    import statistics
    cfg = LlamaConfig(**json.loads(a.cfg)) if a.cfg else CONFIGS[a.config]
    name = a.name or (a.config if not a.cfg else "custom")
    formats, batches = a.compare.split(","), [int(b) for b in a.batches.split(",")]
    B = max(batches)
    base = TinyLlama(cfg, device="cuda", max_batch=B)
    weights = dict(embed=base.embed, final_norm=base.final_norm, lm_head=base.lm_head, layers=base.layers)
    models = {f: base if f == "bf16" else TinyLlama.from_weights(cfg, weights, device="cuda", max_batch=B,
                                                                  weight_dtype=f) for f in formats}
    g = torch.Generator(device="cuda").manual_seed(0)
    kc = torch.randn(base.k_cache.shape, generator=g, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn(base.v_cache.shape, generator=g, device="cuda", dtype=torch.bfloat16)
    for m in models.values():
        m.k_cache.copy_(kc)
        m.v_cache.copy_(vc)
        for b in batches:
            m.capture_graph(rows=b)
    agree = {}
    for f, m in models.items():  # greedy tokens of 4 steps of B rows on identical inputs, against the first format's
        ids = []
        for i in range(4):
            tok = torch.randint(0, cfg.vocab, (B,), generator=g, device="cuda") if f == formats[0] else agree["tok"][i]
            agree.setdefault("tok", []).append(tok)
            p = torch.full((B,), a.ctx + i, dtype=torch.int32, device="cuda")
            ids.append(m.graph_step(tok, p).clone())
        agree[f] = torch.cat(ids)
    times = {(f, b): [] for f in formats for b in batches}
    for w in range(a.windows):
        for b in batches:
            for f in formats:
                m = models[f]
                tok = torch.randint(0, cfg.vocab, (b,), device="cuda")
                for i in range(a.warmup + a.steps):
                    if i == a.warmup:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                    q = a.ctx + 8 + i
                    tok = m.graph_step(tok, torch.full((b,), q, dtype=torch.int32, device="cuda"))
                torch.cuda.synchronize()
                times[f, b].append((time.perf_counter() - t0) * 1e3 / a.steps)
    for (f, b), t in times.items():
        print(json.dumps({"config": name, "batch": b, "ctx": a.ctx, "steps": a.steps, "graph": True, "fused": True,
                          "weight_dtype": f, "weight_bytes": models[f].weight_bytes()["total"],
                          "gemm_weight_bytes": models[f].weight_bytes()["gemm"],
                          "ms_per_step_windows": [round(x, 4) for x in t],
                          "ms_per_step": round(statistics.median(t), 4),
                          "greedy_agreement_with_" + formats[0]: float((agree[f] == agree[formats[0]]).float().mean()),
                          "lib": os.path.basename(__import__("p2p_llm_tunnel_amd").ops.loaded_path())}), flush=True)


def loop(m, a):
    """The decode step as the only work in the graph: the step's ids buffer is
    the next step's token buffer and a pos += 1 kernel follows it, so a replay
    is the fused kernels plus one tiny elementwise kernel."""
    B, c = a.batch, m.cfg
    dec = m.fused_decoder()
    tok = torch.randint(0, c.vocab, (B,), device="cuda")
    pos = torch.full((B,), a.ctx, dtype=torch.int32, device="cuda")
    logits = torch.empty(B, c.vocab, dtype=torch.bfloat16, device="cuda")

    def body():
        dec.step(tok, pos, logits, tok)
        pos.add_(1)

    g, _ = capture(body, m.device, warmup=1)
    pos.fill_(a.ctx)
    for _ in range(a.warmup):
        g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        g.replay()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    nbytes = sum(t.numel() * t.element_size() for t in dec.weights[dec.table.index("lm_head"):]) + m.embed.shape[1] * 2 * B
    print(json.dumps({"config": a.config, "batch": B, "ctx": a.ctx, "steps": a.steps, "graph": True, "loop": True,
                      "weight_dtype": a.weight_dtype,
                      "ms_per_step": dt * 1e3 / a.steps, "tokens_per_s": B * a.steps / dt,
                      "weight_TBps": nbytes / (dt / a.steps) / 1e12}))


if __name__ == "__main__":
    main()
