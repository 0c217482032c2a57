"""Step time of the fused decode with and without LoRA adapters (docs/LORA.md): one captured step (hipGraph) per
variant, replayed in alternating windows, one JSON line with every window's microseconds per step and the medians.

    python scripts/bench_lora.py --config small --batch 16 --rank 16 --adapters 4
    python scripts/bench_lora.py --config tiny --batch 1 --base-only     # also runs on a tree without adapters

Variants: ``base`` (a decoder without ``lora``), ``lora_off`` (a decoder with ``lora``, ``adapters=None``: the base
kernels on the larger workspace) and ``lora`` (every row names an adapter, row b adapter b % --adapters)."""
import argparse
import json
import statistics

import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, LlamaConfig, TinyLlama, capture

SHAPES = dict(CONFIGS, **{"8b": LlamaConfig(vocab=32000, dim=4096, n_layers=8, n_heads=32, n_kv_heads=8, head_dim=128,
                                             ffn=14336, max_seq=2048)})  # Llama-3.1-8B's layer shape, 8 layers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="tiny", choices=sorted(SHAPES))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--rank", type=int, default=16, help="PEFT rank of every module")
    ap.add_argument("--adapters", type=int, default=1)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--base-only", action="store_true")
    a = ap.parse_args()
    cfg, B = SHAPES[a.config], a.batch
    m = TinyLlama(cfg, device="cuda", max_batch=B, seed=0)
    tokens = torch.randint(0, cfg.vocab, (B,), device="cuda")
    pos = torch.full((B,), 512, dtype=torch.int32, device="cuda")
    logits = torch.empty(B, cfg.vocab, dtype=torch.bfloat16, device="cuda")
    ids = torch.empty(B, dtype=torch.int64, device="cuda")
    steps = {"base": lambda: m.fused_decoder().step(tokens, pos, logits, ids)}
    if not a.base_only:
        g = torch.Generator(device="cuda").manual_seed(1)
        lora = [{name: (torch.randn(a.adapters, R, K, generator=g, device="cuda").mul_(K ** -0.5).bfloat16(),
                        torch.randn(a.adapters, sum(sizes), R, generator=g, device="cuda").mul_(0.01).bfloat16())
                 for name, (sizes, K) in ops.lora_shapes(cfg).items()
                 for R in [ops.lora_rank(*[a.rank] * len(sizes))]} for _ in range(cfg.n_layers)]
        dec = ops.FusedLlamaDecoder(m.dims(), m.fused_weights(), m.k_cache, m.v_cache, lora=lora)
        aid = (torch.arange(B, device="cuda") % a.adapters).to(torch.int32)
        steps["lora_off"] = lambda: dec.step(tokens, pos, logits, ids)
        steps["lora"] = lambda: dec.step(tokens, pos, logits, ids, adapters=aid)
    graphs = {k: capture(f, "cuda")[0] for k, f in steps.items()}
    us = {k: [] for k in graphs}
    for _ in range(a.windows):
        for k, graph in graphs.items():  # alternating windows
            graph.replay()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                graph.replay()
            t1.record()
            torch.cuda.synchronize()
            us[k].append(round(t0.elapsed_time(t1) * 1000 / a.iters, 3))
    print(json.dumps({"config": a.config, "batch": B, "rank": a.rank, "adapters": a.adapters, "layers": cfg.n_layers,
                      "iters": a.iters, "us_per_step": us,
                      "median_us": {k: statistics.median(v) for k, v in us.items()}}), flush=True)


if __name__ == "__main__":
    main()
