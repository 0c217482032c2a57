#!/usr/bin/env python3
"""Calibrate per-layer, per-KV-head scales for the FP8 KV cache (``--kv-scales FILE``, docs/KV_FP8.md).

Runs prompts through the model with a bf16 cache on the fused HIP step, takes the largest magnitude of the K rows
(after RoPE) and V rows written per (layer, KV head), and writes

    {"k": [[...]], "v": [[...]]}      one row per layer, one number per KV head

with ``s = absmax / 448`` rounded up to a power of two: the largest value seen lands in (224, 448], which leaves a
headroom of 1 to 2 for values the prompts did not show, and the multiply by 1 / s is exact. The scales are static:
a value beyond 448 s at serving time still saturates.

    python scripts/calibrate_kv.py --checkpoint DIR --prompts prompts.txt --out kv_scales.json
    python scripts/calibrate_kv.py --config micro --random 4x200 --out kv_scales.json

``--prompts``: a text file, one prompt per line (needs the checkpoint's tokenizer). ``--random NxT``: N prompts of T
random token ids, for models without a tokenizer. The reduction itself is ``models.kv_scales.absmax`` /
``scales_from_absmax``: plain functions over cache tensors.
"""
from __future__ import annotations

import argparse
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from p2p_llm_tunnel_amd import ops  # noqa: E402
from p2p_llm_tunnel_amd.models.kv_scales import absmax, scales_from_absmax  # noqa: E402


def prefill(model, prompts: list[list[int]]) -> list[int]:
    """Write the K/V rows of ``prompts`` (one per cache slot) through the fused step, in chunks of up to
    ``ops.MAX_ROWS`` rows; returns the rows each slot holds."""
    dev, S = model.device, model.cfg.max_seq
    lengths = []
    for slot, ids in enumerate(prompts):
        ids = ids[:S]
        for p0 in range(0, len(ids), ops.MAX_ROWS):
            chunk = ids[p0:p0 + ops.MAX_ROWS]
            n = len(chunk)
            model.decode_step(torch.tensor(chunk, dtype=torch.int64, device=dev),
                              torch.arange(p0, p0 + n, dtype=torch.int32, device=dev), (p0, p0 + n - 1),
                              slots=torch.full((n,), slot, dtype=torch.int32, device=dev), emit_rows=1)
        lengths.append(len(ids))
    torch.cuda.synchronize()
    return lengths


def calibrate(model, prompts: list[list[int]]):
    """``KvScales`` of ``model`` (a bf16 cache) over ``prompts``, at most ``model.max_batch`` of them."""
    if model.kv_dtype != "bf16":
        raise ValueError("calibrate with a bf16 cache: an FP8 cache has already rounded, and clamped, what it holds")
    if not 1 <= len(prompts) <= model.max_batch or any(not p for p in prompts):
        raise ValueError(f"need 1..{model.max_batch} non-empty prompts (one cache slot each)")
    lengths = prefill(model, prompts)
    return scales_from_absmax(*absmax(model.k_cache, model.v_cache, lengths))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--config", default="tiny")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--max-seq", type=int, default=None)
    ap.add_argument("--prompts", default=None, help="text file, one prompt per line")
    ap.add_argument("--random", default=None, metavar="NxT", help="N prompts of T random token ids")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    if (a.prompts is None) == (a.random is None):
        ap.error("give exactly one of --prompts and --random")
    tok = None
    if a.prompts:
        with open(a.prompts) as fh:
            lines = [l.strip() for l in fh if l.strip()]
        n = len(lines)
    else:
        n, t = (int(x) for x in a.random.lower().split("x"))
    if a.checkpoint:
        from p2p_llm_tunnel_amd.models.checkpoint import Tokenizer, load_llama
        model = load_llama(a.checkpoint, device=a.device, max_batch=n, max_seq=a.max_seq)
        tok = Tokenizer.for_checkpoint(a.checkpoint)
    else:
        from p2p_llm_tunnel_amd.models.tiny_llm import TinyLlama
        model = TinyLlama(a.config, device=a.device, max_batch=n, seed=a.seed)
    if a.prompts:
        if tok is None:
            ap.error("--prompts needs a checkpoint with a tokenizer; use --random")
        prompts = [tok.encode(l) for l in lines]
    else:
        rng = random.Random(a.seed)
        prompts = [[rng.randrange(model.cfg.vocab) for _ in range(t)] for _ in range(n)]
    scales = calibrate(model, prompts)
    scales.save(a.out)
    print(f"{a.out}: {scales.describe()} from {sum(len(p) for p in prompts)} tokens", flush=True)


if __name__ == "__main__":
    main()
