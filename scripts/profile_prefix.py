#!/usr/bin/env python3
"""Measurements for the prefix cache (Engine(prefix_cache=True), ops/kv_copy.hip)
on one GPU; prints one JSON document (``--out FILE`` also writes it).

  (a) second-turn TTFT: ``tiny``, a conversation whose second turn resends about
      1,024 tokens of history; engine-level (submit -> first token), the engine
      with the cache against a baseline engine on the same conversations, N
      alternating repetitions, medians. The baseline is ``Engine`` from
      ``--baseline-server PATH`` (another revision's models/server.py, e.g. the
      parent commit's) or, without it, this tree's engine with the cache off.
  (b) copy bandwidth: ``ops.kv_copy_`` for the cache geometry of ``tiny`` and
      ``small`` at 64, 512 and 2,048 rows (one job; K and V, every layer),
      against ``k[:, dst, :n].copy_(k[:, src, :n])`` plus the same for V.
      GB/s counts the bytes copied once (the traffic is a read and a write).
  (c) break-even for ``prefix_min``: TTFT of a request that shares an m-token
      prefix with a generating request, cache on (``prefix_min=1``: one copy
      launch, then the shorter prefill) against cache off, for a range of m.

Run it under a time limit (``timeout 600 python scripts/profile_prefix.py``);
any failure raises, so the exit status is non-zero at the first one.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from p2p_llm_tunnel_amd import ops  # noqa: E402
from p2p_llm_tunnel_amd.models import server  # noqa: E402
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS  # noqa: E402


def ids_of(seed: int, n: int, vocab: int) -> list[int]:
    rng = random.Random(seed)
    return [rng.randrange(vocab) for _ in range(n)]


def first_token(eng, req_cls, ids, max_new):
    """Submit; returns (seconds to the first token, the request, engine steps until then)."""
    steps = eng.steps
    t0 = time.perf_counter()
    req = eng.submit(req_cls(list(ids), max_new))
    tok = req.out.get(timeout=120)
    dt = time.perf_counter() - t0
    if tok is None:
        raise RuntimeError("request ended without a token")
    return dt, req, eng.steps - steps, tok


def drain(req, first=None):
    out = [] if first is None else [first]
    while (t := req.out.get(timeout=120)) is not None:
        out.append(t)
    return out


def ttft_second_turn(base_mod, reps: int, history: int, max_batch: int):
    vocab = CONFIGS["tiny"].vocab
    on = server.Engine(device="cuda:0", config="tiny", max_batch=max_batch, prefix_cache=True)
    off = base_mod.Engine(device="cuda:0", config="tiny", max_batch=max_batch)
    runs = {"cache": [], "baseline": []}
    try:
        for rep in range(-1, reps):  # rep -1 warms both engines up
            first = ids_of(1000 + rep, history - 44, vocab)
            for name, eng, mod in (("cache", on, server), ("baseline", off, base_mod)):
                _, r1, _, tok = first_token(eng, mod.Request, first, 24)
                turn2 = first + drain(r1, tok) + ids_of(5000 + rep, 20, vocab)
                dt, r2, steps, tok = first_token(eng, mod.Request, turn2, 4)
                drain(r2, tok)
                if rep >= 0:
                    runs[name].append({"ttft_ms": dt * 1e3, "steps_to_first_token": steps, "prompt_tokens": len(turn2),
                                       "cached_tokens": getattr(r2, "cached_tokens", 0)})
    finally:
        on.stop()
        off.stop()
    med = {k: statistics.median(r["ttft_ms"] for r in v) for k, v in runs.items()}
    return {"history_tokens": history, "repetitions": reps, "median_ttft_ms": med,
            "median_steps": {k: statistics.median(r["steps_to_first_token"] for r in v) for k, v in runs.items()},
            "speedup": med["baseline"] / med["cache"], "runs": runs}


def _time_gpu(fn, iters: int, warm: int = 10) -> float:
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def copy_bandwidth(iters: int):
    out = []
    for name in ("tiny", "small"):
        c = CONFIGS[name]
        shape = (c.n_layers, 9, c.max_seq, c.n_kv_heads, c.head_dim)
        k = torch.randn(shape, device="cuda:0").to(torch.bfloat16)
        v = torch.randn(shape, device="cuda:0").to(torch.bfloat16)
        for n in (64, 512, 2048):
            def torch_copy():
                k[:, 1, :n].copy_(k[:, 0, :n])
                v[:, 1, :n].copy_(v[:, 0, :n])
            nbytes = 2 * c.n_layers * n * c.n_kv_heads * c.head_dim * 2
            t_hip = _time_gpu(lambda: ops.kv_copy_(k, v, [(0, 1, n)]), iters)
            t_torch = _time_gpu(torch_copy, iters)
            t_hip8 = _time_gpu(lambda: ops.kv_copy_(k, v, [(0, d, n) for d in range(1, 9)]), iters)
            if not (torch.equal(k[:, 1, :n], k[:, 0, :n]) and torch.equal(v[:, 8, :n], v[:, 0, :n])):
                raise RuntimeError("copy mismatch")
            out.append({"config": name, "rows": n, "bytes_copied": nbytes,
                        "kv_copy_us": t_hip * 1e6, "kv_copy_GBps": nbytes / t_hip / 1e9,
                        "torch_slices_us": t_torch * 1e6, "torch_slices_GBps": nbytes / t_torch / 1e9,
                        "kv_copy_8_jobs_us": t_hip8 * 1e6, "kv_copy_8_jobs_GBps": 8 * nbytes / t_hip8 / 1e9})
        del k, v
    return out


def break_even(reps: int, lengths, max_batch: int):
    vocab = CONFIGS["tiny"].vocab
    on = server.Engine(device="cuda:0", config="tiny", max_batch=max_batch, prefix_cache=True, prefix_min=1)
    off = server.Engine(device="cuda:0", config="tiny", max_batch=max_batch)
    rows = []
    try:
        for m in lengths:
            t = {"cache": [], "off": []}
            for rep in range(-1, reps):
                shared = ids_of(9000 + 97 * m + rep, m, vocab)
                for name, eng in (("cache", on), ("off", off)):
                    _, bg, _, _ = first_token(eng, server.Request, shared + ids_of(1, 8, vocab), 400)
                    dt, r, _, tok = first_token(eng, server.Request, shared + ids_of(2, 8, vocab), 1)
                    drain(r, tok)
                    if name == "cache" and r.cached_tokens != m:
                        raise RuntimeError(f"expected {m} cached tokens, got {r.cached_tokens}")
                    bg.cancelled = True
                    while any(eng.slots):  # the cancelled background request leaves on the next step
                        time.sleep(0.001)
                    if rep >= 0:
                        t[name].append(dt * 1e3)
            rows.append({"prefix": m, "prompt_tokens": m + 8, "median_ttft_ms_cache": statistics.median(t["cache"]),
                         "median_ttft_ms_off": statistics.median(t["off"])})
    finally:
        on.stop()
        off.stop()
    winners = [r["prefix"] for r in rows if r["median_ttft_ms_cache"] < r["median_ttft_ms_off"]]
    return {"repetitions": reps, "copies_issued": on.kv_copies, "rows": rows,
            "shortest_prefix_where_the_copy_wins": min(winners) if winners else None}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--baseline-server", default=None, help="models/server.py of another revision (its Engine is the "
                    "TTFT baseline); default: this tree's engine with the cache off")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--history", type=int, default=1024)
    ap.add_argument("--max-batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    base_mod, base_name = server, "this tree, prefix_cache=False"
    if a.baseline_server:
        spec = importlib.util.spec_from_file_location("baseline_server", a.baseline_server)
        base_mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(base_mod)
        base_name = f"Engine of {os.path.basename(a.baseline_server)} (another revision)"
        if "prefix_cache" in base_mod.Engine.__init__.__code__.co_varnames:
            raise SystemExit("the baseline server already has the prefix cache")
    res = {"device": torch.cuda.get_device_name(0), "ttft_baseline": base_name,
           "a_second_turn_ttft": ttft_second_turn(base_mod, a.reps, a.history, a.max_batch),
           "b_copy_bandwidth": copy_bandwidth(a.iters),
           "c_break_even": break_even(a.reps, (4, 8, 16, 32, 48, 64, 128, 256), a.max_batch)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
