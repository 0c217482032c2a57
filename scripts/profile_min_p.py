#!/usr/bin/env python3
"""What --min-p costs (docs/MIN_P.md): alternating windows, every window kept.

    python scripts/profile_min_p.py --out profiles/min_p.json [--parent DIR]

Each window is a process of its own that builds an engine (``--config``, tiny
by default: V = 32000; max_batch = 16) and times 200 back-to-back replays of
two of its 16-row captured steps, one row per slot, after a warm-up (device
time per replay from events):

  greedy_us    post = 0: the fused step alone, as an all-greedy batch replays it
  sampled_us   post = 1: the step and the sampler, every row sampling
               (T = 0.8, top_k = 40, top_p = 0.95; with the switch also
               min_p = 0.05)

The windows alternate between the default engine of this tree ("this"), the
default engine of ``--parent`` (a checkout of the parent commit with its
kernels built; "parent") and this tree's ``Engine(min_p=True)`` ("min_p"),
rotated so that no variant always follows the same one. The JSON keeps every
window; ``summary`` holds the medians and the min .. max spread of each."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS, REPS = 5, 200


def _timed(fn, reps=REPS):
    import torch
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us


def window(config: str, min_p: bool) -> dict:
    """One process: the two steps of one engine (runs in the parent's tree too: nothing of min_p unless asked)."""
    from p2p_llm_tunnel_amd.models import engine as S
    from p2p_llm_tunnel_amd.models.server import Engine
    eng = Engine(device="cuda:0", config=config, max_batch=16, seed=0, **({"min_p": True} if min_p else {}))
    try:
        b = eng._bufs[16][0]
        b.np[:] = 0
        b.np[S._SLOT, :] = b.np[S._REC, :] = range(16)
        smp = eng._smp if min_p else S._SMP
        for r in range(16):
            s = S.Sampling(0.8, 40, 0.95, 1000 + r, **({"min_p": 0.05} if min_p else {}))
            b.np[smp, r] = s.column(r, True) if min_p else s.column(r)
        return {"graphs": len(eng._graphs), "vocab": eng.model.cfg.vocab,
                "greedy_us": _timed(eng._graphs[(16, 0, 0)].replay),
                "sampled_us": _timed(eng._graphs[(16, 0, 1)].replay)}
    finally:
        eng.stop()


def _child(tree, what, config):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "profile_min_p.py"), "--child", what,
                        "--config", config], cwd=tree, env={**os.environ, "PYTHONPATH": tree}, capture_output=True,
                       text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{what} in {tree} failed:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "min_p.json"))
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its kernels built")
    ap.add_argument("--config", default="tiny")
    ap.add_argument("--child", default=None, choices=("default", "min_p"))
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, os.getcwd())
        print(json.dumps(window(a.config, a.child == "min_p")))
        return
    order = [("this", ROOT, "default")] + ([("parent", os.path.abspath(a.parent), "default")] if a.parent else []) + \
        [("min_p", ROOT, "min_p")]
    runs = {name: [] for name, _, _ in order}
    for k in range(WINDOWS):
        for name, tree, what in order[k % len(order):] + order[:k % len(order)]:
            runs[name].append(_child(tree, what, a.config))
            print(name, runs[name][-1], flush=True)
    summary = {name: {key: {"median": statistics.median(w[key] for w in ws), "min": min(w[key] for w in ws),
                            "max": max(w[key] for w in ws)} for key in ("greedy_us", "sampled_us")}
               for name, ws in runs.items()}
    res = {"config": a.config, "rows": 16, "windows": WINDOWS, "reps": REPS, "runs": runs, "summary": summary}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
