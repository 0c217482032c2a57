#!/usr/bin/env python3
"""What --penalties costs (docs/PENALTIES.md): medians of 5 alternating runs.

    python scripts/profile_penalty.py --out profiles/penalties.json [--parent DIR]

  kernel   ops.penalize_ alone, every row on with a 3-entry bias list, at
           V = 32000 and 151936 and 1 and 16 rows (device time per call from
           events around 200 back-to-back launches, after a warm-up).
  step     the 16-row captured step of Engine(config, max_batch=16,
           penalties=True): replays of its post = 3 graph (every row on) against
           its post = 2 graph, alternating, 200 replays a run.
  default  the 16-row post = 0 step and the construction time of the default
           engine (no switch) of this tree against the same of ``--parent``
           (a checkout of the parent commit with its kernels built), alternating,
           each run in a process of its own; and construction with the switch on.

Each run is one number; the JSON keeps every run, the table in the docs their
medians and the spread (min .. max) of the parent's runs."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS, REPS = 5, 200


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


def kernel():
    import torch
    from p2p_llm_tunnel_amd import ops
    out = {}
    for V in (32000, 151936):
        for B in (1, 16):
            g = torch.Generator().manual_seed(V + B)
            logits = (torch.randn(B, V, generator=g) * 4).to(torch.bfloat16).cuda()
            work = torch.empty_like(logits)
            ids = torch.zeros(B, dtype=torch.int64, device="cuda")
            tok = torch.randint(0, V, (B,), generator=g).cuda()
            dec = torch.ones(B, dtype=torch.int64, device="cuda")
            slot = torch.arange(B, dtype=torch.int64, device="cuda")
            params = torch.tensor([ops.pack_penalties(1.1, 0.5, 0.5)] * B, dtype=torch.int64).T.contiguous().cuda()
            state = torch.randint(0, 3, (B, V), generator=g, dtype=torch.int32).cuda()
            bias_n = torch.full((B,), 3, dtype=torch.int32, device="cuda")
            bias_ids = torch.arange(300, dtype=torch.int32).repeat(B, 1).cuda()
            bias_val = torch.ones(B, 300, dtype=torch.float32, device="cuda")
            fn = lambda: ops.penalize_(logits, work, ids, tok, dec, slot, params, state, bias_n, bias_ids, bias_val)
            out[f"V{V}_B{B}"] = [_timed(fn) for _ in range(RUNS)]
    return out


def _engine(config, penalties):
    import torch
    kw = {"penalties": True} if penalties else {}
    from p2p_llm_tunnel_amd.models.server import Engine
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng = Engine(device="cuda:0", config=config, max_batch=16, seed=0, **kw)
    torch.cuda.synchronize()
    return eng, time.perf_counter() - t0


def step(config):
    """post = 3 against post = 2 on one engine: 16 rows, one per slot, every row on."""
    from p2p_llm_tunnel_amd.models import engine as S
    eng, _ = _engine(config, True)
    try:
        b = eng._bufs[16][0]
        b.np[:] = 0
        b.np[S._SLOT, :] = b.np[S._REC, :] = range(16)
        b.np[S._PEN, :] = [[c] * 16 for c in S.Penalties(1.1, 0.5, 0.5).column()]
        b.np[S._LP, :] = 1
        runs = {2: [], 3: []}
        for _ in range(RUNS):
            for post in (2, 3):
                runs[post].append(_timed(eng._graphs[(16, 0, post)].replay))
        return {"post2_us": runs[2], "post3_us": runs[3]}
    finally:
        eng.stop()


def default(config, penalties):
    """One process: construction time and the 16-row post = 0 step of an engine."""
    eng, built = _engine(config, penalties)
    try:
        return {"construct_s": built, "step_us": _timed(eng._graphs[(16, 0, 0)].replay), "graphs": len(eng._graphs)}
    finally:
        eng.stop()


def _child(tree, what, config):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "profile_penalty.py"), "--child", what,
                        "--config", config], cwd=tree, env={**os.environ, "PYTHONPATH": tree}, capture_output=True,
                       text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{what} in {tree} failed:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "penalties.json"))
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its kernels built")
    ap.add_argument("--config", default="tiny")
    ap.add_argument("--child", default=None, choices=("default", "switch"))
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, os.getcwd())
        print(json.dumps(default(a.config, a.child == "switch")))
        return
    sys.path.insert(0, ROOT)
    res = {"config": a.config, "runs": RUNS, "reps": REPS, "kernel_us": kernel(), "step": step(a.config)}
    trees = {"this": ROOT, **({"parent": os.path.abspath(a.parent)} if a.parent else {})}
    runs = {k: [] for k in trees}
    runs["switch"] = []
    order = [(name, tree, "default") for name, tree in trees.items()] + [("switch", ROOT, "switch")]
    for k in range(RUNS):  # alternating, and rotated so that no variant always follows the same one
        for name, tree, what in order[k % len(order):] + order[:k % len(order)]:
            runs[name].append(_child(tree, what, a.config))
    res["default"] = runs
    med = lambda xs: statistics.median(xs)
    res["medians"] = {"kernel_us": {k: med(v) for k, v in res["kernel_us"].items()},
                      "step_us": {k: med(v) for k, v in res["step"].items()},
                      **{k: {"construct_s": med([r["construct_s"] for r in v]),
                             "step_us": med([r["step_us"] for r in v]),
                             "step_us_min_max": [min(r["step_us"] for r in v), max(r["step_us"] for r in v)]}
                         for k, v in runs.items()}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["medians"], indent=1))


if __name__ == "__main__":
    main()
