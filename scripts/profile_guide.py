#!/usr/bin/env python3
"""What --guided costs (docs/GUIDED.md): medians of 5 alternating runs.

    python scripts/profile_guide.py --out profiles/guided.json [--parent DIR]

  kernel   ops.guide_ alone, every row on and advancing, about half the
           vocabulary allowed, at V = 32000 and 151936 and 1 and 16 rows. 50
           launches are captured into one graph and the replay is timed (events
           around 20 replays, after a warm-up), so the figure is device time per
           launch: launched one by one from Python the host's launch rate, about
           12.6 us a call, hides it. ``--only kernel`` measures this part alone
           and puts it into the existing JSON.
  step     the 16-row captured step of Engine(config, max_batch=16,
           guided=True): replays of its post = 4 graph (every row on) against its
           post = 2 graph, alternating, 200 replays a run.
  default  the 16-row post = 0 step and the construction time of the default
           engine (no switch) of this tree against the same of ``--parent``
           (a checkout of the parent commit with its kernels built), alternating
           and rotated, each run in a process of its own; and construction with
           the switch on.
  compile  host time of ``compile_guide`` for the test patterns over a synthetic
           vocabulary (256 bytes, merges, fillers of 2..12 bytes) of 32000 and
           151936 tokens.

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
IN_GRAPH = 50  # launches of guide_ in the graph whose replay ``kernel`` times
PATTERNS = [r"(yes|no|maybe)", r"[0-9]{3}-[0-9]{4}", r"-?[1-9][0-9]*(\.[0-9]+)?"]


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
    from p2p_llm_tunnel_amd.models.tiny_llm import capture
    out = {}
    for V in (32000, 151936):
        g = torch.Generator().manual_seed(V)
        # 8 states that all lead to one another: every launch advances and masks.
        arena = torch.randint(0, 8, (8, V), generator=g, dtype=torch.int16)
        arena[torch.rand(8, V, generator=g) < 0.5] = -1
        arena = arena.cuda()
        for B in (1, 16):
            logits = (torch.randn(B, V, generator=g) * 4).to(torch.bfloat16).cuda()
            work = torch.empty_like(logits)
            ids = torch.zeros(B, dtype=torch.int64, device="cuda")
            tok = torch.randint(0, V, (B,), generator=g).cuda()
            dec = torch.ones(B, dtype=torch.int64, device="cuda")
            slot = torch.arange(B, dtype=torch.int64, device="cuda")
            base = torch.zeros(B, dtype=torch.int32, device="cuda")
            cur = torch.zeros(B, dtype=torch.int32, device="cuda")
            def fifty():
                for _ in range(IN_GRAPH):
                    ops.guide_(logits, work, ids, tok, dec, slot, base, cur, arena)
            graph, _ = capture(fifty, torch.device("cuda:0"))
            out[f"V{V}_B{B}"] = [_timed(graph.replay, reps=20) / IN_GRAPH for _ in range(RUNS)]
    return out


def _engine(config, guided):
    import torch
    kw = {"guided": True, "guided_states": 64} if guided else {}
    from p2p_llm_tunnel_amd.models.server import Engine
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng = Engine(device="cuda:0", config=config, max_batch=16, seed=0, **kw)
    torch.cuda.synchronize()
    return eng, time.perf_counter() - t0


def step(config):
    """post = 4 against post = 2 on one engine: 16 rows, one per slot, every row on."""
    import torch
    from p2p_llm_tunnel_amd.models import engine as S
    eng, _ = _engine(config, True)
    try:
        V = eng.model.cfg.vocab
        g = torch.Generator().manual_seed(1)
        table = torch.randint(0, 8, (8, V), generator=g, dtype=torch.int16)
        table[torch.rand(8, V, generator=g) < 0.5] = -1
        eng._gd.arena[:8].copy_(table)
        eng._gd.base[:16] = 0
        b = eng._bufs[16][0]
        b.np[:] = 0
        b.np[S._SLOT, :] = b.np[S._REC, :] = range(16)
        b.np[S._DEC, :] = 1
        b.np[S._LP, :] = 1
        runs = {2: [], 4: []}
        for _ in range(RUNS):
            for post in (2, 4):
                runs[post].append(_timed(eng._graphs[(16, 0, post)].replay))
        return {"post2_us": runs[2], "post4_us": runs[4]}
    finally:
        eng.stop()


def default(config, guided):
    """One process: construction time and the 16-row post = 0 step of an engine."""
    eng, built = _engine(config, guided)
    try:
        return {"construct_s": built, "step_us": _timed(eng._graphs[(16, 0, 0)].replay), "graphs": len(eng._graphs)}
    finally:
        eng.stop()


def compile_times():
    import random
    from p2p_llm_tunnel_amd.models.guided import compile_guide
    out = {}
    for V in (32000, 151936):
        rng = random.Random(V)
        alphabet = b"abcdefghijklmnopqrstuvwxyz0123456789 .-"
        tb = [bytes([i]) for i in range(256)] + [b"yes", b"no", b"may", b"be", b"00", b"12", b"-1", b".5", b"345"]
        tb += [bytes(rng.choice(alphabet) for _ in range(rng.randint(2, 12))) for _ in range(V - len(tb) - 2)]
        tb += [b"", b""]
        for p in PATTERNS:
            runs = []
            for _ in range(RUNS):
                t0 = time.perf_counter()
                g = compile_guide("regex", p, tb, [V - 2, V - 1], 1024)
                runs.append(time.perf_counter() - t0)
            out[f"V{V} {p}"] = {"seconds": runs, "states": g.n_states}
    return out


def _child(tree, what, config):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "profile_guide.py"), "--child", what,
                        "--config", config], cwd=tree, env={**os.environ, "PYTHONPATH": tree}, capture_output=True,
                       text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{what} in {tree} failed:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided.json"))
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its kernels built")
    ap.add_argument("--config", default="tiny")
    ap.add_argument("--child", default=None, choices=("default", "switch"))
    ap.add_argument("--only", default=None, choices=("kernel",), help="measure this part alone into the existing --out")
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, os.getcwd())
        print(json.dumps(default(a.config, a.child == "switch")))
        return
    sys.path.insert(0, ROOT)
    if a.only:
        with open(a.out) as f:
            res = json.load(f)
        res["kernel_us"] = kernel()
        res["kernel_in_graph"] = IN_GRAPH
        res["medians"]["kernel_us"] = {k: statistics.median(v) for k, v in res["kernel_us"].items()}
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["medians"]["kernel_us"], indent=1))
        return
    res = {"config": a.config, "runs": RUNS, "reps": REPS, "kernel_us": kernel(), "kernel_in_graph": IN_GRAPH, "step": step(a.config),
           "compile": compile_times()}
    trees = {"this": ROOT, **({"parent": os.path.abspath(a.parent)} if a.parent else {})}
    runs = {k: [] for k in trees}
    runs["switch"] = []
    order = [(name, tree, "default") for name, tree in trees.items()] + [("switch", ROOT, "switch")]
    for k in range(RUNS):  # alternating, and rotated so that no variant always follows the same one
        for name, tree, what in order[k % len(order):] + order[:k % len(order)]:
            runs[name].append(_child(tree, what, a.config))
    res["default"] = runs
    med = statistics.median
    res["medians"] = {"kernel_us": {k: med(v) for k, v in res["kernel_us"].items()},
                      "step_us": {k: med(v) for k, v in res["step"].items()},
                      "compile_s": {k: med(v["seconds"]) for k, v in res["compile"].items()},
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
