#!/usr/bin/env python3
"""Perplexity of a text file under a model, scored on the device (docs/PROMPT_LOGPROBS.md).

    python scripts/perplexity.py FILE --checkpoint DIR [--weight-dtype fp8] [--kv-dtype fp8] [--max-seq 2048]
    python scripts/perplexity.py FILE --config tiny          (random weights: shows the tool, not a model's quality)

The file is tokenised with the checkpoint's tokenizer (bytes for a --config model), cut into windows of --max-seq - 1
tokens, and every window goes through ``Engine(prompt_logprobs=True)`` as a scoring request without generation. A
window's first token has no log-probability, so windows do not overlap and each scores its tokens 1... One JSON line:
the tokens scored, the mean negative log-likelihood in nats and its exponential, the perplexity."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("file")
    ap.add_argument("--config", default="tiny")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--max-seq", type=int, default=None, help="window length (default: the model's context)")
    ap.add_argument("--weight-dtype", default="bf16")
    ap.add_argument("--kv-dtype", default="bf16")
    ap.add_argument("--expert-dtype", default="bf16")
    a = ap.parse_args(argv)

    from p2p_llm_tunnel_amd.models.engine import Engine, Request
    kw = dict(device=a.device, max_batch=8, kv_dtype=a.kv_dtype, weight_dtype=a.weight_dtype,
              expert_dtype=a.expert_dtype, prompt_logprobs=True)
    data = open(a.file, "rb").read()
    if a.checkpoint:
        from p2p_llm_tunnel_amd.models.checkpoint import Tokenizer, load_llama
        model = load_llama(a.checkpoint, device=a.device, max_batch=8, max_seq=a.max_seq, kv_dtype=a.kv_dtype,
                           weight_dtype=a.weight_dtype, expert_dtype=a.expert_dtype)
        ids = Tokenizer.for_checkpoint(a.checkpoint).encode(data.decode("utf-8", "replace"))
        engine = Engine(model=model, **kw)
    else:
        ids = list(data)
        engine = Engine(config=a.config, **kw)
    try:
        cfg = engine.model.cfg
        win = min(a.max_seq or cfg.max_seq, cfg.max_seq) - 1
        reqs = [engine.submit(Request(ids[i:i + win], 0, score=True)) for i in range(0, len(ids), win)
                if len(ids[i:i + win]) > 1]
        nll, n = 0.0, 0
        for r in reqs:
            r.out.get()
            nll -= sum(rec[0] for rec in r.prompt_lp[1:])
            n += len(r.prompt_lp) - 1
    finally:
        engine.stop()
    if not n:
        raise SystemExit("nothing to score: the file has fewer than two tokens")
    print(json.dumps({"file": a.file, "model": a.checkpoint or a.config, "weight_dtype": a.weight_dtype,
                      "kv_dtype": a.kv_dtype, "expert_dtype": a.expert_dtype, "window": win, "tokens": n,
                      "nll": nll / n, "perplexity": math.exp(nll / n)}))


if __name__ == "__main__":
    main()
