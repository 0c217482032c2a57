"""MXFP4 (OCP Microscaling FP4) GEMM weights in the fused decode step, on the device (docs/WEIGHT_MXFP4.md).

The oracle needs no tolerance. Every MXFP4 value is an e2m1 number times a power of two, so an exact bf16 number, and
``k_skinny<.., W8 = 2>`` differs from the bf16 kernel only in how a B fragment is fetched and decoded: the A operand,
the k-step order, the MFMA, the reductions and every epilogue are the same code. So the step on ``(bytes, scales)``
must equal the bf16 step on ``dequantize_weight_mxfp4(bytes, scales)`` bit for bit, for every scale: every workspace
buffer, both caches whole, the logits and the ids. The LM head of an MXFP4 model is FP8; here it carries power-of-two
row scales, with which the FP8 kernel equals the bf16 one bit for bit too (tests/test_gpu_weight_fp8.py).

The weights are planted so that every nibble of both signs and every block exponent from 2^-20 to 2^8 occurs in each
of a layer's four GEMMs (asserted on the host before the launch), and every MXFP4 tensor is a view into a larger
buffer whose surroundings decode to large values (bytes 0x77, scale byte 254): a read one block or one row off
changes the result.
"""
import functools
import http.client
import json
import math
import os
import signal
import subprocess
import sys
from dataclasses import replace

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, GEMM_WEIGHTS, TinyLlama, llama_dims
from test_gpu_fused_stages import BF, SENTINEL_BITS, SENTINEL_ID, _cfg, fmt, inputs, step_plan
from test_gpu_kv_fp8 import LOGIT_BOUND, N_NEW, SCALING, _ids, collect, reference_generation
from test_gpu_weight_fp8 import _case, as_bytes, assert_same_step, pow2_scales

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu

F8 = torch.float8_e4m3fn
MICRO = CONFIGS["micro"]
FAMILIES = {"plain": {}, "bias": {"qkv_bias": True}, "table": {"rope_scaling": SCALING}, "qk_norm": {"qk_norm": True}}
EXPONENTS = range(-20, 9)  # E - 127 of the planted blocks


# ---------------------------------------------------------------- cases
def _bit_cases():
    """(dim, ffn, H, Hkv, D) x rows, with the family, the cache format and the layer count cycling through them.
    dim 64 / 256 / 544: 2, 8 and 17 k-steps on QKV and gate/up (17: the first width with 8 waves); ffn 32, 64, 96, 160
    and 512: 1, 2, 3, 5 and 16 k-steps on down (um 1, 2 and 4, uneven wave shares); rows 1 and 2 plan 4 K parts where
    K splits into them (O at H * D = 256 and 512, down at ffn 512), 16 fills a row tile, 17 and 40 run two and three
    (blockIdx.y). dim 2048 at 8 rows: 2 K parts."""
    shapes = [(64, 32, 1, 1, 64), (256, 64, 2, 1, 128), (544, 96, 8, 2, 64), (256, 160, 4, 2, 64),
              (544, 512, 4, 1, 128), (64, 512, 4, 2, 64)]
    fams = [(f, kv8) for f in FAMILIES for kv8 in (0, 1)]
    cs, i = [], 0
    for shape in shapes:
        for rows in (1, 2, 16, 17, 40):
            fam, kv8 = fams[i % len(fams)]
            cfg = replace(_cfg(*shape, 64), n_layers=1 + i % 2, **FAMILIES[fam])
            cs.append((_case(f"d{shape[0]}-f{shape[1]}-D{shape[4]}-r{rows}-{fam}-kv{8 if kv8 else 16}-L{cfg.n_layers}",
                             cfg, rows, 300 + i), kv8))
            i += 1
    cs.append((_case("d2048-f512-D128-r8-plain-kv16-L1", _cfg(2048, 512, 16, 4, 128, 64), 8, 399), 0))
    return cs


BIT_CASES = _bit_cases()
BIT_IDS = [c.name for c, _ in BIT_CASES]


def test_the_cases_cover_what_they_claim():
    seen, ksteps, fams = set(), set(), set()
    for case, kv8 in BIT_CASES:
        p, c = step_plan(case), case.cfg
        for s in ("qkv", "o", "gate_up", "down"):
            g = getattr(p, s)
            seen.add((g.nw, g.um, 1 << g.kpl))
            ksteps.add(g.K // 32)
        fams.add((c.qkv_bias, c.rope_scaling is not None, c.qk_norm, kv8, c.n_layers))
    assert {nw for nw, _, _ in seen} == {4, 8} and {um for _, um, _ in seen} == {1, 2, 4}
    assert {kp for _, _, kp in seen} == {1, 2, 4} and {1, 2, 3, 5, 16, 17} <= ksteps
    assert len({f[:4] for f in fams}) == 8 and {f[4] for f in fams} == {1, 2}
    assert {c.rows for c, _ in BIT_CASES} >= {1, 2, 16, 17, 40} and {c.cfg.head_dim for c, _ in BIT_CASES} == {64, 128}


# ---------------------------------------------------------------- tables
def planted(w, salt):
    """``w`` (fp32 [N, K]) with block j (row-major) rescaled so that its largest magnitude is 6 * 2^t, t cycling through
    EXPONENTS, and with the 15 non-zero e2m1 values of both signs and a zero written into the first 16 elements of the
    first block of every row, at that block's scale."""
    N, K = w.shape
    b = w.reshape(N, K // 32, 32).clone()
    t = ((torch.arange(N * (K // 32)) + salt) % len(EXPONENTS) + EXPONENTS[0]).reshape(N, K // 32)
    amax = b.abs().amax(2).clamp_min(1e-30)
    b = b * (torch.ldexp(torch.full_like(amax, 6.0), t.to(torch.int32)) / amax)[:, :, None]
    vals = torch.tensor([v * s for s in (1, -1) for v in ops.E2M1_VALUES])  # 0 .. 6, -0 .. -6
    b[:, 0, :16] = torch.ldexp(vals[None, :].expand(N, 16), t[:, :1].to(torch.int32))
    return b.reshape(N, K).contiguous()


def census(packed, scales):
    """Asserts that every nibble of both signs (zero once: -0 is never emitted) and every planted exponent occur."""
    codes = set(ops.unpack_weight_mxfp4(packed).flatten().tolist())
    assert codes == set(range(16)) - {8}, sorted(codes)
    exps = set((scales.to(torch.int32) - 127).flatten().tolist())
    assert exps == set(EXPONENTS), sorted(exps)


@functools.lru_cache(maxsize=None)
def tables(case):
    """(MXFP4 table, bf16 table) of a case, CPU: the case's own folded, interleaved bf16 table W' with every layer GEMM
    replaced by the quantised planted(W') on one side and its dequantisation as bf16 (exact) on the other; the LM head
    is e4m3(W' / s) with power-of-two row scales s on one side and decode(q) * s on the other."""
    cfg, W = case.cfg, inputs(case).weights
    T = ops.WeightTable(llama_dims(cfg, 1))
    mx, bf = list(W), list(W)
    i = T.index("lm_head")
    s = pow2_scales(cfg.vocab, 3)
    q = (W[i].float() / s[:, None]).to(F8)
    mx[i], bf[i] = q, (q.float() * s[:, None]).to(BF)
    scales = [s]
    for L in range(cfg.n_layers):
        for j, name in enumerate(GEMM_WEIGHTS):
            i = T.index(name, L)
            packed, e = ops.quantize_weight_mxfp4(planted(W[i].float(), 5 * L + j))
            if packed.shape[1] >= 16:  # a row of at least one block: every case
                census(packed, e)
            deq = ops.dequantize_weight_mxfp4(packed, e)
            mx[i], bf[i] = packed, deq.to(BF)
            assert torch.equal(bf[i].float(), deq) and bool(torch.isfinite(deq).all())
            scales.append(e)
    return mx + scales, bf


def guarded(t, fill):
    """``t`` on the device as a view into a larger buffer of ``fill`` bytes (4096 on either side)."""
    pad = 4096
    buf = torch.full((t.numel() + 2 * pad,), fill, dtype=torch.uint8, device="cuda")
    buf[pad:pad + t.numel()] = t.flatten().cuda()
    return buf[pad:pad + t.numel()].view(t.shape), buf


def run_step(case, table, weight_format, kv8, guard=False):
    """One step of a fresh decoder over ``table`` on caches that start from the case's kc0 / vc0; returns every
    workspace buffer, both caches, logits and ids as bytes. ``guard``: the MXFP4 tensors inside guard bytes."""
    inp, B, cfg = inputs(case), case.rows, case.cfg
    cache = lambda t: (t.float().clamp(-448, 448).to(F8) if kv8 else t)[None].expand(
        cfg.n_layers, *t.shape).contiguous().cuda()
    kc, vc = cache(inp.kc0), cache(inp.vc0)
    dev, bufs = [], []
    T = ops.WeightTable(llama_dims(cfg, case.max_batch + 1, kv8), weight_format=weight_format)
    for e, t in zip(T, table):
        if guard and e.dtypes == (torch.uint8,):
            view, buf = guarded(t, 254 if e.name.endswith(" scale") else 0x77)
            dev.append(view)
            bufs.append((buf, buf.clone()))
        else:
            dev.append(t.cuda())
    dec = ops.FusedLlamaDecoder(llama_dims(cfg, case.max_batch + 1, kv8), dev, kc, vc, weight_format=weight_format)
    logits = torch.empty(B, cfg.vocab, dtype=BF, device="cuda")
    logits.view(torch.int16).fill_(SENTINEL_BITS)
    ids = torch.full((B,), SENTINEL_ID, dtype=torch.int64, device="cuda")
    dec.step(inp.tokens.cuda(), inp.pos.cuda(), logits, ids, inp.slots.cuda() if inp.slots is not None else None,
             case.emit_rows)
    torch.cuda.synchronize()
    for buf, before in bufs:  # read-only inputs
        assert torch.equal(buf, before)
    out = {name: as_bytes(v).cpu() for name, v in dec.workspace_views().items()}
    out.update(k_cache=as_bytes(kc).cpu(), v_cache=as_bytes(vc).cpu(), logits=as_bytes(logits).cpu(), ids=ids.cpu())
    return out, (as_bytes(cache(inp.kc0)).cpu(), as_bytes(cache(inp.vc0)).cpu())


@cuda
@gpu
@pytest.mark.parametrize("case,kv8", BIT_CASES, ids=BIT_IDS)
def test_mxfp4_step_equals_the_bf16_step_on_the_dequantised_weights(case, kv8):
    mx, bf = tables(case)
    got, before = run_step(case, mx, "mxfp4", kv8, guard=True)
    want, _ = run_step(case, bf, "bf16", kv8)
    # q, the attention output, the SwiGLU output, the final residual and every other workspace buffer of the last
    # layer; the appended K / V rows of every layer (the caches whole); the logits and the ids.
    assert_same_step(got, want, (case.name, [fmt(getattr(step_plan(case), s)) for s in ("qkv", "o", "gate_up", "down")]))
    assert {"q", "attn", "h", "resid", "ss"} <= set(got)
    assert bool((got["ids"] != SENTINEL_ID).all())
    inp, c = inputs(case), case.cfg
    for cb, b in ((got["k_cache"], before[0]), (got["v_cache"], before[1])):  # appended rows alone changed
        diff = (cb != b).view(c.n_layers, case.max_batch + 1, c.max_seq, -1).any(-1)
        assert bool(diff.any(-1).any(-1).all())
        diff[:, inp.slots.long(), inp.pos.long()] = False
        assert not bool(diff.any())


@cuda
@gpu
def test_the_first_residual_matches_too():
    """``resid`` above is the residual after down. With w_down's nibbles zeroed on both sides the final residual of
    a one-layer model is the residual after O: the other residual stage, bit for bit."""
    case, kv8 = BIT_CASES[16]
    assert case.cfg.n_layers == 1
    mx, bf = (list(t) for t in tables(case))
    T = ops.WeightTable(llama_dims(case.cfg, 1))
    i = T.index("w_down", 0)
    mx[i], bf[i] = torch.zeros_like(mx[i]), torch.zeros_like(bf[i])
    got, _ = run_step(case, mx, "mxfp4", kv8, guard=True)
    want, _ = run_step(case, bf, "bf16", kv8)
    assert_same_step(got, want, case.name)
    full, _ = run_step(case, tables(case)[0], "mxfp4", kv8)
    assert not torch.equal(full["resid"], got["resid"])


# ---------------------------------------------------------------- validation, before any launch
@cuda
@gpu
def test_the_decoder_validates_an_mxfp4_table_on_the_host():
    case, _ = BIT_CASES[3]
    mx, bf = tables(case)
    dims = llama_dims(case.cfg, case.max_batch + 1)
    shape = (case.cfg.n_layers, case.max_batch + 1, case.cfg.max_seq, case.cfg.n_kv_heads, case.cfg.head_dim)
    kc, vc = torch.zeros(shape, dtype=BF, device="cuda"), torch.zeros(shape, dtype=BF, device="cuda")
    good = [t.cuda() for t in mx]
    T = ops.WeightTable(dims, weight_format="mxfp4")
    wq, sq, lm = T.index("wqkv", 0), T.scale_index("wqkv", 0), T.index("lm_head")

    def build(table, **kw):
        return ops.FusedLlamaDecoder(dims, table, kc, vc, **(kw or {"weight_format": "mxfp4"}))

    def with_(i, t):
        return good[:i] + [t] + good[i + 1:]

    build(good)
    with pytest.raises(TypeError, match="^layer 0: wqkv: the weight format is mxfp4.*nibble bytes"):
        build(with_(wq, bf[wq].cuda()))
    with pytest.raises(TypeError, match="^layer 0: wqkv scale: the weight format is mxfp4.*e8m0 bytes"):
        build(with_(sq, good[sq].float()))
    with pytest.raises(TypeError, match="^lm_head: weight_fp8 is set"):  # the LM head is the FP8 one
        build(with_(lm, bf[lm].cuda()))
    with pytest.raises(ValueError, match="^layer 0: wqkv has shape.*two nibbles per byte"):
        build(with_(wq, good[wq].repeat(1, 2)))
    with pytest.raises(ValueError, match="^layer 0: wqkv scale has shape.*one e8m0 byte per 32-element block"):
        build(with_(sq, good[sq][:, :-1].contiguous()))
    with pytest.raises(ValueError, match="HIP device"):
        build(with_(sq, good[sq].cpu()))
    wide = torch.zeros(good[wq].shape[0], 2 * good[wq].shape[1], dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        build(with_(wq, wide[:, ::2]))
    raw = torch.zeros(good[wq].numel() + 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="^layer 0: wqkv must be 4-byte aligned"):
        build(with_(wq, raw[2:2 + good[wq].numel()].view(good[wq].shape)))
    with pytest.raises(ValueError, match="weight table"):
        build(good[:-1])
    with pytest.raises(ValueError, match="weight table"):
        build([t.cuda() for t in bf])
    with pytest.raises((TypeError, ValueError)):
        build(good, weight_fp8=True)  # an MXFP4 table called FP8
    with pytest.raises(ValueError, match="not both"):
        build(good, weight_fp8=True, weight_format="mxfp4")
    with pytest.raises(ValueError, match="weight_format"):
        build(good, weight_format="int4")
    with pytest.raises(ValueError, match="weight_format"):
        build(good, weight_format=ops.WeightFormat(2, 2))
    # the library refuses a format it does not run, and an MXFP4 weight without its scales, before any launch
    lib, f = ops.lib(), ops.WeightFormat(2, 2)
    assert lib.p2pt_llama_plan_kernels_fmt(dims, 1, 0, f, None) == -1
    assert lib.p2pt_llama_decode_fmt(dims, f, None, None, None, None, None, None, None, None, 1, 0, None, 0, None, None,
                                     None) != 0


# ---------------------------------------------------------------- graph replay, the engine, the endpoint
@cuda
@gpu
def test_graph_replay_equals_the_eager_step_bit_for_bit():
    torch.manual_seed(3)
    m = TinyLlama(MICRO, device="cuda", max_batch=4, seed=2, weight_dtype="mxfp4")
    for c in (m.k_cache, m.v_cache):
        c.copy_(torch.randn(c.shape, device="cuda").to(BF))
    m.capture_graph(rows=4)
    toks = torch.randint(0, MICRO.vocab, (4,), device="cuda")
    pos = torch.tensor([5, 130, 0, 300], dtype=torch.int32, device="cuda")
    kc, vc = m.k_cache.clone(), m.v_cache.clone()
    ids_g, logits_g = m.graph_step(toks, pos, return_logits=True)
    ids_g, logits_g, kg, vg = ids_g.clone(), logits_g.clone(), m.k_cache.clone(), m.v_cache.clone()
    m.k_cache.copy_(kc)
    m.v_cache.copy_(vc)
    ids_e, logits_e = m.decode_step(toks, pos, (0, 300), return_logits=True)
    assert torch.equal(ids_g, ids_e) and torch.equal(as_bytes(logits_g), as_bytes(logits_e))
    assert torch.equal(as_bytes(kg), as_bytes(m.k_cache)) and torch.equal(as_bytes(vg), as_bytes(m.v_cache))
    assert not torch.equal(as_bytes(kg), as_bytes(kc))  # the step appended
    with pytest.raises(ValueError, match="fused step only"):
        TinyLlama(MICRO, device="cuda", max_batch=1, weight_dtype="mxfp4", fused=False).decode_step(
            torch.tensor([1], device="cuda"), torch.tensor([0], dtype=torch.int32, device="cuda"), (0, 0))


# Prompts searched on the CPU for a top-2 margin above LOGIT_BOUND at every generated token under the reference of
# the config, seed 0, with MXFP4 weights, for a bf16 and an FP8 cache alike. ``confident_prompts`` re-checks every one.
PROMPT_SEEDS = {"micro": ((325, 37), (283, 1), (255, 2), (267, 71)), "tiny": ((431, 9), (261, 3))}


@functools.lru_cache(maxsize=None)
def confident_prompts(config, kv_dtype):
    ref = TinyLlama(CONFIGS[config], device="cpu", max_batch=1, seed=0, weight_dtype="mxfp4", kv_dtype=kv_dtype)
    out = []
    for seed, n in PROMPT_SEEDS[config]:
        prompt = _ids(seed, n, CONFIGS[config].vocab)
        want, margin = reference_generation(ref, prompt, N_NEW)
        assert margin > LOGIT_BOUND, (seed, margin)  # every compared token is decided; none is skipped
        out.append((prompt, want))
    return out


@cuda
@gpu
@pytest.mark.parametrize("config,kv_dtype,prefix_cache", [("micro", "bf16", False), ("micro", "fp8", True),
                                                          ("tiny", "bf16", False)])
def test_engine_serves_mxfp4_weights(config, kv_dtype, prefix_cache):
    from p2p_llm_tunnel_amd.models.server import Engine, Request, Sampling
    eng = Engine(device="cuda:0", config=config, max_batch=4, seed=0, prefix_cache=prefix_cache, kv_dtype=kv_dtype,
                 weight_dtype="mxfp4")
    try:
        m = eng.model
        assert len(eng._graphs) == 12 and m.weight_dtype == "mxfp4" and m.kv_dtype == kv_dtype
        assert m.lm_head is None and m.lm_head_q.dtype == F8 and all(n not in L for L in m.layers for n in GEMM_WEIGHTS)
        assert all(L[n + "_q"].dtype == torch.uint8 and L[n + "_s"].dtype == torch.uint8
                   for L in m.layers for n in GEMM_WEIGHTS)
        prompts = confident_prompts(config, kv_dtype)
        for prompt, want in prompts:  # one by one, then all at once: token for token
            assert collect(eng.submit(Request(list(prompt), N_NEW))) == want
        reqs = [eng.submit(Request(list(prompt), N_NEW)) for prompt, want in prompts]
        assert [collect(r) for r in reqs] == [want for _, want in prompts]
        # a sampled request with logprobs: the sampler and the logprobs kernel follow the MXFP4 step in its graph
        s = eng.submit(Request(list(prompts[0][0]), N_NEW, sampling=Sampling(temperature=0.8, top_p=0.9, seed=7),
                               logprobs=3))
        toks = collect(s)
        assert len(toks) == N_NEW and all(0 <= t < m.cfg.vocab for t in toks)
        assert len(s.lp) == N_NEW and all(math.isfinite(lp[0]) and lp[0] <= 0.0 and len(lp[1]) == 3 for lp in s.lp)
    finally:
        eng.stop()


def _chat(port, messages, n):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    c.request("POST", "/v1/chat/completions", body=json.dumps({"stream": True, "max_tokens": n, "messages": messages}))
    r = c.getresponse()
    data = r.read()
    assert r.status == 200 and data.rstrip().endswith(b"data: [DONE]")
    objs = [json.loads(l[6:]) for l in data.split(b"\n") if l.startswith(b"data: {")]
    return "".join(o["choices"][0]["delta"].get("content", "") for o in objs)


@cuda
@gpu
def test_endpoint_serves_a_checkpoint_with_mxfp4_weights(tmp_path):
    from test_checkpoint import _tokenizer_dir
    from test_gpu_qwen2 import SERVED_MESSAGES, SERVED_NEW
    from test_qwen2_checkpoint import qwen2_checkpoint
    from p2p_llm_tunnel_amd.models.checkpoint import Tokenizer, load_llama
    from p2p_llm_tunnel_amd.models.server import start_server, weights_line
    from p2p_llm_tunnel_amd.utils.procs import free_port
    qwen2_checkpoint(str(tmp_path), tie=True, seed=2)  # searched on the CPU for the margin asserted below (0.070)
    _tokenizer_dir(str(tmp_path))
    tok = Tokenizer(str(tmp_path))
    ref = load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=256, weight_dtype="mxfp4")
    new, margin = reference_generation(ref, tok.chat(SERVED_MESSAGES), SERVED_NEW)
    assert margin > LOGIT_BOUND and not set(new) & tok.eos_ids, (new, margin)
    srv, port, eng = start_server(port=0, device="cuda:0", max_batch=2, checkpoint=str(tmp_path), max_seq=256,
                                  weight_dtype="mxfp4")
    try:
        m = eng.model
        assert eng.use_graph and len(eng._graphs) == 12 and m.cfg.qkv_bias and m.weight_dtype == "mxfp4"
        # a tied model: the bf16 embedding stays and the LM head is an FP8 copy of it
        assert m.embed.dtype == BF and m.lm_head is None and m.lm_head_q.shape == m.embed.shape
        assert m.weight_bytes() == ref.weight_bytes() and "mxfp4 GEMM weights" in weights_line(m, "mxfp4")
        text = _chat(port, SERVED_MESSAGES, SERVED_NEW)
        assert text == tok.decode(new).rstrip("�"), (text, new)
    finally:
        srv.shutdown()
        eng.stop()
    # once more through --gpus 1: the parent starts one replica, which must have been given the switch
    port = free_port()
    p = subprocess.Popen([sys.executable, "-m", "p2p_llm_tunnel_amd.models.server", "--gpus", "1", "--port", str(port),
                          "--checkpoint", str(tmp_path), "--max-seq", "256", "--max-batch", "2", "--weight-dtype",
                          "mxfp4"], stdout=subprocess.PIPE, text=True, start_new_session=True,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        lines = []
        for line in p.stdout:  # the replica shares the parent's stdout
            lines.append(line)
            if line.startswith("inference endpoint on"):
                break
        assert any("mxfp4 GEMM weights" in l and str(ref.weight_bytes()["total"]) in l for l in lines), lines
        assert _chat(port, SERVED_MESSAGES, SERVED_NEW) == text
    finally:
        os.killpg(p.pid, signal.SIGINT)
        try:
            p.wait(timeout=30)
        finally:
            if p.poll() is None:
                os.killpg(p.pid, signal.SIGKILL)
