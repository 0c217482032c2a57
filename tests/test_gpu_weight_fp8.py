"""FP8 (e4m3) GEMM weights with per-row scales in the fused decode step, on the device (docs/WEIGHT_FP8.md).

The oracle of the first two tests needs no tolerance. ``k_skinny<.., W8 = 1>`` keeps the bf16 kernel's arithmetic:
the same A fragments, the same k-step order, the same MFMA on the decoded bytes (``e4m3x8_to_bf16x8`` is exact), the
same reductions; the row scale multiplies the reduced accumulator once, ahead of 1/rms. With a scale that is a power
of two that product is exact and commutes with every rounding before it, so the FP8 step on ``(q, s)`` must equal the
bf16 step on the weights ``decode(q) * s`` (exact in bf16: three mantissa bits, exponents well inside bf16's) bit for
bit: every workspace buffer, both caches whole, the logits and the ids. Scales of 1.0 pin the stream and the decode;
scales of 2^-3 .. 2^3, different for neighbouring rows and so for gate_j and up_j, pin the scale's index, order and
placement.

General scales (``ops.quantize_weight_fp8``) are held to fp64 element by element with tests/test_gpu_fused_stages.py's
``stage_ratios`` on the dequantised table, see ``test_general_scales_match_fp64``.

Cases are the one-layer micro shapes of tests/test_gpu_fused_stages.py (its ``Case``, ``inputs`` and helpers), with
rows mapped onto permuted cache slots and a prefill chunk behind the decode rows.
"""
import functools
import http.client
import json
import math
from dataclasses import replace

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, GEMM_WEIGHTS, TinyLlama, llama_dims
from test_gpu_fused_stages import (BF, CASES, F64, SENTINEL_BITS, SENTINEL_ID, Case, _cfg, fmt, inputs, stage_ratios,
                                   step_plan, table_layout)
from test_gpu_kv_fp8 import LOGIT_BOUND, N_NEW, SCALING, _ids, collect, reference_generation

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu

F8 = torch.float8_e4m3fn
MICRO = CONFIGS["micro"]


# ---------------------------------------------------------------- cases
def _rows(rows, max_seq=64):
    """Row -> (position, slot): up to three decode rows on permuted slots 2, 0, 1, then a prefill chunk on slot 3
    at consecutive positions."""
    dec = min(rows, 3)
    pos = [(17 * r + 5) % (max_seq - 1) for r in range(dec)] + list(range(1, 1 + rows - dec))
    slots = [(2, 0, 1)[r] for r in range(dec)] + [3] * (rows - dec)
    return tuple(pos), tuple(slots)


def _case(name, cfg, rows, seed):
    pos, slots = _rows(rows, cfg.max_seq)
    return Case(name, cfg, pos, slots=slots, seed=seed)


FAMILY_FLAGS = {"plain": {}, "bias": {"qkv_bias": True}, "table": {"rope_scaling": SCALING},
                "bias+table": {"qkv_bias": True, "rope_scaling": SCALING}, "qk_norm": {"qk_norm": True}}


def _bit_cases():
    cs = []
    # dim 256, ffn 512, D 64, 4 waves: rows 1 plans 4 K parts on O and down (um 1); from 5 rows on none, O um 2,
    # down um 4; 17, 40 and 64 rows run 2, 3 and 4 row tiles.
    g = _cfg(256, 512, 4, 2, 64, 64)
    for rows in (1, 5, 16, 17, 40, 64):
        cs.append((_case(f"rows{rows}", g, rows, 40 + rows), 0))
    # 8 waves: down <8,1,RESID,4> (K 2816); QKV <8,1,ROPE,4>, gate/up <8,1,SILU,4> (K 1536, 4 K parts on O and
    # down); D 128 with 2 K parts at 8 rows and none at 9 (K 2048).
    cs.append((_case("down8w", _cfg(256, 2816, 4, 2, 64, 64), 5, 51), 0))
    cs.append((_case("qkv8w-kp4", _cfg(1536, 1152, 4, 2, 64, 64), 2, 52), 0))
    wide = _cfg(2048, 512, 16, 4, 128, 64)
    cs.append((_case("D128-kp2", wide, 8, 53), 0))
    cs.append((_case("D128-r9", wide, 9, 54), 0))
    # Every family at both head sizes and both cache formats, 5 rows (no K parts) and 2 rows (K parts).
    i = 60
    for fam, flags in FAMILY_FLAGS.items():
        for D, rows in ((64, 5), (128, 2)):
            for kv8 in (0, 1):
                cfg = replace(_cfg(256, 512, 256 // D, 2 if D == 64 else 1, D, 64), **flags)
                cs.append((_case(f"{fam}-D{D}-kv{8 if kv8 else 16}", cfg, rows, i), kv8))
                i += 1
    return cs


BIT_CASES = _bit_cases()
BIT_IDS = [c.name for c, _ in BIT_CASES]


def test_the_cases_cover_the_plans_they_claim():
    seen = set()
    for case, _ in BIT_CASES:
        p = step_plan(case)
        for s in ("qkv", "o", "gate_up", "down", "lm_head"):
            g = getattr(p, s)
            seen.add((g.nw, g.um, 1 << g.kpl))
    assert {nw for nw, _, _ in seen} == {4, 8} and {um for _, um, _ in seen} == {1, 2, 4}
    assert {kp for _, _, kp in seen} == {1, 2, 4}


# ---------------------------------------------------------------- tables
def gemm_indices(cfg):
    """Indices of the five GEMM weights in the fused table, in the order of their scales."""
    T = table_layout(cfg)
    return [T.index("lm_head")] + [T.index(n, L) for L in range(cfg.n_layers) for n in GEMM_WEIGHTS]


def pow2_scales(n, salt):
    """2^-3 .. 2^3, a step of 5 (mod 7) from one row to the next: neighbours, so gate_j and up_j, always differ."""
    e = (5 * torch.arange(n) + salt) % 7 - 3
    return torch.ldexp(torch.ones(n), e.to(torch.int32))


@functools.lru_cache(maxsize=None)
def tables(case, kind):
    """(FP8 table, bf16 table) of a case, CPU: the case's own folded, interleaved bf16 table W', with every GEMM
    weight replaced by q = e4m3(W' / s) and s on one side and by decode(q) * s as bf16 (exact) on the other."""
    cfg, W = case.cfg, inputs(case).weights
    f8, bf, scales = list(W), list(W), []
    for salt, i in enumerate(gemm_indices(cfg)):
        w = W[i].float()
        s = torch.ones(w.shape[0]) if kind == "ones" else pow2_scales(w.shape[0], salt)
        q = (w / s[:, None]).to(F8)
        deq = q.float() * s[:, None]
        f8[i], bf[i] = q, deq.to(BF)
        assert torch.equal(bf[i].float(), deq) and bool(torch.isfinite(deq).all())
        scales.append(s)
    return f8 + scales, bf


def dims_of(case, kv8):
    return llama_dims(case.cfg, case.max_batch + 1, kv8)


def as_bytes(t):
    return t.contiguous().view(torch.uint8)


def run_step(case, table, weight_fp8, kv8):
    """One step of a fresh decoder over ``table`` (device tensors or CPU ones) on caches that start from the case's
    kc0 / vc0, a finite pattern everywhere; returns every workspace buffer, both caches, logits and ids as bytes."""
    inp = inputs(case)
    B = case.rows
    cache = lambda t: (t.float().clamp(-448, 448).to(F8) if kv8 else t)[None].contiguous().cuda()
    kc, vc = cache(inp.kc0), cache(inp.vc0)
    dec = ops.FusedLlamaDecoder(dims_of(case, kv8), [t.cuda() if not t.is_cuda else t for t in table], kc, vc,
                                weight_fp8=weight_fp8)
    logits = torch.empty(B, case.cfg.vocab, dtype=BF, device="cuda")
    logits.view(torch.int16).fill_(SENTINEL_BITS)
    ids = torch.full((B,), SENTINEL_ID, dtype=torch.int64, device="cuda")
    dec.step(inp.tokens.cuda(), inp.pos.cuda(), logits, ids, inp.slots.cuda() if inp.slots is not None else None,
             case.emit_rows)
    torch.cuda.synchronize()
    out = {name: as_bytes(v).cpu() for name, v in dec.workspace_views().items()}
    out.update(k_cache=as_bytes(kc).cpu(), v_cache=as_bytes(vc).cpu(), logits=as_bytes(logits).cpu(), ids=ids.cpu())
    return out, (as_bytes(cache(inp.kc0)).cpu(), as_bytes(cache(inp.vc0)).cpu())


def assert_same_step(a, b, what):
    assert set(a) == set(b)
    for name in a:
        assert torch.equal(a[name], b[name]), (what, name, int((a[name] != b[name]).sum()))


@cuda
@gpu
@pytest.mark.parametrize("kind", ("ones", "pow2"))
@pytest.mark.parametrize("case,kv8", BIT_CASES, ids=BIT_IDS)
def test_fp8_step_equals_the_bf16_step_on_the_decoded_weights(case, kv8, kind):
    f8, bf = tables(case, kind)
    got, before = run_step(case, f8, True, kv8)
    want, _ = run_step(case, bf, False, kv8)
    assert_same_step(got, want, (case.name, kind, [fmt(getattr(step_plan(case), s)) for s in ("qkv", "o", "down")]))
    # The step did something: ids were written, and the caches changed in the appended rows alone.
    assert bool((got["ids"] != SENTINEL_ID).all())
    inp = inputs(case)
    for c, b in ((got["k_cache"], before[0]), (got["v_cache"], before[1])):
        diff = (c != b).view(1, case.max_batch + 1, case.cfg.max_seq, -1).any(-1)[0]
        assert bool(diff.any())
        diff[inp.slots.long(), inp.pos.long()] = False
        assert not bool(diff.any())


# ---------------------------------------------------------------- general scales against fp64
GENERAL = [c for c in CASES if c.name in ("gemm-d256-f512-r1", "gemm-d256-f512-r5", "gemm-d256-f512-r17",
                                          "gemm-d256-f352-r3", "gemm-d256-f2816-r5", "gemm-d1536-f1152-r2",
                                          "gemm-d2048-r8", "ids-emit3of5", "attn-ragged-D64-G2")]


@functools.lru_cache(maxsize=None)
def quantized_model(case):
    return TinyLlama(case.cfg, device="cpu", max_batch=case.max_batch, seed=case.seed, weight_dtype="fp8")


def dequantized_table(table, cfg):
    """The FP8 table as the references read it: every GEMM weight q * s in fp64 (exact), everything else as is."""
    T = table_layout(cfg, True)
    W = list(table[:len(table_layout(cfg))])
    for name, L in [("lm_head", None)] + [(n, L) for L in range(cfg.n_layers) for n in GEMM_WEIGHTS]:
        W[T.index(name, L)] = table[T.index(name, L)].to(F64) * table[T.scale_index(name, L)].to(F64)[:, None]
    return W


@cuda
@gpu
@pytest.mark.parametrize("case", GENERAL, ids=[c.name for c in GENERAL])
def test_general_scales_match_fp64(case):
    """Weights quantised by ``ops.quantize_weight_fp8`` (scales absmax / 448, no powers of two), every stage held to
    fp64 element by element by ``stage_ratios`` on the dequantised table q * s (fp64, exact).

    The bound is the stage bound as it stands. The kernel's value before any bf16 rounding is
    fl(fl(sum_k a_k q_k) * s) * rs. The decoded q_k are exact bf16 values, so the sum is what ``gemm_ref`` bounds with
    w = q: at most (K + n) U sum|a_k||q_k| with n <= 12 adds for the wave split (8) and the K parts (4), of the 16
    that ``gemm_ref`` grants. The scale multiply is one more fp32 rounding, U |y| <= U sum|a_k||q_k| s: n <= 13. Scaling
    both sides by s, (K + 16) U sum|a_k||q_k s| holds with the reference on w = q * s. Nothing is scaled by a global
    maximum: each element has its own sum."""
    m = quantized_model(case)
    inp = inputs(case)
    assert torch.equal(m.embed, inp.model.embed)  # the same seed: tokens, positions and caches are the case's
    B = case.rows
    dev = TinyLlama.from_weights(case.cfg, {"embed": m.embed.cuda(), "final_norm": m.final_norm.cuda(),
                                            "lm_head": m.embed.cuda(),  # replaced below: the table is the CPU model's
                                            "layers": [{k: v.cuda() for k, v in L.items()} for L in m.layers]},
                                 device="cuda", max_batch=case.max_batch, weight_dtype="fp8")
    dev.lm_head_q, dev.lm_head_s = m.lm_head_q.cuda(), m.lm_head_s.cuda()
    dev.k_cache[0].copy_(inp.kc0)
    dev.v_cache[0].copy_(inp.vc0)
    dec = dev.fused_decoder()
    for a, b in zip(dec.weights, m.fused_weights()):
        assert torch.equal(as_bytes(a).cpu(), as_bytes(b))
    views = dec.workspace_views()
    logits = torch.empty(B, case.cfg.vocab, dtype=BF, device="cuda")
    ids = torch.empty(B, dtype=torch.int64, device="cuda")
    slots = inp.slots.cuda() if inp.slots is not None else None

    def run():
        dec.step(inp.tokens.cuda(), inp.pos.cuda(), logits, ids, slots, case.emit_rows)
        torch.cuda.synchronize()
        return {k: views[k][:B].cpu() for k in ("q", "attn", "h", "resid")}

    w_down = dec.weights[dec.table.index("w_down", 0)]  # zero bytes: the final residual of the first pass is the residual after O
    saved = w_down.clone()
    w_down.view(torch.uint8).zero_()
    first = run()
    w_down.view(torch.uint8).copy_(saved.view(torch.uint8))
    second = run()
    obs = {"q": second["q"], "attn": second["attn"], "h": second["h"], "r1": first["resid"], "r2": second["resid"],
           "kc": dev.k_cache[0].cpu(), "vc": dev.v_cache[0].cpu(), "logits": logits.cpu(), "ids": ids.cpu()}
    ratios = stage_ratios(case, dequantized_table(m.fused_weights(), case.cfg), obs)
    print("RATIO w8", case.name, {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios


# ---------------------------------------------------------------- reads stay inside the buffers
@cuda
@gpu
@pytest.mark.parametrize("case,kv8", [BIT_CASES[0], BIT_CASES[3], BIT_CASES[7], BIT_CASES[8]],
                         ids=[BIT_IDS[i] for i in (0, 3, 7, 8)])
def test_reads_stay_inside_the_weights_and_scales(case, kv8):
    """Every FP8 weight is a uint8 view into the middle of a buffer of 0x7F (the e4m3 NaN) and every scale a view
    into a buffer of NaN: a byte or a scale read from outside reaches the outputs as NaN."""
    f8, _ = tables(case, "pow2")
    n = len(table_layout(case.cfg))
    pad = 4096
    wrapped, bufs = [t.cuda() for t in f8], []
    for j, i in enumerate(gemm_indices(case.cfg)):
        q, s = f8[i], f8[n + j]
        wb = torch.full((q.numel() + 2 * pad,), 0x7F, dtype=torch.uint8, device="cuda")
        wb[pad:pad + q.numel()] = q.view(torch.uint8).flatten().cuda()
        sb = torch.full((s.numel() + 2 * pad,), float("nan"), dtype=torch.float32, device="cuda")
        sb[pad:pad + s.numel()] = s.cuda()
        wrapped[i] = wb[pad:pad + q.numel()].view(q.shape)
        wrapped[n + j] = sb[pad:pad + s.numel()]
        bufs += [(wb, wb.clone()), (sb, sb.clone())]
    got, _ = run_step(case, wrapped, True, kv8)
    want, _ = run_step(case, f8, True, kv8)
    assert_same_step(got, want, case.name)
    B = case.rows
    assert bool(torch.isfinite(got["logits"].view(BF).float()).all())
    for buf, before in bufs:  # read-only inputs
        assert torch.equal(as_bytes(buf), as_bytes(before))


# ---------------------------------------------------------------- validation, before any launch
@cuda
@gpu
def test_the_decoder_validates_an_fp8_table_on_the_host():
    case, _ = BIT_CASES[1]
    f8, bf = tables(case, "ones")
    n = len(bf)
    dims = dims_of(case, 0)
    shape = (1, case.max_batch + 1, case.cfg.max_seq, case.cfg.n_kv_heads, case.cfg.head_dim)
    kc, vc = torch.zeros(shape, dtype=BF, device="cuda"), torch.zeros(shape, dtype=BF, device="cuda")
    good = [t.cuda() for t in f8]

    def build(table, fp8=True):
        return ops.FusedLlamaDecoder(dims, table, kc, vc, weight_fp8=fp8)

    def with_(i, t):
        return good[:i] + [t] + good[i + 1:]

    build(good)
    T = table_layout(case.cfg, True)
    wq, sq = T.index("wqkv", 0), T.scale_index("wqkv", 0)  # layer 0's wqkv and its scale
    with pytest.raises(TypeError, match="weight_fp8 is set"):
        build(with_(wq, bf[wq].cuda()))  # a bf16 weight in an FP8 table
    with pytest.raises(TypeError, match="weight_fp8 is set"):
        build(with_(2, good[2].to(torch.float16)))
    with pytest.raises(ValueError, match="shape"):
        build(with_(wq, good[wq][:-16].contiguous()))
    with pytest.raises(ValueError, match="one fp32 scale per output row"):
        build(with_(sq, good[sq][:-1].contiguous()))
    with pytest.raises(TypeError, match="scale"):
        build(with_(sq, good[sq].double()))
    with pytest.raises(ValueError, match="HIP device"):
        build(with_(sq, good[sq].cpu()))
    with pytest.raises(ValueError, match="contiguous"):
        build(with_(sq, good[sq].repeat_interleave(2)[::2]))
    wide = torch.zeros(good[wq].shape[0], 2 * good[wq].shape[1], dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        build(with_(wq, wide[:, ::2]))
    raw = torch.zeros(good[wq].numel() + 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="8-byte aligned"):
        build(with_(wq, raw[4:4 + good[wq].numel()].view(good[wq].shape)))
    with pytest.raises(ValueError, match="weight table"):
        build([t.cuda() for t in bf])  # a bf16 table with the FP8 flag
    with pytest.raises((TypeError, ValueError)):
        build(good, fp8=False)  # an FP8 table without it
    with pytest.raises(TypeError, match="needs weight_fp8"):
        build(good[:n], fp8=False)
    with pytest.raises(ValueError, match="weight table"):
        build(good[:-1])


# ---------------------------------------------------------------- graph replay, the model, the engine, the endpoint
# Prompts searched on the CPU for a top-2 margin above LOGIT_BOUND at every generated token under the reference of
# micro, seed 0, with FP8 weights, for a bf16 and an FP8 cache alike: 37 tokens, one token, two tokens, 71 tokens (more
# than one 64-row step). ``confident_prompts`` re-checks every margin.
PROMPT_SEEDS = ((336, 37), (810, 1), (478, 2), (267, 71))  # margins 0.077, 0.057, 0.086, 0.086 (the smaller format's)


@functools.lru_cache(maxsize=None)
def confident_prompts(kv_dtype):
    ref = TinyLlama(MICRO, device="cpu", max_batch=1, seed=0, weight_dtype="fp8", kv_dtype=kv_dtype)
    out = []
    for seed, n in PROMPT_SEEDS:
        prompt = _ids(seed, n)
        want, margin = reference_generation(ref, prompt, N_NEW)
        assert margin > LOGIT_BOUND, (seed, margin)  # every compared token is decided; none is skipped
        out.append((prompt, want))
    return out


@cuda
@gpu
def test_graph_replay_equals_the_eager_step_bit_for_bit():
    torch.manual_seed(3)
    m = TinyLlama(MICRO, device="cuda", max_batch=4, seed=2, weight_dtype="fp8")
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
        TinyLlama(MICRO, device="cuda", max_batch=1, weight_dtype="fp8", fused=False).decode_step(
            torch.tensor([1], device="cuda"), torch.tensor([0], dtype=torch.int32, device="cuda"), (0, 0))


@cuda
@gpu
@pytest.mark.parametrize("kv_dtype,prefix_cache,penalties", [("bf16", False, False), ("fp8", True, False),
                                                             ("bf16", True, True)])
def test_engine_serves_fp8_weights(kv_dtype, prefix_cache, penalties):
    from p2p_llm_tunnel_amd.models.server import Engine, Request, Sampling
    eng = Engine(device="cuda:0", config="micro", max_batch=4, seed=0, prefix_cache=prefix_cache, kv_dtype=kv_dtype,
                 penalties=penalties, weight_dtype="fp8")
    try:
        m = eng.model
        assert len(eng._graphs) == (16 if penalties else 12) and m.weight_dtype == "fp8" and m.kv_dtype == kv_dtype
        assert m.lm_head is None and m.lm_head_q.dtype == F8 and all(n not in L for L in m.layers for n in GEMM_WEIGHTS)
        prompts = confident_prompts(kv_dtype)
        for prompt, want in prompts:  # one by one, then all at once
            assert collect(eng.submit(Request(list(prompt), N_NEW))) == want
        reqs = [eng.submit(Request(list(prompt), N_NEW)) for prompt, want in prompts]
        assert [collect(r) for r in reqs] == [want for _, want in prompts]
        # a sampled request with logprobs: the sampler and the logprobs kernel follow the FP8 step in its graph
        s = eng.submit(Request(list(prompts[0][0]), N_NEW, sampling=Sampling(temperature=0.8, top_p=0.9, seed=7),
                               logprobs=3))
        toks = collect(s)
        assert len(toks) == N_NEW and all(0 <= t < MICRO.vocab for t in toks)
        assert len(s.lp) == N_NEW and all(math.isfinite(lp[0]) and lp[0] <= 0.0 and len(lp[1]) == 3 for lp in s.lp)
    finally:
        eng.stop()


@cuda
@gpu
def test_endpoint_serves_a_checkpoint_with_fp8_weights(tmp_path):
    from test_checkpoint import _tokenizer_dir
    from test_gpu_qwen2 import SERVED_MESSAGES, SERVED_NEW, SERVED_SEED
    from test_qwen2_checkpoint import qwen2_checkpoint
    from p2p_llm_tunnel_amd.models.checkpoint import Tokenizer, load_llama
    from p2p_llm_tunnel_amd.models.server import start_server, weights_line
    qwen2_checkpoint(str(tmp_path), tie=True, seed=SERVED_SEED)
    _tokenizer_dir(str(tmp_path))
    tok = Tokenizer(str(tmp_path))
    ref = load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=256, weight_dtype="fp8")
    prompt = tok.chat(SERVED_MESSAGES)
    new, margin = reference_generation(ref, prompt, SERVED_NEW)
    assert margin > LOGIT_BOUND and not set(new) & tok.eos_ids, (new, margin)
    srv, port, eng = start_server(port=0, device="cuda:0", max_batch=2, checkpoint=str(tmp_path), max_seq=256,
                                  weight_dtype="fp8")
    bf = load_llama(str(tmp_path), device="cpu", max_batch=2, max_seq=256)
    try:
        m = eng.model
        assert eng.use_graph and len(eng._graphs) == 12 and m.cfg.qkv_bias and m.weight_dtype == "fp8"
        # a tied model: the bf16 embedding stays and the LM head is an FP8 copy of it
        assert m.embed.dtype == BF and m.lm_head is None and m.lm_head_q.shape == m.embed.shape
        assert m.weight_bytes()["gemm"] < bf.weight_bytes()["gemm"] + m.embed.numel() + 4 * m.cfg.vocab
        assert "fp8 GEMM weights" in weights_line(m, "fp8")
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        c.request("POST", "/v1/chat/completions", body=json.dumps(
            {"stream": True, "max_tokens": SERVED_NEW, "messages": SERVED_MESSAGES}))
        r = c.getresponse()
        data = r.read()
        assert r.status == 200 and data.rstrip().endswith(b"data: [DONE]")
        objs = [json.loads(l[6:]) for l in data.split(b"\n") if l.startswith(b"data: {")]
        text = "".join(o["choices"][0]["delta"].get("content", "") for o in objs)
        assert text == tok.decode(new).rstrip("�"), (text, new)
    finally:
        srv.shutdown()
        eng.stop()
