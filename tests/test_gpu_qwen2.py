"""Qwen2 / Qwen2.5 in the fused decode step: the QKV bias epilogue (``k_skinny<.., EPI_ROPE_BIAS, ..>``,
decode_fused_kernels.h) and the attention kernel at GQA ratios 5, 6 and 7, element by element against fp64, then
the model, the engine and a loaded Qwen2 checkpoint.

The bias epilogue. For output column n (row order of the interleaved weight) of token row m the kernel computes,
in fp32, ``t = acc[m][n] * rs[m] + bias[n]`` (acc the K-split MFMA sum, rs = 1/rms of the residual row), rounds t
to bf16 once, and for q and k rotates the pair (t[2i], t[2i+1]) = dims (i, i + D/2) and rounds again; v is stored
as the rounded t. The fp64 reference does the same from the exact bf16 residual (embed[token]: one-layer models),
weights and bias that the kernel read. The bound of an element is the q / k / v bound of
tests/test_gpu_fused_stages.py (``stage_qkv``) with y = proj * rs replaced by y + bias where a rounding applies
to it (U = 2^-24, ulp: the bf16 spacing):

* E = gemm_ref's bound on acc * rs (accumulation and 1/rms), unchanged: the bias is exact in fp32;
* the sum y + bias rounds once in fp32: E' = E + U |y + bias|;
* v = bf(y + bias): E' + ulp(|y + bias| + E') / 2, the output half ulp at |proj * rs + bias|;
* q, k: the inner rounding of y + bias flips only within E' of a tie (``flip``), then the rotation's own terms
  (cos/sin error, two products and an add) and the output half ulp, exactly as in ``stage_qkv``.

Nothing is scaled by a maximum over a row or the tensor. tests/test_qwen2_checkpoint.py holds an fp32 NumPy
emulation to this bound on the CPU, and six slips (bias dropped, added before the scale, added after RoPE, not
interleaved, missing on v, q's used for k) that each leave it.

Attention at G = 5, 6, 7 goes through test_gpu_fused_stages' own observation and stage references (every stage of
the step is judged, from its own observed inputs), on cases whose rows reach 1, 4, 11 and all 12 span slots.
"""
import functools
import http.client
import json
import math
import random
from dataclasses import dataclass, replace

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig, TinyLlama
from test_gpu_fused_stages import (BF, F64, U, Case as StepCase, _cfg, bf64, flip, gemm_ref, observe_gpu, plan_strings,
                                   rope_tables, rounded, stage_ratios, step_plan)

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu

POISON_BITS = 0x7B7B  # cache contents before the step; every row it must not touch keeps this pattern
EPS = 1e-6
EPI_ROPE, EPI_ROPE_BIAS = 1, 5
MAX_SEQ, N_SLOTS = 96, 5  # cache slots 0..4, and the scratch slot 5


# ---------------------------------------------------------------- the bias epilogue: cases
@dataclass(frozen=True)
class BiasCase:
    H: int
    Hkv: int
    D: int
    rows: int
    bias: str = "random"  # "random": the model's own draw (a few units); "big": up to 64; "zero"
    seed: int = 0

    @property
    def name(self):
        return f"H{self.H}-Hkv{self.Hkv}-D{self.D}-r{self.rows}-{self.bias}"

    @property
    def cfg(self):
        return LlamaConfig(vocab=512, dim=256, n_layers=1, n_heads=self.H, n_kv_heads=self.Hkv, head_dim=self.D,
                           ffn=256, max_seq=MAX_SEQ, eps=EPS, rope_theta=1e6, qkv_bias=True)


SHAPES = ((4, 2, 64), (14, 2, 64), (6, 1, 128))  # GQA ratios 2, 7 and 6
BIAS_CASES = [BiasCase(H, Hkv, D, rows, seed=10 * i + j) for i, (H, Hkv, D) in enumerate(SHAPES)
              for j, rows in enumerate((1, 16, 17, 40))]
BIAS_CASES += [BiasCase(14, 2, 64, 17, "big", seed=50), BiasCase(6, 1, 128, 17, "zero", seed=51)]
BIAS_IDS = [c.name for c in BIAS_CASES]


def layout(rows):
    """(pos, slots) of a step: up to three decode rows on slots 0, 1 and 3 (the first and the last position of the
    cache among them), then a prefill chunk of up to 8 consecutive positions on slot 2 and a second chunk with the
    rest on slot 4. One row alone sits in the middle of slot 3."""
    if rows == 1:
        return (37,), (3,)
    pos, slots = [0, MAX_SEQ - 1, 50][:min(rows, 3)], [0, 1, 3][:min(rows, 3)]
    a = min(8, rows - len(pos))
    pos += list(range(20, 20 + a))
    slots += [2] * a
    b = rows - len(pos)
    pos += list(range(3, 3 + b))
    slots += [4] * b
    assert len(set(zip(slots, pos))) == rows and max(pos) < MAX_SEQ
    return tuple(pos), tuple(slots)


@dataclass
class BiasInputs:
    model: TinyLlama  # on the CPU
    weights: list  # its fused weight table
    tokens: torch.Tensor
    pos: torch.Tensor
    slots: torch.Tensor


def _set_bias(m, case):
    if case.bias == "random":
        return
    g = torch.Generator().manual_seed(900 + case.seed)
    L = m.layers[0]
    if case.bias == "zero":
        L["bqkv"] = torch.zeros_like(L["bqkv"])
    else:  # magnitudes up to 64, both signs, a few exactly at it
        b = (torch.rand(L["bqkv"].shape, generator=g) * 128 - 64)
        b[::97] = 64.0
        b[5::97] = -64.0
        L["bqkv"] = b.to(BF).to(L["bqkv"].device)


@functools.lru_cache(maxsize=None)
def bias_inputs(case: BiasCase) -> BiasInputs:
    """Seeded inputs of a case, made once and shared (never modified) by every test."""
    m = TinyLlama(case.cfg, device="cpu", max_batch=N_SLOTS, seed=case.seed)
    _set_bias(m, case)
    g = torch.Generator().manual_seed(700 + case.seed)
    tokens = torch.randint(0, case.cfg.vocab, (case.rows,), generator=g)
    pos, slots = layout(case.rows)
    return BiasInputs(m, m.fused_weights(), tokens, torch.tensor(pos, dtype=torch.int32),
                      torch.tensor(slots, dtype=torch.int32))


# ---------------------------------------------------------------- the bias epilogue: fp64 reference and bound
def stage_qkv_bias(cfg, wqkv, bias, x0, pos):
    """(q, k, v) references and bounds [M, heads, D] from the residual rows x0, the folded and interleaved wqkv
    and the interleaved bias (all bf16, as the kernel read them): ``stage_qkv`` of test_gpu_fused_stages with the
    bias added to y where the module docstring says."""
    H, Hkv, half = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim // 2
    y, E = gemm_ref(x0, wqkv, cfg.eps)
    y = y + bias.to(F64)[None, :]
    E = E + U * y.abs()
    M = y.shape[0]
    y, E = y.view(M, H + 2 * Hkv, half, 2), E.view(M, H + 2 * Hkv, half, 2)  # pairs (dim i, dim i + D/2)
    vy, vE = y[:, H + Hkv:], E[:, H + Hkv:]
    v = torch.cat([vy[..., 0], vy[..., 1]], -1)
    vE = torch.cat([vE[..., 0], vE[..., 1]], -1)
    ry, rE = y[:, :H + Hkv], E[:, :H + Hkv]
    x1, x2 = bf64(ry[..., 0]), bf64(ry[..., 1])
    f1, f2 = flip(ry[..., 0], rE[..., 0]), flip(ry[..., 1], rE[..., 1])
    cs, sn, dsc = rope_tables(cfg, pos)
    o1, o2 = x1 * cs - x2 * sn, x2 * cs + x1 * sn
    common = (x1.abs() + x2.abs()) * dsc
    E1 = f1 * cs.abs() + f2 * sn.abs() + common + 3 * U * ((x1 * cs).abs() + (x2 * sn).abs())
    E2 = f2 * cs.abs() + f1 * sn.abs() + common + 3 * U * ((x2 * cs).abs() + (x1 * sn).abs())
    o, Eo = torch.cat([o1, o2], -1), torch.cat([E1, E2], -1)
    bo = rounded(o, Eo)
    return (o[:, :H], bo[:, :H]), (o[:, H:], bo[:, H:]), (v, rounded(v, vE))


@functools.lru_cache(maxsize=None)
def bias_reference(case: BiasCase):
    inp = bias_inputs(case)
    W = inp.weights
    return stage_qkv_bias(case.cfg, W[4], W[9], W[0][inp.tokens], inp.pos)


def bias_ratios(q, k_rows, v_rows, refs):
    """Largest |got - reference| / bound of q [M, H, D] and the appended k and v rows [M, Hkv, D]."""
    out = {}
    for name, got, (ref, bound) in zip("qkv", (q, k_rows, v_rows), refs):
        out[name] = ((got.to(F64).reshape(ref.shape) - ref).abs() / bound).max().item()
    return out


def poisoned(shape, device="cpu"):
    return torch.full(shape, POISON_BITS, dtype=torch.int16, device=device).view(BF)


def run_step(m, inp, rows):
    """One fused step of ``m`` (on the GPU) over poisoned caches: q rows, whole K and V caches of layer 0 (CPU)."""
    m.k_cache.view(torch.int16).fill_(POISON_BITS)
    m.v_cache.view(torch.int16).fill_(POISON_BITS)
    pos, slots = inp.pos.tolist(), inp.slots
    m.decode_step(inp.tokens.cuda(), inp.pos.cuda(), (min(pos), max(pos)), slots=slots.cuda())
    torch.cuda.synchronize()
    return m.fused_decoder().workspace_views()["q"][:rows].cpu(), m.k_cache[0].cpu(), m.v_cache[0].cpu()


def on_gpu(inp, cfg):
    """A device copy of the case's CPU model (the same weights, bit for bit), as ``cfg``."""
    src = inp.model
    w = dict(embed=src.embed.cuda(), final_norm=src.final_norm.cuda(), lm_head=src.lm_head.cuda(),
             layers=[{k: v.cuda() for k, v in L.items()} for L in src.layers])
    return TinyLlama.from_weights(cfg, w, device="cuda", max_batch=N_SLOTS)


@cuda
@gpu
@pytest.mark.parametrize("case", BIAS_CASES, ids=BIAS_IDS)
def test_bias_epilogue_matches_fp64(case):
    inp = bias_inputs(case)
    cfg, rows = case.cfg, case.rows
    m = on_gpu(inp, cfg)
    dec = m.fused_decoder()
    assert len(dec.weights) == 3 + 7
    for a, b in zip(dec.weights, inp.weights):  # the decoder's own table is what the reference used
        assert torch.equal(a.cpu(), b)
    plan = ops.step_plan(dec.dims, rows)
    assert plan.qkv.epi == plan.qkv_first.epi == EPI_ROPE_BIAS and plan.qkv.kpl == 0 and plan.qk_norm_grid == 0
    assert plan.attn.G == case.H // case.Hkv
    q, kc, vc = run_step(m, inp, rows)
    sl, ps = inp.slots.long(), inp.pos.long()
    ratios = bias_ratios(q, kc[sl, ps], vc[sl, ps], bias_reference(case))
    print("RATIO bias", case.name, {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    # The step appended one K and one V row per token row and touched nothing else in either cache.
    for got in (kc, vc):
        same = got.view(torch.int16) == POISON_BITS
        same[sl, ps] = True
        assert bool(same.all())
    assert not bool((kc[sl, ps].view(torch.int16) == POISON_BITS).all(-1).any())
    if case.bias == "big":
        assert float(inp.model.layers[0]["bqkv"].float().abs().max()) == 64.0
    if case.bias == "zero":
        # A zero bias changes no bit: the same weights without the bias (EPI_ROPE) give the same q, k and v rows.
        plain = on_gpu(inp, replace(cfg, qkv_bias=False))
        p_plan = ops.step_plan(plain.fused_decoder().dims, rows)
        assert p_plan.qkv.epi == EPI_ROPE and len(plain.fused_decoder().weights) == 3 + 6
        q0, kc0, vc0 = run_step(plain, inp, rows)
        for a, b in ((q, q0), (kc, kc0), (vc, vc0)):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@cuda
@gpu
def test_decoder_checks_the_weight_table():
    cfg = LlamaConfig(vocab=64, dim=64, n_layers=2, n_heads=2, n_kv_heads=1, head_dim=64, ffn=64, max_seq=8,
                      qkv_bias=True)
    m = TinyLlama(cfg, device="cuda", max_batch=1, seed=0)
    table = m.fused_weights()
    dims = ops.LlamaDims(vocab=64, dim=64, n_layers=2, H=2, Hkv=1, D=64, ffn=64, max_seq=8, max_batch=2, eps=1e-5,
                         theta=1e4, qkv_bias=1)
    with pytest.raises(ValueError, match="7 per layer"):
        ops.FusedLlamaDecoder(dims, table[:-1], m.k_cache, m.v_cache)
    short = list(table)
    short[3 + 7 + 6] = short[3 + 7 + 6][:-2].contiguous()
    with pytest.raises(ValueError, match="layer 1: bqkv"):
        ops.FusedLlamaDecoder(dims, short, m.k_cache, m.v_cache)
    both = ops.LlamaDims(vocab=64, dim=64, n_layers=2, H=2, Hkv=1, D=64, ffn=64, max_seq=8, max_batch=2, eps=1e-5,
                         theta=1e4, qkv_bias=1, qk_norm=1)
    with pytest.raises(ValueError):  # the 8-entry table of a QK-norm model, or unsupported dims: refused either way
        ops.FusedLlamaDecoder(both, table, m.k_cache, m.v_cache)
    ops.FusedLlamaDecoder(dims, table, m.k_cache, m.v_cache)


# ---------------------------------------------------------------- attention at GQA ratios 5, 6, 7
def _attn_cases():
    # 7 rows x 2 KV heads on a 768-token cache: attn_slots = min(256 / 14, 768 / 64) = 12 span slots. Decode rows at
    # pos 40 (one slot, written directly), 200 (span 64: 4 slots, the last of 9 tokens) and 767 (all 12 slots) on
    # cache slots 0..2, and a 4-row prefill chunk on slot 3 at 697..700 (11 slots; each row sees 0..its own pos).
    cs = []
    for D in (64, 128):
        for G in (5, 6, 7):
            cs.append(StepCase(f"attn-qwen2-D{D}-G{G}", _cfg(256, 256, 2 * G, 2, D, 768),
                               (40, 200, 767, 697, 698, 699, 700), slots=(0, 1, 2, 3, 3, 3, 3), seed=60 + len(cs)))
    return cs


ATTN_CASES = _attn_cases()
ATTN_IDS = [c.name for c in ATTN_CASES]


@cuda
@gpu
@pytest.mark.parametrize("case", ATTN_CASES, ids=ATTN_IDS)
def test_attention_at_the_new_ratios_matches_fp64(case):
    plan = step_plan(case)
    assert (plan.attn.G, plan.attn.slots, plan.attn.grid_y) == (case.cfg.n_heads // 2, 12, 14)
    obs, W = observe_gpu(case)
    ratios = stage_ratios(case, W, obs)
    print("RATIO", case.name, {k: round(v, 3) for k, v in ratios.items()}, "PLAN", plan_strings(plan))
    assert max(ratios.values()) <= 1.0, ratios


# ---------------------------------------------------------------- model, engine, checkpoint
# Two layers, 14 / 2 heads of 64 (Qwen2.5-0.5B's ratio), with the bias.
Q2 = LlamaConfig(vocab=4096, dim=256, n_layers=2, n_heads=14, n_kv_heads=2, head_dim=64, ffn=512, max_seq=512,
                 eps=EPS, rope_theta=1e6, qkv_bias=True)


def _ids(seed, n, vocab=4096):
    rng = random.Random(seed)
    return [rng.randrange(vocab) for _ in range(n)]


# Prompts of the engine test with their greedy continuations under the fp32 reference (model seed 0), searched on
# the CPU for a top-2 gap of at least 3 % of the largest logit at every generated index:
# tests/test_qwen2_checkpoint.py::test_engine_prompts_are_confident re-checks them.
# 37 tokens (chunked prefill next to nothing), one token, 71 tokens (more than one 64-row step)
ENGINE_PROMPTS = [(_ids(31, 37), [3190, 1470, 3528, 2678, 3819, 3190]), (_ids(43, 1), [1032, 186, 1663, 945, 2396, 3878]),
                  (_ids(176, 71), [3454, 3321, 190, 1470, 3528, 2678])]


@cuda
@gpu
def test_bias_model_fused_unfused_and_reference():
    # tests/test_gpu_qk_norm.py's tolerances and confident-argmax rule, on the 2-layer bias model at ratio 7.
    B, T = 3, 70  # crosses a 64-token attention split
    mf = TinyLlama(Q2, device="cuda", max_batch=B, seed=4, fused=True)
    mu = TinyLlama(Q2, device="cuda", max_batch=B, seed=4, fused=False)
    assert len(mf.fused_weights()) == 3 + 7 * Q2.n_layers
    torch.manual_seed(1)
    seqs = torch.randint(0, Q2.vocab, (B, T), device="cuda")
    for p in range(T):
        pos = torch.full((B,), p, dtype=torch.int32, device="cuda")
        idf, lf = mf.decode_step(seqs[:, p], pos, (p, p), return_logits=True)
        idu, lu = mu.decode_step(seqs[:, p], pos, (p, p), return_logits=True)
    scale = lu.float().abs().max().item()
    assert (lf.float() - lu.float()).abs().max().item() < 0.03 * scale
    top2 = lu.float().topk(2, -1).values
    confident = (top2[:, 0] - top2[:, 1]) > 0.03 * scale
    assert torch.equal(idf[confident], idu[confident])
    kdiff = (mf.k_cache[:, :B, :T].float() - mu.k_cache[:, :B, :T].float()).abs().max().item()
    assert kdiff < 0.05 * mu.k_cache[:, :B, :T].float().abs().max().item()

    ref = mf.reference_logits(seqs)
    for logits in (lf, lu):
        scale = ref.abs().max().item()
        assert (logits.float() - ref).abs().max().item() < 0.05 * scale
        top2 = ref.topk(2, -1).values
        confident = (top2[:, 0] - top2[:, 1]) > 0.05 * scale
        assert torch.equal(logits.float().argmax(-1)[confident], ref.argmax(-1)[confident])
    # The bias is in the result: the same weights without it give other logits.
    plain = TinyLlama.from_weights(replace(Q2, qkv_bias=False),
                                   dict(embed=mf.embed, final_norm=mf.final_norm, lm_head=mf.lm_head, layers=mf.layers),
                                   device="cuda", max_batch=B)
    assert (plain.reference_logits(seqs) - ref).abs().max().item() > 0.05 * scale


@cuda
@gpu
def test_bias_model_graph_replay_matches_eager():
    torch.manual_seed(3)
    m = TinyLlama(Q2, device="cuda", max_batch=4, seed=2)
    m.k_cache.normal_()
    m.v_cache.normal_()
    m.capture_graph(rows=4)
    toks = torch.randint(0, Q2.vocab, (4,), device="cuda")
    pos = torch.tensor([5, 130, 0, 300], dtype=torch.int32, device="cuda")
    kc, vc = m.k_cache.clone(), m.v_cache.clone()
    ids_g, logits_g = m.graph_step(toks, pos, return_logits=True)
    logits_g, kg = logits_g.clone(), m.k_cache.clone()
    m.k_cache.copy_(kc)
    m.v_cache.copy_(vc)
    ids_e, logits_e = m.decode_step(toks, pos, (0, 300), return_logits=True)
    assert torch.equal(ids_g, ids_e)
    assert (logits_g.float() - logits_e.float()).abs().max().item() < 1e-2
    assert torch.equal(kg.view(torch.int16), m.k_cache.view(torch.int16))


@cuda
@gpu
def test_engine_serves_a_bias_model():
    from p2p_llm_tunnel_amd.models.server import Engine, Request
    model = TinyLlama(Q2, device="cuda:0", max_batch=4, seed=0)
    twin = TinyLlama(Q2, device="cuda:0", max_batch=1, seed=0)
    eng = Engine(model=model)
    try:
        assert len(eng._graphs) == 12
        assert ENGINE_PROMPTS
        # all at once (batched, chunked prefill next to decode rows), then one by one: the same greedy tokens
        reqs = [eng.submit(Request(list(prompt), len(want))) for prompt, want in ENGINE_PROMPTS]
        for r, (prompt, want) in zip(reqs, ENGINE_PROMPTS):
            got = []
            while (t := r.out.get(timeout=60)) is not None:
                got.append(t)
            assert got == list(want), len(prompt)
        for prompt, want in ENGINE_PROMPTS:
            r = eng.submit(Request(list(prompt), len(want)))
            got = []
            while (t := r.out.get(timeout=60)) is not None:
                got.append(t)
            assert got == twin.generate(list(prompt), len(want)) == list(want)
    finally:
        eng.stop()


# The checkpoint the endpoint test serves: transformers' own Qwen2 (6 / 1 heads of 64 on hidden size 128), seeded.
# The seed was searched on the CPU so that the fp32 reference decides every compared token by at least 3 % of the
# largest logit and emits only ids the test tokenizer knows, with a printable text: ``served_reference`` and the
# tests that call it re-check that.
SERVED_SEED = 27  # margin 0.127; a model this small repeats one token, here " round"
SERVED_MESSAGES = [{"role": "user", "content": "hello world"}]
SERVED_NEW = 6


def served_reference(path, tok):
    """Greedy continuation of the served chat under the fp32 reference of the checkpoint at ``path`` (CPU), with
    the smallest top-2 gap / max|logit| over its tokens: (prompt ids, new ids, margin)."""
    from p2p_llm_tunnel_amd.models.checkpoint import load_llama
    m = load_llama(path, device="cpu", max_batch=1, max_seq=256)
    prompt = tok.chat(SERVED_MESSAGES)
    seq, margin = list(prompt), math.inf
    for _ in range(SERVED_NEW):
        lg = m.reference_logits(torch.tensor([seq]))[0]
        top = lg.topk(2).values
        margin = min(margin, float(top[0] - top[1]) / float(lg.abs().max()))
        seq.append(int(lg.argmax()))
    return prompt, seq[len(prompt):], margin


@cuda
@gpu
def test_fused_decode_on_a_loaded_qwen2_checkpoint(tmp_path):
    from test_checkpoint import _tokenizer_dir
    from test_qwen2_checkpoint import hf_logits, qwen2_checkpoint
    from p2p_llm_tunnel_amd.models.checkpoint import Tokenizer, load_llama
    from p2p_llm_tunnel_amd.models.server import start_server
    hf = qwen2_checkpoint(str(tmp_path), tie=True, seed=SERVED_SEED)
    ours = load_llama(str(tmp_path), device="cuda", max_batch=2, max_seq=256)
    assert ours.cfg.qkv_bias and ours.fused and ours.cfg.n_heads // ours.cfg.n_kv_heads == 6
    torch.manual_seed(5)
    T = 33
    seqs = torch.randint(0, ours.cfg.vocab, (2, T))
    d = seqs.cuda()
    for p in range(T):
        _, logits = ours.decode_step(d[:, p], torch.full((2,), p, dtype=torch.int32, device="cuda"), (p, p),
                                     return_logits=True)
    want = hf_logits(hf, seqs)
    scale = want.abs().max().item()
    assert (logits.float().cpu() - want).abs().max().item() < 0.05 * scale
    assert torch.nn.functional.cosine_similarity(logits.float().cpu(), want, dim=-1).min().item() > 0.995

    # ... and the endpoint serves it (hipGraph path) with a tokenizer next to it: one streamed chat completion,
    # whose tokens are the fp32 reference's (margin re-checked here, on the CPU).
    _tokenizer_dir(str(tmp_path))
    tok = Tokenizer(str(tmp_path))
    _, new, margin = served_reference(str(tmp_path), tok)
    assert margin >= 0.03 and max(new) < tok.tok.get_vocab_size() and not set(new) & tok.eos_ids, (new, margin)
    assert len(tok.decode(new).strip()) >= SERVED_NEW
    srv, port, eng = start_server(port=0, device="cuda:0", max_batch=2, checkpoint=str(tmp_path), max_seq=256)
    try:
        assert eng.use_graph and srv.tok is not None and eng.model.cfg.qkv_bias and len(eng._graphs) == 12
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        c.request("POST", "/v1/chat/completions", body=json.dumps(
            {"stream": True, "max_tokens": SERVED_NEW, "messages": SERVED_MESSAGES}))
        r = c.getresponse()
        data = r.read()
        assert r.status == 200 and data.rstrip().endswith(b"data: [DONE]")
        objs = [json.loads(l[6:]) for l in data.split(b"\n") if l.startswith(b"data: {")]
        text = "".join(o["choices"][0]["delta"].get("content", "") for o in objs)
        assert objs[-1]["choices"][0]["finish_reason"] == "length"
        assert text == tok.decode(new).rstrip("�"), (text, new)
    finally:
        srv.shutdown()
        eng.stop()
