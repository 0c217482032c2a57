"""Sliding-window attention in the fused decode step on the GPU (``k_attn<D, G, KV8, true>``,
docs/SLIDING_WINDOW.md): the attention stage element by element against fp64, then the model, graph replay, the
engine and the endpoint.

Attention stage. One-layer models, one step, q and the attention output read back through ``workspace_views`` and the
cache after the step. A row at position p with window W attends to [lo, p], lo = max(0, p + 1 - W). Its reference is
``test_gpu_fused_stages.stage_attn`` itself, bound included, called on the row's own slice ``cache[slot, lo:]`` with
the position ``p - lo``: the same fp64 softmax over exactly the attended rows, and no tolerance of this module's.
Every cache row below the smallest ``lo`` of the rows that read its slot is NaN before the step (a bf16 NaN, or the
byte 0x7F of an FP8 cache): a kernel that loaded such a row into a score, however small its weight, gives NaN.

The cases and the NumPy emulation of the span walk are shared with tests/test_sliding_window.py, which holds the
emulation to the same bound without a GPU.
"""
import http.client
import json
import math
import random
from dataclasses import dataclass, replace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.kv_scales import KvScales
from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig, TinyLlama
from test_gpu_fused_stages import BF, F64, stage_attn, worst

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu
F8 = torch.float8_e4m3fn
MAX_SEQ = 512
NAN_BF16 = 0x7FC0
NAN_E4M3 = 0x7F
KINDS = ("bf16", "fp8", "fp8-scaled")
SCALES = KvScales([[2.0, 0.25]], [[0.5, 4.0]])  # one layer, two KV heads; powers of two: the decode is exact


def win_cfg(D, G, W, n_layers=1, windows=None):
    return LlamaConfig(vocab=512, dim=256, n_layers=n_layers, n_heads=2 * G, n_kv_heads=2, head_dim=D, ffn=256,
                       max_seq=MAX_SEQ, windows=windows if windows is not None else (W,) * n_layers)


@dataclass(frozen=True)
class WinCase:
    """One step: row r at position ``pos[r]`` of cache slot ``slots[r]``, every layer with window ``W``."""
    name: str
    W: int
    pos: tuple
    slots: tuple

    @property
    def rows(self):
        return len(self.pos)

    @property
    def n_slots(self):
        return max(self.slots) + 1

    def lo(self, r):
        return max(0, self.pos[r] + 1 - self.W)

    def slot_floor(self, s):
        """The smallest ``lo`` of the rows that read slot ``s``: every cache row below it is poisoned."""
        return min(self.lo(r) for r in range(self.rows) if self.slots[r] == s)


def _lens_case(W):
    # Contexts W - 1, W, W + 1 (lo = 0, 0, 1), 2 W + 5 and 300, each row in a slot of its own, then three rows that
    # share slot 5 at consecutive positions. W = 500 (the most span slots max_seq = 512 allows: 8) keeps the lengths
    # that fit the cache. lo is 1, 18, 44, 71, 111, 168, 201, 237, 268 ...: no multiple of 8 or 32 in general.
    lens = [n for n in (W - 1, W, W + 1, 2 * W + 5, 300) if n <= MAX_SEQ] + ([MAX_SEQ] if 2 * W + 5 > MAX_SEQ else [])
    shared = min(2 * W + 10, MAX_SEQ - 3)
    pos = [n - 1 for n in lens] + [shared, shared + 1, shared + 2]
    slots = list(range(len(lens))) + [len(lens)] * 3
    return WinCase(f"lens-W{W}", W, tuple(pos), tuple(slots))


def _chunk_case(W):
    # A 40-row prefill chunk at positions 260..299 of one slot: every row has another lo (228..267 at W = 33).
    return WinCase(f"chunk40-W{W}", W, tuple(range(260, 300)), (0,) * 40)


STEPS = [_lens_case(W) for W in (33, 64, 100, 500)] + [_chunk_case(W) for W in (33, 100)]
STEP_IDS = [s.name for s in STEPS]
SHAPES = [(D, G) for D in (64, 128) for G in (1, 4, 7)]


def plan_slots(step, D, G):
    """gridDim.x of the windowed layer of ``step``, from the library's own plan."""
    from p2p_llm_tunnel_amd.models.tiny_llm import llama_dims
    return ops.window_plan(llama_dims(win_cfg(D, G, step.W), step.n_slots + 1), step.rows, step.W).slots


def windowed_attn_ratio(cfg, step, q, kd, vd, attn):
    """Largest |attn - reference| / bound over the rows of ``step``: ``stage_attn`` on each row's own slice of the
    (decoded) cache ``kd`` / ``vd`` [n_slots, max_seq, Hkv, D]. NaN anywhere in the output is inf."""
    worst_r = 0.0
    for r in range(step.rows):
        lo, s = step.lo(r), step.slots[r]
        ref = stage_attn(SimpleNamespace(cfg=cfg), q[r:r + 1], kd[s:s + 1, lo:], vd[s:s + 1, lo:],
                         torch.tensor([step.pos[r] - lo]), None)
        worst_r = max(worst_r, worst(attn[r:r + 1], ref))
    return worst_r


def poison_(kc, vc, step, fp8):
    """NaN into every row of ``kc`` / ``vc`` ([n_slots + 1, max_seq, Hkv, D]; bf16, or uint8 bytes) below the slot's
    ``slot_floor``. Returns the number of rows poisoned."""
    n = 0
    for s in range(step.n_slots):
        floor = step.slot_floor(s)
        for c in (kc, vc):
            if fp8:
                c[s, :floor] = NAN_E4M3
            else:
                c[s, :floor] = torch.tensor(NAN_BF16, dtype=torch.int32).to(torch.int16).view(BF)
        n += floor
    return n


def decoded(c, scale=None):
    """e4m3 bytes [.., Hkv, D] in fp64, times the KV head's scale."""
    x = c.view(F8).to(F64)
    return x * scale.to(F64)[:, None] if scale is not None else x


def step_inputs(step, D, G, kind, seed=0):
    """Seeded cache contents (poisoned), tokens: CPU tensors."""
    g = torch.Generator().manual_seed(7000 + 97 * D + 13 * G + step.W + seed)
    shape = (step.n_slots + 1, MAX_SEQ, 2, D)
    fp8 = kind != "bf16"
    if fp8:
        kc = (torch.randn(shape, generator=g) * 2.5).to(F8).view(torch.uint8)
        vc = torch.randn(shape, generator=g).to(F8).view(torch.uint8)
    else:
        kc, vc = (torch.randn(shape, generator=g) * 2.5).to(BF), torch.randn(shape, generator=g).to(BF)
    assert poison_(kc, vc, step, fp8) > 0
    tokens = torch.randint(0, 512, (step.rows,), generator=g)
    return kc, vc, tokens


def run_step(m, step, kc0, vc0, tokens, layer=0):
    """One step of ``m`` over ``step``'s rows with layer ``layer``'s cache set to kc0 / vc0 first; returns q, attn
    and that layer's cache after the step (CPU). Only the last layer's q and attn are left in the workspace."""
    raw = (lambda t: t.view(torch.uint8)) if m.kv_dtype == "fp8" else (lambda t: t)
    raw(m.k_cache[layer]).copy_(kc0.cuda())
    raw(m.v_cache[layer]).copy_(vc0.cuda())
    pos = torch.tensor(step.pos, dtype=torch.int32)
    m.decode_step(tokens.cuda(), pos.cuda(), (min(step.pos), max(step.pos)),
                  slots=torch.tensor(step.slots, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    views = m.fused_decoder().workspace_views()
    B = step.rows
    return (views["q"][:B].cpu(), views["attn"][:B].cpu(), raw(m.k_cache[layer]).cpu(), raw(m.v_cache[layer]).cpu())


# ---------------------------------------------------------------- 1. the attention stage
@cuda
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,G", SHAPES, ids=[f"D{D}-G{G}" for D, G in SHAPES])
@pytest.mark.parametrize("step", STEPS, ids=STEP_IDS)
def test_windowed_attention_matches_fp64(step, D, G, kind):
    cfg = win_cfg(D, G, step.W)
    fp8 = kind != "bf16"
    scales = SCALES if kind == "fp8-scaled" else None
    m = TinyLlama(cfg, device="cuda", max_batch=step.n_slots, seed=3, kv_dtype="fp8" if fp8 else "bf16",
                  kv_scales=scales)
    wp = ops.window_plan(m.dims(), step.rows, step.W)
    assert (wp.win, wp.window) == (1, step.W) and wp.slots == {33: 1, 64: 1, 100: 2, 500: 8}[step.W]
    assert ops.kv_plan(m.dims()).attn_kv8 == int(fp8) and ops.plan_kernels_ok(m.dims(), step.rows, windows=cfg.windows)
    kc0, vc0, tokens = step_inputs(step, D, G, kind)
    q, attn, kc, vc = run_step(m, step, kc0, vc0, tokens)
    # the step appended its rows and touched nothing else: the poison is still where it was
    for got, before in ((kc, kc0), (vc, vc0)):
        a, b = (got, before) if fp8 else (got.view(torch.int16), before.view(torch.int16))
        same = a == b
        same[list(step.slots), list(step.pos)] = True
        assert bool(same.all())
    if fp8:
        kd = decoded(kc, scales.k[0] if scales else None)
        vd = decoded(vc, scales.v[0] if scales else None)
    else:
        kd, vd = kc, vc
    assert bool(torch.isfinite(attn.float()).all())  # no poisoned row entered a softmax
    ratio = windowed_attn_ratio(cfg, step, q, kd, vd, attn)
    print("RATIO window attn", step.name, D, G, kind, "slots", wp.slots, round(ratio, 4))
    assert ratio <= 1.0, ratio


@cuda
@gpu
def test_the_window_is_in_the_result():
    # The output the windowed kernel gives is not full attention's: judged against stage_attn over [0, pos] (the
    # poison replaced by finite rows), rows whose lo > 0 are far outside the bound and rows with lo == 0 inside it.
    step, D, G = STEPS[2], 64, 4
    cfg = win_cfg(D, G, step.W)
    m = TinyLlama(cfg, device="cuda", max_batch=step.n_slots, seed=3)
    kc0, vc0, tokens = step_inputs(step, D, G, "bf16")
    q, attn, kc, vc = run_step(m, step, kc0, vc0, tokens)
    kc, vc = torch.nan_to_num(kc.float(), nan=1.0).to(BF), torch.nan_to_num(vc.float(), nan=1.0).to(BF)
    for r in range(step.rows):
        full = worst(attn[r:r + 1], stage_attn(SimpleNamespace(cfg=cfg), q[r:r + 1], kc, vc,
                                               torch.tensor([step.pos[r]]), torch.tensor([step.slots[r]])))
        assert (full > 10.0) == (step.lo(r) > 0), (r, full)


# ---------------------------------------------------------------- 2. mixed layers
@cuda
@gpu
@pytest.mark.parametrize("windows", [(0, 100), (100, 0)], ids=["full-then-window", "window-then-full"])
def test_mixed_layers_stage_by_stage(windows):
    # Two layers, one full and one windowed. Layer 1's attention is judged from the q and attn the workspace holds
    # after the step and layer 1's cache; layer 0's from a one-layer twin with the same weights and layer 0's window
    # (layer 0 of both computes the same thing from the same inputs: its K and V rows are compared bit for bit).
    step, D, G = STEPS[2], 64, 4
    cfg = win_cfg(D, G, 0, n_layers=2, windows=windows)
    m = TinyLlama(cfg, device="cuda", max_batch=step.n_slots, seed=5)
    plans = [ops.window_plan(m.dims(), step.rows, w) for w in windows]
    full = ops.step_plan(m.dims(), step.rows).attn.slots
    assert [(p.win, p.slots) for p in plans] == [(int(w > 0), 2 if w else full) for w in windows]
    kc0, vc0, tokens = step_inputs(step, D, G, "bf16")
    clean_k, clean_v = torch.nan_to_num(kc0.float(), nan=0.5).to(BF), torch.nan_to_num(vc0.float(), nan=0.5).to(BF)
    for layer in (0, 1):  # the windowed layer's cache poisoned, the full layer's finite
        src = (kc0, vc0) if windows[layer] else (clean_k, clean_v)
        m.k_cache[layer].copy_(src[0].cuda())
        m.v_cache[layer].copy_(src[1].cuda())
    k1, v1 = (kc0, vc0) if windows[1] else (clean_k, clean_v)
    q, attn, kc, vc = run_step(m, step, k1, v1, tokens, layer=1)
    assert bool(torch.isfinite(attn.float()).all())
    as_full = replace(step, W=MAX_SEQ)
    r1 = windowed_attn_ratio(cfg, step if windows[1] else as_full, q, kc, vc, attn)
    # layer 0: the one-layer twin
    twin = TinyLlama.from_weights(win_cfg(D, G, 0, windows=windows[:1]),
                                  dict(embed=m.embed, final_norm=m.final_norm, lm_head=m.lm_head, layers=m.layers[:1]),
                                  device="cuda", max_batch=step.n_slots)
    k0, v0 = (kc0, vc0) if windows[0] else (clean_k, clean_v)
    q0, attn0, kc_t, vc_t = run_step(twin, step, k0, v0, tokens)
    assert torch.equal(kc_t.view(torch.int16), m.k_cache[0].cpu().view(torch.int16))
    r0 = windowed_attn_ratio(cfg, step if windows[0] else as_full, q0, kc_t, vc_t, attn0)
    print("RATIO window mixed", windows, round(r0, 4), round(r1, 4))
    assert r0 <= 1.0 and r1 <= 1.0, (r0, r1)


# ---------------------------------------------------------------- 3. identity
@cuda
@gpu
@pytest.mark.parametrize("kind", ("bf16", "fp8"))
def test_a_window_as_long_as_the_cache_is_full_attention_bit_for_bit(kind):
    D, G = 128, 4
    base = replace(win_cfg(D, G, 0, n_layers=2), windows=None)
    g = torch.Generator().manual_seed(11)
    pos = torch.tensor([0, 63, 64, 300, 511, 129, 130, 131], dtype=torch.int32)
    slots = torch.tensor([0, 1, 2, 3, 4, 5, 5, 5], dtype=torch.int32)
    tokens = torch.randint(0, 512, (8,), generator=g)
    out = []
    for windows in (None, (MAX_SEQ, MAX_SEQ), (MAX_SEQ + 1000, 0)):
        m = TinyLlama(replace(base, windows=windows), device="cuda", max_batch=6, seed=8,
                      kv_dtype="fp8" if kind == "fp8" else "bf16")
        gg = torch.Generator().manual_seed(12)
        for c, s in ((m.k_cache, 2.5), (m.v_cache, 1.0)):
            c.copy_((torch.randn(c.shape, generator=gg) * s).to(c.dtype))
        if windows:
            assert ops.window_plan(m.dims(), 8, windows[0]).slots == ops.step_plan(m.dims(), 8).attn.slots
        ids, logits = m.decode_step(tokens.cuda(), pos.cuda(), (0, 511), return_logits=True, slots=slots.cuda())
        torch.cuda.synchronize()
        attn = m.fused_decoder().workspace_views()["attn"][:8].clone()
        out.append((ids.cpu(), logits.cpu(), attn.cpu(), m.k_cache.cpu().view(torch.uint8)))
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert torch.equal(a.view(torch.int16) if a.dtype == BF else a, b.view(torch.int16) if b.dtype == BF else b)


# ---------------------------------------------------------------- 4. the model
# Two layers, 4 / 2 heads of 64, window 24: the model of the model-level tests (seed 0 unless said otherwise).
WM = LlamaConfig(vocab=4096, dim=256, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512, max_seq=512,
                 sliding_window=24)
WM_FULL = replace(WM, windows=None)


def _ids(seed, n, vocab=4096):
    rng = random.Random(seed)
    return [rng.randrange(vocab) for _ in range(n)]


def greedy_reference(model, prompt, n_new):
    """Greedy continuation under the fp32 reference, with the smallest top-2 gap / max|logit| over its tokens."""
    seq, margin = list(prompt), math.inf
    for _ in range(n_new):
        lg = model.reference_logits(torch.tensor([seq], device=model.device))[0]
        top = lg.topk(2).values
        margin = min(margin, float(top[0] - top[1]) / float(lg.abs().max()))
        seq.append(int(lg.argmax()))
    return seq[len(prompt):], margin


# Prompts of the engine test, all longer than the window or crossing it while generating, with their greedy
# continuations under the fp32 reference of the windowed model (seed 0), searched on the CPU for a top-2 gap of at
# least 3 % of the largest logit at every generated index and for a continuation that the same model without its
# window does not give: tests/test_sliding_window.py::test_engine_prompts_are_confident_and_need_the_window re-checks
# both. 37 tokens (chunked prefill past the window), 27 tokens (just past it), 71 tokens (more than one 64-row step).
ENGINE_PROMPTS = [(_ids(2, 37), [243, 146, 1177, 3852, 2766, 2395]), (_ids(19, 27), [2857, 1595, 2311, 1332, 2755, 3780]),
                  (_ids(3, 71), [800, 2628, 3761, 1850, 2302, 2391])]
ENGINE_NEW = 6


@cuda
@gpu
def test_windowed_model_fused_against_the_reference():
    B, T = 3, 70  # far past the window of 24, across a 64-token boundary
    mf = TinyLlama(WM, device="cuda", max_batch=B, seed=4)
    assert mf.fused_decoder().windows == (24, 24)
    torch.manual_seed(1)
    seqs = torch.randint(0, WM.vocab, (B, T), device="cuda")
    for p in range(T):
        pos = torch.full((B,), p, dtype=torch.int32, device="cuda")
        _, lf = mf.decode_step(seqs[:, p], pos, (p, p), return_logits=True)
    ref = mf.reference_logits(seqs)
    scale = ref.abs().max().item()
    assert (lf.float() - ref).abs().max().item() < 0.05 * scale
    top2 = ref.topk(2, -1).values
    confident = (top2[:, 0] - top2[:, 1]) > 0.05 * scale
    assert torch.equal(lf.float().argmax(-1)[confident], ref.argmax(-1)[confident])
    # The window is in the result: the same weights without it give other logits.
    plain = TinyLlama.from_weights(WM_FULL, dict(embed=mf.embed, final_norm=mf.final_norm, lm_head=mf.lm_head,
                                                 layers=mf.layers), device="cuda", max_batch=B)
    assert (plain.reference_logits(seqs) - ref).abs().max().item() > 0.05 * scale
    # The unfused cross-check path refuses a windowed model.
    mu = TinyLlama(WM, device="cuda", max_batch=B, seed=4, fused=False)
    with pytest.raises(ValueError, match="sliding window runs the fused step only"):
        mu.decode_step(seqs[:, 0], torch.zeros(B, dtype=torch.int32, device="cuda"), (0, 0))


@cuda
@gpu
def test_windowed_model_graph_replay_matches_eager():
    torch.manual_seed(3)
    m = TinyLlama(WM, device="cuda", max_batch=4, seed=2)
    m.k_cache.normal_()
    m.v_cache.normal_()
    m.capture_graph(rows=4)
    toks = torch.randint(0, WM.vocab, (4,), device="cuda")
    pos = torch.tensor([5, 130, 0, 300], dtype=torch.int32, device="cuda")
    kc, vc = m.k_cache.clone(), m.v_cache.clone()
    ids_g, logits_g = m.graph_step(toks, pos, return_logits=True)
    logits_g, kg = logits_g.clone(), m.k_cache.clone()
    m.k_cache.copy_(kc)
    m.v_cache.copy_(vc)
    ids_e, logits_e = m.decode_step(toks, pos, (0, 300), return_logits=True)
    assert torch.equal(ids_g, ids_e)
    assert torch.equal(logits_g.view(torch.int16), logits_e.view(torch.int16))
    assert torch.equal(kg.view(torch.int16), m.k_cache.view(torch.int16))


def _collect(r):
    got = []
    while (t := r.out.get(timeout=60)) is not None:
        got.append(t)
    return got


@cuda
@gpu
@pytest.mark.parametrize("prefix_cache", (False, True), ids=("plain", "prefix-cache"))
def test_engine_serves_a_windowed_model(prefix_cache):
    from p2p_llm_tunnel_amd.models.server import Engine, Request
    model = TinyLlama(WM, device="cuda:0", max_batch=4, seed=0)
    eng = Engine(model=model, prefix_cache=prefix_cache, prefix_min=8)
    try:
        assert len(eng._graphs) == 12 and ENGINE_PROMPTS
        # all at once (batched, chunked prefill next to decode rows), then one by one: the CPU reference's tokens
        reqs = [eng.submit(Request(list(prompt), len(want))) for prompt, want in ENGINE_PROMPTS]
        for r, (prompt, want) in zip(reqs, ENGINE_PROMPTS):
            assert _collect(r) == list(want), len(prompt)
        for prompt, want in ENGINE_PROMPTS:
            assert _collect(eng.submit(Request(list(prompt), len(want)))) == list(want), len(prompt)
        if prefix_cache:
            assert eng.prefix_hits > 0  # the second round reused resident rows, and still gave the same tokens
    finally:
        eng.stop()


@cuda
@gpu
def test_eager_engine_refuses_a_windowed_model():
    from p2p_llm_tunnel_amd.models.server import Engine
    model = TinyLlama(WM, device="cuda:0", max_batch=2, seed=0)
    with pytest.raises(ValueError, match="a sliding window needs the graph-captured HIP step"):
        Engine(model=model, use_graph=False)


# ---------------------------------------------------------------- 5. a windowed Mistral checkpoint, served
# The seed was searched on the CPU so that the fp32 reference decides every compared token by at least 3 % of the
# largest logit and emits printable text: tests/test_sliding_window.py::test_served_chat_is_confident_and_needs_the_window
# re-checks that. The chat is 23 prompt tokens and 6 new ones against a window of 8.
SERVED_SEED = 13  # margin 0.0495
SERVED_MESSAGES = [{"role": "user", "content": "hello world"}]
SERVED_NEW = 6


def served_reference(path, tok, sliding_window=True):
    """Greedy continuation of the served chat under the fp32 reference of the checkpoint at ``path`` (CPU), with the
    smallest top-2 gap / max|logit| over its tokens: (prompt ids, new ids, margin)."""
    from p2p_llm_tunnel_amd.models.checkpoint import load_llama
    m = load_llama(path, device="cpu", max_batch=1, max_seq=256, sliding_window=sliding_window)
    prompt = tok.chat(SERVED_MESSAGES)
    new, margin = greedy_reference(m, prompt, SERVED_NEW)
    return prompt, new, margin


@cuda
@gpu
def test_a_windowed_mistral_checkpoint_behind_the_endpoint(tmp_path, capsys):
    from test_checkpoint import _tokenizer_dir
    from test_sliding_window import MISTRAL_W, hf_all_logits, mistral_checkpoint
    from p2p_llm_tunnel_amd.models.checkpoint import Tokenizer, load_llama
    from p2p_llm_tunnel_amd.models.server import start_server, window_line
    hf = mistral_checkpoint(str(tmp_path), seed=SERVED_SEED)
    ours = load_llama(str(tmp_path), device="cuda", max_batch=2, max_seq=256, sliding_window=True)
    assert ours.cfg.windows == (MISTRAL_W, MISTRAL_W) and ours.cfg.max_seq == 256 and ours.fused
    torch.manual_seed(5)
    T = 40
    seqs = torch.randint(0, ours.cfg.vocab, (2, T))
    d = seqs.cuda()
    for p in range(T):
        _, logits = ours.decode_step(d[:, p], torch.full((2,), p, dtype=torch.int32, device="cuda"), (p, p),
                                     return_logits=True)
    want = hf_all_logits(hf, seqs)[:, -1]
    scale = want.abs().max().item()
    assert (logits.float().cpu() - want).abs().max().item() < 0.05 * scale
    assert torch.nn.functional.cosine_similarity(logits.float().cpu(), want, dim=-1).min().item() > 0.995

    _tokenizer_dir(str(tmp_path))
    tok = Tokenizer(str(tmp_path))
    prompt, new, margin = served_reference(str(tmp_path), tok)
    assert len(prompt) + SERVED_NEW > MISTRAL_W  # the chat runs past the window
    assert margin >= 0.03 and max(new) < tok.tok.get_vocab_size() and not set(new) & tok.eos_ids, (new, margin)
    srv, port, eng = start_server(port=0, device="cuda:0", max_batch=2, checkpoint=str(tmp_path), max_seq=256,
                                  sliding_window=True)
    try:
        assert eng.use_graph and srv.tok is not None and eng.model.cfg.windowed and len(eng._graphs) == 12
        assert window_line(eng.model).startswith(f"sliding window: {MISTRAL_W} tokens on 2 of 2 layers; context 256")
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
