"""Chunk attention on the GPU (``k_attn_chunk<D, G, KV8>``, docs/CHUNK_ATTN.md) against ``stage_attn``'s fp64 softmax,
whose bound is carried here as ``chunk_ref`` with the two terms re-derived that this kernel's chain changes."""
import http.client
import json
import math

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig, TinyLlama
from test_gpu_fused_stages import BF, F64, U, rounded, worst
from test_gpu_sliding_window import _collect, _ids

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]
F8 = torch.float8_e4m3fn
MAX_SEQ, NSLOTS, HKV = 512, 6, 2
KINDS = ("bf16", "fp8", "fp8-scaled")
K_SCALE, V_SCALE = torch.tensor([2.0, 0.25]), torch.tensor([0.5, 4.0])  # powers of two: the decode is exact

# Row layouts (pos, slots). (c): row 0 is the 16th row of the 15-row chunk of slot 1 (the engine's emit-first sort), 5
# decode rows on slots 0..4, a 43-row chunk on slot 3 and the 15-row chunk on slot 1: tile 0 makes 5 passes, slot 5 is
# unused. Decode rows share slots 1 and 3 with the chunks above their positions, so a pass masks rows at different pos.
LAYOUTS = {
    "a-16rows": (tuple(range(16)), (0,) * 16),
    "b-33rows": (tuple(range(60, 93)), (2,) * 33),
    "c-mixed": ((15, 0, 31, 32, 200, 511) + tuple(range(150, 193)) + tuple(range(15)),
                (1, 0, 1, 2, 3, 4) + (3,) * 43 + (1,) * 15),
    "d-end": (tuple(range(495, 512)), (5,) * 17),
}


def chunk_ref(D, G, q, kd, vd, pos, slots):
    """``stage_attn``'s reference and bound [M, H*D] for ``k_attn_chunk``, two terms re-derived from the kernel's chain
    and the library's own ``chunk_plan`` (nothing fitted):

    * the score (D exact bf16 products summed in fp32 by D / 32 MFMA steps, then scaled) stays inside (D + 8) U.
    * __expf passes of a weight: its own, the corr rescale of each later piece of its span (span / 32 - 1 of them, one
      workgroup walks a span piece by piece) and the span merge's weight: span / 32 + 1, where stage_attn has 6.
    * fp32 adds into the sums: a product p v passes the 32 adds of its MFMA step and the 2 further MFMAs of P's
      three-term split (exact terms: hi + mid + lo = p) in every piece of its span, and one add per span in the
      merge: 35 span / 32 + spans, where stage_attn has 64. The row sum l has fewer (8 + 2 per piece).
    The span is ``attn_span`` of the longest row on the plan's slots, its upper bound for every pass.
    """
    M, H = q.shape[0], q.shape[1]
    dims = ops.LlamaDims(vocab=512, dim=256, n_layers=1, H=H, Hkv=H // G, D=D, ffn=256, max_seq=kd.shape[1],
                         max_batch=kd.shape[0], eps=1e-5, theta=1e4)
    spans = ops.chunk_plan(dims, M).slots
    pieces = ops.attn_span(max(pos) + 1, spans) // 32
    scale = 1.0 / math.sqrt(D)
    refs, bounds = [], []
    for b in range(M):
        n = int(pos[b]) + 1
        K, V = kd[slots[b], :n].to(F64), vd[slots[b], :n].to(F64)
        qd = q[b].to(F64).view(H // G, G, D)
        s = torch.einsum("hgd,lhd->hgl", qd, K) * scale
        ds = (D + 8) * U * scale * torch.einsum("hgd,lhd->hgl", qd.abs(), K.abs()).amax(-1)
        R = s.amax(-1) - s.amin(-1)
        p = torch.softmax(s, -1)
        o = torch.einsum("hgl,lhd->hgd", p, V)
        A = torch.einsum("hgl,lhd->hgd", p, V.abs())
        eta = 2 * ds + (pieces + 1) * (2 * R + 4) * U + (35 * pieces + spans) * U
        refs.append(o.reshape(H * D))
        bounds.append(rounded(o, (2 * eta + 4 * U)[..., None] * A).reshape(H * D))
    return torch.stack(refs), torch.stack(bounds)


def make_caches(D, kind, seed, poison_above=None):
    """Seeded caches [NSLOTS, MAX_SEQ, HKV, D] (bf16, or e4m3 bytes) and their decoded values. ``poison_above``: slot ->
    highest attended position; every row above it (all rows of a slot not named) becomes NaN / 0x7F bytes."""
    g = torch.Generator().manual_seed(seed)
    shape = (NSLOTS, MAX_SEQ, HKV, D)
    k, v = torch.randn(shape, generator=g) * 2.5, torch.randn(shape, generator=g)
    fp8 = kind != "bf16"
    kc, vc = (k.to(F8), v.to(F8)) if fp8 else (k.to(BF), v.to(BF))
    kd, vd = kc.to(F64), vc.to(F64)
    if kind == "fp8-scaled":
        kd, vd = kd * K_SCALE.to(F64)[:, None], vd * V_SCALE.to(F64)[:, None]
    for s in range(NSLOTS if poison_above is not None else 0):
        for c in (kc, vc):
            (c.view(torch.uint8) if fp8 else c)[s, poison_above.get(s, -1) + 1:] = 0x7F if fp8 else float("nan")
    return kc, vc, kd, vd


def run_op(D, G, kind, layout, poison=False, seed=0):
    pos, slots = LAYOUTS[layout]
    top = {s: max(p for p, t in zip(pos, slots) if t == s) for s in set(slots)}
    kc, vc, kd, vd = make_caches(D, kind, 100 * D + G + seed, top if poison else None)
    g = torch.Generator().manual_seed(5 + seed)
    q = torch.randn((len(pos), HKV * G, D), generator=g).to(BF)
    sc = (K_SCALE.cuda(), V_SCALE.cuda()) if kind == "fp8-scaled" else (None, None)
    out = ops.chunk_attention(q.cuda(), kc.cuda(), vc.cuda(), torch.tensor(pos, dtype=torch.int32).cuda(),
                              torch.tensor(slots, dtype=torch.int32).cuda(), *sc)
    torch.cuda.synchronize()
    return q, kd, vd, out.cpu().reshape(len(pos), -1)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("G", (1, 4, 5, 8))
@pytest.mark.parametrize("D", (64, 128))
def test_chunk_attention_matches_fp64(D, G, kind, layout):
    pos, slots = LAYOUTS[layout]
    q, kd, vd, out = run_op(D, G, kind, layout)
    ratio = worst(out, chunk_ref(D, G, q, kd, vd, pos, slots))
    print("RATIO chunk attn", layout, D, G, kind, round(ratio, 4))
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,G", ((64, 4), (128, 8)))
def test_rows_above_the_attended_positions_are_never_read(D, G, kind):
    pos, slots = LAYOUTS["c-mixed"]
    q, kd, vd, out = run_op(D, G, kind, "c-mixed", poison=True)
    assert bool(torch.isfinite(out.float()).all())
    ratio = worst(out, chunk_ref(D, G, q, kd, vd, pos, slots))
    assert ratio <= 1.0, ratio
    # The planted slip: row 20 (slot 3, pos 164) judged against the reference of pos + 1, one extra token of finite
    # data, lies outside the bound. The bound is sharp enough to see a causal mask that is off by one.
    r = 20
    slip = chunk_ref(D, G, q[r:r + 1], kd, vd, (pos[r] + 1,), (slots[r],))
    assert worst(out[r:r + 1], slip) > 1.0


_STEP = dict(vocab=512, dim=256, n_layers=2, n_kv_heads=HKV, ffn=256, max_seq=MAX_SEQ)
STEP_CFGS = {"D64-G4": LlamaConfig(n_heads=8, head_dim=64, **_STEP),
             "D128-G8-qknorm": LlamaConfig(n_heads=16, head_dim=128, qk_norm=True, **_STEP)}


def run_model_step(m, rows, kc, vc, tokens):
    pos, slots = (x[:rows] for x in LAYOUTS["c-mixed"])
    for L in range(m.cfg.n_layers):
        m.k_cache[L].copy_(kc.cuda())
        m.v_cache[L].copy_(vc.cuda())
    ids, logits = m.decode_step(tokens[:rows].cuda(), torch.tensor(pos, dtype=torch.int32).cuda(), (min(pos), max(pos)),
                                return_logits=True, slots=torch.tensor(slots, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    v = m.fused_decoder().workspace_views()
    return ids.cpu(), logits.cpu(), v["q"][:rows].cpu(), v["attn"][:rows].cpu(), m.k_cache[-1].cpu(), m.v_cache[-1].cpu()


@pytest.mark.parametrize("name", STEP_CFGS)
def test_fused_step_with_chunk_attention(name):
    cfg = STEP_CFGS[name]
    D, G = cfg.head_dim, cfg.n_heads // cfg.n_kv_heads
    kc, vc, _, _ = make_caches(D, "bf16", 77)
    tokens = torch.randint(0, cfg.vocab, (64,), generator=torch.Generator().manual_seed(9))
    on = TinyLlama(cfg, device="cuda", max_batch=NSLOTS - 1, seed=3, chunk_attn=True)
    off = TinyLlama(cfg, device="cuda", max_batch=NSLOTS - 1, seed=3)
    assert on.fused_decoder().chunk_attn and not off.fused_decoder().chunk_attn
    pos, slots = LAYOUTS["c-mixed"]
    _, _, q, attn, k1, v1 = run_model_step(on, 64, kc, vc, tokens)
    ratio = worst(attn, chunk_ref(D, G, q, k1, v1, pos, slots))
    assert ratio <= 1.0, ratio
    # 16 rows: k_attn still runs, so the step is the unflagged decoder's bit for bit.
    for a, b in zip(run_model_step(on, 16, kc, vc, tokens), run_model_step(off, 16, kc, vc, tokens)):
        assert torch.equal(a.view(torch.int16) if a.dtype == BF else a, b.view(torch.int16) if b.dtype == BF else b)


# (seed, length) of the prompts: under the fp32 CPU reference of `tiny` (seed 0) the top-2 logit gap at each of the 8
# greedy steps is at least 4 bf16 ulps of the top logit (2^-5 of it at the least), so the order of an fp32 sum cannot
# decide a token. Checked on the CPU when the prompts were chosen (the first seed from 1 up that qualifies): the smallest
# gap over the 8 steps is 4.53 ulps for the 70-token prompt, 5.55 for the 130-token one and 4.31 for the 200-token one.
ENGINE_PROMPTS, ENGINE_NEW = ((34, 70), (44, 130), (36, 200)), 8


def test_engine_gives_the_default_engines_tokens():
    from p2p_llm_tunnel_amd.models.server import Engine, Request
    got = []
    for flag in (False, True):
        eng = Engine(device="cuda:0", config="tiny", chunk_attn=flag)
        try:
            assert eng.chunk_attn == flag and len(eng._graphs) == 12
            reqs = [eng.submit(Request(_ids(*p, vocab=32000), ENGINE_NEW)) for p in ENGINE_PROMPTS]
            got.append([_collect(r) for r in reqs])
        finally:
            eng.stop()
    assert all(len(t) == ENGINE_NEW for t in got[0]) and got[1] == got[0]


def test_endpoint_with_chunk_attention():
    from p2p_llm_tunnel_amd.models.server import start_server
    got = []
    for flag in (True, False):
        srv, port, eng = start_server(port=0, device="cuda:0", config="tiny", max_batch=2, chunk_attn=flag)
        try:
            c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
            c.request("POST", "/api/chat", body=json.dumps(
                {"messages": [{"role": "user", "content": "chunk attention reads keys and values once per tile " * 2}],
                 "stream": False, "num_predict": 6}))
            r = c.getresponse()
            got.append(json.loads(r.read()))
            assert r.status == 200 and eng.chunk_attn == flag, got[-1]
        finally:
            srv.shutdown()
            eng.stop()
    assert got[0]["prompt_eval_count"] > 16  # more than one row tile: the prompt ran through 64-row steps
    assert got[0]["eval_count"] == 6 and got[0]["message"] == got[1]["message"]
