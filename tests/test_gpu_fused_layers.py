"""Layer 1 of the fused decode step, stage by stage against fp64 (decode_fused.hip, two-layer models).

tests/test_gpu_fused_stages.py, test_gpu_qwen2.py and test_gpu_qk_norm.py judge every kernel of the step from its
own observed inputs, on one-layer models. What the step does only from its second layer on is judged here, with
their references and their bounds (no tolerance of this module's own, except the sum-of-squares check below):

* the QKV GEMM reading the previous down projection's sum-of-squares partials (16 to 384 of them: below, at and
  above the 32 * NW that k_skinny holds in registers, the rest going through its late loop), as ROPE (Llama),
  ROPE_BIAS (Qwen2) and STORE + k_qknorm_rope (Qwen3);
* the cache offset L * layer_cache, with and without a row-to-slot map;
* layer 1's entries of the 6-, 7- and 8-entry weight table;
* what one layer leaves for the next inside a step: the attention tickets, the ss buffer, the residual.

How layer 1 is observed. The decoder passes ``dec.weights[i]`` to the kernels as is, so a weight zeroed in place
is zero in the step. The same step runs three times, both layers' caches restored to kc0 / vc0 before each:

1. layer 1's wo and w_down zeroed: the final residual is bf(x1 + bf(0)) = x1, layer 1's input, bit for bit;
2. layer 1's w_down zeroed: the final residual is r1, layer 1's residual after O; the ss buffer holds the down
   projection's partials over r1;
3. nothing zeroed: the final residual r2, the ss partials over r2, logits, ids, and both layers' caches.

The workspace views (q, attn, h, and qkv for a QK-norm model) hold the last layer's values after any pass; q and
attn depend on x1 alone and must be bit-identical in all three passes, h in passes 2 and 3.

The ss partials are also checked directly, after passes 2 and 3: for each row b < B the fp64 sum of the
down.grid_x partials ss[p, b] lies within (dim + 16) U S of S = sum_c resid[b, c]^2, computed in fp64 from the
observed bf16 residual. The squares of bf16 values are exact in fp32, and a sum of dim non-negative terms carries
at most dim U relatively in any order; 16 is the usual allowance for the adds across lanes. Rows >= B are
undefined and not looked at.

CPU tests hold the fp32 emulation (``test_gpu_fused_stages.emulate``, two layers) to the same ratios and the same
ss check on every case, and apply the slips of a later layer (``LAYER_SLIPS``) to it: each leaves the bound of
the stage it hits and no other. Slip ``drop_ss_partial`` (down leaves one partial out) fails the direct ss check
on every case (by 25 times the bound where one of 384 partials is lost, by thousands where one of 16 is). It
also shows in what layer 1's QKV GEMM makes of the previous down's partials (q, k, v; the raw qkv of a QK-norm
model, whose q and k are judged from it) where the lost share moves an element across a bf16 rounding tie. On the
CPU that is every case: ``SS_ONLY``, the cases where the direct check alone would catch it, is empty. The
narrowest are dim 1536 (1 partial of 384: 1/rms moves by 0.13 %, a third of the 0.39 % half ulp at the bottom of a
binade; q 2.7, k 2.5, v 1.002 times the bound) and dim 2048 at 8 rows (1 of 256: q 3.2, v 1.3).
"""
from dataclasses import replace

import pytest
import torch

from p2p_llm_tunnel_amd.models.tiny_llm import TinyLlama
import test_gpu_qk_norm as qk3
import test_gpu_qwen2 as qw2
from test_gpu_fused_stages import (BF, CASES as STEP_CASES, EPI_NAMES, F64, LAYER_SLIPS, SENTINEL_BITS, SENTINEL_ID, U,
                                   Case, emulate, gemm_ref, inputs, layer_w, plan_strings, rounded, stage_qkv,
                                   stage_ratios, step_plan, table_layout, table_stride, worst)

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")


# ---------------------------------------------------------------- cases
def _two(cfg):
    return replace(cfg, n_layers=2)


def _cases():
    step = {c.name: c for c in STEP_CASES}
    cs = []
    # Two-layer versions of test_gpu_fused_stages' cases. dim 256, ffn 512: layer 1's QKV <4,1,ROPE,2> holds 128
    # partials in registers and reads 64 (down in 4 K parts, 1 row) or 16 (5 and 17 rows, which end in a partial
    # row tile; 17 spans two, so the partial index p * 64 + m0 + row runs with m0 = 16).
    # dim 1536: <8,1,ROPE,4> reads 384 partials, 256 in registers and 128 in the late loop.
    # dim 2048: 256 partials at 8 rows, exactly the registers (the late loop runs zero times), 128 at 9 rows.
    # The attention shapes: 16 span slots, 2 span slots, and a prefill chunk behind decode rows with a row-to-slot
    # map (tickets and split partials used again by layer 1; L * layer_cache under a slot map).
    for name in ("gemm-d256-f512-r1", "gemm-d256-f512-r5", "gemm-d256-f512-r17", "gemm-d1536-f1152-r2",
                 "gemm-d2048-r8", "gemm-d2048-r9", "attn-ragged-D64-G2", "attn-B-D128-G4", "attn-C-D64-G4"):
        c = step[name]
        # attn-C: only the 4 decode rows sample; the 32 prefill rows keep their logits and ids untouched
        cs.append(replace(c, name="llama-" + name, cfg=_two(c.cfg), emit_rows=4 if name.startswith("attn-C") else 0))
    # Qwen2, the bias epilogue: wl[6] of layer 1. test_gpu_qwen2's shapes, positions and slots.
    for H, Hkv, D, rows in ((14, 2, 64, 17), (6, 1, 128, 1)):
        pos, slots = qw2.layout(rows)
        cs.append(Case(f"qwen2-H{H}-Hkv{Hkv}-D{D}-r{rows}", _two(qw2.BiasCase(H, Hkv, D, rows).cfg), pos, slots))
    # Qwen3, QK-norm: wl[6] and wl[7] of layer 1 and the STORE QKV. test_gpu_qk_norm's configs and layout.
    for name, rows, emit in (("D128", 16, 0), ("D64", 40, 3)):
        cfg = qk3.STAGE_CFGS[name]
        pos, slots = qk3.layout(qk3.Case(cfg.head_dim, cfg.n_heads, cfg.n_kv_heads, rows, cfg.rope_theta, seed=rows))
        cs.append(Case(f"qwen3-{name}-r{rows}", _two(cfg), tuple(pos), tuple(slots), emit_rows=emit))
    return [replace(c, seed=101 + i) for i, c in enumerate(cs)]


CASES = _cases()
CASE_IDS = [c.name for c in CASES]
FAMILY = [c for c in CASES if not c.name.startswith("llama-")]


# ---------------------------------------------------------------- layer 1 against fp64
def qkv_stage_of(case, obs):
    """The (q, k, v) references of layer ``layer`` for the case's family, as ``stage_ratios`` calls them."""
    c = case.cfg
    if c.qkv_bias:
        return lambda case, W, x0, pos, layer: qw2.stage_qkv_bias(c, layer_w(c, W, layer, "wqkv"), layer_w(c, W, layer, "bqkv"),
                                                                  x0, pos)
    if c.qk_norm:  # k_qknorm_rope, from the raw projection it read; v is copied: bound 0, bit equality
        def stage(case, W, x0, pos, layer):
            qr, kr, v = qk3.reference(obs["qkv"], layer_w(c, W, layer, "q_norm"), layer_w(c, W, layer, "k_norm"), pos, c.n_heads,
                                      c.n_kv_heads, c.head_dim, c.eps, c.rope_theta)
            return qr, kr, (v.to(F64), torch.zeros(v.shape, dtype=F64))
        return stage
    return stage_qkv


def ss_ratio(ss, resid, parts):
    """The direct check of the sum-of-squares partials ss [>= parts, >= B] against the bf16 residual rows
    resid [B, dim]: largest |sum_p ss[p, b] - S_b| / ((dim + 16) U S_b) (module docstring)."""
    B, dim = resid.shape
    S = resid.to(F64).pow(2).sum(1)
    return worst(ss[:parts, :B].to(F64).sum(0), (S, (dim + 16) * U * S))


def layer1_ratios(case, W, obs):
    """Every layer-1 stage ratio of ``stage_ratios``, the raw QKV projection of a QK-norm model (the STORE
    epilogue: gemm_ref's E and the one rounding) and the two direct ss checks."""
    c = case.cfg
    out = stage_ratios(case, W, obs, layer=1, qkv_stage=qkv_stage_of(case, obs))
    if c.qk_norm:
        y, E = gemm_ref(obs["x0"], layer_w(c, W, 1, "wqkv"), c.eps)
        out["qkv"] = worst(obs["qkv"], (y, rounded(y, E)))
    parts = step_plan(case).down.grid_x
    out["ss_r1"] = ss_ratio(obs["ss2"], obs["r1"], parts)
    out["ss_r2"] = ss_ratio(obs["ss3"], obs["r2"], parts)
    return out


def cache_problems(case, caches):
    """What is wrong with the caches [(kc, vc) of layer 0, of layer 1] after one step over kc0 / vc0 (empty: nothing).
    Every layer's K and V cache changed in exactly the rows (slot[b], pos[b]), and the rows appended to layer 0 and
    to layer 1 differ (a stride that writes one layer twice leaves them equal, or one layer unwritten)."""
    inp = inputs(case)
    sl = inp.slots.long() if inp.slots is not None else torch.arange(case.rows)
    ps = inp.pos.long()
    bad = []
    for i, (name, before) in enumerate((("K", inp.kc0), ("V", inp.vc0))):
        for L, pair in enumerate(caches):
            same = pair[i].view(torch.int16) == before.view(torch.int16)
            if bool(same[sl, ps].flatten(1).all(1).any()):
                bad.append(f"layer {L} {name}: a token row's cache row was not written")
            same[sl, ps] = True
            if not bool(same.all()):
                bad.append(f"layer {L} {name}: changed outside the token rows")
        a, b = caches[0][i][sl, ps].view(torch.int16), caches[1][i][sl, ps].view(torch.int16)
        if bool((a == b).flatten(1).all(1).any()):
            bad.append(f"{name}: layer 0 and layer 1 hold the same row")
    return bad


def layers_differ(case, W):
    """Layer 1's table entries are not layer 0's: a kernel that reads the wrong one computes something else."""
    T = table_layout(case.cfg)
    return all(not torch.equal(W[T.index(e.name, 0)], W[T.index(e.name, 1)]) for e in T if e.layer == 0)


def show(ratios):
    return {k: round(v, 3) for k, v in ratios.items()}


# ---------------------------------------------------------------- the emulation (CPU)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_fp32_emulation_of_layer_1_stays_inside_the_bounds(case):
    W = inputs(case).weights
    assert case.cfg.n_layers == 2 and len(W) == 3 + 2 * table_stride(case.cfg) and layers_differ(case, W)
    obs = emulate(case)
    ratios = layer1_ratios(case, W, obs)
    print("EMU", case.name, show(ratios))
    assert max(ratios.values()) <= 1.0, ratios
    assert cache_problems(case, obs["caches"]) == []


# slip -> the layer-1 outputs of which at least one must leave its bound; every other stage must stay inside
SLIP_HITS = {
    "late_loop": ("q", "k", "v"), "stale_ss": ("q", "k", "v"), "table:wqkv": ("q", "k", "v", "qkv"),
    "table:bias": ("q", "k", "v"), "table:qk_norm": ("q", "k"), "attend_layer0": ("attn",),
    "kv_into_layer0": ("k", "v"), "drop_ss_partial": ("ss_r1", "ss_r2"),
}
assert set(SLIP_HITS) == set(LAYER_SLIPS)
# Cases whose QKV outputs stay inside their bounds when down drops one partial (module docstring): none.
SS_ONLY = set()


def _slip_params():
    by = {c.name: c for c in CASES}
    out = [(by["llama-gemm-d1536-f1152-r2"], "late_loop")]
    for name in ("llama-gemm-d256-f512-r5", "llama-gemm-d1536-f1152-r2", "llama-attn-C-D64-G4"):
        out += [(by[name], s) for s in ("stale_ss", "table:wqkv", "attend_layer0", "kv_into_layer0")]
    for c in FAMILY:
        out += [(c, "table:wqkv"), (c, "table:bias" if c.cfg.qkv_bias else "table:qk_norm"), (c, "kv_into_layer0")]
    out += [(c, "drop_ss_partial") for c in CASES]
    return [pytest.param(c, s, id=f"{c.name}-{s}") for c, s in out]


@pytest.mark.parametrize("case,slip", _slip_params())
def test_a_slip_in_layer_1_leaves_the_bound(case, slip):
    obs = emulate(case, slip=slip)
    ratios = layer1_ratios(case, inputs(case).weights, obs)
    print("SLIP", case.name, slip, show(ratios))
    hit = [s for s in SLIP_HITS[slip] if s in ratios]
    assert max(ratios[s] for s in hit) > 1.0, ratios
    if slip == "drop_ss_partial":  # both direct checks fail; the QKV GEMM's outputs follow except on the SS_ONLY cases
        assert min(ratios[s] for s in hit) > 1.0, ratios
        fed = ["qkv"] if case.cfg.qk_norm else ["q", "k", "v"]  # a QK-norm model's q and k are judged from qkv
        assert (max(ratios[s] for s in fed) > 1.0) == (case.name not in SS_ONLY), ratios
        hit += fed
    # The appended rows landing in the other layer is the cache check's to catch; nothing else upsets it.
    assert bool(cache_problems(case, obs["caches"])) == (slip == "kv_into_layer0")
    clean = {s: r for s, r in ratios.items() if s not in hit and s != "ids"}
    assert max(clean.values()) <= 1.0, ratios


# ---------------------------------------------------------------- the plan (CPU: the library, no device)
# What each case launches, (qkv, attn, o, gate_up, down, lm_head) and the partials that layer 1's QKV, gate/up and
# the LM head read, as the library plans it. Literals: a heuristic that moves a case off its instantiation fails here.
_G = ("<4,1,ROPE,2>", "<4,1,SILU,2>", "<4,2,ARGMAX,2>")
_W = ("<8,1,ROPE,4>", "<8,1,SILU,4>", "<4,2,ARGMAX,4>")


def _row(attn, o, down, ss_in, three=_G, qkv=None):
    return ((qkv or three[0], attn, o, three[1], down, three[2]), (ss_in,) * 3)


EXPECTED_PLAN = {
    "llama-gemm-d256-f512-r1": _row("k_attn<64,2> 1 slots", "<4,1,RESID,1> kp4", "<4,1,RESID,1> kp4", 64),
    "llama-gemm-d256-f512-r5": _row("k_attn<64,2> 1 slots", "<4,1,RESID,2>", "<4,1,RESID,4>", 16),
    "llama-gemm-d256-f512-r17": _row("k_attn<64,2> 1 slots", "<4,1,RESID,2>", "<4,1,RESID,4>", 16),
    "llama-gemm-d1536-f1152-r2": _row("k_attn<64,2> 1 slots", "<4,1,RESID,1> kp4", "<4,1,RESID,4> kp4", 384, _W),
    "llama-gemm-d2048-r8": _row("k_attn<128,4> 1 slots", "<8,1,RESID,4> kp2", "<4,1,RESID,2> kp2", 256, _W),
    "llama-gemm-d2048-r9": _row("k_attn<128,4> 1 slots", "<8,1,RESID,4>", "<4,1,RESID,4>", 128, _W),
    "llama-attn-ragged-D64-G2": _row("k_attn<64,2> 16 slots", "<4,1,RESID,1> kp4", "<4,1,RESID,1> kp4", 64),
    "llama-attn-B-D128-G4": _row("k_attn<128,4> 2 slots", "<8,1,RESID,4>", "<4,1,RESID,2>", 16),
    "llama-attn-C-D64-G4": _row("k_attn<64,4> 1 slots", "<8,1,RESID,4>", "<4,1,RESID,2>", 16),
    "qwen2-H14-Hkv2-D64-r17": _row("k_attn<64,7> 2 slots", "<8,1,RESID,4>", "<4,1,RESID,2>", 16, qkv="<4,1,ROPE_BIAS,2>"),
    "qwen2-H6-Hkv1-D128-r1": _row("k_attn<128,6> 2 slots", "<4,1,RESID,2> kp4", "<4,1,RESID,1> kp4", 64,
                                  qkv="<4,1,ROPE_BIAS,2>"),
    "qwen3-D128-r16": _row("k_attn<128,2> 2 slots", "<4,1,RESID,4>", "<4,1,RESID,2>", 16, qkv="<4,1,STORE,2>"),
    "qwen3-D64-r40": _row("k_attn<64,4> 2 slots", "<4,1,RESID,2>", "<4,1,RESID,2>", 16, qkv="<4,1,STORE,2>"),
}


def test_plan_of_every_case_is_the_recorded_one():
    assert set(EXPECTED_PLAN) == set(CASE_IDS)
    for case in CASES:
        p = step_plan(case)
        assert (plan_strings(p), (p.qkv.ss_in, p.gate_up.ss_in, p.lm_head.ss_in)) == EXPECTED_PLAN[case.name], case.name
        assert p.qkv.ss_in == p.down.grid_x and p.qkv_first.ss_in == 1


def test_cases_cover_the_layer_1_qkv_paths_they_claim():
    # As P.qkv, between them: each QKV epilogue, and partial counts below, at and above what the registers hold.
    epis, fill = set(), set()
    for case in CASES:
        p = step_plan(case).qkv
        epis.add(EPI_NAMES[p.epi])
        fill.add((p.ss_in > 32 * p.nw) - (p.ss_in < 32 * p.nw))
    assert epis == {"ROPE", "ROPE_BIAS", "STORE"} and fill == {-1, 0, 1}


# ---------------------------------------------------------------- the kernels (GPU)
def observe_gpu(case):
    """Three passes of one step on the device (module docstring): layer 1's observations as ``emulate`` names them
    (CPU tensors), and the decoder's weight table."""
    inp = inputs(case)
    c, B = case.cfg, case.rows
    m = TinyLlama(c, device="cuda", max_batch=case.max_batch, seed=case.seed)
    dec = m.fused_decoder()
    views = dec.workspace_views()
    tokens, pos = inp.tokens.cuda(), inp.pos.cuda()
    slots = inp.slots.cuda() if inp.slots is not None else None
    kc0, vc0 = inp.kc0.cuda(), inp.vc0.cuda()
    logits = torch.empty(B, c.vocab, dtype=BF, device="cuda")
    ids = torch.empty(B, dtype=torch.int64, device="cuda")
    names = ("q", "attn", "h", "resid", "ss") + (("qkv",) if c.qk_norm else ())

    def run(zeroed):
        for L in range(c.n_layers):
            m.k_cache[L].copy_(kc0)
            m.v_cache[L].copy_(vc0)
        logits.view(torch.int16).fill_(SENTINEL_BITS)
        ids.fill_(SENTINEL_ID)
        saved = [w.clone() for w in zeroed]
        for w in zeroed:
            w.zero_()
        dec.step(tokens, pos, logits, ids, slots, case.emit_rows)
        torch.cuda.synchronize()
        for w, s in zip(zeroed, saved):
            w.copy_(s)
        return {k: (views[k] if k == "ss" else views[k][:B]).cpu() for k in names}

    wo, w_down = layer_w(c, dec.weights, 1, "wo"), layer_w(c, dec.weights, 1, "w_down")
    p1, p2, p3 = run([wo, w_down]), run([w_down]), run([])
    for k in names[:2] + names[5:]:  # q, attn (and qkv) depend on x1 alone: the same bits in every pass
        assert torch.equal(p1[k], p3[k]) and torch.equal(p2[k], p3[k]), k
    assert torch.equal(p2["h"], p3["h"])
    caches = [(m.k_cache[L].cpu(), m.v_cache[L].cpu()) for L in range(c.n_layers)]
    obs = {"x0": p1["resid"], "q": p3["q"], "attn": p3["attn"], "h": p3["h"], "r1": p2["resid"], "r2": p3["resid"],
           "ss2": p2["ss"], "ss3": p3["ss"], "qkv": p3.get("qkv"), "kc": caches[1][0], "vc": caches[1][1],
           "caches": caches, "logits": logits.cpu(), "ids": ids.cpu(), "counters": views["counters"].cpu()}
    return obs, [w.cpu() for w in dec.weights]


@cuda
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_layer_1_stages_match_fp64(case):
    inp = inputs(case)
    obs, W = observe_gpu(case)
    assert len(W) == len(inp.weights) == 3 + 2 * table_stride(case.cfg)
    for a, b in zip(W, inp.weights):  # the decoder's own table is what the references use
        assert torch.equal(a, b)
    assert layers_differ(case, W)
    ratios = layer1_ratios(case, W, obs)
    print("RATIO layer1", case.name, show(ratios), "PLAN", plan_strings(step_plan(case)))
    assert max(ratios.values()) <= 1.0, ratios
    assert cache_problems(case, obs["caches"]) == []
    # The attention arrival tickets are back at rest: layer 1 found them so, and so will the next step.
    assert not bool(obs["counters"].any())
    # Rows at or past emit_rows keep what logits and ids held before the step.
    emit = case.emit_rows or case.rows
    assert bool((obs["logits"][emit:].view(torch.int16) == SENTINEL_BITS).all())
    assert bool((obs["ids"][emit:] == SENTINEL_ID).all())
