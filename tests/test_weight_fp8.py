"""FP8 (e4m3) GEMM weights with per-row scales, without a GPU (docs/WEIGHT_FP8.md): the quantiser against the NumPy
e4m3 reference (``utils/kv_fp8_ref.py``), the plans and pinned layouts, the switches, and an fp32 emulation of the FP8
GEMM + epilogue held to fp64, with the slips the bound must catch. tests/test_gpu_weight_fp8.py runs the kernels.
"""
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models import server
from p2p_llm_tunnel_amd.models.tiny_llm import (GEMM_WEIGHTS, LlamaConfig, TinyLlama, fused_row_perm,
                                                quantize_gemm_weight)
from p2p_llm_tunnel_amd.utils import kv_fp8_ref as ref
from test_gpu_fused_stages import (BF, F64, Case, _cfg, _emulate_attn, first_argmax, inputs, layer_w, stage_ratios,
                                   step_plan)
from test_gpu_qwen2 import stage_qkv_bias
from test_kv_fp8 import FAMILIES, dims, flat

F8 = torch.float8_e4m3fn


def u8(q):
    return q.view(torch.uint8).numpy()


# ---------------------------------------------------------------- the quantiser
@functools.lru_cache(maxsize=None)
def sample():
    g = torch.Generator().manual_seed(11)
    w = torch.randn(96, 160, generator=g) * torch.exp(3 * torch.randn(96, 1, generator=g))  # rows of many magnitudes
    w[7] = 0.0
    w[8, 5:] = 0.0
    w[9] *= 1e-30
    return w


def test_torch_decodes_every_byte_as_the_reference_does():
    b = torch.arange(256, dtype=torch.uint8)
    got, want = b.view(F8).float().numpy(), ref.decode(b.numpy())
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


def test_quantiser_matches_the_reference_encoding():
    w = sample()
    q, s = ops.quantize_weight_fp8(w)
    assert q.dtype == F8 and s.dtype == torch.float32 and q.shape == w.shape and s.shape == (w.shape[0],)
    assert q.is_contiguous() and s.is_contiguous()
    amax = w.abs().amax(1)
    assert torch.equal(s, torch.where(amax > 0, amax / 448.0, torch.ones(())))
    # every byte is the reference encoding of W' / s, the division in fp32
    assert np.array_equal(u8(q), ref.encode((w / s[:, None]).numpy()))
    dec = ref.decode(u8(q)).astype(np.float64)
    assert not np.isnan(dec).any()  # no NaN byte
    # each row's largest magnitude maps to +-448 exactly
    top = np.abs(dec).max(1)
    assert np.array_equal(top[amax.numpy() > 0], np.full(int((amax > 0).sum()), 448.0))
    i = w.abs().argmax(1)
    assert np.array_equal(dec[np.arange(len(i)), i.numpy()], 448.0 * np.sign(w[torch.arange(len(i)), i].numpy()))
    # |W' - q s| <= s half_ulp(q) element by element (plus the fp32 roundings of the division and of this product)
    s64, w64 = s.numpy().astype(np.float64)[:, None], w.numpy().astype(np.float64)
    slack = 2.0 ** -22 * np.abs(w64)
    assert (np.abs(w64 - dec * s64) <= s64 * ref.half_ulp(dec) + slack).all()
    # a zero row: scale 1 and zero bytes
    assert s[7].item() == 1.0 and not u8(q)[7].any()
    assert ops.dequantize_weight_fp8(q, s).dtype == torch.float32
    assert torch.equal(ops.dequantize_weight_fp8(q.view(torch.uint8), s), q.float() * s[:, None])


def test_quantiser_refuses_what_it_cannot_represent():
    w = sample().clone()
    for bad in (float("nan"), float("inf"), float("-inf")):
        x = w.clone()
        x[3, 4] = bad
        with pytest.raises(ValueError, match="non-finite"):
            ops.quantize_weight_fp8(x)
    with pytest.raises(TypeError, match="fp32"):
        ops.quantize_weight_fp8(w.to(BF))
    with pytest.raises(TypeError, match="fp32"):
        ops.quantize_weight_fp8(w[0])
    m = TinyLlama(MICRO1, device="cpu", max_batch=1)
    m.layers[0]["wo"][2, 3] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        TinyLlama.from_weights(MICRO1, dict(embed=m.embed, final_norm=m.final_norm, lm_head=m.lm_head,
                                            layers=m.layers), device="cpu", weight_dtype="fp8")


def test_the_fold_happens_in_fp32_before_quantising():
    # Row 0: 1.0 * 1.0 sets the scale, 1 / 448. 0.7265625 * 0.8359375 = 0.607360..., times 448 = 272.097: above the
    # e4m3 tie at 272, so 288 (0x79). Through bf16 the product rounds to 0.60546875, times 448 = 271.25: 256 (0x78).
    w = torch.tensor([[1.0, 0.7265625, 0.0, -0.7265625]], dtype=BF)
    g = torch.tensor([1.0, 0.8359375, 1.0, 0.8359375], dtype=BF)
    q, s = quantize_gemm_weight(w, g, None)
    assert u8(q).tolist() == [[0x7E, 0x79, 0x00, 0xF9]] and s.item() == np.float32(1.0) / np.float32(448.0)
    through_bf16 = (w.float() * g.float()[None]).to(BF).float()
    assert u8(ops.quantize_weight_fp8(through_bf16)[0]).tolist() == [[0x7E, 0x78, 0x00, 0xF8]]


MICRO1 = LlamaConfig(vocab=512, dim=256, n_layers=1, n_heads=4, n_kv_heads=2, head_dim=64, ffn=256, max_seq=64)


@pytest.mark.parametrize("flags", ({}, {"qkv_bias": True}, {"qk_norm": True}))
def test_rows_and_scales_are_interleaved_together(flags):
    # Scale i belongs to row i of the interleaved matrix: each table row, dequantised, is the plain weight's row
    # perm[i] folded in fp32, to within that row's own quantisation step.
    cfg = replace(MICRO1, **flags)
    a = TinyLlama(cfg, device="cpu", max_batch=1, seed=5)
    for L in a.layers:  # rows of very different magnitudes, so a scale on the wrong row shows
        for n in GEMM_WEIGHTS:
            L[n] = (L[n].float() * torch.exp2(torch.arange(L[n].shape[0]) % 5)[:, None]).to(BF)
    b = TinyLlama.from_weights(cfg, dict(embed=a.embed, final_norm=a.final_norm, lm_head=a.lm_head, layers=a.layers),
                               device="cpu", max_batch=1, weight_dtype="fp8")
    assert b.lm_head is None and all(n not in L for L in b.layers for n in GEMM_WEIGHTS)
    wa, wb = a.fused_weights(), b.fused_weights()
    n = len(wa)
    assert len(wb) == n + 1 + 4 * cfg.n_layers
    L, Lq = a.layers[0], b.layers[0]
    for name, norm, k, si in (("wqkv", "attn_norm", 4, n + 1), ("wo", None, 5, n + 2), ("w_gate_up", "ffn_norm", 7, n + 3),
                              ("w_down", None, 8, n + 4)):
        perm = fused_row_perm(cfg, name, "cpu")
        assert (perm is None) == (name in ("wo", "w_down") or (name == "wqkv" and cfg.qk_norm))
        plain = L[name].float() * (L[norm].float()[None] if norm else 1.0)
        want = plain if perm is None else plain[perm]
        q, s = wb[k], wb[si]
        assert q is Lq[name + "_q"] and s is Lq[name + "_s"] and q.dtype == F8
        assert torch.equal(s, want.abs().amax(1) / 448.0)
        # half a step of e4m3 at most (16 below 448), and the fp32 rounding of the division at a tie
        assert bool(((q.float() * s[:, None] - want).abs() <= s[:, None] * 16.0 + 2.0 ** -22 * want.abs()).all())
        # the reference multiplies the same matrix, back in plain order
        assert torch.equal(b.reference_weight(name, 0), (q.float() * s[:, None])[torch.argsort(perm)]
                           if perm is not None else q.float() * s[:, None])
    for i in (0, 1, 3, 6):  # embed, norms: as they were
        assert wb[i] is wa[i] or torch.equal(wb[i], wa[i])
    assert torch.equal(wb[n], b.lm_head_s) and wb[2] is b.lm_head_q


def test_a_tied_model_keeps_its_embedding_and_gets_an_fp8_head():
    a = TinyLlama(MICRO1, device="cpu", max_batch=1, seed=1)
    tied = dict(embed=a.embed, final_norm=a.final_norm, lm_head=a.embed, layers=a.layers)
    b = TinyLlama.from_weights(MICRO1, tied, device="cpu", max_batch=1, weight_dtype="fp8")
    assert b.embed is a.embed and b.embed.dtype == BF and b.lm_head_q.shape == a.embed.shape
    sizes, plain = b.weight_bytes(), TinyLlama.from_weights(MICRO1, tied, device="cpu", max_batch=1).weight_bytes()
    assert sizes["embed"] == plain["embed"] == a.embed.numel() * 2
    n_gemm = sum(a.layers[0][n].numel() for n in GEMM_WEIGHTS)
    n_rows = sum(a.layers[0][n].shape[0] for n in GEMM_WEIGHTS)
    assert plain["gemm"] == 2 * n_gemm  # tied: the head is the embedding
    assert sizes["gemm"] == n_gemm + 4 * n_rows + a.embed.numel() + 4 * MICRO1.vocab  # + the head's FP8 copy
    assert str(sizes["total"]) in server.weights_line(b, "fp8") and "fp8" in server.weights_line(b, "fp8")


def test_the_reference_of_an_fp8_model_uses_the_dequantised_weights():
    a = TinyLlama(MICRO1, device="cpu", max_batch=1, seed=3)
    b = TinyLlama(MICRO1, device="cpu", max_batch=1, seed=3, weight_dtype="fp8")
    seq = torch.arange(5, 25)[None]
    la, lb = a.reference_logits(seq), b.reference_logits(seq)
    d = (la - lb).abs().max().item()
    assert 0 < d < 0.2 * la.abs().max().item()  # the quantisation error: reported, a separate quantity
    # ... and the same function as a bf16-free model built from q * s by hand
    hand = b.reference_hidden(seq)[:, -1] @ (b.lm_head_q.float() * b.lm_head_s[:, None]).T
    assert torch.equal(lb, hand)


# ---------------------------------------------------------------- plans and layouts
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("kv_fp8", (0, 1))
def test_fp8_weights_move_nothing_in_the_step_plan(family, kv_fp8):
    for D, H in ((64, 8), (128, 14)):
        d = dims(kv_fp8, D=D, H=H, **FAMILIES[family])
        assert (ops.weight_plan(d).w8, ops.weight_plan(d, False).w8, ops.weight_plan(d, True).w8) == (0, 0, 1)
        for B in (1, 5, 16, 17, 64):
            before = flat(ops.step_plan(d, B))
            assert ops.plan_kernels_ok(d, B) and ops.plan_kernels_ok(d, B, 0, weight_fp8=True)
            assert ops.plan_kernels_ok(d, B, 1, weight_fp8=True)
            assert flat(ops.step_plan(d, B)) == before  # a pure function: the format is no input of it
        assert flat(ops.kv_plan(d)) == {"attn_kv8": kv_fp8, "qk_norm_kv8": kv_fp8 if "qk_norm" in family else 0}


def test_every_fp8_plan_names_an_instantiated_kernel():
    # 1 to 256 k-steps on QKV and gate/up: every (nw, um) plan_gemm can give (tests/test_gpu_fused_stages.py).
    for family, flags in FAMILIES.items():
        for kv_fp8, D, dim in ((0, 64, 32), (1, 128, 64), (0, 64, 256), (1, 64, 512), (0, 128, 544), (1, 64, 1024),
                               (0, 128, 2048), (1, 128, 4096), (0, 64, 8192)):
            d = dims(kv_fp8, D=D, H=4, dim=dim, **flags)
            for B in (1, 2, 4, 5, 16, 17, 64):
                assert ops.plan_kernels_ok(d, B, 0, weight_fp8=True), (family, kv_fp8, D, dim, B)


def test_the_weight_plan_refuses_what_the_step_refuses():
    bad = dims(D=96)
    with pytest.raises(ValueError):
        ops.weight_plan(bad, True)
    with pytest.raises(ValueError):
        ops.plan_kernels_ok(bad, 1, 0, weight_fp8=True)
    with pytest.raises(ValueError):
        ops.plan_kernels_ok(dims(), 65, 0, weight_fp8=True)
    out = ops.WeightPlan()
    assert ops.lib().p2pt_llama_weight_plan(dims(), 2, out) != 0
    assert ops.lib().p2pt_llama_plan_kernels_w(dims(), 1, 0, ops.WeightPlan(w8=2)) == -1


def test_the_pinned_layouts_are_unchanged():
    names = lambda s: [n for n, _ in s._fields_]
    assert names(ops.LlamaDims) == ["vocab", "dim", "n_layers", "H", "Hkv", "D", "ffn", "max_seq", "max_batch", "eps",
                                    "theta", "kv_fp8", "rope_table", "qk_norm", "qkv_bias"]
    assert names(ops.GemmPlan) == ["epi", "nw", "tn", "um", "kpl", "grid_x", "grid_y", "ss_in", "M", "N", "K"]
    assert names(ops.AttnPlan) == ["D", "G", "slots", "stride", "grid_y"]
    assert names(ops.StepPlan) == ["rows", "emit_rows", "qkv_first", "qkv", "o", "gate_up", "down", "lm_head", "attn",
                                   "am_parts", "qk_norm_grid", "qk_norm_table"]
    assert names(ops.KvPlan) == ["attn_kv8", "qk_norm_kv8"]
    assert names(ops.WeightPlan) == ["w8"]
    # the entry points that existed keep their signatures
    lib = ops.lib()
    assert len(lib.p2pt_llama_decode.argtypes) == 14 and len(lib.p2pt_llama_plan_kernels.argtypes) == 3
    assert len(lib.p2pt_llama_decode_w.argtypes) == 15 and len(lib.p2pt_llama_plan_kernels_w.argtypes) == 4


# ---------------------------------------------------------------- the switches
def test_weight_dtype_parsing():
    assert server.arg_parser().parse_args([]).weight_dtype == "bf16"
    assert server.arg_parser().parse_args(["--weight-dtype", "fp8"]).weight_dtype == "fp8"
    with pytest.raises(SystemExit):
        server.arg_parser().parse_args(["--weight-dtype", "int4"])
    assert server.parse_weight_dtype("bf16") == "bf16" and server.parse_weight_dtype("fp8") == "fp8"
    for bad in ("int4", "e4m3", None, 8):
        with pytest.raises(ValueError, match="weight_dtype"):
            server.parse_weight_dtype(bad)
    with pytest.raises(ValueError, match="weight_dtype"):
        server.start_server(weight_dtype="int4")
    with pytest.raises(ValueError, match="weight_dtype"):
        TinyLlama(MICRO1, device="cpu", weight_dtype="int4")


def test_replicas_carry_the_switch():
    a = server.arg_parser().parse_args(["--gpus", "2", "--weight-dtype", "fp8", "--kv-dtype", "fp8", "--port", "9000"])
    for i in range(2):
        cmd = server.replica_cmd(a, i)
        assert cmd[cmd.index("--weight-dtype") + 1] == "fp8" and cmd[cmd.index("--kv-dtype") + 1] == "fp8"
        assert cmd[cmd.index("--device") + 1] == f"cuda:{i}" and "--gpus" not in cmd
    assert "--weight-dtype" not in server.replica_cmd(server.arg_parser().parse_args(["--gpus", "2"]), 0)


def test_the_eager_engine_and_the_unfused_path_refuse_fp8_weights():
    m = TinyLlama("micro", device="cpu", max_batch=2, weight_dtype="fp8")
    with pytest.raises(ValueError, match="fp8 weights need the graph-captured HIP step"):
        server.Engine(model=m)
    with pytest.raises(ValueError, match="injected model"):
        server.Engine(model=TinyLlama("micro", device="cpu", max_batch=2), weight_dtype="fp8")
    u = TinyLlama(MICRO1, device="cpu", max_batch=2, weight_dtype="fp8", fused=False)
    with pytest.raises(ValueError, match="fused step only"):
        u.decode_step(torch.tensor([1]), torch.tensor([0], dtype=torch.int32), (0, 0))
    with pytest.raises(ValueError, match="weight_dtype='fp8'"):
        TinyLlama.from_weights(MICRO1, dict(embed=m.embed, final_norm=m.final_norm, lm_head=m.embed,
                                            layers=m.layers), device="cpu")


def test_the_loader_quantises_layer_by_layer(tmp_path):
    from test_qwen2_checkpoint import qwen2_checkpoint
    from p2p_llm_tunnel_amd.models.checkpoint import load_llama
    qwen2_checkpoint(str(tmp_path), tie=True, seed=4)
    a = load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64)
    b = load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64, weight_dtype="fp8")
    assert b.weight_dtype == "fp8" and b.lm_head is None and b.embed.dtype == BF
    for La, Lb in zip(a.layers, b.layers):
        assert not set(GEMM_WEIGHTS) & set(Lb) and torch.equal(La["bqkv"], Lb["bqkv"])
        q, s = quantize_gemm_weight(La["wo"], None, None)
        assert np.array_equal(u8(q), u8(Lb["wo_q"])) and torch.equal(s, Lb["wo_s"])
    with pytest.raises(ValueError, match="weight_dtype"):
        load_llama(str(tmp_path), device="cpu", weight_dtype="int4")


# ---------------------------------------------------------------- fp32 emulation of the FP8 GEMM + epilogue
# 3 rows of a QKV-bias model, dim 256, ffn 512: O and down run in 4 K parts, QKV adds a bias in its epilogue.
EMU = Case("w8-emu", replace(_cfg(256, 512, 4, 2, 64, 64), qkv_bias=True), (5, 0, 33), seed=77)
SLIPS = ("scale_dropped", "neighbour_scale", "plain_order_scale", "scale_after_bias", "scale_after_rounding",
         "per_tensor_scale", "gate_scale_for_up", "scale_twice_under_k_parts")


@functools.lru_cache(maxsize=None)
def emu_model():
    return TinyLlama(EMU.cfg, device="cpu", max_batch=EMU.max_batch, seed=EMU.seed, weight_dtype="fp8")


def gemm8(x, q, s, rs=None, bias=None, slip=None, perm=None, kparts=1):
    """The FP8 GEMM and the head of its epilogue in NumPy fp32, in the kernel's order: the accumulator over the
    decoded bytes, times the column's scale, times 1/rms, plus the bias; the caller rounds to bf16."""
    x = x.float().numpy()
    w = ref.decode(q.view(torch.uint8).numpy())  # fp32, exact
    s = s.numpy().astype(np.float32)
    if slip == "scale_dropped":
        s = np.ones_like(s)
    elif slip == "neighbour_scale":
        s = np.roll(s, 1)
    elif slip == "plain_order_scale" and perm is not None:
        s = s[np.argsort(perm.numpy())]  # the scales in the plain weight's row order
    elif slip == "per_tensor_scale":
        s = np.full_like(s, s.max())
    elif slip == "gate_scale_for_up" and perm is not None and len(perm) == 2 * EMU.cfg.ffn:
        s = np.repeat(s[0::2], 2)
    acc = (x @ w.T).astype(np.float32)
    one = np.float32(1.0) if rs is None else rs.numpy().astype(np.float32)[:, None]
    b = np.float32(0.0) if bias is None else bias.float().numpy()[None, :]
    if slip == "scale_after_bias":
        y = (acc * one + b) * s[None, :]
    elif slip == "scale_after_rounding":
        y = torch.from_numpy(acc * one + b).to(BF).float().numpy() * s[None, :]
    else:
        y = (acc * s[None, :]) * one + b
        if slip == "scale_twice_under_k_parts" and kparts > 1:
            y = ((acc * s[None, :]) * s[None, :]) * one + b
    return torch.from_numpy(y.astype(np.float32))


def emulate_w8(slip=None):
    """One step of the one-layer FP8 model in fp32 with the kernels' bf16 stores; what ``stage_ratios`` judges."""
    case, m, inp = EMU, emu_model(), inputs(EMU)
    c, B, W = case.cfg, case.rows, emu_model().fused_weights()
    n = len(W) - 5
    H, Hkv, D, half = c.n_heads, c.n_kv_heads, c.head_dim, c.head_dim // 2
    plan = step_plan(case)
    assert plan.o.kpl == 2 and plan.down.kpl == 2 and plan.qkv.kpl == 0
    pos, sl = inp.pos.long(), torch.arange(B)
    bf32 = lambda t: t.to(BF).float()
    rs_of = lambda x: torch.rsqrt(x.float().pow(2).sum(1) / x.shape[1] + c.eps)
    x0 = W[0][inp.tokens]
    y = bf32(gemm8(x0, W[4], W[n + 1], rs_of(x0), W[9], slip, fused_row_perm(c, "wqkv", "cpu")))
    y = y.view(B, H + 2 * Hkv, half, 2)
    x1, x2 = y[:, :H + Hkv, :, 0], y[:, :H + Hkv, :, 1]
    v = torch.cat([y[:, H + Hkv:, :, 0], y[:, H + Hkv:, :, 1]], -1).to(BF)
    inv = torch.exp2(-np.log2(c.rope_theta) * 2 * torch.arange(half, dtype=torch.float32) / D)
    ang = pos.float()[:, None, None] * inv[None, None, :]
    cs, sn = torch.cos(ang), torch.sin(ang)
    qk = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1).to(BF)
    q = qk[:, :H].contiguous()
    kc, vc = inp.kc0.clone(), inp.vc0.clone()
    kc[sl, pos], vc[sl, pos] = qk[:, H:], v
    attn = _emulate_attn(case, q, kc, vc, None)
    r1 = bf32(x0.float() + bf32(gemm8(attn, W[5], W[n + 2], slip=slip, kparts=4))).to(BF)
    gu = bf32(gemm8(r1, W[7], W[n + 3], rs_of(r1), None, slip, fused_row_perm(c, "w_gate_up", "cpu"))).view(B, c.ffn, 2)
    g_, u_ = gu[..., 0], gu[..., 1]
    h = (g_ / (1 + torch.exp(-g_)) * u_).to(BF)
    r2 = bf32(r1.float() + bf32(gemm8(h, W[8], W[n + 4], slip=slip, kparts=4))).to(BF)
    logits = gemm8(r2, W[2], W[n], rs_of(r2), slip=slip).to(BF)
    return {"q": q, "kc": kc, "vc": vc, "attn": attn, "r1": r1, "h": h, "r2": r2, "logits": logits,
            "ids": first_argmax(logits)}


def emu_ratios(obs):
    W = emu_model().fused_weights()
    n = len(W) - 5
    D64 = list(W[:n])
    for j, i in enumerate((2, 4, 5, 7, 8)):
        D64[i] = W[i].to(F64) * W[n + j].to(F64)[:, None]
    stage = lambda case, W, x0, pos, layer: stage_qkv_bias(case.cfg, layer_w(case.cfg, W, layer, "wqkv"),
                                                           layer_w(case.cfg, W, layer, "bqkv"), x0, pos)
    return stage_ratios(EMU, D64, obs, qkv_stage=stage)


def test_fp32_emulation_of_the_fp8_step_stays_inside_the_fp64_bounds():
    """The bound is the stage bound of tests/test_gpu_fused_stages.py on the dequantised weights w = q * s (fp64,
    exact) plus one fp32 rounding for the scale multiply. Before any bf16 rounding the emulation, like the kernel,
    holds fl(fl(sum_k a_k q_k) * s) * rs. The sum is within (K + 12) U sum|a_k||q_k| of its exact value (``gemm_ref``
    grants K + 16 for the chain, the wave split and the K parts, which use at most K + 12); the product with s adds
    U |y| <= U sum|a_k||q_k| s: (K + 13) U sum|a_k||q_k s| in all, inside the (K + 16) U sum|a_k||w_k| the stage
    helpers apply, each element with its own sum."""
    ratios = emu_ratios(emulate_w8())
    print("EMU w8", {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("slip", SLIPS)
def test_every_scale_slip_leaves_the_bound_or_changes_an_id(slip):
    clean, ratios = emulate_w8(), emu_ratios(emulate_w8(slip))
    assert max(v for k, v in ratios.items() if k != "ids") > 1.0 or \
        not torch.equal(emulate_w8(slip)["ids"], clean["ids"]), (slip, ratios)
