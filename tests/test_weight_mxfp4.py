"""MXFP4 (OCP Microscaling FP4) GEMM weights, without a GPU (docs/WEIGHT_MXFP4.md): the quantiser against a
brute-force NumPy reference, exactness and the error bound, the byte layout, the identity of an MXFP4 model with the
bf16 model built from its dequantised weights, the plans, the weight table against the library's, an fp32 emulation
of the MXFP4 GEMM stage held to fp64 with the slips the bound must catch, and the switches.
tests/test_gpu_weight_mxfp4.py runs the kernels.
"""
import ctypes
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models import server
from p2p_llm_tunnel_amd.models.tiny_llm import (CONFIGS, GEMM_WEIGHTS, TinyLlama, fused_row_perm, llama_dims,
                                                quantize_gemm_weight)
from test_gpu_fused_stages import BF, F64, _emulate_attn, first_argmax, inputs, layer_w, stage_ratios, step_plan
from test_gpu_qwen2 import stage_qkv_bias
from test_kv_fp8 import FAMILIES, dims, flat
from test_weight_fp8 import EMU, MICRO1, gemm8
from test_weight_table import BASE, ROLES
from test_weight_table import FAMILIES as TABLE_FAMILIES

MICRO = CONFIGS["micro"]
VALUES = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6], dtype=np.float64)  # by nibble


# ---------------------------------------------------------------- the reference: brute force, one block at a time
def ref_block(x):
    """(codes [32], E) of one block of fp32 values by the rules of the format, written out independently: the scale
    from floor(log2(amax)) - 2 clamped to [2, 252]; each element the nearest of the 16 signed values to x / scale
    (exact in fp64), a tie going to the candidate with the even mantissa bit (bit 0 of the nibble), and between +0 and
    -0 to +0. Saturation is the nearest value itself: beyond 6 that is 6."""
    x = x.astype(np.float64)
    amax = np.abs(x).max()
    if amax == 0:
        return np.zeros(32, dtype=np.uint8), 127
    E = int(min(max(int(np.floor(np.log2(amax))) - 2 + 127, 2), 252))
    y = x / 2.0 ** (E - 127)
    codes = np.empty(32, dtype=np.uint8)
    for i, v in enumerate(y):
        d = np.abs(v - VALUES)
        cand = [c for c in range(16) if d[c] == d.min()]
        even = [c for c in cand if c & 1 == 0]
        codes[i] = (even or cand)[0]
    return codes, E


def ref_quantize(w):
    N, K = w.shape
    codes, E = np.empty((N, K), dtype=np.uint8), np.empty((N, K // 32), dtype=np.uint8)
    for n in range(N):
        for b in range(K // 32):
            codes[n, 32 * b:32 * b + 32], E[n, b] = ref_block(w[n, 32 * b:32 * b + 32])
    return codes, E


def quantized(w):
    packed, e = ops.quantize_weight_mxfp4(w)
    assert packed.dtype == torch.uint8 and e.dtype == torch.uint8 and packed.is_contiguous() and e.is_contiguous()
    assert packed.shape == (w.shape[0], w.shape[1] // 2) and e.shape == (w.shape[0], w.shape[1] // 32)
    return ops.unpack_weight_mxfp4(packed).numpy(), e.numpy()


def blocks(rows):
    """Hand-written blocks as an fp32 [len(rows), 32] tensor, each row zero-padded to one block."""
    out = torch.zeros(len(rows), 32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.tensor(r, dtype=torch.float32)
    return out


@functools.lru_cache(maxsize=None)
def sample():
    g = torch.Generator().manual_seed(21)
    w = torch.randn(48, 96, generator=g) * torch.exp2(torch.randint(-30, 30, (48, 3), generator=g).float()
                                                      ).repeat_interleave(32, 1)
    w[5] = 0.0
    w[6, :32] = 0.0
    w[6, 3] = -0.0
    w[7, 40:] = 0.0
    return w


def test_quantiser_matches_the_reference_on_random_blocks():
    w = sample()
    codes, E = quantized(w)
    want_codes, want_E = ref_quantize(w.numpy())
    assert np.array_equal(E, want_E) and np.array_equal(codes, want_codes)
    assert not codes[5].any() and (E[5] == 127).all() and E[6, 0] == 127 and not codes[6, :32].any()
    assert E.min() >= ops.MXFP4_EXP_MIN and E.max() <= ops.MXFP4_EXP_MAX and 8 not in set(codes.flatten().tolist())


MIDPOINTS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


def test_quantiser_on_the_edges_of_the_format():
    rows, names = [], []
    for k in (-9, 0, 5):
        s = 2.0 ** k
        rows += [[s, -s / 2, s / 3], [6 * s, -6 * s, s], [6.5 * s, -7.99 * s, 7 * s, 5.9 * s],
                 [6 * 4 * s] + [m * 4 * s for m in MIDPOINTS] + [-m * 4 * s for m in MIDPOINTS]]
        names += [f"amax 2^{k}", f"amax 6 2^{k}", f"saturating 2^{k}", f"midpoints 2^{k}"]
    rows += [[0.0] * 32, [0.0, -0.0, 0.0], [2.0 ** -130, -2.0 ** -140], [2.0 ** -124, 2.0 ** -126],
             [2.0 ** -123, -2.0 ** -125], [1.5 * 2.0 ** 127, -2.0 ** 125, 2.0 ** 120],
             [float(np.finfo(np.float32).max), 1.0]]
    names += ["zeros", "-0.0", "subnormal", "below the clamp", "at the clamp", "top binade", "fp32 max"]
    w = blocks(rows)
    codes, E = quantized(w)
    want_codes, want_E = ref_quantize(w.numpy())
    for i, name in enumerate(names):
        assert E[i, 0] == want_E[i, 0] and np.array_equal(codes[i], want_codes[i]), name
    at = lambda name: names.index(name)
    # the scale rule, by hand: amax 2^k and 6 2^k both give E - 127 = k - 2 + (0 or 2)
    assert [int(E[at(f"amax 2^{k}"), 0]) - 127 for k in (-9, 0, 5)] == [-11, -2, 3]
    assert [int(E[at(f"amax 6 2^{k}"), 0]) - 127 for k in (-9, 0, 5)] == [-9, 0, 5]
    assert codes[at("amax 2^0"), :3].tolist() == [6, 12, 3]  # 4, -2, 1.5 (1.333 rounds up)
    assert codes[at("amax 6 2^0"), :3].tolist() == [7, 15, 2]
    assert codes[at("saturating 2^0"), :4].tolist() == [7, 15, 7, 7] and E[at("saturating 2^0"), 0] == 127
    # every midpoint of both signs goes to the even mantissa: 0, 1, 1, 2, 2, 4, 4
    mid = codes[at("midpoints 2^0")]
    assert mid[0] == 7 and mid[1:8].tolist() == [0, 2, 2, 4, 4, 6, 6] and mid[8:15].tolist() == [0, 10, 10, 12, 12, 14, 14]
    # the clamps: blocks below 2^-123 stay at E = 2 and round towards zero there; the top binade is 252, never 255
    assert E[at("zeros"), 0] == 127 and E[at("-0.0"), 0] == 127 and not codes[at("-0.0")].any()
    assert E[at("subnormal"), 0] == 2 and not codes[at("subnormal")].any()
    assert E[at("below the clamp"), 0] == 2 and codes[at("below the clamp"), :2].tolist() == [4, 1]
    assert E[at("at the clamp"), 0] == 2 and codes[at("at the clamp"), :2].tolist() == [6, 10]
    assert E[at("top binade"), 0] == 252 and codes[at("top binade"), :3].tolist() == [7, 10, 0]
    assert E[at("fp32 max"), 0] == 252 and codes[at("fp32 max"), 0] == 7


def test_quantiser_refuses_what_it_cannot_represent():
    w = sample().clone()
    for bad in (float("nan"), float("inf"), float("-inf")):
        x = w.clone()
        x[3, 4] = bad
        with pytest.raises(ValueError, match="non-finite"):
            ops.quantize_weight_mxfp4(x)
    for bad in (w.to(BF), w[0], w[:, :48], w.double()):
        with pytest.raises(TypeError, match="fp32"):
            ops.quantize_weight_mxfp4(bad)
    m = TinyLlama(MICRO1, device="cpu", max_batch=1)
    m.layers[0]["wo"][2, 3] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        TinyLlama.from_weights(MICRO1, dict(embed=m.embed, final_norm=m.final_norm, lm_head=m.lm_head,
                                            layers=m.layers), device="cpu", weight_dtype="mxfp4")


def test_every_emitted_value_is_an_exact_bf16_number_within_the_bound():
    # every (nibble, E) the quantiser can emit: 16 x 251 values, decoded and sent through bf16 and back
    E = torch.arange(ops.MXFP4_EXP_MIN, ops.MXFP4_EXP_MAX + 1, dtype=torch.uint8)[:, None]
    codes = torch.arange(16, dtype=torch.uint8).repeat(2)[None, :].expand(len(E), 32).contiguous()
    deq = ops.dequantize_weight_mxfp4(ops.pack_weight_mxfp4(codes), E)
    assert deq.dtype == torch.float32 and torch.equal(deq.to(BF).float(), deq)
    want = VALUES[None, :] * np.exp2(E.numpy().astype(np.float64) - 127)
    assert np.array_equal(deq[:, :16].numpy().astype(np.float64), want)
    normal = deq[deq != 0].abs()
    assert normal.min().item() >= 2.0 ** -126 and bool(torch.isfinite(deq).all())
    # per element, the docstring's bound from the block's scale s = 2^(E - 127): a quarter, a half or one s by the
    # binade of y = |x| / s, y - 6 where the value saturates; below 2 s <= amax / 2 where the lower clamp did not bind
    w = torch.cat([sample(), blocks([[6.5, -7.99, 7.0, 5.0, 3.5, 0.1], [2.0 ** -130, 2.0 ** -127]]).repeat(1, 3)])
    packed, e = ops.quantize_weight_mxfp4(w)
    x = w.numpy().astype(np.float64)
    err = np.abs(ops.dequantize_weight_mxfp4(packed, e).numpy().astype(np.float64) - x)
    s = np.repeat(np.exp2(e.numpy().astype(np.float64) - 127), 32, 1)
    y = np.abs(x) / s
    bound = np.where(y <= 2, 0.25, np.where(y <= 4, 0.5, np.where(y <= 6, 1.0, y - 6))) * s
    amax = np.repeat(np.abs(x).reshape(x.shape[0], -1, 32).max(2), 32, 1)
    assert (err <= bound).all() and (y < 8).all() and (err <= amax / 2)[amax >= 2.0 ** -123].all()
    assert (amax < 2.0 ** -123).any() and (err <= 2.0 ** -127)[amax < 2.0 ** -123].all()
    assert (y > 6).any() and (err[y > 6] == (np.abs(x) - 6 * s)[y > 6]).all()  # the worst case is there, and exact


def test_pack_and_unpack_are_inverse_and_in_the_stated_order():
    g = torch.Generator().manual_seed(2)
    codes = torch.randint(0, 16, (7, 64), generator=g, dtype=torch.uint8)
    packed = ops.pack_weight_mxfp4(codes)
    assert packed.shape == (7, 32) and torch.equal(ops.unpack_weight_mxfp4(packed), codes)
    raw = torch.randint(0, 256, (5, 48), generator=g, dtype=torch.uint8)
    assert torch.equal(ops.pack_weight_mxfp4(ops.unpack_weight_mxfp4(raw)), raw)
    # the order WeightTable's docstring states, on a hand-written row: element 2 j in the low nibble of byte j
    row = torch.tensor([[0x1, 0x2, 0xF, 0x0, 0x7, 0x8, 0x3, 0xC]], dtype=torch.uint8)
    assert ops.pack_weight_mxfp4(row).tolist() == [[0x21, 0x0F, 0x87, 0xC3]]
    assert "low nibble" in ops.WeightTable.__doc__ and "2 j + 1" in ops.WeightTable.__doc__
    w = blocks([[1.0, -6.0, 0.5, 3.0]])
    packed, e = ops.quantize_weight_mxfp4(w)
    assert packed[0, :2].tolist() == [0xF2, 0x51] and e.tolist() == [[127]]
    assert ops.dequantize_weight_mxfp4(packed, e)[0, :4].tolist() == [1.0, -6.0, 0.5, 3.0]
    with pytest.raises(ValueError, match="0..15"):
        ops.pack_weight_mxfp4(torch.full((1, 2), 16, dtype=torch.uint8))
    with pytest.raises(TypeError):
        ops.pack_weight_mxfp4(codes.int())
    with pytest.raises(TypeError, match="scales"):
        ops.dequantize_weight_mxfp4(packed, e.float())


# ---------------------------------------------------------------- the model
def test_the_fold_happens_in_fp32_before_quantising():
    # 1.0 * 1.0 = 1 sets the block's scale to 2^-2. 0.7265625 * 0.8359375 = 0.60736 in fp32: 2.4294 in units of the
    # scale, below the tie at 2.5, so 2 (nibble 4). Were the product first rounded to bf16 the same; so take the pair
    # 0.6171875 * 1.015625 = 0.626831 (2.5073: nibble 5), which bf16 rounds to 0.625 (2.5, the tie: nibble 4).
    w = torch.tensor([[1.0, 0.6171875, 0.0, -0.6171875] + [0.0] * 28], dtype=BF)
    g = torch.tensor([1.0, 1.015625, 1.0, 1.015625] + [1.0] * 28, dtype=BF)
    packed, e = quantize_gemm_weight(w, g, None, "mxfp4")
    assert e.tolist() == [[125]] and ops.unpack_weight_mxfp4(packed)[0, :4].tolist() == [6, 5, 0, 13]
    through_bf16 = (w.float() * g.float()[None]).to(BF).float()
    assert ops.unpack_weight_mxfp4(ops.quantize_weight_mxfp4(through_bf16)[0])[0, :4].tolist() == [6, 4, 0, 12]


@pytest.mark.parametrize("flags", ({}, {"qkv_bias": True}, {"qk_norm": True}))
def test_an_mxfp4_model_is_the_bf16_model_of_its_dequantised_weights(flags):
    """Every dequantised value is a bf16 number, so a bf16 model built by hand from them (plain row order, unit norm
    weights: the fold is in the weights) with the same FP8 LM head computes the same function, bit for bit."""
    cfg = replace(MICRO, **flags)
    a = TinyLlama(cfg, device="cpu", max_batch=1, seed=4, weight_dtype="mxfp4")
    assert a.lm_head is None and a.lm_head_q.dtype == torch.float8_e4m3fn and a.lm_head_s.dtype == torch.float32
    layers = []
    for L in a.layers:
        assert not set(GEMM_WEIGHTS) & set(L)
        H = {k: v for k, v in L.items() if k[:-2] not in GEMM_WEIGHTS}
        for n in GEMM_WEIGHTS:
            assert L[n + "_q"].dtype == torch.uint8 and L[n + "_s"].dtype == torch.uint8
            deq = ops.dequantize_weight_mxfp4(L[n + "_q"], L[n + "_s"])
            perm = fused_row_perm(cfg, n, "cpu")
            deq = deq[torch.argsort(perm)] if perm is not None else deq
            H[n] = deq.to(BF)
            assert torch.equal(H[n].float(), deq) and torch.equal(a.reference_weight(n, len(layers)), deq)
        H["attn_norm"], H["ffn_norm"] = torch.ones_like(L["attn_norm"]), torch.ones_like(L["ffn_norm"])
        layers.append(H)
    head = ops.dequantize_weight_fp8(a.lm_head_q, a.lm_head_s)
    b = TinyLlama.from_weights(cfg, dict(embed=a.embed, final_norm=torch.ones_like(a.final_norm), lm_head=a.embed,
                                         layers=layers), device="cpu", max_batch=1)
    seq = torch.arange(7, 31)[None]
    hb = b.reference_hidden(seq)
    assert torch.equal(a.reference_hidden(seq), hb)
    assert torch.equal(a.reference_logits(seq), hb[:, -1] @ head.T)
    # the quantisation error against the original model: there, and a separate quantity
    d = (TinyLlama(cfg, device="cpu", max_batch=1, seed=4).reference_logits(seq) - a.reference_logits(seq)).abs().max()
    assert d.item() > 0


def test_weight_bytes_and_the_tied_head():
    a = TinyLlama(MICRO1, device="cpu", max_batch=1, seed=1)
    tied = dict(embed=a.embed, final_norm=a.final_norm, lm_head=a.embed, layers=a.layers)
    b = TinyLlama.from_weights(MICRO1, tied, device="cpu", max_batch=1, weight_dtype="mxfp4")
    assert b.embed is a.embed and b.embed.dtype == BF and b.lm_head_q.shape == a.embed.shape
    n_gemm = sum(a.layers[0][n].numel() for n in GEMM_WEIGHTS)
    sizes = b.weight_bytes()
    assert sizes["embed"] == a.embed.numel() * 2
    assert sizes["gemm"] == n_gemm // 2 + n_gemm // 32 + a.embed.numel() + 4 * MICRO1.vocab  # + the head's FP8 copy
    line = server.weights_line(b, "mxfp4")
    assert str(sizes["total"]) in line and "mxfp4 GEMM weights" in line
    with pytest.raises(ValueError, match="weight_dtype='mxfp4'"):
        TinyLlama.from_weights(MICRO1, dict(embed=b.embed, final_norm=b.final_norm, lm_head=b.embed, layers=b.layers),
                               device="cpu", weight_dtype="fp8")


# ---------------------------------------------------------------- plans
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("kv_fp8", (0, 1))
def test_the_format_moves_nothing_in_the_step_plan(family, kv_fp8):
    for D, H in ((64, 8), (128, 14)):
        d = dims(kv_fp8, D=D, H=H, **FAMILIES[family])
        for name, pair in ops.WEIGHT_FORMATS.items():
            f = ops.weight_plan(d, weight_format=name)
            assert (f.layers, f.lm_head) == pair == (ops.as_weight_format(weight_format=name).layers,
                                                     ops.as_weight_format(weight_format=name).lm_head)
        assert ops.weight_plan(d, True).w8 == 1  # the old question keeps its answer
        for B in (1, 5, 16, 17, 64):
            before = flat(ops.step_plan(d, B))
            assert ops.plan_kernels_ok(d, B, weight_format="mxfp4") and ops.plan_kernels_ok(d, B, 1, weight_format="mxfp4")
            assert ops.plan_kernels_ok(d, B, weight_format="fp8") == ops.plan_kernels_ok(d, B, weight_fp8=True)
            assert ops.plan_kernels_ok(d, B, weight_format="bf16") == ops.plan_kernels_ok(d, B)
            assert flat(ops.step_plan(d, B)) == before  # a pure function: the format is no input of it


def test_every_mxfp4_plan_names_an_instantiated_kernel():
    # tests/test_weight_fp8.py's dims: 1 to 256 k-steps on QKV and gate/up, every (nw, um) plan_gemm can give
    for family, flags in FAMILIES.items():
        for kv_fp8, D, dim in ((0, 64, 32), (1, 128, 64), (0, 64, 256), (1, 64, 512), (0, 128, 544), (1, 64, 1024),
                               (0, 128, 2048), (1, 128, 4096), (0, 64, 8192)):
            d = dims(kv_fp8, D=D, H=4, dim=dim, **flags)
            for B in (1, 2, 4, 5, 16, 17, 64):
                assert ops.plan_kernels_ok(d, B, 0, weight_format="mxfp4"), (family, kv_fp8, D, dim, B)
                assert ops.plan_kernels_ok(d, B, 0, weight_format="mxfp4", windows=(3,) * d.n_layers)


def test_bad_formats_are_refused_and_the_old_entry_points_still_refuse_w8_2():
    lib, d = ops.lib(), dims()
    for bad in ("int4", "e2m1", 4, ops.WeightFormat(2, 2), ops.WeightFormat(2, 0), ops.WeightFormat(0, 1),
                ops.WeightFormat(1, 0), ops.WeightFormat(3, 1), ops.WeightFormat(-1, -1)):
        with pytest.raises(ValueError, match="weight_format"):
            ops.as_weight_format(weight_format=bad)
        with pytest.raises(ValueError, match="weight_format"):
            ops.plan_kernels_ok(d, 1, weight_format=bad)
        with pytest.raises(ValueError, match="weight_format"):
            ops.WeightTable(d, weight_format=bad)
    with pytest.raises(ValueError, match="not both"):
        ops.WeightTable(d, True, "mxfp4")
    out, n = ops.WeightFormat(), len(ROLES) * d.n_layers
    at, sc = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    for layers, head in ((2, 2), (2, 0), (0, 1), (1, 0), (3, 1), (-1, 0)):
        f = ops.WeightFormat(layers, head)
        assert lib.p2pt_llama_weight_format(d, layers, head, out) != 0
        assert lib.p2pt_llama_plan_kernels_fmt(d, 1, 0, f, None) == -1
        assert lib.p2pt_llama_weight_layout_fmt(d, f, at, sc, n) == -1
    for bad in (dims(D=96),):
        with pytest.raises(ValueError):
            ops.weight_plan(bad, weight_format="mxfp4")
        with pytest.raises(ValueError):
            ops.plan_kernels_ok(bad, 1, weight_format="mxfp4")
    with pytest.raises(ValueError):
        ops.plan_kernels_ok(d, 65, weight_format="mxfp4")
    # WeightPlan keeps its one field and its refusal of 2 at every entry point that takes it
    wp = ops.WeightPlan(w8=2)
    assert [n for n, _ in ops.WeightPlan._fields_] == ["w8"]
    assert lib.p2pt_llama_weight_plan(d, 2, ops.WeightPlan()) != 0
    assert lib.p2pt_llama_plan_kernels_w(d, 1, 0, wp) == -1 and lib.p2pt_llama_plan_kernels_win(d, 1, 0, wp, None) == -1
    assert lib.p2pt_llama_weight_layout(d, wp, at, sc, n) == -1
    assert len(lib.p2pt_llama_decode_win.argtypes) == len(lib.p2pt_llama_decode_fmt.argtypes) == 17


# ---------------------------------------------------------------- the weight table
@pytest.mark.parametrize("n_layers", (1, 3))
@pytest.mark.parametrize("family", sorted(TABLE_FAMILIES))
def test_python_and_the_library_agree_on_every_index_of_an_mxfp4_table(family, n_layers):
    lib = ops.lib()
    d = llama_dims(replace(BASE, n_layers=n_layers, **TABLE_FAMILIES[family]), 2)
    layout = ops.WeightTable(d, weight_format="mxfp4")
    n = len(ROLES) * n_layers
    at, sc = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    size = lib.p2pt_llama_weight_layout_fmt(ctypes.byref(d), ctypes.byref(ops.WeightFormat(2, 1)), at, sc, n)
    key = lambda j: (ROLES[j % len(ROLES)], None if j % len(ROLES) < 4 else j // len(ROLES))
    theirs = {key(j): at[j] for j in range(n) if at[j] >= 0}
    theirs_sc = {key(j): sc[j] for j in range(n) if sc[j] >= 0}
    ours = {(e.name, e.layer): i for i, e in enumerate(layout) if not e.name.endswith(" scale")}
    ours_sc = {(e.name[:-len(" scale")], e.layer): i for i, e in enumerate(layout) if e.name.endswith(" scale")}
    assert size == len(layout) and theirs == ours and theirs_sc == ours_sc
    assert sorted(list(theirs.values()) + list(theirs_sc.values())) == list(range(size))
    # the same places as an FP8 table; what sits there differs for a layer's GEMMs alone
    fp8 = ops.WeightTable(d, True)
    assert [(e.name, e.layer) for e in fp8] == [(e.name, e.layer) for e in layout]
    for e, f in zip(layout, fp8):
        base = e.name[:-len(" scale")] if e.name.endswith(" scale") else e.name
        if base in GEMM_WEIGHTS:
            N, K = fp8[fp8.index(base, e.layer)].shape
            want = ((torch.uint8,), (N, K // 32), 1) if e.name.endswith(" scale") else ((torch.uint8,), (N, K // 2), 4)
            assert (e.dtypes, e.shape, e.align) == want
        else:
            assert e == f
    # and a model's table is what the layout says
    m = TinyLlama(replace(BASE, n_layers=n_layers, **TABLE_FAMILIES[family]), device="cpu", max_batch=1,
                  weight_dtype="mxfp4")
    for e, t in zip(layout, m.fused_weights()):
        assert t.dtype in e.dtypes and tuple(t.shape) == e.shape, e


def test_a_bad_mxfp4_entry_is_refused_by_name():
    m = TinyLlama(replace(BASE, n_layers=2), device="cpu", max_batch=1, weight_dtype="mxfp4")
    table, T = m.fused_weights(), ops.WeightTable(m.dims(), weight_format="mxfp4")
    build = lambda t: ops.FusedLlamaDecoder(m.dims(), t, m.k_cache, m.v_cache, weight_format="mxfp4")
    swap = lambda i, t: table[:i] + [t] + table[i + 1:]
    wq, sq = T.index("w_down", 1), T.scale_index("w_down", 1)
    with pytest.raises(ValueError, match="HIP device"):  # a valid table passes every host check
        build(table)
    with pytest.raises(ValueError, match="^layer 1: w_down has shape .*two nibbles per byte"):
        build(swap(wq, table[wq].repeat(1, 2)))
    with pytest.raises(ValueError, match="^layer 1: w_down scale has shape .*one e8m0 byte per 32-element block"):
        build(swap(sq, table[sq].repeat(1, 2)))
    with pytest.raises(TypeError, match="^layer 1: w_down: the weight format is mxfp4.*nibble bytes.*bfloat16"):
        build(swap(wq, table[wq].to(BF)))
    with pytest.raises(TypeError, match="^layer 1: w_down scale: the weight format is mxfp4.*e8m0 bytes.*float32"):
        build(swap(sq, table[sq].float()))
    raw = torch.zeros(table[wq].numel() + 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="^layer 1: w_down must be 4-byte aligned"):
        build(swap(wq, raw[2:2 + table[wq].numel()].view(table[wq].shape)))
    with pytest.raises(ValueError, match="weight table"):
        build(table[:-1])
    with pytest.raises(ValueError, match="weight table"):
        build(TinyLlama(replace(BASE, n_layers=2), device="cpu", max_batch=1).fused_weights())


# ---------------------------------------------------------------- fp32 emulation of the MXFP4 GEMM stage
SLIPS = ("nibble_order_swapped", "neighbour_block_scale", "one_scale_per_row", "exponent_bias_off_by_one",
         "sign_bit_dropped", "scale_offset_ignores_the_k_part")


@functools.lru_cache(maxsize=None)
def emu_model():
    return TinyLlama(EMU.cfg, device="cpu", max_batch=EMU.max_batch, seed=EMU.seed, weight_dtype="mxfp4")


def gemm4(x, packed, e, rs=None, bias=None, slip=None, kparts=1):
    """The MXFP4 GEMM and the head of its epilogue in NumPy fp32, in the kernel's order: each byte's two nibbles and
    the byte at ``n K / 32 + part * (K / parts) / 32 + s`` decoded to nibble * 2^(E - 127), the accumulator over that,
    times 1/rms, plus the bias; the caller rounds to bf16. No row scale anywhere."""
    x = x.float().numpy()
    b, E = packed.numpy(), e.numpy().astype(np.int32)
    lo, hi = b & 15, b >> 4
    if slip == "nibble_order_swapped":
        lo, hi = hi, lo
    codes = np.stack([lo, hi], 2).reshape(b.shape[0], -1)
    if slip == "sign_bit_dropped":
        codes = codes & 7
    nb = E.shape[1]
    if slip == "neighbour_block_scale":
        E = np.roll(E, 1, 1)
    elif slip == "one_scale_per_row":
        E = np.repeat(E[:, :1], nb, 1)
    elif slip == "scale_offset_ignores_the_k_part" and kparts > 1:
        E = np.tile(E[:, :nb // kparts], (1, kparts))  # every part reads part 0's blocks
    bias_e = 126 if slip == "exponent_bias_off_by_one" else 127
    w = (VALUES[codes] * np.exp2(np.repeat(E, 32, 1).astype(np.float64) - bias_e)).astype(np.float32)  # exact
    acc = (x @ w.T).astype(np.float32)
    one = np.float32(1.0) if rs is None else rs.numpy().astype(np.float32)[:, None]
    bb = np.float32(0.0) if bias is None else bias.float().numpy()[None, :]
    return torch.from_numpy((acc * one + bb).astype(np.float32))


def emulate_mx(slip=None):
    """One step of the one-layer MXFP4 model in fp32 with the kernels' bf16 stores; what ``stage_ratios`` judges.
    tests/test_weight_fp8.py's ``emulate_w8`` with the four layer GEMMs through ``gemm4``; the LM head is its FP8 one."""
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
    y = bf32(gemm4(x0, W[4], W[n + 1], rs_of(x0), W[9], slip)).view(B, H + 2 * Hkv, half, 2)
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
    r1 = bf32(x0.float() + bf32(gemm4(attn, W[5], W[n + 2], slip=slip, kparts=4))).to(BF)
    gu = bf32(gemm4(r1, W[7], W[n + 3], rs_of(r1), None, slip)).view(B, c.ffn, 2)
    g_, u_ = gu[..., 0], gu[..., 1]
    h = (g_ / (1 + torch.exp(-g_)) * u_).to(BF)
    r2 = bf32(r1.float() + bf32(gemm4(h, W[8], W[n + 4], slip=slip, kparts=4))).to(BF)
    logits = gemm8(r2, W[2], W[n], rs_of(r2)).to(BF)
    return {"q": q, "kc": kc, "vc": vc, "attn": attn, "r1": r1, "h": h, "r2": r2, "logits": logits,
            "ids": first_argmax(logits)}


def emu_ratios(obs):
    W = emu_model().fused_weights()
    n = len(W) - 5
    D64 = list(W[:n])
    D64[2] = W[2].to(F64) * W[n].to(F64)[:, None]
    for j, i in enumerate((4, 5, 7, 8)):
        D64[i] = ops.dequantize_weight_mxfp4(W[i], W[n + 1 + j]).to(F64)
    stage = lambda case, W, x0, pos, layer: stage_qkv_bias(case.cfg, layer_w(case.cfg, W, layer, "wqkv"),
                                                           layer_w(case.cfg, W, layer, "bqkv"), x0, pos)
    return stage_ratios(EMU, D64, obs, qkv_stage=stage)


def test_fp32_emulation_of_the_mxfp4_step_stays_inside_the_fp64_bounds():
    """The bound is the stage bound of tests/test_gpu_fused_stages.py as it stands, on the dequantised weights (fp64,
    exact). The decoded fragment is the dequantised weight itself, an exact bf16 number, and there is no scale
    multiply after the sum: what the emulation and the kernel hold before any bf16 rounding is the bf16 kernel's
    fl(sum_k a_k w_k) * rs, which ``gemm_ref`` bounds with (K + 16) U sum|a_k||w_k|, each element with its own sum."""
    ratios = emu_ratios(emulate_mx())
    print("EMU mxfp4", {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("slip", SLIPS)
def test_every_decode_slip_leaves_the_bound(slip):
    ratios = emu_ratios(emulate_mx(slip))
    assert max(v for k, v in ratios.items() if k != "ids") > 1.0, (slip, ratios)


# ---------------------------------------------------------------- the switches
def test_weight_dtype_parsing():
    assert server.arg_parser().parse_args(["--weight-dtype", "mxfp4"]).weight_dtype == "mxfp4"
    assert server.parse_weight_dtype("mxfp4") == "mxfp4"
    with pytest.raises(SystemExit):
        server.arg_parser().parse_args(["--weight-dtype", "int4"])
    for bad in ("int4", "fp4", "MXFP4", None):
        with pytest.raises(ValueError, match="weight_dtype"):
            server.parse_weight_dtype(bad)
    with pytest.raises(ValueError, match="weight_dtype"):
        server.start_server(weight_dtype="mxfp8")
    a = server.arg_parser().parse_args(["--gpus", "2", "--weight-dtype", "mxfp4", "--kv-dtype", "fp8", "--port", "9000"])
    for i in range(2):
        cmd = server.replica_cmd(a, i)
        assert cmd[cmd.index("--weight-dtype") + 1] == "mxfp4" and cmd[cmd.index("--kv-dtype") + 1] == "fp8"
        assert cmd[cmd.index("--device") + 1] == f"cuda:{i}" and "--gpus" not in cmd


def test_the_eager_engine_and_the_unfused_path_refuse_mxfp4_weights():
    m = TinyLlama("micro", device="cpu", max_batch=2, weight_dtype="mxfp4")
    with pytest.raises(ValueError, match="mxfp4 weights need the graph-captured HIP step"):
        server.Engine(model=m)
    with pytest.raises(ValueError, match="injected model"):
        server.Engine(model=TinyLlama("micro", device="cpu", max_batch=2), weight_dtype="mxfp4")
    with pytest.raises(ValueError, match="injected engine's model"):
        server.start_server(weight_dtype="mxfp4", engine=server.Engine(model=TinyLlama("micro", device="cpu", max_batch=2)))
    u = TinyLlama(MICRO1, device="cpu", max_batch=2, weight_dtype="mxfp4", fused=False)
    with pytest.raises(ValueError, match="mxfp4 weights run the fused step only"):
        u.decode_step(torch.tensor([1]), torch.tensor([0], dtype=torch.int32), (0, 0))
    with pytest.raises(ValueError, match="weight_dtype='mxfp4'"):
        TinyLlama.from_weights(MICRO1, dict(embed=m.embed, final_norm=m.final_norm, lm_head=m.embed,
                                            layers=m.layers), device="cpu")


def test_the_loader_quantises_layer_by_layer(tmp_path):
    from test_qwen2_checkpoint import qwen2_checkpoint
    from p2p_llm_tunnel_amd.models.checkpoint import load_llama
    qwen2_checkpoint(str(tmp_path), tie=True, seed=4)
    a = load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64)
    b = load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64, weight_dtype="mxfp4")
    assert b.weight_dtype == "mxfp4" and b.lm_head is None and b.embed.dtype == BF
    q8, s8 = quantize_gemm_weight(a.lm_head, a.final_norm, None)
    assert torch.equal(b.lm_head_q.view(torch.uint8), q8.view(torch.uint8)) and torch.equal(b.lm_head_s, s8)
    for La, Lb in zip(a.layers, b.layers):
        assert not set(GEMM_WEIGHTS) & set(Lb) and torch.equal(La["bqkv"], Lb["bqkv"])
        for name, norm in (("wo", None), ("wqkv", "attn_norm")):
            q, s = quantize_gemm_weight(La[name], La[norm] if norm else None, fused_row_perm(b.cfg, name, "cpu"), "mxfp4")
            assert torch.equal(q, Lb[name + "_q"]) and torch.equal(s, Lb[name + "_s"]) and s.dtype == torch.uint8
    assert b.weight_bytes()["gemm"] < a.weight_bytes()["gemm"]
