"""llama3 and linear RoPE scaling (models/rope.py; Llama 3.1 / 3.2 / 3.3 checkpoints) without a GPU: the frequency
table against transformers' own functions, the loader against transformers' ``LlamaForCausalLM`` on synthetic
checkpoints written here, the refusals, what the fused step plans for a scaled model, and an fp32 NumPy emulation
of the table epilogue (``k_skinny<.., EPI_ROPE_TAB, ..>``, decode_fused_kernels.h) held to the fp64 bound that
tests/test_gpu_llama3_rope.py uses on the device, with nine one-line slips that each leave it.

The bound of the rotation (``rotation``, shared with the GPU tests). The table entry f = inv_freq[i] is an exact
fp32 input, and so is the position p (an int below 2^24). With U = 2^-24 and ulp(y) the bf16 spacing at |y|:

* the angle a = fl(p * f) rounds once: off by |p f| U;
* sincosf is good to 2 ulp of a value <= 1 (ops/build.py compiles without fast-math); 4 U covers cos and sin
  each, as in test_gpu_fused_stages.rope_tables. Each of cos and sin is off by dsc = |p f| U + 4 U (their
  derivatives are at most 1);
* the rotation x1 cos - x2 sin is two products and one add (or an fma and a product): 3 U (|x1 cos| + |x2 sin|);
* inputs that were rounded to bf16 from a value with error bound E (the GEMM, on the device) can land on the
  other neighbour within E of a tie: flip(x1) |cos| + flip(x2) |sin| (test_gpu_fused_stages.flip); exact
  inputs, as here on the CPU, have flip = 0;
* the one bf16 store: half an ulp, taken at |o| + E.

Nothing is scaled by a maximum over a row or the tensor. Unlike the inline path there is no exp2f / log2f term:
with the table the angle error is one rounding. Inputs for which the unslipped emulation is held to the bound
here: x bf16 N(0, 1.5) and a few values scaled by 2^20 and 2^-20, positions 0, 1, seams of the table's bands and
the cache's last row, up to 131071 (Llama 3's max_position_embeddings - 1), D = 64 and 128, Llama 3.1 and 3.2
parameters at theta 500000.
"""
import ctypes
import functools
import json
import math
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models import rope
from p2p_llm_tunnel_amd.models.checkpoint import load_llama, read_config
from p2p_llm_tunnel_amd.models.rope import RopeScaling
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, LlamaConfig, TinyLlama
from test_checkpoint import MICRO, _hf_logits
from test_gpu_fused_stages import F64, U, rounded

BF = torch.bfloat16
EPI_STORE, EPI_ROPE, EPI_ROPE_BIAS, EPI_ROPE_TAB, EPI_ROPE_BIAS_TAB = 0, 1, 5, 6, 7

L31 = RopeScaling("llama3", 8.0, 1.0, 4.0, 8192)  # Llama 3.1 (and 3.3, R1-Distill-Llama)
L32 = RopeScaling("llama3", 32.0, 1.0, 4.0, 8192)  # Llama 3.2
SHORT = RopeScaling("llama3", 8.0, 1.0, 4.0, 64)  # most frequencies scaled inside short sequences
LINEAR4 = RopeScaling("linear", 4.0)
THETA3 = 500000.0


def hf_dict(s: RopeScaling, spelling="rope_type"):
    d = {spelling: s.kind, "factor": s.factor}
    if s.kind == "llama3":
        d.update(low_freq_factor=s.low_freq_factor, high_freq_factor=s.high_freq_factor,
                 original_max_position_embeddings=s.original_max_seq)
    return d


# ---------------------------------------------------------------- the table
def bands(theta, head_dim, s):
    """Indices i of the kept, the interpolated and the divided frequencies of a ``llama3`` table, from the rule's
    own two comparisons on the unscaled wavelengths (spelled out here, not taken from models/rope.py)."""
    base = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    wavelen = 2 * math.pi / base
    hi = wavelen < s.original_max_seq / s.high_freq_factor
    lo = wavelen > s.original_max_seq / s.low_freq_factor
    idx = range(head_dim // 2)
    return ([i for i in idx if hi[i]], [i for i in idx if not hi[i] and not lo[i]], [i for i in idx if lo[i]])


def _hf_table(s, theta, D):
    transformers = pytest.importorskip("transformers")
    from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
    cfg = transformers.LlamaConfig(hidden_size=4 * D, num_attention_heads=4, head_dim=D,
                                   max_position_embeddings=131072,
                                   rope_parameters=dict(hf_dict(s), rope_theta=theta))
    inv, attention_factor = ROPE_INIT_FUNCTIONS[s.kind](cfg, "cpu")
    assert attention_factor == 1.0  # so the kernels take no cos / sin scale
    return inv


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("s", [L31, L32, LINEAR4, SHORT], ids=["llama3.1", "llama3.2", "linear4", "short"])
def test_table_is_transformers_own(s, D):
    """Bit for bit (no ulp allowance was needed: models/rope.py orders every operation as transformers does)."""
    ours = rope.inv_freq(THETA3, D, s)
    assert ours.dtype == torch.float32 and ours.shape == (D // 2,) and ours.is_contiguous()
    assert torch.equal(ours, _hf_table(s, THETA3, D))
    assert bool((torch.isfinite(ours) & (ours > 0)).all())
    base = 1.0 / (THETA3 ** (torch.arange(0, D, 2).float() / D))
    if s.kind == "linear":
        assert torch.equal(ours, base / 4.0)
        return
    keep, smooth, div = bands(THETA3, D, s)
    assert keep and smooth and div and keep + smooth + div == list(range(D // 2))  # three non-empty bands, in order
    assert torch.equal(ours[keep], base[keep]) and torch.equal(ours[div], base[div] / s.factor)
    for i in smooth:  # strictly between kept and divided, or at an end of the band
        assert float(base[i]) / s.factor <= float(ours[i]) <= float(base[i])
    if D == 64 and s is not SHORT:
        assert smooth == [15, 16, 17] and div[0] == 18


# ---------------------------------------------------------------- parity with transformers
def scaled_checkpoint(path, s, tie=False, seed=0, spelling="rope_parameters"):
    """test_checkpoint._hf_checkpoint with ``rope_parameters`` of ``s``: transformers' Llama, random weights rounded
    to bf16, max_position_embeddings 512. ``spelling``: how config.json carries the scaling afterwards:
    "rope_parameters" as transformers 5 saves it, or "rope_scaling" / "type": rewritten by hand to the transformers 4
    layout (rope_theta at the top level, a rope_scaling dict with the rope_type or the legacy type key)."""
    transformers = pytest.importorskip("transformers")
    micro = {k: v for k, v in MICRO.items() if k != "rope_theta"}
    cfg = transformers.LlamaConfig(**micro, tie_word_embeddings=tie,
                                   rope_parameters=dict(hf_dict(s), rope_theta=MICRO["rope_theta"]))
    torch.manual_seed(seed)
    m = transformers.LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in m.parameters():
            p.normal_(0, 0.05) if p.dim() > 1 else p.uniform_(0.8, 1.2)
            p.copy_(p.to(torch.bfloat16).float())
    m.save_pretrained(path, safe_serialization=True)
    f = f"{path}/config.json"
    with open(f) as fh:
        raw = json.load(fh)
    assert raw["rope_parameters"]["rope_type"] == s.kind
    if spelling != "rope_parameters":
        raw.pop("rope_parameters")
        raw["rope_theta"] = MICRO["rope_theta"]
        raw["rope_scaling"] = hf_dict(s, "rope_type" if spelling == "rope_scaling" else "type")
        with open(f, "w") as fh:
            json.dump(raw, fh)
    return m


@pytest.mark.parametrize("s,tie,spelling", [(SHORT, False, "rope_scaling"), (SHORT, True, "rope_scaling"),
                                            (SHORT, False, "rope_parameters"), (SHORT, True, "type"),
                                            (LINEAR4, False, "rope_scaling"), (LINEAR4, True, "rope_parameters")],
                         ids=lambda v: v.kind if isinstance(v, RopeScaling) else str(v))
def test_loader_matches_transformers_with_scaling(tmp_path, s, tie, spelling):
    m = scaled_checkpoint(str(tmp_path), s, tie=tie, spelling=spelling)
    ours = load_llama(str(tmp_path), device="cpu", max_batch=2)
    c = ours.cfg
    assert c.rope_scaling == s and c.max_seq == 512 and c.rope_theta == 10000.0 and hash(c) is not None
    assert (ours.lm_head is ours.embed) == tie
    torch.manual_seed(3)
    seqs = torch.randint(0, c.vocab, (2, 29))
    ref = ours.reference_logits(seqs)
    hf = _hf_logits(m, seqs)
    scale = hf.abs().max().item()
    # the tolerance of test_checkpoint.test_loader_matches_transformers_llama
    assert (ref - hf).abs().max().item() < 0.03 * scale
    assert torch.nn.functional.cosine_similarity(ref, hf, dim=-1).min().item() > 0.999
    # ... which the scaling decides: the same weights with default RoPE are another model
    plain = TinyLlama.from_weights(replace(c, rope_scaling=None), dict(
        embed=ours.embed, final_norm=ours.final_norm, lm_head=ours.lm_head, layers=ours.layers), device="cpu",
        max_batch=2)
    assert (plain.reference_logits(seqs) - hf).abs().max().item() > 0.03 * scale
    # the fused weight table carries the frequency table as a fourth global entry
    table = ours.fused_weights()
    assert len(table) == 4 + 6 * c.n_layers and table[3].dtype == torch.float32
    assert torch.equal(table[3], rope.inv_freq(c.rope_theta, c.head_dim, s))
    assert len(plain.fused_weights()) == 3 + 6 * c.n_layers and plain.rope_inv_freq() is None


# ---------------------------------------------------------------- refusals
CONF = {"architectures": ["LlamaForCausalLM"], "vocab_size": 512, "hidden_size": 256, "intermediate_size": 512,
        "num_hidden_layers": 2, "num_attention_heads": 4, "num_key_value_heads": 2,
        "max_position_embeddings": 131072, "rms_norm_eps": 1e-5, "rope_theta": THETA3}


def _read(tmp_path, **conf):
    (tmp_path / "config.json").write_text(json.dumps(dict(CONF, **conf)))
    return read_config(str(tmp_path), max_seq=256)[0]


def test_config_parsing_and_refusals(tmp_path):
    full = hf_dict(L32)
    assert _read(tmp_path, rope_scaling=full).rope_scaling == L32
    assert _read(tmp_path, rope_scaling=hf_dict(L31, "type")).rope_scaling == L31
    assert _read(tmp_path, rope_scaling=hf_dict(LINEAR4)).rope_scaling == LINEAR4
    assert _read(tmp_path).rope_scaling is None
    assert _read(tmp_path, rope_scaling={"rope_type": "default"}).rope_scaling is None
    c = _read(tmp_path, rope_parameters=dict(full, rope_theta=12345.0))
    assert c.rope_scaling == L32 and c.rope_theta == 12345.0 and c.max_seq == 256
    # every missing key, by name; nothing is defaulted
    for k in ("factor", "low_freq_factor", "high_freq_factor", "original_max_position_embeddings"):
        with pytest.raises(ValueError, match=f"rope.*{k}"):
            _read(tmp_path, rope_scaling={a: b for a, b in full.items() if a != k})
    with pytest.raises(ValueError, match="rope.*factor"):
        _read(tmp_path, rope_scaling={"rope_type": "linear"})
    # the range rules
    for bad, msg in ((dict(factor=0.5), "factor"), (dict(factor=float("inf")), "factor"),
                     (dict(low_freq_factor=4.0), "low_freq_factor"), (dict(low_freq_factor=5.0), "low_freq_factor"),
                     (dict(original_max_position_embeddings=0), "original_max_position_embeddings"),
                     (dict(original_max_position_embeddings=-8192), "original_max_position_embeddings"),
                     (dict(original_max_position_embeddings=float("inf")), "original_max_position_embeddings"),
                     (dict(original_max_position_embeddings=8192.5), "original_max_position_embeddings"),
                     (dict(factor=float("nan")), "factor"),
                     (dict(factor="8"), "factor")):
        with pytest.raises(ValueError, match=f"rope.*{msg}"):
            _read(tmp_path, rope_scaling=dict(full, **bad))
    with pytest.raises(ValueError, match="rope.*factor"):
        _read(tmp_path, rope_scaling={"rope_type": "linear", "factor": 0.25})
    # every other type stays refused, with today's message
    for kind in ("yarn", "dynamic", "longrope", "proportional", "su"):
        for spelling in ("rope_type", "type"):
            with pytest.raises(ValueError, match=f"rope type '{kind}' is not supported by the decode kernels"):
                _read(tmp_path, rope_scaling={spelling: kind, "factor": 4.0})
    with pytest.raises(ValueError, match="yarn"):
        RopeScaling("yarn", 4.0)
    # bias and QK-norm families take the scaling too
    q2 = _read(tmp_path, architectures=["Qwen2ForCausalLM"], rope_scaling=full)
    q3 = _read(tmp_path, architectures=["Qwen3ForCausalLM"], head_dim=128, rope_scaling=hf_dict(LINEAR4))
    assert q2.qkv_bias and q2.rope_scaling == L32 and q3.qk_norm and q3.rope_scaling == LINEAR4
    for c in (q2, q3):
        c = replace(c, max_seq=16)
        m = TinyLlama(c, device="cpu", max_batch=1, seed=0)
        per = 8 if c.qk_norm else 7
        assert len(m.fused_weights()) == 4 + per * c.n_layers
        seqs = torch.randint(0, c.vocab, (1, 9))
        plain = TinyLlama(replace(c, rope_scaling=None), device="cpu", max_batch=1, seed=0)
        assert not torch.equal(m.reference_logits(seqs), plain.reference_logits(seqs))
    assert all(c.rope_scaling is None for c in CONFIGS.values()) and LlamaConfig().rope_scaling is None


# ---------------------------------------------------------------- planning (the library, no device)
def _lib_or_skip():
    """The HIP library; a skip only where there is neither a built library nor a compiler to build one with. A
    build that fails, or a library that does not load, fails the test."""
    from p2p_llm_tunnel_amd.ops import build as ops_build
    if not os.path.exists(ops_build.OUT):
        try:
            ops_build.hipcc()
        except FileNotFoundError as e:
            pytest.skip(f"no built HIP library and no compiler on this host: {e}")
    return ops.lib()


SHAPES = {  # Llama-3.2-1B; micro; a Qwen2-shaped and a Qwen3-shaped model
    "llama-3.2-1b": dict(vocab=128256, dim=2048, n_layers=16, H=32, Hkv=8, D=64, ffn=8192, max_seq=4096, max_batch=17,
                         eps=1e-5, theta=5e5),
    "micro": dict(vocab=4096, dim=256, n_layers=2, H=4, Hkv=2, D=64, ffn=512, max_seq=512, max_batch=5, eps=1e-5,
                  theta=1e4),
    "bias": dict(vocab=512, dim=256, n_layers=1, H=14, Hkv=2, D=64, ffn=256, max_seq=96, max_batch=5, eps=1e-6,
                 theta=1e6, qkv_bias=1),
    "qk-norm": dict(vocab=512, dim=256, n_layers=1, H=4, Hkv=2, D=128, ffn=256, max_seq=96, max_batch=5, eps=1e-6,
                    theta=1e6, qk_norm=1),
}
# What the commit before the table planned for the unscaled shapes (rows, emit_rows, six GemmPlans of 11 ints,
# the AttnPlan, am_parts, qk_norm_grid), recorded from its library.
PARENT_PLANS = {
    ("llama-3.2-1b", 1): [1, 1, 1, 8, 1, 4, 0, 192, 1, 1, 1, 3072, 2048, 1, 8, 1, 4, 0, 192, 1, 256, 1, 3072, 2048, 3, 8,
                          1, 4, 1, 256, 1, 0, 1, 2048, 2048, 2, 8, 1, 4, 0, 1024, 1, 256, 1, 16384, 2048, 3, 8, 1, 4, 1,
                          256, 1, 0, 1, 2048, 8192, 4, 4, 2, 4, 0, 4008, 1, 256, 1, 128256, 2048, 64, 4, 16, 16, 8, 4008,
                          0],
    ("llama-3.2-1b", 16): [16, 16, 1, 8, 1, 4, 0, 192, 1, 1, 16, 3072, 2048, 1, 8, 1, 4, 0, 192, 1, 128, 16, 3072, 2048, 3,
                           8, 1, 4, 0, 128, 1, 0, 16, 2048, 2048, 2, 8, 1, 4, 0, 1024, 1, 128, 16, 16384, 2048, 3, 8, 1, 4,
                           0, 128, 1, 0, 16, 2048, 8192, 4, 4, 2, 4, 0, 4008, 1, 128, 16, 128256, 2048, 64, 4, 2, 16, 128,
                           4008, 0],
    ("micro", 1): [1, 1, 1, 4, 1, 2, 0, 32, 1, 1, 1, 512, 256, 1, 4, 1, 2, 0, 32, 1, 64, 1, 512, 256, 3, 4, 1, 1, 2, 64, 1,
                   0, 1, 256, 256, 2, 4, 1, 2, 0, 64, 1, 64, 1, 1024, 256, 3, 4, 1, 1, 2, 64, 1, 0, 1, 256, 512, 4, 4, 2,
                   2, 0, 128, 1, 64, 1, 4096, 256, 64, 2, 8, 8, 2, 128, 0],
    ("bias", 16): [16, 16, 5, 4, 1, 2, 0, 72, 1, 1, 16, 1152, 256, 5, 4, 1, 2, 0, 72, 1, 16, 16, 1152, 256, 3, 8, 1, 4, 0,
                   16, 1, 0, 16, 256, 896, 2, 4, 1, 2, 0, 32, 1, 16, 16, 512, 256, 3, 4, 1, 2, 0, 16, 1, 0, 16, 256, 256,
                   4, 4, 2, 2, 0, 16, 1, 16, 16, 512, 256, 64, 7, 2, 2, 32, 16, 0],
    ("qk-norm", 1): [1, 1, 0, 4, 1, 2, 0, 64, 1, 1, 1, 1024, 256, 0, 4, 1, 2, 0, 64, 1, 64, 1, 1024, 256, 3, 4, 1, 1, 2,
                     64, 1, 0, 1, 256, 512, 2, 4, 1, 2, 0, 32, 1, 64, 1, 512, 256, 3, 4, 1, 1, 2, 64, 1, 0, 1, 256, 256,
                     4, 4, 2, 2, 0, 16, 1, 64, 1, 512, 256, 128, 2, 2, 2, 2, 16, 1],
}


def _ints(plan):
    return list((ctypes.c_int * (ctypes.sizeof(plan) // 4)).from_buffer_copy(plan))


def test_plan_of_a_scaled_model():
    lib = _lib_or_skip()
    assert ops.LlamaDims(vocab=1).rope_table == 0  # every construction without the keyword keeps the old step
    assert [n for n, _ in ops.StepPlan._fields_][-2:] == ["qk_norm_grid", "qk_norm_table"]
    for name, shape in SHAPES.items():
        for B in (1, 16, 17, 64):
            on, off = ops.step_plan(ops.LlamaDims(rope_table=1, **shape), B), ops.step_plan(ops.LlamaDims(**shape), B)
            a, b = _ints(on), _ints(off)
            assert b[-1] == 0
            if (name, B) in PARENT_PLANS:  # the unscaled plan is the parent's, int for int
                assert b[:-1] == PARENT_PLANS[name, B], (name, B)
            if shape.get("qk_norm"):  # only the variant flag of k_qknorm_rope moves
                assert a[-1] == on.qk_norm_table == 1 and a[:-1] == b[:-1] and on.qkv.epi == EPI_STORE
                continue
            want = (EPI_ROPE_BIAS_TAB, EPI_ROPE_BIAS) if shape.get("qkv_bias") else (EPI_ROPE_TAB, EPI_ROPE)
            assert (on.qkv.epi, off.qkv.epi) == (on.qkv_first.epi, off.qkv_first.epi) == want
            assert on.qk_norm_table == 0 and on.qk_norm_grid == 0
            epi_at = (2, 13)  # qkv_first.epi and qkv.epi in the flat plan
            assert [x for i, x in enumerate(a) if i not in epi_at] == [x for i, x in enumerate(b) if i not in epi_at]
        # the workspace layout does not move
        assert lib.p2pt_llama_ws_bytes(ctypes.byref(ops.LlamaDims(rope_table=1, **shape))) == \
            lib.p2pt_llama_ws_bytes(ctypes.byref(ops.LlamaDims(**shape))) != 0
    # batch 1 of the 1B shape keeps its K parts on O and down
    one = ops.step_plan(ops.LlamaDims(rope_table=1, **SHAPES["llama-3.2-1b"]), 1)
    assert (one.o.kpl, one.down.kpl, one.qkv.kpl) == (1, 1, 0) and (one.qkv.nw, one.qkv.um) == (8, 4)
    for bad in (2, -1):
        d = ops.LlamaDims(rope_table=bad, **SHAPES["micro"])
        assert lib.p2pt_llama_ws_bytes(ctypes.byref(d)) == 0
        with pytest.raises(ValueError):
            ops.step_plan(d, 1)
    # the table epilogues carry the (nw, um) pairs plan_gemm can give a QKV projection: all of them are planned
    seen = set()
    for dim in range(32, 4097, 32):
        p = ops.step_plan(ops.LlamaDims(rope_table=1, **dict(SHAPES["micro"], dim=dim)), 1).qkv
        seen.add((p.nw, p.um))
    assert seen == {(4, 1), (4, 2), (4, 4), (8, 4)}


# ---------------------------------------------------------------- the rotation: fp64 reference and bound
def ulp(a):
    _, e = torch.frexp(a.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(a), e - 8)


def table_angles(pos, table):
    """cos, sin [M, 1, D/2] in fp64 of pos * table (the exact fp32 entries) and dsc, the bound on the kernel's
    fp32 cos / sin: |p f| U for the one rounding of the product, 4 U for sincosf (module docstring)."""
    ang = pos.to(F64)[:, None, None] * table.to(F64)[None, None, :]
    return torch.cos(ang), torch.sin(ang), ang.abs() * U + 4 * U


def rotation(x1, x2, f1, f2, cs, sn, dsc):
    """The rotated pair (o1 | o2 concatenated on the last axis, dims i and i + D/2) in fp64 and its bound, from the
    pair's bf16 values x1, x2 (fp64) and how far each can be from the kernel's own (f1, f2: ``flip``, 0 for exact
    inputs): module docstring."""
    o1, o2 = x1 * cs - x2 * sn, x2 * cs + x1 * sn
    common = (x1.abs() + x2.abs()) * dsc
    E1 = f1 * cs.abs() + f2 * sn.abs() + common + 3 * U * ((x1 * cs).abs() + (x2 * sn).abs())
    E2 = f2 * cs.abs() + f1 * sn.abs() + common + 3 * U * ((x2 * cs).abs() + (x1 * sn).abs())
    o, E = torch.cat([o1, o2], -1), torch.cat([E1, E2], -1)
    return o, rounded(o, E)


# ---------------------------------------------------------------- fp32 NumPy emulation of the table epilogue
def np_bf16(x):
    """fp32 -> bf16 (round to nearest even) -> fp32, in NumPy."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((b + (0x7FFF + ((b >> 16) & 1))) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32)


def slipped_table(theta, D, s, slip):
    """models/rope.py's llama3 rule in fp32 NumPy, from its unscaled frequencies (torch's pow; NumPy's differs by an
    ulp), with one of the table slips."""
    base = (1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))).numpy()
    f = np.float32(s.factor)
    if slip == "all_divided":  # llama3 treated as linear
        return base / f
    if slip == "none_divided":
        return base
    wavelen = (np.float32(2 * math.pi) / base).astype(np.float32)
    low, high = s.original_max_seq / s.low_freq_factor, s.original_max_seq / s.high_freq_factor
    if slip == "bands_swapped":  # the two comparisons take each other's threshold
        low, high = high, low
    out = np.where(wavelen > low, base / f, base)
    smooth = (np.float32(s.original_max_seq) / wavelen - np.float32(s.low_freq_factor)) / \
        np.float32(s.high_freq_factor - s.low_freq_factor)
    if slip == "smooth_wrong_operand":  # the interpolation weights take each other's term
        smoothed = smooth * out / f + (1 - smooth) * out
    else:
        smoothed = (1 - smooth) * out / f + smooth * out
    medium = ~(wavelen < high) & ~(wavelen > low)
    return np.where(medium, smoothed, out).astype(np.float32)


SLIPS = ("all_divided", "none_divided", "bands_swapped", "smooth_wrong_operand", "index_d", "index_no_mod",
         "v_rotated", "sin_sign", "pos_plus_one")
PAD = np.float32(0.37)  # what a read past the table's D/2 entries finds


def emulate_epilogue(y, pos, table, H, Hkv, D, slip=None):
    """The EPI_ROPE_TAB epilogue after the rounding of the projection, column by column as the kernel does it:
    ``y`` fp32 [M, N] holds bf16 values in the interleaved row order of wqkv (column 2i = dim i, 2i + 1 = dim
    i + D/2 of head col / D). Returns (q [M, H, D], k [M, Hkv, D], v [M, Hkv, D]) as fp32 arrays of bf16 values."""
    M, N = y.shape
    half = D // 2
    col = np.arange(N)
    head, i, second = col // D, (col % D) >> 1, (col & 1).astype(bool)
    d = i + np.where(second, half, 0)
    idx = d if slip == "index_d" else (col >> 1) if slip == "index_no_mod" else i
    f = np.concatenate([table.astype(np.float32), np.full(N, PAD, np.float32)])[idx]  # the table lookup
    p = pos.astype(np.float32) + (np.float32(1) if slip == "pos_plus_one" else np.float32(0))
    a = (p[:, None] * f[None, :]).astype(np.float32)  # the fp32 product p * f
    sn = np.sin(a.astype(np.float64)).astype(np.float32)  # sincosf: correctly rounded here
    cs = np.cos(a.astype(np.float64)).astype(np.float32)
    if slip == "sin_sign":
        sn = -sn
    mine, other = y, y[:, col ^ 1]
    x1, x2 = np.where(second, other, mine), np.where(second, mine, other)
    o = np.where(second, x2 * cs + x1 * sn, x1 * cs - x2 * sn).astype(np.float32)
    rot = head < (H + 2 * Hkv if slip == "v_rotated" else H + Hkv)
    out = np_bf16(np.where(rot[None, :], o, y))  # one bf16 rounding; v is stored as it came
    plain = np.empty((M, H + 2 * Hkv, D), np.float32)
    plain[:, head, d] = out
    return plain[:, :H], plain[:, H:H + Hkv], plain[:, H + Hkv:]


def epilogue_reference(y, pos, table, H, Hkv, D):
    """(q, bound), (k, bound) in fp64 and v (to be matched bit for bit) for ``emulate_epilogue``'s inputs."""
    M = y.shape[0]
    yt = torch.from_numpy(y).to(F64).view(M, H + 2 * Hkv, D // 2, 2)
    cs, sn, dsc = table_angles(torch.from_numpy(pos), torch.from_numpy(table))
    r = yt[:, :H + Hkv]
    zero = torch.zeros_like(r[..., 0])
    o, bound = rotation(r[..., 0], r[..., 1], zero, zero, cs, sn, dsc)
    v = torch.cat([yt[:, H + Hkv:, :, 0], yt[:, H + Hkv:, :, 1]], -1)
    return (o[:, :H], bound[:, :H]), (o[:, H:], bound[:, H:]), v


def epilogue_ratios(got, refs):
    (q, k, v), (qr, kr, vr) = got, refs
    out = {}
    for name, g, (ref, bound) in (("q", q, qr), ("k", k, kr)):
        out[name] = ((torch.from_numpy(g).to(F64) - ref).abs() / bound).max().item()
    out["v"] = 0.0 if torch.equal(torch.from_numpy(v).to(F64), vr) else float("inf")
    return out


EMU_CASES = [(64, 8, 2, L32, 131072), (128, 8, 1, L31, 131072), (128, 4, 1, L32, 4096), (64, 4, 1, SHORT, 512)]


@functools.lru_cache(maxsize=None)
def emu_inputs(D, H, Hkv, s, smax):
    """y, pos, table of an emulation case. Positions: 0, 1, the last row, and for each band seam index i the
    positions that put p * f next to pi / 2 and 2 pi there (where a wrong neighbour's frequency shows)."""
    theta = 10000.0 if s is SHORT else THETA3
    table = rope.inv_freq(theta, D, s).numpy()
    keep, smooth, div = bands(theta, D, s)
    pos = [0, 1, smax - 1, smax // 2 + 1]
    for i in (keep[-1], smooth[0], smooth[-1], div[0]):
        for turn in (0.5 * math.pi, 2 * math.pi):
            pos.append(min(smax - 1, max(1, int(round(turn / float(table[i]))))))
    g = torch.Generator().manual_seed(11 + D + H)
    y = (torch.randn(len(pos), (H + 2 * Hkv) * D, generator=g) * 1.5).to(BF).float()
    y[3, ::7] *= 2.0 ** 20
    y[4, ::5] *= 2.0 ** -20
    return y.to(BF).float().numpy(), np.array(pos, dtype=np.int32), table, theta


@pytest.mark.parametrize("D,H,Hkv,s,smax", EMU_CASES, ids=[f"D{c[0]}-f{c[3].factor:g}-S{c[4]}" for c in EMU_CASES])
def test_emulation_within_the_bound_and_slips_leave_it(D, H, Hkv, s, smax):
    y, pos, table, theta = emu_inputs(D, H, Hkv, s, smax)
    # the NumPy rule is the module's own, to an ulp (torch and NumPy contract the interpolation differently); the
    # unslipped emulation below runs on the module's table, the slips are worth 10 % and more of an entry
    assert np.allclose(table, slipped_table(theta, D, s, None), rtol=2.0 ** -22, atol=0.0)
    refs = epilogue_reference(y, pos, table, H, Hkv, D)
    ok = emulate_epilogue(y, pos, table, H, Hkv, D)
    ratios = epilogue_ratios(ok, refs)
    assert max(ratios.values()) <= 1.0, ratios
    for slip in SLIPS:
        t = slipped_table(theta, D, s, slip) if slip in SLIPS[:4] else table
        assert (not np.array_equal(t, table)) == (slip in SLIPS[:4])
        bad = emulate_epilogue(y, pos, t, H, Hkv, D, slip=slip)
        r = epilogue_ratios(bad, refs)
        assert max(r.values()) > 1.0, (slip, r)
        assert any(not np.array_equal(a, b) for a, b in zip(ok, bad)), slip  # and a stored bit changed


def test_model_tokens_depend_on_the_scaling():
    """The prompts of tests/test_gpu_llama3_rope.py's engine test, re-checked on the CPU: under the fp32 reference the
    scaled ``micro`` model continues each with the recorded greedy tokens, every one of which wins by at least 3 % of
    the largest logit; where a continuation under default RoPE is recorded, the same holds for it and it differs."""
    from test_gpu_llama3_rope import ENGINE_PROMPTS, M3, MODEL_SEED

    def continuation(m, prompt, n):
        seq, margin = list(prompt), math.inf
        for _ in range(n):
            lg = m.reference_logits(torch.tensor([seq]))[0]
            top = lg.topk(2).values
            margin = min(margin, float(top[0] - top[1]) / float(lg.abs().max()))
            seq.append(int(lg.argmax()))
        return seq[len(prompt):], margin

    scaled = TinyLlama(M3, device="cpu", max_batch=1, seed=MODEL_SEED)
    plain = TinyLlama(replace(M3, rope_scaling=None), device="cpu", max_batch=1, seed=MODEL_SEED)
    differ = 0
    for prompt, want, without in ENGINE_PROMPTS:
        got, margin = continuation(scaled, prompt, len(want))
        assert got == list(want) and margin >= 0.03, (len(prompt), got, margin)
        if without is not None:
            got, margin = continuation(plain, prompt, len(without))
            assert got == list(without) != list(want) and margin >= 0.03, (len(prompt), got, margin)
            differ += 1
    assert differ >= 1
