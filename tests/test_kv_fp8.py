"""FP8 (OCP e4m3fn, scale 1) KV cache, the host side: the NumPy reference of the store
(``utils/kv_fp8_ref.py``), the rule the GPU tests judge stored bytes by (``judge``), the plan with
``LlamaDims.kv_fp8``, ``--kv-dtype`` and the decoder's dtype checks. No GPU.

The store. A K or V value is held by the epilogue in fp32 (x'), clamped to [-448, 448] and rounded ONCE to the
nearest e4m3 value, ties to even, subnormals (multiples of 2^-9) included; NaN stays NaN. Against an fp64 reference
x with |x' - x| <= e_pre the decoded byte y satisfies

    |y - clamp(x)| <= hu + e_pre,   hu = 2^(floor(log2(|x| + e_pre)) - 4) for |x| >= 2^-6, 2^-10 below

(half the e4m3 spacing at |x|: 3 mantissa bits, so the spacing is 2^(e - 3)), and wherever x lies farther than
e_pre from every rounding boundary of the format, x' rounds as x does: the byte is RNE(clamp(x)) exactly. ``judge``
returns the worst ratio to the bound, the decided bytes that differ and the share of undecided elements.
"""
import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models import server
from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig, TinyLlama, e4m3_round
from p2p_llm_tunnel_amd.utils import kv_fp8_ref as ref

POISON = 0x5B  # the byte a test cache holds before a store


# ---------------------------------------------------------------- the rule
def rne64(x):
    """The byte of an fp64 value under clamp + round-to-nearest-even, from the format's own value table (no fp32
    step in between). NaN -> 0x7f | sign."""
    x = np.asarray(x, dtype=np.float64)
    a = np.minimum(np.abs(np.nan_to_num(x, nan=0.0)), ref.MAX)
    b = ref.boundaries()
    idx = np.searchsorted(b, a, side="left")  # boundaries strictly below a
    tie = (idx < len(b)) & (b[np.minimum(idx, len(b) - 1)] == a)
    idx = np.where(tie & (idx % 2 == 1), idx + 1, idx)  # a tie goes to the even byte of idx, idx + 1
    byte = np.where(np.isnan(x), 0x7F, idx).astype(np.uint8)
    return byte | (np.signbit(x).astype(np.uint8) << 7)


def judge(x, e_pre, got):
    """x, e_pre: fp64 arrays; got: uint8 bytes of the same shape. Returns (worst |y - clamp(x)| / (hu + e_pre),
    number of decided elements whose byte is not RNE(x), share of undecided elements). A NaN reference asks for a
    NaN byte (either sign); a NaN byte anywhere else counts as an infinite error."""
    x, e_pre, got = np.asarray(x, np.float64), np.asarray(e_pre, np.float64), np.asarray(got, np.uint8)
    nan = np.isnan(x)
    y = ref.decode(got).astype(np.float64)
    cx = np.clip(np.where(nan, 0.0, x), -ref.MAX, ref.MAX)
    hu = ref.half_ulp(np.abs(cx) + e_pre)
    with np.errstate(invalid="ignore"):
        ratio = np.abs(y - cx) / (hu + e_pre)
    ratio = np.where(np.isnan(y), np.inf, ratio)
    ratio = np.where(nan, np.where((got & 0x7F) == 0x7F, 0.0, np.inf), ratio)
    # An exact input (e_pre = 0) is decided even on a boundary: round-to-nearest-even says which byte.
    decided = nan | (ref.boundary_distance(np.where(nan, 0.0, x)) > e_pre) | (e_pre == 0)
    want = rne64(x)
    wrong = decided & np.where(nan, (got & 0x7F) != 0x7F, got != want)
    return float(ratio.max()), int(wrong.sum()), float(1.0 - decided.mean())


# ---------------------------------------------------------------- the reference against torch
def test_every_byte_decodes_and_encodes_like_torch():
    b = np.arange(256, dtype=np.uint8)
    t = torch.from_numpy(b.copy()).view(torch.float8_e4m3fn).float().numpy()
    d = ref.decode(b)
    assert np.array_equal(np.isnan(d), np.isnan(t)) and np.isnan(d).sum() == 2
    ok = ~np.isnan(d)
    assert np.array_equal(d[ok].view(np.uint32), t[ok].view(np.uint32))  # -0.0 included
    assert np.array_equal(ref.encode(d), b)  # NaN bytes 0x7f / 0xff keep their sign
    assert ref.decode(np.uint8([0x7E]))[0] == 448.0 and ref.decode(np.uint8([0x01]))[0] == 2.0 ** -9


def sweep():
    """fp32 inputs: a dense grid over [-470, 470], every rounding boundary with its two fp32 neighbours (both
    signs), small values around the subnormals, the zeros, tiny and huge values, infinities."""
    b = ref.boundaries().astype(np.float32)
    assert np.array_equal(b.astype(np.float64), ref.boundaries())  # every boundary is an fp32 value
    near = np.concatenate([b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(1e9))])
    rng = np.random.default_rng(7)
    return np.concatenate([np.linspace(-470, 470, 400001, dtype=np.float32), near, -near,
                           (rng.standard_normal(200000) * 0.02).astype(np.float32),
                           np.float32([0.0, -0.0, 2.0 ** -10, -2.0 ** -10, 2.0 ** -11, 1e-30, -1e-30, 1e-45, 448.0, -448.0,
                                       463.9, 464.0, 1e9, -1e9, np.inf, -np.inf])])


def test_encode_matches_torch_on_a_dense_sweep():
    x = sweep()
    mine = ref.encode(x)
    theirs = torch.from_numpy(ref.clamp(x)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(mine, theirs)
    assert np.array_equal(mine, e4m3_round(torch.from_numpy(x)).to(torch.float8_e4m3fn).view(torch.uint8).numpy())
    # what the issue states about torch's cast, re-checked: ties to even, 2^-10 flushes, NaN above 464 without a clamp
    c = lambda v: int(torch.tensor([v]).to(torch.float8_e4m3fn).view(torch.uint8))
    assert c(2.0 ** -10) == 0 and c(3 * 2.0 ** -10) == 2 and c(17.0) == c(16.0) and c(19.0) == c(20.0)
    assert c(463.9) == 0x7E and c(464.0) == 0x7E and c(465.0) == 0x7F  # 464 is a tie, to even
    nan = ref.encode(np.float32([np.nan, -np.nan]))
    assert list(nan & 0x7F) == [0x7F, 0x7F]


def test_encode_holds_the_fp64_bound_and_is_decided_everywhere():
    x = sweep()
    x = x[np.isfinite(x)]
    ratio, wrong, undecided = judge(x.astype(np.float64), np.zeros(len(x)), ref.encode(x))
    assert ratio <= 1.0 and wrong == 0 and undecided <= 0.01  # e_pre = 0: only exact ties are "undecided"
    assert np.array_equal(rne64(x.astype(np.float64)), ref.encode(x))


# ---------------------------------------------------------------- one-line slips
D = 64


def rows_for_slips():
    """K / V rows [12, 64] in fp32 as an epilogue holds them: a few units of noise, planted values in (448, 464),
    beyond 464, subnormals, values that round to +-0, and NaN."""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((12, D)) * 3.0).astype(np.float32)
    x[1, :6] = [450.0, -455.5, 463.0, 470.0, -1000.0, 3.0e4]
    x[2, :8] = [2.0 ** -7, -3 * 2.0 ** -9, 5 * 2.0 ** -10, -2.0 ** -9, 2.0 ** -12, -2.0 ** -12, 0.0, -0.0]
    x[3, 10] = np.nan
    x[3, 11] = -np.nan
    x[4] = (rng.standard_normal(D) * 0.004).astype(np.float32)  # a row of subnormals
    return x


def bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u + (0x7FFF + ((u >> 16) & 1))) & 0xFFFF0000).astype(np.uint32)
    return np.where(np.isnan(x), x, r.view(np.float32))


def encode_noclamp(x):
    """The conversion alone, as a cast without saturation does it: NaN above 464."""
    return np.where(np.abs(x) > 464.0, np.uint8(0x7F) | (np.signbit(x).astype(np.uint8) << 7), ref.encode(x))


def store(x, slip=None):
    """The byte rows [rows, D] a cache holds after the store of x, starting from POISON bytes."""
    out = np.full(x.shape, POISON, np.uint8)
    if slip is None:
        out[:] = ref.encode(x)
    elif slip == "through_bf16":  # a double rounding
        out[:] = ref.encode(bf16_round(x))
    elif slip == "truncation":  # toward zero: the next byte down wherever the rounding went up
        b = ref.encode(x)
        up = np.abs(ref.decode(b).astype(np.float64)) > np.abs(ref.clamp(x).astype(np.float64))
        out[:] = np.where(up & ~np.isnan(x), b - 1, b)
    elif slip == "fnuz_bias":  # exponent bias 8: every value's bit pattern is that of twice the value
        out[:] = ref.encode(x * np.float32(2))
    elif slip == "no_clamp":
        out[:] = encode_noclamp(x)
    elif slip == "clamp_after":  # convert, then bound the byte's magnitude at 0x7e: NaN inputs end as 448
        b = encode_noclamp(x)
        out[:] = (b & 0x80) | np.minimum(b & 0x7F, 0x7E)
    elif slip == "v_as_bf16":  # two bytes per element: the row holds the first D / 2 elements' bf16 bits
        bits = (np.ascontiguousarray(bf16_round(x[:, :D // 2]), np.float32).view(np.uint32) >> 16).astype(np.uint16)
        out[:] = bits.view(np.uint8).reshape(x.shape)
    elif slip == "k_at_bf16_stride":  # the right byte at offset 2 d
        out[:, 0::2] = ref.encode(x)[:, :D // 2]
    elif slip == "sign_dropped_on_subnormals":
        b = ref.encode(x)
        out[:] = np.where((b & 0x78) == 0, b & 0x7F, b)
    else:
        raise KeyError(slip)
    return out


SLIPS = ("through_bf16", "truncation", "fnuz_bias", "no_clamp", "clamp_after", "v_as_bf16", "k_at_bf16_stride",
         "sign_dropped_on_subnormals")


def test_the_store_passes_its_own_rule():
    x = rows_for_slips()
    e = np.abs(x.astype(np.float64)) * 2.0 ** -20  # a pre-rounding error of the size the GEMM bounds have
    e = np.where(np.isnan(e), 0.0, e)
    ratio, wrong, undecided = judge(x.astype(np.float64), e, store(x))
    assert ratio <= 1.0 and wrong == 0 and undecided <= 0.01, (ratio, wrong, undecided)


@pytest.mark.parametrize("slip", SLIPS)
def test_every_slip_leaves_the_bound_or_changes_a_decided_byte(slip):
    x = rows_for_slips()
    e = np.where(np.isnan(x), 0.0, np.abs(x.astype(np.float64)) * 2.0 ** -20)
    ratio, wrong, _ = judge(x.astype(np.float64), e, store(x, slip))
    assert ratio > 1.0 or wrong > 0, (slip, ratio, wrong)


# ---------------------------------------------------------------- the plan
def dims(kv_fp8=None, **kw):
    base = dict(vocab=512, dim=256, n_layers=2, H=8, Hkv=2, D=64, ffn=512, max_seq=256, max_batch=5, eps=1e-5,
                theta=1e4)
    base.update(kw)
    if kv_fp8 is not None:
        base["kv_fp8"] = kv_fp8
    return ops.LlamaDims(**base)


def flat(s):
    """Every int of a plan structure as {dotted name: value}."""
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        if hasattr(v, "_fields_"):
            out.update({f"{name}.{k}": w for k, w in flat(v).items()})
        else:
            out[name] = v
    return out


FAMILIES = {"plain": {}, "bias": {"qkv_bias": 1}, "table": {"rope_table": 1}, "bias_table": {"qkv_bias": 1, "rope_table": 1},
            "qk_norm": {"qk_norm": 1}, "qk_norm_table": {"qk_norm": 1, "rope_table": 1}}
KV8 = 8  # kEpiKv8: the distance from a RoPE epilogue to its FP8-cache counterpart


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("D,H", ((64, 8), (128, 14)))
def test_kv_fp8_moves_only_the_appending_and_reading_variants(family, D, H):
    for B in (1, 5, 16, 17, 64):
        old = flat(ops.step_plan(dims(D=D, H=H, **FAMILIES[family]), B))
        off = flat(ops.step_plan(dims(0, D=D, H=H, **FAMILIES[family]), B))
        on = flat(ops.step_plan(dims(1, D=D, H=H, **FAMILIES[family]), B))
        assert off == old
        kv_off, kv_on = ops.kv_plan(dims(0, D=D, H=H, **FAMILIES[family])), ops.kv_plan(dims(1, D=D, H=H, **FAMILIES[family]))
        assert (kv_off.attn_kv8, kv_off.qk_norm_kv8) == (0, 0) == tuple(flat(ops.kv_plan(dims(D=D, H=H, **FAMILIES[family]))).values())
        moved = {k for k in on if on[k] != off[k]}
        if "qk_norm" in family:  # EPI_STORE stays; k_qknorm_rope and k_attn change variant
            assert moved == set() and on["qkv.epi"] == 0 and kv_on.qk_norm_kv8 == 1
        else:
            assert moved == {"qkv.epi", "qkv_first.epi"}
            assert on["qkv.epi"] == on["qkv_first.epi"] == off["qkv.epi"] + KV8 and kv_on.qk_norm_kv8 == 0
        assert kv_on.attn_kv8 == 1
        # the workspace does not depend on the cache format
        assert ops.lib().p2pt_llama_ws_bytes(dims(1, D=D, H=H, **FAMILIES[family])) == \
            ops.lib().p2pt_llama_ws_bytes(dims(D=D, H=H, **FAMILIES[family])) > 0


def test_the_field_leaves_earlier_constructions_alone():
    # kv_fp8 follows theta, ahead of the three family flags: tests of those families pin qkv_bias as the last field
    # and the layout of StepPlan int for int, so the FP8-cache choices are reported in a KvPlan of their own.
    names = [n for n, _ in ops.LlamaDims._fields_]
    assert names[-4:] == ["kv_fp8", "rope_table", "qk_norm", "qkv_bias"] and names[-5] == "theta"
    assert [n for n, _ in ops.StepPlan._fields_][-2:] == ["qk_norm_grid", "qk_norm_table"]
    assert [n for n, _ in ops.AttnPlan._fields_] == ["D", "G", "slots", "stride", "grid_y"]
    assert [n for n, _ in ops.KvPlan._fields_] == ["attn_kv8", "qk_norm_kv8"]
    d = ops.LlamaDims(512, 256, 2, 8, 2, 64, 512, 256, 5, 1e-5, 1e4)  # positional up to theta, as before the field
    assert (d.kv_fp8, d.rope_table, d.qk_norm, d.qkv_bias) == (0, 0, 0, 0)
    assert ops.LlamaDims(vocab=1, qkv_bias=1, rope_table=1).kv_fp8 == 0


def test_other_values_of_kv_fp8_are_refused():
    out = ops.StepPlan()
    for bad in (2, -1):
        d = dims(bad)
        assert ops.lib().p2pt_llama_ws_bytes(d) == 0 and ops.lib().p2pt_llama_plan(d, 4, 0, out) != 0
        with pytest.raises(ValueError):
            ops.step_plan(d, 4)
        with pytest.raises(ValueError):
            ops.kv_plan(d)


# ---------------------------------------------------------------- the switch
def test_kv_dtype_parsing():
    assert server.arg_parser().parse_args([]).kv_dtype == "bf16"
    assert server.arg_parser().parse_args(["--kv-dtype", "fp8"]).kv_dtype == "fp8"
    with pytest.raises(SystemExit):
        server.arg_parser().parse_args(["--kv-dtype", "fp4"])
    assert server.parse_kv_dtype("bf16") == "bf16" and server.parse_kv_dtype("fp8") == "fp8"
    for bad in ("fp4", "e4m3", None, 8):
        with pytest.raises(ValueError, match="kv_dtype"):
            server.parse_kv_dtype(bad)
    with pytest.raises(ValueError, match="kv_dtype"):
        server.start_server(kv_dtype="int8")


def test_replicas_carry_the_switch():
    a = server.arg_parser().parse_args(["--gpus", "2", "--kv-dtype", "fp8", "--port", "9000", "--penalties"])
    for i in range(2):
        cmd = server.replica_cmd(a, i)
        assert cmd[cmd.index("--kv-dtype") + 1] == "fp8" and cmd[cmd.index("--device") + 1] == f"cuda:{i}"
        assert cmd[cmd.index("--port") + 1] == str(9000 + i) and "--penalties" in cmd and "--gpus" not in cmd
    assert "--kv-dtype" not in server.replica_cmd(server.arg_parser().parse_args(["--gpus", "2"]), 0)


def test_the_eager_engine_refuses_an_fp8_cache():
    m = TinyLlama("micro", device="cpu", max_batch=2, kv_dtype="fp8")
    with pytest.raises(ValueError, match="fp8 KV cache needs the graph-captured HIP step"):
        server.Engine(model=m)
    with pytest.raises(ValueError, match="injected model"):
        server.Engine(model=TinyLlama("micro", device="cpu", max_batch=2), kv_dtype="fp8")


# ---------------------------------------------------------------- model and decoder
MICRO1 = LlamaConfig(vocab=512, dim=256, n_layers=1, n_heads=4, n_kv_heads=2, head_dim=64, ffn=256, max_seq=64)


def test_fp8_model_allocates_half_the_bytes():
    a, b = TinyLlama(MICRO1, device="cpu", max_batch=3), TinyLlama(MICRO1, device="cpu", max_batch=3, kv_dtype="fp8")
    assert a.kv_dtype == "bf16" and a.k_cache.dtype == torch.bfloat16
    assert b.k_cache.dtype == b.v_cache.dtype == torch.float8_e4m3fn and b.k_cache.element_size() == 1
    assert b.k_cache.shape == a.k_cache.shape and 2 * b.k_cache.nbytes == a.k_cache.nbytes
    assert 2 * b.kv_cache_bytes() == a.kv_cache_bytes()
    assert str(b.kv_cache_bytes()) in server.kv_cache_line(b, "fp8")
    with pytest.raises(ValueError, match="kv_dtype"):
        TinyLlama(MICRO1, device="cpu", kv_dtype="fp16")


def test_the_unfused_path_refuses_an_fp8_cache():
    m = TinyLlama(MICRO1, device="cpu", max_batch=2, kv_dtype="fp8", fused=False)
    with pytest.raises(ValueError, match="fused step only"):
        m.decode_step(torch.tensor([1]), torch.tensor([0], dtype=torch.int32), (0, 0))


def test_reference_rounds_kv_once_and_only_with_the_hook():
    a, b = TinyLlama(MICRO1, device="cpu", max_batch=1, seed=3), TinyLlama(MICRO1, device="cpu", max_batch=1, seed=3,
                                                                         kv_dtype="fp8")
    seq = torch.arange(5, 25)[None]
    la, lb = a.reference_logits(seq), b.reference_logits(seq)
    assert torch.equal(la, b.reference_logits(seq, kv_round=lambda t: t.to(torch.bfloat16).float()))
    assert torch.equal(lb, a.reference_logits(seq, kv_round=e4m3_round))
    d = (la - lb).abs().max().item()
    assert 0 < d < 0.2 * la.abs().max().item()
    x = torch.tensor([500.0, -1e4, 460.0, 1.0625, float("nan")])
    assert e4m3_round(x)[:4].tolist() == [448.0, -448.0, 448.0, 1.0] and bool(e4m3_round(x)[4].isnan())


def test_decoder_refuses_a_cache_of_the_other_format():
    bf = torch.zeros(1, 3, 64, 2, 64, dtype=torch.bfloat16)
    f8 = torch.zeros(1, 3, 64, 2, 64, dtype=torch.float8_e4m3fn)
    d0 = dims(0, n_layers=1, H=4, max_seq=64, max_batch=3)
    d1 = dims(1, n_layers=1, H=4, max_seq=64, max_batch=3)
    with pytest.raises(TypeError, match="kv_fp8 is set"):
        ops.FusedLlamaDecoder(d1, [], bf, bf)
    with pytest.raises(TypeError, match="kv_fp8 is set"):
        ops.FusedLlamaDecoder(d1, [], f8, bf)
    with pytest.raises(TypeError, match="needs dims.kv_fp8 = 1"):
        ops.FusedLlamaDecoder(d0, [], f8, f8)
    with pytest.raises(TypeError, match="needs dims.kv_fp8 = 1"):
        ops.FusedLlamaDecoder(d0, [], f8.view(torch.uint8), f8.view(torch.uint8))
    with pytest.raises(ValueError, match="kv_fp8 must be 0 or 1"):
        ops.FusedLlamaDecoder(dims(2, n_layers=1, H=4, max_seq=64, max_batch=3), [], f8, f8)
