"""The standalone decode kernels of ``ops/kernels.hip`` (``ops.rmsnorm``, ``ops.silu_mul``,
``ops.rope_qkv_cache``, ``ops.decode_attention``, ``ops.argmax``: the unfused path that the model tests use
as their oracle) against fp64 references computed from the exact bf16 inputs, element by element. Inputs are
bf16 bit patterns made with numpy from fixed seeds. No error is scaled by a global maximum and no element is
left out. Every bound is derived here from the operations the kernel performs, never fitted to what it
returns. U = 2^-24 is the fp32 unit roundoff, ulp(x) the bf16 spacing at |x| (2^-133 below the normal range),
TINY = 2^-126 absorbs fp32 roundings (or flushes) below the normal range, and second-order terms are covered
by a factor 1.01 where a first-order term is not tiny. ``ops/build.py`` compiles without a fast-math flag, so
rsqrtf, exp2f, sincosf and the division are the precise library versions (<= 2 ulp = 4 U); ``__expf(x)`` is
v_exp_f32(log2(e) x).

An output stored as bf16 whose fp32 value before rounding is within E of the reference Y is within

    rounded(Y, E) = E + ulp(|Y| + E) / 2

of it (a Y whose magnitude reaches 2^128 - 2^119 rounds to an infinity, and must).

* RMSNorm. Y_c = x_c g_c / sqrt(mean(x^2) + eps), eps the fp32 number it is passed as. The squares of bf16
  values are exact in fp32; their sum has non-negative terms, so with at most ``hidden`` roundings on any path
  it carries hidden U relative; the 1 / hidden factor, the multiply and the eps add: U each; all halved by the
  power -1/2; rsqrtf 4 U: 1/rms within (hidden / 2 + 8) U (the figure of test_gpu_fused_stages.py). Two
  products, (x rs) g: E = (hidden / 2 + 10) U |Y| + TINY. With a residual the kernel adds in fp32, rounds
  to bf16 (``res_out``, compared bit for bit with the same two steps on the host) and normalises the rounded
  sum, so the reference starts from that rounded sum. An all-zero row gives zeros exactly. A row whose fp32
  sum of squares overflows is outside this op's domain (1/rms becomes 0) and is not tested.
* SwiGLU. Y = g u / (1 + exp(-g)). ``__expf(-g)``: the rounding of log2(e) (-g) and of the constant move the
  result by <= 2 |g| U, v_exp_f32 by 1 ulp: (2 |g| + 2) U, which 1 / (1 + e) damps to at most as much; the
  add, the division and the product: 3 U. E = (2 |g| + 8) U |Y| + 2^-149 |u| + TINY (the middle term: an
  fp32 rounding of silu(g) below the normal range is absolute, 2^-150, and is scaled by u). Flush to zero: where
  exp(-g) reaches 2^128 (1 - 2^-10) the fp32 exponential may be +inf (its relative error there is below
  200 U), the quotient is then -0 and the output a zero, although |Y| = |g u| / (1 + exp(-g)) can be as
  large as 89 * 2^-128 |u|: there the allowed error is E + |Y|. This is the formula's range, not an
  arithmetic error; for |u| <= 1 it is below 23 TINY.
* RoPE (rotate-half, inv_freq_i = theta^(-2 i / D)). inv_freq = exp2f(t), t = -log2f(theta) (2 i) / D: log2f,
  the product and the division round once each, so t is off by 3 |t| U and inv_freq by ln 2 times that,
  relatively, plus exp2f and the rounding of float(p) inv_freq: the angle a is within a (3 ln 2 |t| + 3) U
  radians; sincosf adds 4 U. With dsc the sum of the two, o1 = x1 cos - x2 sin has
  E = (|x1| + |x2|) dsc + 3 U (|x1 cos| + |x2 sin|) + TINY (two products and an add), o2 likewise. The V row
  is a copy and every element of both caches outside the one written row keeps its poison bit pattern.
* Attention. o_d = sum_t p_t v_td, p = softmax(scale q.k_t) over t < len. The kernel scales q in fp32 (U per
  element) and sums D products in fp32: a score is within ds = (D + 8) U scale max_t sum_d |q_d k_td|. The
  weight a token ends up with is a product of ``__expf`` factors whose exponents telescope to s_t - M (its
  own tile's, the ``corr`` rescale at every later tile of its split, the reduce's exp(m_s - M)): at most
  nf = ceil(chunk / 64) + 1 factors, each off by (3 R + 4) U relatively (R: the row's score range, which
  bounds every exponent; the subtraction R U, the log2(e) product 2 R U, v_exp_f32 2 U, applying the factor
  U). M is common to numerator and denominator and cancels, so a weight is off by eta = ds + nf (3 R + 4) U
  relatively. A term passes at most n_add = 65 ceil(chunk / 64) + 2 splits + 8 fp32 additions (64 per tile in
  P.V, the rescale, 6 wave levels, the merge). Numerator and denominator are then each off by
  eta + n_add U relative to sum_t p_t |v_td| =: A_d and to 1, 1 / L and the last product add 2 U:

      E_d = 1.01 (2 eta + 2 n_add U + 4 U) A_d + len 2^-123 max|v|

  (the last term: a weight of which any partial product drops below 2^-126 is flushed or rounded absolutely;
  its true value is then below 2^-125 of the largest). Rows of the cache at and beyond a sequence's length
  hold NaN and must not matter, nor must the uninitialised partials of idle splits when ``max_len`` is the
  cache capacity (the captured-graph case).
* Argmax. Exact: the first index of the largest non-NaN entry; 0 when nothing is above -inf.

The CPU tests hold a plain fp32 numpy emulation of each kernel (same tiles, splits and merge) to the same
bounds on the same cases and show that a list of one-line slips each break a bound or an exact comparison.
"""
import math

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd import ops

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -126
BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127
POISON = 0x7B7B  # cache elements that must stay untouched hold this bf16 bit pattern
NAN_BITS = 0x7FC0
F32 = np.float32
LOG2E = F32(1.4426950408889634)


# ---------------------------------------------------------------- bf16 and bounds
def bf16_of(a):
    """array -> (bf16 bit patterns uint16, their exact float32 values), round to nearest even."""
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    bits = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return bits, val(bits)


def val(bits):
    return (np.asarray(bits).astype(np.uint32) << 16).view(F32)


def ulp(a):
    _, e = np.frexp(np.maximum(np.abs(a), TINY))  # |a| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, e - 8)


def ratio(got, ref, E):
    """Largest |got - ref| / rounded(ref, E) over every element; ``got`` must hold no NaN."""
    got = np.asarray(got, dtype=np.float64)
    assert not np.isnan(got).any()
    bound = E + 0.5 * ulp(np.minimum(np.abs(ref) + E, BF16_MAX))
    top = 2.0 ** 128  # an infinity stands for "at least 2^128"
    return float((np.abs(np.clip(got, -top, top) - np.clip(ref, -top, top)) / bound).max())


def expf(x):
    """``__expf`` in fp32: v_exp_f32(log2(e) x), results below the normal range flushed."""
    with np.errstate(all="ignore"):
        e = np.exp2(LOG2E * np.asarray(x, dtype=F32)).astype(F32)
    return np.where(e < F32(TINY), F32(0), e)


# ================================================================ RMSNorm
HIDDENS = (8, 264, 2048, 2056, 4096, 4104, 8192, 8200, 16384)  # hidden / 8 at and across 256, 512, 1024; the limit


def rms_cases(hidden):
    """(name, x bits, residual bits or None, weight bits, eps): 1 and 3 ordinary rows and 3 special ones (all
    zero; scaled by 1e-3 so that eps decides 1/rms; scaled by 2^50, large but summable in fp32)."""
    out = []
    for n, (eps, with_res) in enumerate(((1e-5, False), (1e-6, False), (1e-5, True), (1e-6, True))):
        rng = np.random.default_rng(HIDDENS.index(hidden) * 10 + n)
        for kind, rows in (("r1", 1), ("r3", 3), ("special", 3)):
            x = rng.standard_normal((rows, hidden)) * 3.0
            r = rng.standard_normal((rows, hidden)) * 3.0
            if kind == "special":
                for a in (x, r):
                    a[0] = 0.0
                    a[1] *= 1e-3
                    a[2] *= 2.0 ** 50
            w = 1.0 + 0.1 * rng.standard_normal(hidden)
            out.append((f"{kind}-eps{eps}-res{int(with_res)}", bf16_of(x)[0], bf16_of(r)[0] if with_res else None,
                        bf16_of(w)[0], eps))
    return out


def residual_sum(x_bits, r_bits):
    """bf16(fp32(x + r)) on the host: bits and values."""
    return bf16_of(val(x_bits) + val(r_bits))


def rms_check(case, out_bits, res_out_bits):
    name, xb, rb, wb, eps = case
    hidden = xb.shape[1]
    x = val(xb)
    if rb is not None:
        want_bits, x = residual_sum(xb, rb)
        assert np.array_equal(res_out_bits, want_bits), (name, "res_out")
    X, g = x.astype(np.float64), val(wb).astype(np.float64)
    Y = X * g / np.sqrt((X * X).mean(axis=1, keepdims=True) + float(F32(eps)))
    got = val(out_bits)
    zero = ~X.any(axis=1)
    assert zero.any() == name.startswith("special") and not got[zero].any(), (name, "zero row")
    return ratio(got, Y, (hidden / 2 + 10) * U * np.abs(Y) + TINY)


def rms_emulate(case, slip=None):
    name, xb, rb, wb, eps = case
    hidden = xb.shape[1]
    v, res_bits = val(xb), None
    with np.errstate(all="ignore"):
        if rb is not None:
            s = v + val(rb)
            res_bits, v = bf16_of(s)
            if slip == "unrounded_residual":
                v = s
        ss = np.sum(v * v, axis=1, dtype=F32)
        inv_h = F32(1) / F32(hidden // 8 if slip == "mean_over_words" else hidden)
        rs = F32(1) / np.sqrt(ss * inv_h + (F32(0) if slip == "eps_dropped" else F32(eps)), dtype=F32)
        out = np.nan_to_num(v * rs[:, None] * val(wb)[None, :], nan=7.0)  # a NaN (0 * inf) must not pass as a zero
    return bf16_of(out)[0], res_bits


@pytest.mark.parametrize("hidden", HIDDENS)
def test_rmsnorm_emulation_is_inside_the_bounds(hidden):
    for case in rms_cases(hidden):
        assert rms_check(case, *rms_emulate(case)) <= 1.0, case[0]


def _breaks(check, *args):
    try:
        return not check(*args) <= 1.0
    except AssertionError:
        return True


@pytest.mark.parametrize("slip", ("eps_dropped", "mean_over_words", "unrounded_residual"))
def test_rmsnorm_slip_breaks_a_bound(slip):
    assert any(_breaks(rms_check, case, *rms_emulate(case, slip)) for case in rms_cases(264)), slip


# ================================================================ SwiGLU
UPS = (1.0, -3.140625, 2.0 ** -126, 2.0 ** 100)


SILU_CASES = ("every-gate", "r3-F8", "r33-F524288")


def silu_case(name, big=True):
    """(name, gate bits [rows, F], up bits [rows, F]). "every-gate": every bf16 bit pattern as the gate, against
    four constant ups. (33, 524288) is 2,162,688 words, above the launch's 2,097,152-word grid cap; the
    emulation, which has no grid, runs it at F = 512 (``big`` False)."""
    if name == "every-gate":
        every = np.arange(65536, dtype=np.uint16)
        return name, np.tile(every, (4, 1)), np.repeat(bf16_of(np.array(UPS))[0][:, None], 65536, axis=1)
    rows, F = (3, 8) if name == "r3-F8" else (33, 524288 if big else 512)
    rng = np.random.default_rng(rows)
    return (name, bf16_of(3.0 * rng.standard_normal((rows, F), dtype=F32))[0],
            bf16_of(rng.standard_normal((rows, F), dtype=F32))[0])


def silu_check(case, out_bits):
    name, gb, ub = case
    with np.errstate(invalid="ignore"):  # the signalling NaN patterns among the gates
        g, u = val(gb).astype(np.float64), val(ub).astype(np.float64)
    ok = np.isfinite(g)  # only finite gates are asserted
    g, u, got = g[ok], u[ok], val(out_bits)[ok]
    with np.errstate(over="ignore"):
        e = np.exp(-g)
    Y = g * u / (1.0 + e)
    E = (2 * np.abs(g) + 8) * U * np.abs(Y) + 2.0 ** -149 * np.abs(u) + TINY
    E = E + np.where(e >= 2.0 ** 128 * (1 - 2.0 ** -10), np.abs(Y), 0.0)  # exp(-g) may be +inf in fp32
    return ratio(got, Y, E)


def silu_emulate(case, slip=None):
    name, gb, ub = case
    g, u = (val(ub), val(gb)) if slip == "gate_up_swapped" else (val(gb), val(ub))
    with np.errstate(all="ignore"):
        return bf16_of(g / (F32(1) + expf(-g)) * u)[0]


@pytest.mark.parametrize("name", SILU_CASES)
def test_silu_emulation_is_inside_the_bounds(name):
    case = silu_case(name, big=False)
    assert silu_check(case, silu_emulate(case)) <= 1.0


@pytest.mark.parametrize("name", SILU_CASES)
def test_silu_slip_breaks_a_bound(name):
    case = silu_case(name, big=False)
    assert _breaks(silu_check, case, silu_emulate(case, "gate_up_swapped"))


# ================================================================ RoPE + cache append
ROPE_HEADS = ((1, 1, 64), (8, 2, 64), (32, 8, 128), (8, 1, 128))  # 64 pairs (< 256 threads) up to 2560 (10 passes)
THETAS = (10000.0, 500000.0)
SMAX = 4096
SMAX_LONG = 131072


def rope_case(H, Hkv, D, theta, smax=SMAX):
    """Seeded qkv rows, one per position. The long cache: B = 2, at Smax - 1 and 4095."""
    pos = (smax - 1, 4095) if smax == SMAX_LONG else (0, 1, 17, smax - 1)
    rng = np.random.default_rng(H * 1000 + D + int(theta) % 97 + smax)
    qkv = bf16_of(rng.standard_normal((len(pos), (H + 2 * Hkv) * D)))[0]
    return dict(H=H, Hkv=Hkv, D=D, theta=theta, smax=smax, pos=np.array(pos, dtype=np.int32), qkv=qkv)


def rope_check(c, q_bits, k_rows, v_rows):
    """q [B, H, D] and the written cache rows [B, Hkv, D] (bit patterns) against the reference."""
    H, Hkv, D, half = c["H"], c["Hkv"], c["D"], c["D"] // 2
    B = len(c["pos"])
    x = val(c["qkv"]).astype(np.float64).reshape(B, H + 2 * Hkv, D)
    assert np.array_equal(v_rows, c["qkv"].reshape(B, H + 2 * Hkv, D)[:, H + Hkv:]), "V row is not a copy"
    t = -math.log2(c["theta"]) * 2.0 * np.arange(half) / D
    ang = c["pos"].astype(np.float64)[:, None, None] * np.exp2(t)[None, None, :]
    dsc = ang * ((3 * math.log(2) * np.abs(t) + 3) * U)[None, None, :] + 4 * U
    cs, sn = np.cos(ang), np.sin(ang)
    x1, x2 = x[:, :H + Hkv, :half], x[:, :H + Hkv, half:]
    common = (np.abs(x1) + np.abs(x2)) * dsc + TINY
    ref = np.concatenate([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1)
    E = np.concatenate([common + 3 * U * (np.abs(x1 * cs) + np.abs(x2 * sn)),
                        common + 3 * U * (np.abs(x2 * cs) + np.abs(x1 * sn))], -1)
    got = np.concatenate([val(q_bits), val(k_rows)], 1)
    return ratio(got, ref, E)


def rope_emulate(c, slip=None):
    H, Hkv, D, half = c["H"], c["Hkv"], c["D"], c["D"] // 2
    B = len(c["pos"])
    x = val(c["qkv"]).reshape(B, H + 2 * Hkv, D)
    i = np.arange(half, dtype=F32)
    t = (-np.log2(F32(c["theta"])) * (i if slip == "exponent_i_over_D" else F32(2) * i)) / F32(D)
    ang = c["pos"].astype(F32)[:, None, None] * np.exp2(t.astype(F32)).astype(F32)[None, None, :]
    cs, sn = np.cos(ang.astype(np.float64)).astype(F32), np.sin(ang.astype(np.float64)).astype(F32)
    if slip == "sin_sign":
        sn = -sn
    r = x[:, :H + Hkv]
    if slip == "interleaved":
        o = np.empty_like(r)
        o[..., 0::2] = r[..., 0::2] * cs - r[..., 1::2] * sn
        o[..., 1::2] = r[..., 1::2] * cs + r[..., 0::2] * sn
    else:
        x1, x2 = r[..., :half], r[..., half:]
        o = np.concatenate([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1)
    bits = bf16_of(o)[0]
    return bits[:, :H], bits[:, H:], c["qkv"].reshape(B, H + 2 * Hkv, D)[:, H + Hkv:]


ROPE_CASES = [(h, th, SMAX) for h in ROPE_HEADS for th in THETAS] + [((1, 1, 64), th, SMAX_LONG) for th in THETAS]
ROPE_IDS = [f"H{h[0]}-Hkv{h[1]}-D{h[2]}-theta{int(th)}-S{s}" for h, th, s in ROPE_CASES]


@pytest.mark.parametrize("heads,theta,smax", ROPE_CASES, ids=ROPE_IDS)
def test_rope_emulation_is_inside_the_bounds(heads, theta, smax):
    c = rope_case(*heads, theta, smax)
    assert rope_check(c, *rope_emulate(c)) <= 1.0


@pytest.mark.parametrize("slip", ("interleaved", "exponent_i_over_D", "sin_sign"))
def test_rope_slip_breaks_a_bound(slip):
    for heads, theta, smax in ROPE_CASES:
        c = rope_case(*heads, theta, smax)
        assert _breaks(rope_check, c, *rope_emulate(c, slip)), (slip, heads, theta, smax)


# ================================================================ decode attention
ATT_SMAX = 600
ATT_HKV = 2
FAMILIES = ("random", "census", "spike", "rising")
ATT_GRID = [(D, chunk) for D in (64, 128) for chunk in (32, 64, 96, 256)]


def att_lens(chunk, capture):
    """Ragged lens of one launch; ``capture``: every len below the capacity that is passed as max_len."""
    top = ATT_SMAX - 7 if capture else ATT_SMAX
    return list(dict.fromkeys([1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk, top]))


def att_case(D, G, chunk, family, capture, scale=None, seed=0):
    """One launch: q [B, H, D], caches [B, Smax, Hkv, D] as bit patterns, NaN at and beyond each len."""
    rng = np.random.default_rng([D, G, chunk, FAMILIES.index(family), int(capture), seed])
    Hkv, H, S = ATT_HKV, ATT_HKV * G, ATT_SMAX
    sc = float(F32(1.0 / math.sqrt(D) if scale is None else scale))
    lens = att_lens(chunk, capture)
    spikes = None
    if family == "spike":  # the spike token in turn at 0, 63, 64, chunk - 1, chunk and len - 1
        top = lens[-1]
        lens = [2 * chunk, top, 65, chunk + 1, 2 * chunk, top]
        spikes = [0, 63, 64, chunk - 1, chunk, top - 1]
    B = len(lens)
    q = rng.standard_normal((B, Hkv, G, D))
    k = rng.standard_normal((B, S, Hkv, D))
    v = rng.standard_normal((B, S, Hkv, D))
    base = rng.standard_normal((B, Hkv, D))
    norm2 = (base * base).sum(-1)
    if family == "census":  # uniform weights; a token missing, counted twice or shifted moves the mean by >= 1 / len
        k[:] = 0.0
        v = rng.integers(1, 9, v.shape) * rng.choice((-1.0, 1.0), v.shape)
    elif family == "spike":  # one score about 30 above the rest, for every head of the group
        q = base[:, :, None, :] + 0.3 * q
        k *= 0.5
        for b, t in enumerate(spikes):
            k[b, t] = base[b] * (30.0 / (sc * norm2[b]))[:, None]
    elif family == "rising":  # scores climb from -200 to +200 along the sequence: every tile and split raises the max
        q = base[:, :, None, :] + 0.1 * q
        target = -200.0 + 400.0 * np.arange(S) / (S - 1) + 0.5 * rng.standard_normal(S)
        k = base[:, None] * (target[None, :, None] / (sc * norm2[:, None, :]))[..., None]
    qb, kb, vb = bf16_of(q.reshape(B, H, D))[0], bf16_of(k)[0], bf16_of(v)[0]
    for b, n in enumerate(lens):
        kb[b, n:], vb[b, n:] = NAN_BITS, NAN_BITS
    return dict(D=D, G=G, chunk=chunk, family=family, lens=lens, max_len=ATT_SMAX if capture else None,
                scale=scale, sc=sc, q=qb, k=kb, v=vb)


def att_check(c, out_bits):
    D, G, chunk, sc = c["D"], c["G"], c["chunk"], c["sc"]
    worst = 0.0
    got = val(out_bits)
    tiles = -(-chunk // 64)
    for b, n in enumerate(c["lens"]):
        K, V = val(c["k"][b, :n]).astype(np.float64), val(c["v"][b, :n]).astype(np.float64)
        q = val(c["q"][b]).astype(np.float64).reshape(ATT_HKV, G, D)
        s = np.einsum("hgd,thd->hgt", q, K) * sc
        ds = (D + 8) * U * sc * np.einsum("hgd,thd->hgt", np.abs(q), np.abs(K)).max(-1)
        R = s.max(-1) - s.min(-1) + 2 * ds
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        o = np.einsum("hgt,thd->hgd", p, V)
        A = np.einsum("hgt,thd->hgd", p, np.abs(V))
        eta = ds + (tiles + 1) * (3 * R + 4) * U
        n_add = 65 * tiles + 2 * -(-n // chunk) + 8
        E = 1.01 * (2 * eta + 2 * n_add * U + 4 * U)[..., None] * A + n * 2.0 ** -123 * np.abs(V).max()
        worst = max(worst, ratio(got[b].reshape(ATT_HKV, G, D), o, E))
    return worst


ATT_SLIPS = ("tile_last_token_skipped", "acc_not_rescaled", "reduce_reads_nsplit", "scale_twice")


def att_emulate(c, slip=None):
    """k_decode_attn + k_attn_reduce in fp32: 64-token tiles, online softmax per split, partials, merge. The
    partials start as NaN, as an uninitialised workspace may."""
    D, G, chunk = c["D"], c["G"], c["chunk"]
    B, H = len(c["lens"]), ATT_HKV * G
    sc = F32(c["sc"])
    max_len = c["max_len"] or max(c["lens"])
    nsplit = max(1, -(-max_len // chunk))
    out = np.zeros((B, H, D), dtype=F32)
    with np.errstate(all="ignore"):
        for b, n in enumerate(c["lens"]):
            qf = val(c["q"][b]).reshape(ATT_HKV, G, D) * sc
            if slip == "scale_twice":
                qf = qf * sc
            K, V = val(c["k"][b]), val(c["v"][b])
            po = np.full((nsplit, ATT_HKV, G, D), np.nan, dtype=F32)
            pm, pl = np.full((nsplit, ATT_HKV, G), np.nan, dtype=F32), np.full((nsplit, ATT_HKV, G), np.nan, dtype=F32)
            for split in range(nsplit):
                start, stop = split * chunk, min(split * chunk + chunk, n)
                if start >= n:
                    continue
                m = np.full((ATT_HKV, G), -np.inf, dtype=F32)
                l, acc = np.zeros((ATT_HKV, G), dtype=F32), np.zeros((ATT_HKV, G, D), dtype=F32)
                for t0 in range(start, stop, 64):
                    nt = min(64, stop - t0)
                    if slip == "tile_last_token_skipped":
                        nt = min(nt, 63)
                    s = np.einsum("hgd,thd->hgt", qf, K[t0:t0 + nt])
                    mnew = np.maximum(m, s.max(-1))
                    p = expf(s - mnew[..., None])
                    corr = expf(m - mnew)
                    l = l * corr + p.sum(-1, dtype=F32)
                    if slip != "acc_not_rescaled":
                        acc = acc * corr[..., None]
                    acc = acc + np.einsum("hgt,thd->hgd", p, V[t0:t0 + nt])
                    m = mnew
                po[split], pm[split], pl[split] = acc, m, l
            used = nsplit if slip == "reduce_reads_nsplit" else min(nsplit, -(-n // chunk))
            M = pm[:used].max(0)
            w = expf(pm[:used] - M[None])
            L = (pl[:used] * w).sum(0, dtype=F32)
            o = (po[:used] * w[..., None]).sum(0, dtype=F32)
            out[b] = (o * (F32(1) / L)[..., None]).reshape(H, D)
    return bf16_of(np.nan_to_num(out, nan=np.inf))[0]  # a NaN must fail the check, not abort it


def att_cases(D, chunk):
    for G in (1, 2, 4, 8):
        for family in FAMILIES:
            for capture in (False, True):
                yield att_case(D, G, chunk, family, capture)
    if (D, chunk) == (64, 64):
        yield att_case(D, 2, chunk, "random", False, scale=0.05)


def _att_id(c):
    return (c["D"], c["G"], c["chunk"], c["family"], c["max_len"], c["scale"])


@pytest.mark.parametrize("D,chunk", ATT_GRID)
def test_attention_emulation_is_inside_the_bounds(D, chunk):
    for c in att_cases(D, chunk):
        assert att_check(c, att_emulate(c)) <= 1.0, _att_id(c)


@pytest.mark.parametrize("slip", ATT_SLIPS)
def test_attention_slip_breaks_a_bound(slip):
    # which family each slip must break (G = 2; D and chunk chosen so that a split holds more than one tile)
    family, capture = {"tile_last_token_skipped": ("census", False), "acc_not_rescaled": ("rising", False),
                       "reduce_reads_nsplit": ("random", True), "scale_twice": ("random", False)}[slip]
    for D, chunk in ((64, 96), (128, 256)):
        c = att_case(D, 2, chunk, family, capture)
        assert _breaks(att_check, c, att_emulate(c, slip)), (slip, D, chunk)
    if slip == "tile_last_token_skipped":  # the spike at token 63 sees it too
        c = att_case(64, 2, 96, "spike", False)
        assert _breaks(att_check, c, att_emulate(c, slip))


# ================================================================ argmax
VOCABS = (1, 7, 8, 9, 1001, 4104, 32000, 128256)
NEG_INF, NEG_ZERO = 0xFF80, 0x8000


def argmax_rows(V):
    """bf16 bit patterns [rows, V]; rows of an odd V start 2 bytes off a 4-byte boundary."""
    rng = np.random.default_rng(V)
    vec = V // 8 * 8  # [0, vec): 16-byte loads; [vec, V): the tail loop
    rows = [bf16_of(rng.standard_normal(V) * 3.0)[0] for _ in range(3)]

    def planted(*idx):
        r = bf16_of(rng.uniform(-4.0, 1.0, V))[0]
        r[list(idx)] = bf16_of(np.array([5.0]))[0][0]
        return r

    pairs = [(7, 8), (2047, 2048), (2055, 4096), (0, V - 1), (V - 1, V - 1)]
    if V > vec:
        pairs += [(vec // 2, vec), (vec - 1, V - 1)] if vec else []  # one in the vector part, one in the tail
        pairs += [(vec, V - 1), (vec + 1, V - 2)] if V - vec >= 4 else []  # both in the tail
    rows += [planted(a, b) for a, b in pairs if a < V and b < V]
    for first, second in ((NEG_ZERO, 0), (0, NEG_ZERO)):  # -0.0 and +0.0 are one maximum: the first index
        r = bf16_of(rng.uniform(-4.0, -1.0, V))[0]
        r[V // 3], r[V - 1] = first, second
        rows.append(r)
    for special in (bf16_of(np.array([-7.0]))[0][0], NAN_BITS, NEG_INF):  # -inf and one finite / one NaN / all -inf
        r = np.full(V, NEG_INF, dtype=np.uint16)
        r[(2 * V) // 3] = special
        rows.append(r)
    rows.append(np.full(V, NAN_BITS, dtype=np.uint16))
    rows.append(np.where(np.arange(V) % 2 == 0, NAN_BITS, NEG_INF).astype(np.uint16))
    r = bf16_of(rng.standard_normal(V))[0]  # NaN never wins, wherever it sits
    r[::3] = 0xFFC0
    rows.append(r)
    return np.stack(rows)


def first_maximum(bits):
    """Per row: the first index of the largest non-NaN value; 0 when nothing is above -inf."""
    x = val(bits).astype(np.float64)
    x = np.where(np.isnan(x), -np.inf, x)
    m = x.max(axis=1, keepdims=True)
    idx = np.where(x == m, np.arange(x.shape[1])[None, :], x.shape[1]).min(axis=1)
    return np.where(m[:, 0] == -np.inf, 0, idx).astype(np.int64)


def argmax_emulate(bits, slip=None):
    """k_argmax: 256 threads, each scanning its 16-byte words and then its tail entries with a strict
    comparison, then merged by (value, lower index)."""
    rows, V = bits.shape
    vv = V // 8
    i = np.arange(V)
    owner = np.where(i < vv * 8, (i // 8) % 256, (i - vv * 8) % 256)
    out = np.zeros(rows, dtype=np.int64)
    threads = [i[owner == t] for t in range(min(256, V))]  # ascending: a thread's words first, its tail after them
    for r in range(rows):
        x = val(bits[r])
        best, bi = -np.inf, 0x7FFFFFFF
        for mine in threads:
            tb, ti = -np.inf, 0x7FFFFFFF
            for j in _candidates(x, mine):
                if x[j] > tb or (slip == "last_on_ties" and x[j] == tb):
                    tb, ti = x[j], j
            if tb > best or (tb == best and (ti > bi if slip == "last_on_ties" else ti < bi)):
                best, bi = tb, ti
        out[r] = 0 if bi == 0x7FFFFFFF else bi
    return out


def _candidates(x, mine):
    """The entries of a long scan that can change its outcome: those equal to the scan's maximum."""
    v = x[mine]
    ok = ~np.isnan(v)
    return mine[ok & (v == v[ok].max())] if ok.any() else mine[:0]


@pytest.mark.parametrize("V", VOCABS)
def test_argmax_emulation_matches_the_first_maximum(V):
    bits = argmax_rows(V)
    want = first_maximum(bits)
    assert ((0 <= want) & (want < V)).all()
    assert np.array_equal(argmax_emulate(bits), want)


def test_argmax_slip_changes_an_id():
    for V in (9, 4104):
        bits = argmax_rows(V)
        assert not np.array_equal(argmax_emulate(bits, "last_on_ties"), first_maximum(bits)), V


# ================================================================ the kernels
def _dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).cuda()


def _host(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@gpu
@cuda
@pytest.mark.parametrize("hidden", HIDDENS)
def test_rmsnorm_kernel(hidden):
    worst = 0.0
    for case in rms_cases(hidden):
        name, xb, rb, wb, eps = case
        if rb is None:
            out, res_out = ops.rmsnorm(_dev(xb), _dev(wb), eps), None
        else:
            out, res_out = ops.rmsnorm(_dev(xb), _dev(wb), eps, residual=_dev(rb))
        r = rms_check(case, _host(out), _host(res_out) if res_out is not None else None)
        assert r <= 1.0, (name, r)
        worst = max(worst, r)
    print(f"rmsnorm hidden {hidden}: worst error / bound = {worst:.3f}")


@gpu
@cuda
@pytest.mark.parametrize("name", SILU_CASES)
def test_silu_mul_kernel(name):
    case = silu_case(name)
    _, gb, ub = case
    out = ops.silu_mul(_dev(np.concatenate([gb, ub], axis=1)))
    r = silu_check(case, _host(out))
    print(f"silu_mul {name}: worst error / bound = {r:.3f}")
    assert r <= 1.0


@gpu
@cuda
@pytest.mark.parametrize("heads,theta,smax", ROPE_CASES, ids=ROPE_IDS)
def test_rope_qkv_cache_kernel(heads, theta, smax):
    c = rope_case(*heads, theta, smax)
    H, Hkv, D = heads
    B = len(c["pos"])
    kc = torch.full((B, smax, Hkv, D), POISON, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    vc = kc.clone()
    q = ops.rope_qkv_cache(_dev(c["qkv"]), torch.from_numpy(c["pos"]).cuda(), kc, vc, H, Hkv, D, theta=theta)
    kh, vh = _host(kc), _host(vc)
    rows = np.arange(B)
    k_rows, v_rows = kh[rows, c["pos"]].copy(), vh[rows, c["pos"]].copy()
    kh[rows, c["pos"]], vh[rows, c["pos"]] = POISON, POISON
    assert (kh == POISON).all() and (vh == POISON).all(), "a cache element outside the appended row changed"
    r = rope_check(c, _host(q), k_rows, v_rows)
    print(f"rope_qkv_cache H{H} Hkv{Hkv} D{D} theta {theta:g} Smax {smax}: worst error / bound = {r:.3f}")
    assert r <= 1.0


def _poison_next_allocation(n_floats):
    """Fill a block of the workspace's size with NaN and release it, so that the allocator's next block of that
    size, the op's uninitialised workspace, most likely is it."""
    torch.full((n_floats,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()


@gpu
@cuda
@pytest.mark.parametrize("D,chunk", ATT_GRID)
def test_decode_attention_kernel(D, chunk):
    worst = {}
    for c in att_cases(D, chunk):
        q, k, v = _dev(c["q"]), _dev(c["k"]), _dev(c["v"])
        lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
        B, H = len(c["lens"]), ATT_HKV * c["G"]
        nsplit = max(1, -(-(c["max_len"] or max(c["lens"])) // chunk))
        _poison_next_allocation(B * H * nsplit * (D + 2))
        out = ops.decode_attention(q, k, v, lens, chunk=chunk, max_len=c["max_len"], scale=c["scale"])
        r = att_check(c, _host(out))
        assert r <= 1.0, (_att_id(c), r)
        worst[c["family"]] = max(worst.get(c["family"], 0.0), r)
    print(f"decode_attention D {D} chunk {chunk}: worst error / bound = "
          + ", ".join(f"{f} {r:.3f}" for f, r in worst.items()))


@gpu
@cuda
@pytest.mark.parametrize("V", VOCABS)
def test_argmax_kernel(V):
    bits = argmax_rows(V)
    got = ops.argmax(_dev(bits)).cpu().numpy()
    assert ((0 <= got) & (got < V)).all(), got
    assert np.array_equal(got, first_maximum(bits)), (got, first_maximum(bits))


@gpu
@cuda
def test_fused_step_with_nan_logits_returns_ids_in_range():
    # k_argmax_merge (decode_fused_kernels.h) shares the contract: an LM head of NaNs leaves no row a winner.
    from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig, TinyLlama
    cfg = LlamaConfig(vocab=512, dim=256, n_layers=1, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512, max_seq=64)
    m = TinyLlama(cfg, device="cuda", max_batch=3, seed=5)
    dec = m.fused_decoder()
    tokens = torch.tensor([3, 500, 77], dtype=torch.int64, device="cuda")
    pos = torch.tensor([0, 5, 63], dtype=torch.int32, device="cuda")
    logits = torch.zeros(3, cfg.vocab, dtype=torch.bfloat16, device="cuda")
    ids = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    dec.step(tokens, pos, logits, ids)
    torch.cuda.synchronize()
    want = first_maximum(_host(logits))
    assert np.array_equal(ids.cpu().numpy(), want) and want.any()  # the ordinary step, for contrast
    dec.weights[2].fill_(float("nan"))  # the LM head, passed to the kernel as it is
    dec.step(tokens, pos, logits, ids)
    torch.cuda.synchronize()
    assert torch.isnan(logits).all()
    assert ids.tolist() == [0, 0, 0]


@gpu
@cuda
def test_decode_attention_validates_before_launching():
    bf = torch.bfloat16
    q = torch.ones(2, 4, 64, dtype=bf, device="cuda")
    kc = torch.ones(2, 128, 2, 64, dtype=bf, device="cuda")
    lens = torch.tensor([5, 128], dtype=torch.int32, device="cuda")
    for chunk in (0, -1, -64):
        with pytest.raises(ValueError):
            ops.decode_attention(q, kc, kc, lens, chunk=chunk)
    bad = [
        (q.float(), kc, kc, lens, {}), (q, kc.float(), kc, lens, {}), (q, kc, kc, lens.long(), {}),   # dtypes
        (q.cpu(), kc, kc, lens, {}), (q, kc, kc.cpu(), lens, {}),                                     # devices
        (q, kc[:, ::2], kc[:, ::2], lens, {}),                                                        # contiguity
        (q, kc, kc[:, :64].contiguous(), lens, {}), (q, kc[:1].contiguous(), kc[:1].contiguous(), lens, {}),
        (torch.ones(2, 4, 32, dtype=bf, device="cuda"), torch.ones(2, 128, 2, 32, dtype=bf, device="cuda"),
         torch.ones(2, 128, 2, 32, dtype=bf, device="cuda"), lens, {}),                               # D in (64, 128)
        (torch.ones(2, 3, 64, dtype=bf, device="cuda"), kc, kc, lens, {}),                            # H % Hkv
        (torch.ones(2, 18, 64, dtype=bf, device="cuda"), kc, kc, lens, {}),                           # G <= 8
        (q, kc, kc, lens[:1], {}),                                                                    # lens [B]
        (q, kc, kc, torch.tensor([0, 5], dtype=torch.int32, device="cuda"), {}),                      # len >= 1
        (q, kc, kc, lens, {"max_len": 129}),                                                          # capacity
    ]
    for n, (qq, kk, vv, ll, kw) in enumerate(bad):
        with pytest.raises((TypeError, ValueError)):
            ops.decode_attention(qq, kk, vv, ll, **kw)
            pytest.fail(f"bad call {n} was launched")
    out = ops.decode_attention(q, kc, kc, lens)  # and the good call does run: V is all ones
    assert (out.float() == 1.0).all()
