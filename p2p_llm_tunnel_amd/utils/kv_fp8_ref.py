"""Host reference for the FP8 KV cache's store (``f32_to_e4m3x2`` in decode_fused_kernels.h), NumPy only.

The format is OCP ``e4m3fn`` at scale 1: 1 sign, 4 exponent (bias 7) and 3
mantissa bits; no infinities; 0x7f and 0xff are NaN; the largest finite value
is 448 (0x7e); subnormals are the multiples of 2^-9 below 2^-6.

``encode``    an fp32 value to its byte the way the kernels store it: finite
              values clamped to [-448, 448], then ONE rounding to nearest-even
              (subnormals included; half the smallest subnormal, 2^-10, ties to
              zero, and the sign of a value that rounds to zero is kept). NaN
              becomes 0x7f | sign.
``decode``    a byte to its fp32 value (exact: every e4m3 value is an fp32 value).
``boundaries``  the rounding boundaries of the format (midpoints of neighbouring
              values), for tests that ask which inputs a bound decides.
``half_ulp``  the issue's hu: half the e4m3 spacing at a magnitude.

With per-head scales (``models/kv_scales.py``) the byte of head h is ``encode(x * fp32(1 / s[h]))``
(``encode_scaled``: the reciprocal once, the product rounded to fp32 as the kernel's multiply rounds it, then the one
rounding to e4m3) and the value it stands for is ``decode(byte) * s[h]`` (``decode_scaled``). ``attend`` is the
scaled read as ``k_attn<D, G, true>`` does it, in fp32: the bytes themselves enter the dot products, K's scale joins
the score scale and V's the final normalisation, at the single-slot exit or in the cross-slot merge.

Everything in ``encode`` is integer arithmetic on the fp32 bit pattern: no library cast
decides a rounding here.
"""
from __future__ import annotations

import numpy as np

MAX = 448.0  # the largest finite e4m3fn value (0x7e)
NAN = 0x7F  # | sign
MIN_NORMAL = 2.0 ** -6
MIN_SUBNORMAL = 2.0 ** -9


def clamp(x: np.ndarray) -> np.ndarray:
    """Finite values to [-448, 448]; NaN passes (``e4m3_clamp``). +-inf is clamped like any value beyond 448."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), x, np.minimum(np.maximum(x, np.float32(-MAX)), np.float32(MAX))).astype(np.float32)


def encode(x: np.ndarray) -> np.ndarray:
    """fp32 -> e4m3fn bytes (uint8): clamp, then one round-to-nearest-even."""
    x = clamp(x)
    u = np.ascontiguousarray(x).view(np.uint32).astype(np.int64)
    sign = ((u >> 24) & 0x80).astype(np.uint8)
    mag = u & 0x7FFFFFFF
    exp = (mag >> 23) - 127  # unbiased fp32 exponent (-127: fp32 zero / subnormal, far below 2^-10)
    man = (mag & 0x7FFFFF) | 0x800000  # 24-bit significand: value = man * 2^(exp - 23)

    # The result as an integer count q of e4m3 steps at the value's own scale. Normal range (exp >= -6): steps of
    # 2^(exp - 3), so q = man >> 20 rounded, in [8, 16]; below it: steps of 2^-9 whatever the exponent, so the
    # shift grows by -6 - exp and q lands in [0, 8].
    shift = 20 + np.clip(-6 - exp, 0, 40)
    q = man >> shift
    rem = man & ((np.int64(1) << shift) - 1)
    half = np.int64(1) << (shift - 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    # Byte: normal inputs carry the implicit one in q (8..16 -> exponent field + mantissa, a carry to 16 moves up
    # one exponent by plain addition); subnormal inputs have q = 0..8 and q == 8 is the smallest normal, again by
    # plain addition.
    e_field = np.clip(exp + 7, 0, None)
    normal = exp >= -6
    byte = np.where(normal, (e_field << 3) + (q - 8), q)
    byte = np.where(exp < -40, 0, byte)  # fp32 zero, subnormals and anything a 40-bit shift no longer holds
    out = (byte.astype(np.uint8) & 0x7F) | sign
    return np.where(np.isnan(x), np.uint8(NAN) | sign, out).astype(np.uint8)


def decode(b: np.ndarray) -> np.ndarray:
    """e4m3fn bytes -> fp32 (0x7f / 0xff: NaN)."""
    b = np.asarray(b, dtype=np.uint8).astype(np.int32)
    e, m = (b >> 3) & 0xF, b & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (8 + m) * np.exp2((e - 10).astype(np.float64)))
    mag = np.where((b & 0x7F) == 0x7F, np.nan, mag)
    return np.where(b & 0x80, -mag, mag).astype(np.float32)


def values() -> np.ndarray:
    """The 127 non-negative finite values, ascending (fp64)."""
    return decode(np.arange(0x7F, dtype=np.uint8)).astype(np.float64)


def boundaries() -> np.ndarray:
    """The 126 positive rounding boundaries: midpoints of neighbouring non-negative values (fp64, exact)."""
    v = values()
    return (v[:-1] + v[1:]) / 2


def half_ulp(a: np.ndarray) -> np.ndarray:
    """Half the e4m3 spacing at magnitude a (fp64): 2^(floor(log2 a) - 4) for a >= 2^-6, 2^-10 below."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    _, e = np.frexp(np.maximum(a, MIN_NORMAL))  # a = m 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    return np.ldexp(1.0, e - 1 - 4)


def boundary_distance(x: np.ndarray) -> np.ndarray:
    """Distance of |clamp(x)| from the nearest rounding boundary (fp64). Beyond 448 nothing is left to decide:
    the distance is taken from the clamped value, and 448 lies 16 above the last boundary."""
    a = np.minimum(np.abs(np.asarray(x, dtype=np.float64)), MAX)
    b = boundaries()
    i = np.clip(np.searchsorted(b, a), 1, len(b) - 1)
    return np.minimum(np.abs(a - b[i - 1]), np.abs(a - b[i]))


# ---------------------------------------------------------------- per-head scales
def recip(s) -> np.ndarray:
    """fp32(1 / s): what the host computes once and the writers multiply by."""
    return (np.float32(1.0) / np.asarray(s, dtype=np.float32)).astype(np.float32)


def encode_scaled(x: np.ndarray, s) -> np.ndarray:
    """Rows ``x`` [..., Hkv, D] (fp32) to bytes under the head scales ``s`` [Hkv]: encode(x * fp32(1 / s))."""
    x = np.asarray(x, dtype=np.float32)
    return encode((x * recip(s)[..., :, None]).astype(np.float32))


def decode_scaled(b: np.ndarray, s) -> np.ndarray:
    """Bytes [..., Hkv, D] to the values they stand for under the head scales ``s`` [Hkv] (fp64)."""
    return decode(b).astype(np.float64) * np.asarray(s, dtype=np.float64)[..., :, None]


def attend(q: np.ndarray, kb: np.ndarray, vb: np.ndarray, k_scale: float, v_scale: float, slots: int = 1,
           span: int = 64) -> np.ndarray:
    """One KV head's attention as ``k_attn<D, G, true>`` computes it, in fp32: ``q`` [G, D] (bf16 values), ``kb`` /
    ``vb`` [T, D] bytes of that head, its two scales. The tokens are cut into ``slots`` spans of ``span``; each
    span's running maximum, sum and unnormalised output are kept, and with one span the exit is o * (v_scale / L),
    with several the merge rescales the partials and ends with the same expression. Returns fp32 [G, D]."""
    f = np.float32
    D = q.shape[1]
    sc = f(f(1.0) / np.sqrt(f(D))) * f(k_scale)  # K's scale joins the score scale, once
    k, v = decode(kb).astype(f), decode(vb).astype(f)
    T = k.shape[0]
    nact = max(1, min(slots, -(-T // span)))
    parts = []
    for i in range(nact):
        lo, hi = i * span, T if i == nact - 1 else min(T, (i + 1) * span)
        s = (q.astype(f) @ k[lo:hi].T).astype(f) * sc
        m = s.max(1, keepdims=True)
        p = np.exp(s - m).astype(f)
        parts.append((m[:, 0], p.sum(1, dtype=f), (p @ v[lo:hi]).astype(f)))
    if nact == 1:  # the single-slot exit
        m, l, o = parts[0]
        return (o * (f(v_scale) / l)[:, None]).astype(f)
    M = np.max([m for m, _, _ in parts], axis=0)
    L = np.zeros_like(M)
    o = np.zeros_like(parts[0][2])
    for m, l, po in parts:  # the cross-slot merge
        w = np.exp(m - M).astype(f)
        L += l * w
        o += w[:, None] * po
    return (o * (f(v_scale) / L)[:, None]).astype(f)
