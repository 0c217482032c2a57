"""Host references for ``ops.penalize_`` (penalty.hip), NumPy only.

``emulate``   the kernel's arithmetic in fp32, operation by operation, with
              its bf16 stores and its bookkeeping of ``state``: what the kernel
              is meant to produce, bit for bit.
``exact``     the same rules in fp64 from the exact bf16 inputs, with a
              per-element error bound for a bf16 result (see ``exact``).

Both take plain arrays: ``logits`` uint16 [B, V] (bf16 bits), ``tok`` / ``dec`` /
``slot`` int [B], ``params`` a list of (repetition, frequency, presence, on) per
row, ``state`` int32 [n_slots, V] and ``bias`` {slot: [(id, value), ...]}.
"""
from __future__ import annotations

import numpy as np

COUNT_MASK = 0x3FFFFFFF
PROMPT_BIT = 0x40000000


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16(x: np.ndarray) -> np.ndarray:
    """Round to nearest even; NaN becomes 0x7fc0 (``f2bf_bits`` in bf16_common.h)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u + (0x7FFF + ((u >> 16) & 1))) >> 16).astype(np.uint16)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, np.uint16(0x7FC0), r)


def argmax_rule(bits: np.ndarray) -> int:
    """``k_argmax_merge``'s rules on a bf16 row: the lowest id of the largest
    value above -inf; NaN never wins; 0 without a winner."""
    with np.errstate(invalid="ignore"):  # signalling NaN payloads
        v = bf16_to_f32(bits).astype(np.float64)
    v[np.isnan(v)] = -np.inf
    m = v.max()
    return int(np.argmax(v == m)) if m > -np.inf else 0


def _counts(row_state, tok, dec, V):
    """(count with the decode row's token folded in, prompt bit, the state row to write back)."""
    st = row_state.astype(np.int64)
    cnt = st & COUNT_MASK
    new = row_state.copy()
    if dec and 0 <= tok < V and cnt[tok] < COUNT_MASK:
        cnt[tok] += 1
        new[tok] += 1
    return cnt, (st & PROMPT_BIT) != 0, new


def emulate(logits, ids, tok, dec, slot, params, state, bias):
    """Returns (work bits [B, V], ids [B]); ``state`` is updated in place."""
    B, V = logits.shape
    work, ids = logits.copy(), np.array(ids, dtype=np.int64)
    with np.errstate(all="ignore"):
        for r in range(B):
            rep, freq, pres, on = params[r]
            if not on or not 0 <= slot[r] < state.shape[0]:
                continue
            s = int(slot[r])
            cnt, prompt, state[s] = _counts(state[s], int(tok[r]), bool(dec[r]), V)
            x = bf16_to_f32(logits[r])
            seen = ((cnt > 0) | prompt) & ~np.isnan(x)
            f = np.float32
            y = np.where(x > 0, x / f(rep), x * f(rep)).astype(f)
            y = (y - (f(freq) * cnt.astype(f)).astype(f)).astype(f)
            y = np.where(cnt > 0, (y - f(pres)).astype(f), y)
            work[r] = np.where(seen, f32_to_bf16(y), logits[r])
            for tid, val in bias.get(s, ())[:300]:
                if 0 <= tid < V:
                    work[r, tid] = f32_to_bf16(bf16_to_f32(work[r, tid:tid + 1]) + f(val))[0]
            ids[r] = argmax_rule(work[r])
    return work, ids


def half_ulp_bf16(mag: np.ndarray) -> np.ndarray:
    """Half a bf16 ulp (8 significant bits) at magnitude ``mag`` (fp64, >= 0; normal range)."""
    e = np.floor(np.log2(np.maximum(mag, 2.0 ** -126)))
    return 2.0 ** (e - 8)


def exact(logits, tok, dec, slot, params, state, bias):
    """fp64 from the exact bf16 inputs; ``state`` is not modified. Returns (ref
    [B, V] fp64, bound [B, V], touched [B, V] bool, expected state).

    The bound for a touched element with exact result e: the kernel makes one
    fp32 division or product, one product freq * count and up to two
    subtractions, each correctly rounded, so its fp32 value is within
    err32 = 4 * 2^-24 * (|x / rep or x * rep| + |freq * count| + |pres|) of e
    (every intermediate is at most that sum), and the bf16 store adds at most
    half a bf16 ulp at that value: b1 = err32 + half_ulp(|e| + err32). A biased
    element is stored a second time, from the fp32 sum of the first stored value
    and the bias: with m = |e + bias| + b1, b2 = b1 + 2^-24 * m +
    half_ulp(m * (1 + 2^-24)). Nothing is scaled by a row or tensor maximum.
    Elements no rule touches (rows that are off, ids never seen and not biased)
    have bound 0: they are copied bit for bit."""
    B, V = logits.shape
    with np.errstate(invalid="ignore"):
        x = bf16_to_f32(logits).astype(np.float64)
    ref, bound, touched = x.copy(), np.zeros((B, V)), np.zeros((B, V), dtype=bool)
    new_state = state.copy()
    u = 2.0 ** -24
    with np.errstate(all="ignore"):
        for r in range(B):
            rep, freq, pres, on = params[r]
            if not on or not 0 <= slot[r] < state.shape[0]:
                continue
            s = int(slot[r])
            cnt, prompt, new_state[s] = _counts(state[s], int(tok[r]), bool(dec[r]), V)
            rep, freq, pres = (float(np.float32(v)) for v in (rep, freq, pres))
            seen = ((cnt > 0) | prompt) & ~np.isnan(x[r])
            a = np.where(x[r] > 0, x[r] / rep, x[r] * rep)
            e = a - freq * cnt - pres * (cnt > 0)
            err32 = 4 * u * (np.abs(a) + np.abs(freq * cnt) + abs(pres) * (cnt > 0))
            b1 = err32 + half_ulp_bf16(np.abs(e) + err32)
            ref[r] = np.where(seen, e, x[r])
            bound[r] = np.where(seen, b1, 0.0)
            touched[r] = seen
            for tid, val in bias.get(s, ())[:300]:
                if 0 <= tid < V:
                    val = float(np.float32(val))
                    ref[r, tid] += val
                    m = abs(ref[r, tid]) + bound[r, tid]
                    bound[r, tid] += u * m + half_ulp_bf16(np.float64(m * (1 + u)))
                    touched[r, tid] = True
    return ref, bound, touched, new_state


def check(work_bits, logits, ref, bound, touched):
    """Worst excess over the bound of a bf16 result against ``exact``'s
    reference (<= 0 passes), with untouched elements, NaN and infinities held
    to equality (an excess of inf where they differ)."""
    with np.errstate(invalid="ignore"):
        got = bf16_to_f32(work_bits).astype(np.float64)
    if not np.array_equal(work_bits[~touched], logits[~touched]):
        return np.inf
    t = touched
    fin = t & np.isfinite(ref)
    with np.errstate(all="ignore"):
        if not np.array_equal(np.isnan(got[t]), np.isnan(ref[t])):
            return np.inf
        inf = t & np.isinf(ref)
        if not np.array_equal(got[inf], ref[inf]):
            return np.inf
        if not fin.any():
            return 0.0
        return float(np.nanmax(np.where(fin, np.abs(got - ref) - bound, -np.inf)))
