"""NumPy emulation of ``ops.guide_`` (guide.hip), bit for bit: the kernel makes
no rounding decision, so the emulation is the expected result and the tests
compare with equality. bf16 values travel as their uint16 bits."""
from __future__ import annotations

import numpy as np

NEG_INF = 0xFF80  # bf16 -inf


def bf16_argmax(bits: np.ndarray) -> int:
    """``k_argmax_merge``'s rules on a row of bf16 bits: the lowest id of the
    largest value, NaN never wins, 0 when nothing lies above -inf."""
    v = (bits.astype(np.uint32) << 16).view(np.float32).copy()
    v[np.isnan(v)] = -np.inf
    return int(np.argmax(v)) if v.max() > -np.inf else 0


def guide(x, ids, tok, dec, slot, base, cur, arena):
    """One launch over the B rows of ``x`` (uint16 [B, V]). Returns (work
    uint16 [B, V], ids int64 [B], cur int32 [n_slots]); nothing is changed in
    place. ``dec`` and ``slot`` may be longer than B."""
    x = np.asarray(x, dtype=np.uint16)
    B, V = x.shape
    n_slots, n_states = len(base), arena.shape[0]
    work, ids, cur = x.copy(), np.asarray(ids, dtype=np.int64).copy(), np.asarray(cur, dtype=np.int32).copy()
    for r in range(B):
        s = int(slot[r])
        if not 0 <= s < n_slots:
            continue
        b, c = int(base[s]), int(cur[s])
        if b < 0 or c < 0 or b >= n_states or c >= n_states - b:
            continue
        t = int(tok[r])
        if dec[r] != 0 and 0 <= t < V:
            to = int(arena[b + c, t])
            if 0 <= to < n_states - b:
                c = to
                cur[s] = c
        work[r] = np.where(arena[b + c] >= 0, x[r], NEG_INF).astype(np.uint16)
        ids[r] = bf16_argmax(work[r])
    return work, ids, cur
