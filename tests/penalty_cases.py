"""Inputs shared by test_penalty_params.py (the NumPy emulation of
``ops.penalize_`` on the CPU) and test_gpu_penalty.py (the kernel): one call of
the op over B rows of a V-wide vocabulary, from a seed.

A case mixes, over its rows: rows that are on (at most 12, row 0 and the last
row among them, each with a slot of its own) and off; a row flagged on whose
slot lies outside ``state`` (it must behave as off); repetition below and above
1 on positive and negative logits; negative and positive frequency and presence;
counts of 0, 1, a few, and 40000; the prompt bit alone and with a count; decode
rows whose token is unseen, seen, or biased, and prompt rows (which count
nothing); -inf, NaN (with payloads) and signed zeros among the logits; bias lists
of 0, 3, 300 (or V // 2) and 2 entries, on untouched ids, on penalised ids and on
the decode token. The slots no row owns hold a poison pattern."""
import numpy as np

from p2p_llm_tunnel_amd.utils.penalty_ref import f32_to_bf16

POISON = 0x2BADF00D
REPS = (1.0, 0.7, 1.3, 2.5)
FREQS = (0.0, 0.5, -0.7, 2.0)
PRESS = (0.0, 0.3, -1.5)


def make_case(B: int, V: int, seed: int) -> dict:
    rng = np.random.default_rng(seed)
    n_on = min(B, 12)
    n_slots = n_on + 3
    logits = f32_to_bf16((rng.standard_normal((B, V)) * 4).astype(np.float32))
    k = max(1, V // 200)
    for r in range(B):
        idx = rng.choice(V, 3 * k, replace=False)
        logits[r, idx[:k]] = 0xFF80  # -inf
        logits[r, idx[k:2 * k]] = rng.choice(np.array([0x7FC1, 0xFFC0, 0x7F81], dtype=np.uint16), k)  # NaN
        logits[r, idx[2 * k:]] = rng.choice(np.array([0x8000, 0x0000], dtype=np.uint16), k)  # -0.0, +0.0
    on_rows = {0, B - 1}
    while len(on_rows) < n_on:
        on_rows.add(int(rng.integers(B)))
    on_rows = sorted(on_rows)
    slots_on = rng.permutation(n_on)
    state = np.full((n_slots, V), POISON, dtype=np.int32)
    ids = rng.integers(0, V, B).astype(np.int64)
    tok = rng.integers(0, V, B).astype(np.int64)
    dec = rng.integers(0, 2, B).astype(np.int64)
    slot = rng.integers(-2, n_slots + 2, B).astype(np.int64)
    params = [(float(rng.choice(REPS)), float(rng.choice(FREQS)), float(rng.choice(PRESS)), 0) for _ in range(B)]
    bias = {}
    for j, r in enumerate(on_rows):
        s = int(slots_on[j])
        slot[r] = s
        st = np.zeros(V, dtype=np.int32)
        perm = rng.permutation(V)
        a, b, c, d, e = (max(1, V // n) for n in (8, 16, 32, 8, 16))
        o = 0
        st[perm[o:o + a]] = 1; o += a
        st[perm[o:o + b]] = rng.integers(2, 50, b); o += b
        st[perm[o:o + c]] = 40000; o += c
        st[perm[o:o + d]] = 0x40000000; o += d
        st[perm[o:o + e]] = 0x40000000 + rng.integers(1, 9, e); o += e
        unseen = perm[o:]
        state[s] = st
        params[r] = (REPS[j % 4], FREQS[(j // 2) % 4], PRESS[j % 3], 1)
        dec[r] = j % 3 != 2  # two decode rows, then a prompt row
        tok[r] = (int(unseen[0]), int(perm[0]), int(perm[a + b]))[j % 3]  # unseen / count 1 / count 40000
        kind = j % 4
        if kind == 1:  # an untouched id, a penalised id, the decode token
            bias[s] = [(int(unseen[1]), 3.25), (int(perm[1]), -7.5), (int(tok[r]), 1.125)]
        elif kind == 2:
            n = min(300, V // 2)
            picks = rng.choice(V, n, replace=False)
            bias[s] = [(int(t), float(v)) for t, v in zip(picks, rng.uniform(-100, 100, n).astype(np.float32))]
        elif kind == 3:
            bias[s] = [(int(unseen[2]), 100.0), (int(perm[2]), -100.0)]
    off = [r for r in range(B) if r not in on_rows]
    if off:  # flagged on, but its slot is outside state: behaves as off
        rep, freq, pres, _ = params[off[0]]
        params[off[0]] = (rep, freq, pres, 1)
        slot[off[0]] = n_slots + 1
    return {"B": B, "V": V, "logits": logits, "ids": ids, "tok": tok, "dec": dec, "slot": slot, "params": params,
            "state": state, "bias": bias, "on_rows": on_rows, "n_slots": n_slots}
