"""Shared inputs of the guided-decoding tests (CPU and GPU): a synthetic
vocabulary, brute-force references of the compiler's outputs and random cases
for ``ops.guide_``."""
import numpy as np

from p2p_llm_tunnel_amd.utils import guide_ref

MERGES = [b"yes", b"no", b"may", b"be", b"ye", b"s", b"00", b"12", b"-1", b".5", b"345", b"67-8", b"9.", b"0.25",
          "é".encode(), "日本".encode(), b"\xe6\x97", b"\xa5x", b" the", b"ab", b"abc", b"bca", b"\n\n"]
N_CONTROL = 4


def synthetic_vocab(V: int | None = None):
    """(token_bytes, eos_ids): 256 single bytes, the merges above, four control
    tokens without bytes, two EOS ids, then control tokens up to ``V``."""
    tb = [bytes([i]) for i in range(256)] + list(MERGES) + [b""] * N_CONTROL
    eos = [len(tb), len(tb) + 1]
    tb += [b"", b""]
    if V is not None:
        assert V >= len(tb)
        tb += [b""] * (V - len(tb))
    return tb, eos


def brute_table(guide, token_bytes, eos_ids):
    """The token table by walking every token's bytes one by one through the
    guide's byte DFA, breadth first from the start (the order ``token_table``
    numbers its states in is part of what this checks)."""
    V = len(token_bytes)
    order, index, rows = [0], {0: 0}, []
    i = 0
    while i < len(order):
        s0 = order[i]
        i += 1
        row = [-1] * V
        for t, data in enumerate(token_bytes):
            if not data or t in eos_ids:
                continue
            s = s0
            for b in data:
                s = int(guide.dfa[s, b])
                if s < 0:
                    break
            row[t] = s
        for t in sorted({s for s in row if s >= 0}):
            if t not in index:
                index[t] = len(order)
                order.append(t)
        rows.append(row)
    out = np.array([[index[s] if s >= 0 else -1 for s in row] for row in rows], dtype=np.int16)
    for k, s in enumerate(order):
        if guide.dfa_accept[s]:
            out[k, list(eos_ids)] = k
    return out, np.array([bool(guide.dfa_accept[s]) for s in order])


def completion(tokens, token_bytes, eos_ids):
    """(the bytes of ``tokens`` up to the first EOS id, whether one was found)."""
    out = b""
    for t in tokens:
        if t in eos_ids:
            return out, True
        out += token_bytes[t]
    return out, False


def bf16_bits(a: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bits by truncation (test inputs only: any bits do)."""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def random_case(R: int, V: int, seed: int, n_slots: int = 70, arena_states: int = 96):
    """Inputs of one ``guide_`` launch that touch every branch: tables of 1..40
    states at different arena bases, rows that are off (no table, slot out of
    range, state outside the arena), rows with and without the advance flag, an
    input token whose transition is -1, a state that allows a single token,
    ties at the maximum across the 8-element and per-thread seams, -inf and NaN
    in the logits. Rows that are on have slots of their own. Returns a dict of
    NumPy arrays; ``want`` holds the emulation's (work, ids, cur)."""
    rng = np.random.default_rng(seed)
    arena = rng.integers(-1, 0, size=(arena_states, V), dtype=np.int16)  # all -1
    tables, at = [], 0
    while at < arena_states - 1 and len(tables) < 6:
        n = int(rng.integers(1, 41))
        n = min(n, arena_states - at)
        t = rng.integers(0, n, size=(n, V)).astype(np.int16)
        t[rng.random((n, V)) < 0.6] = -1
        t[0, :] = -1
        t[0, int(rng.integers(0, V))] = n - 1  # state 0 allows a single token
        arena[at:at + n] = t
        tables.append((at, n))
        at += n + int(rng.integers(0, 3))
    arena[arena_states - 1, ::3] = 5  # a stray row whose entries point outside the arena
    base = np.full(n_slots, -1, dtype=np.int32)
    cur = np.zeros(n_slots, dtype=np.int32)
    slots = rng.permutation(n_slots - 1)[:R]  # distinct; the last slot never has a row
    slot = np.concatenate([slots, rng.integers(0, n_slots, size=4)]).astype(np.int64)
    dec = rng.integers(0, 2, size=R + 4).astype(np.int64)
    tok = rng.integers(0, V, size=R).astype(np.int64)
    x = bf16_bits(rng.standard_normal((R, V)) * 4)
    for r in range(R):
        s = int(slot[r])
        mode = r % 8
        if mode == 1:
            continue  # off: no table
        b, n = tables[r % len(tables)]
        base[s] = b
        cur[s] = int(rng.integers(0, n))
        if mode == 2:
            slot[r] = n_slots + 3 if r % 16 == 2 else -1  # off: slot out of range
        elif mode == 3:
            base[s], cur[s] = arena_states - 1, 1  # off: base + cur outside the arena
        elif mode == 4:  # the input token's transition is -1: the state stands
            dec[r] = 1
            arena[b + cur[s], tok[r]] = -1
        elif mode == 5:  # a single allowed token, and the advance lands there
            dec[r] = 1
            arena[b + cur[s], tok[r]] = 0
        elif mode == 6:  # ties at the maximum across seams, all allowed
            dec[r] = 0
            arena[b + cur[s]] = np.where(arena[b + cur[s]] < 0, 0, arena[b + cur[s]])
            x[r, :] = bf16_bits(np.float32([-1.0]))[0]
            for i in (7, 8, 1023 * 8 + 7, 1024 * 8, V - 1):
                if 0 <= i < V:
                    x[r, i] = 0x4110  # 9.0
            arena[b + cur[s], 7 % V] = -1  # the first of the equals is masked
        elif mode == 7:  # -inf and NaN already there
            x[r, ::5] = 0xFF80
            x[r, 1::7] = 0x7FC0
            x[r, 2::11] = 0xFFC1
    base[n_slots - 1], cur[n_slots - 1] = tables[0][0], 0  # a guided slot without a row: must not change
    ids = rng.integers(0, V, size=R).astype(np.int64)
    case = dict(x=x, ids=ids, tok=tok, dec=dec, slot=slot, base=base, cur=cur, arena=arena)
    case["want"] = guide_ref.guide(x, ids, tok, dec, slot, base, cur, arena)
    return case


def ref_generate(model, prompt, guide, n_new, forced=None):
    """Greedy fp32 reference generation under ``guide`` (None: unguided): the
    model's ``reference_logits`` masked with the guide's table, the state
    advanced on the host. Returns (tokens, the smallest gap between the two
    largest allowed logits over max|logit|, at any step)."""
    import math
    import torch
    seq, out, state, worst = list(prompt), [], 0, math.inf
    for k in range(n_new):
        lg = model.reference_logits(torch.tensor([seq]))[0].double()
        x = lg.clone()
        if guide is not None:
            x[torch.from_numpy(guide.next[state] < 0)] = -math.inf
        top = x.topk(2).values
        if top[1] > -math.inf:
            worst = min(worst, float(top[0] - top[1]) / float(lg.abs().max()))
        t = int(x.argmax()) if forced is None else forced[k]
        out.append(t)
        seq.append(t)
        if guide is not None:
            state = int(guide.next[state, t])
            assert state >= 0
    return out, worst
