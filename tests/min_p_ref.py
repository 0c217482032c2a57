"""Host replay of the sampler's ``MINP`` instantiation (ops.sample_minp_, sample.hip), and the cases the min_p
tests share. The replay of temperature, top-k, top-p and the Gumbel-max is tests/test_gpu_sample.py's, imported
and not changed; this module adds the third cut:

* ``lnp`` = the float32 whose bits are params row 5 (the host's ln(min_p), fp64 rounded once); -inf: no cut;
* ``t = fl32(m + lnp)``, m the largest ``z_i = fl32(logit_i * fl32(1 / T))`` of the row;
* token i stays iff ``okey(z_i) >= okey(t)`` (the kernel's order-preserving keys, so that -0.0 < +0.0 here as
  there), and the kept set is top-k's, top-p's and this one's intersection: the final cut is the largest of three.

Every step is one exact IEEE operation on both sides, so unlike the top-p cut this one has no band: a draw that
top-p leaves decided stays decided.
"""
import functools
import math
from dataclasses import dataclass

import numpy as np

from p2p_llm_tunnel_amd import ops
from tests.test_gpu_sample import (KINDS, M64, Draw, _f32, _pick, _row_np, _seed, _ctr, _top_p_cuts, gumbel64)

MINP_VARIANTS = ("linear", "logit_max", "strict", "row4", "skip_with_top_p", "min_combine")
NOTHING = Draw(-1, frozenset([-1]))  # the kept set is empty: the kernel leaves ids[row] alone


def okey(x) -> np.ndarray:
    """sample.hip's order-preserving float32 -> uint32 key."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def replay_minp(logits: np.ndarray, col, variant: str | None = None) -> Draw:
    """One draw of the MINP sampler: ``logits`` the row as float32 (exact bf16 values), ``col`` the six int64 the
    kernel reads. ``variant``: one of ``MINP_VARIANTS``, a one-line slip of the min_p cut."""
    V = len(logits)
    T = _f32(col[0])
    if not T >= np.float32(1e-4):
        return Draw(None)
    k, p = int(col[1]), _f32(col[2])
    seed, ctr = int(col[3]) & M64, int(col[4]) & M64
    if k <= 0 or k > V:
        k = V
    p_on = bool(p > 0 and p < 1)
    with np.errstate(over="ignore"):
        z = logits * (np.float32(1.0) / T)  # float32
    ninf = np.float32(-np.inf)
    kcut = np.partition(z, V - k)[V - k] if k < V else ninf
    keep = z >= kcut
    pcuts = [ninf]
    if p_on:
        pcuts, _, _ = _top_p_cuts(z, keep, p, V, z, band=True)  # the mass over the top-k set, min_p or not
    lnp = _f32(col[4] if variant == "row4" else col[5])
    minp_on = bool(lnp != ninf) and not (variant == "skip_with_top_p" and p_on)
    t = ninf
    if minp_on:
        m = np.fmax.reduce(logits if variant == "logit_max" else z)  # fmaxf: NaN never the maximum
        with np.errstate(invalid="ignore", over="ignore"):
            add = np.float32(np.exp(np.float64(lnp))) if variant == "linear" else lnp
            t = np.float32(np.float32(m) + np.float32(add))

    def kept(pcut):
        if variant == "min_combine":  # a cut that is off is the key 0: the smallest of the three keeps everything
            low = min(float(kcut), float(pcut), float(t))
            return np.flatnonzero(z >= np.float32(low))
        over = okey(z) > okey(t) if variant == "strict" else okey(z) >= okey(t)
        return np.flatnonzero(keep & (z >= pcut) & (over if minp_on else True))

    sets = [kept(c) for c in ((min(pcuts), max(pcuts)) if len(pcuts) > 1 else pcuts)]
    if any(len(s) == 0 for s in sets):
        return NOTHING
    results = [_pick(z, s, seed, ctr, None) for s in sets]
    if len(pcuts) > 1:
        w_lo, P_lo = results[0]
        if all(i in set(sets[1].tolist()) for i in P_lo):  # the best of the largest set lies in every smaller one
            return Draw(w_lo, P_lo)
        every = [_pick(z, kept(c), seed, ctr, None) for c in pcuts]
        return Draw(every[0][0], frozenset().union(*(P for _, P in every)))
    return Draw(*results[0])


# ---------------------------------------------------------------- cases
@dataclass(frozen=True)
class MinPCase:
    name: str
    V: int
    rows: tuple  # row -> float32 numpy row (exact bf16 values)
    block: tuple  # the params block: 6 tuples of ld ints
    planted: bool = False  # built around one cut: every draw is decided
    tags: tuple = ()  # planted rows: which cut each row was built for

    @property
    def B(self):
        return len(self.rows)

    @property
    def ld(self):
        return len(self.block[0])

    def col(self, row: int):
        return tuple(line[row] for line in self.block)


LD = 80
T_LIST = (0.5, 1.0, 2.0)
MIN_P_LIST = (0.0, 1e-6, 0.05, 0.5, 1.0)


def _block(cols, ld=LD):
    """Columns -> the [6, ld] block; the columns past the rows look live (T = 1, top-1, min_p = 1), so that a
    kernel that strides by B instead of ld reads other values."""
    cols = list(cols) + [ops.pack_sampling(1.0, 1, 1.0, 0x5EED0000 + c, c, 1.0) for c in range(len(cols), ld)]
    return tuple(zip(*cols))


@functools.lru_cache(maxsize=None)
def rows_case(V: int, B: int = 64) -> MinPCase:
    """B rows at vocabulary V, ld = 80: every row kind against every T, min_p, and top-k / top-p on and off; every
    ninth row greedy (T = 0)."""
    k_list = (0, 0, 5, 50, V + 1)
    p_list = (1.0, 0.9, 1.0, 0.5)
    rows, cols = [], []
    for r in range(B):
        j = r // 8
        rows.append(_row_np(KINDS[r % 8], V))
        T = 0.0 if r % 9 == 4 else T_LIST[(r + j) % 3]
        cols.append(ops.pack_sampling(T, k_list[(r + 2 * j) % 5], p_list[(r + j) % 4], _seed(r), _ctr(r),
                                      MIN_P_LIST[(r + 3 * j) % 5]))
    return MinPCase(f"rows-V{V}-B{B}", V, tuple(rows), _block(cols))


def _bf16(x: np.ndarray) -> np.ndarray:
    import torch
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


@functools.lru_cache(maxsize=None)
def special_case() -> MinPCase:
    """All-equal rows (everything stays at any min_p, 1 included), half -inf rows, a one-spike row at min_p = 1
    (the spike alone stays) and all-negative rows, at T = 0.5, 1 and 2."""
    V, rows, cols = 1000, [], []
    for r, (kind, mp) in enumerate((k, mp) for k in ("equal", "neginf", "spike", "allneg") for mp in (1.0, 0.5, 1e-6)):
        rows.append(_row_np(kind, V))
        cols.append(ops.pack_sampling(T_LIST[r % 3], 0, 1.0, _seed(r + 40), _ctr(r), mp))
    return MinPCase("special-V1000", V, tuple(rows), _block(cols))


def search_winner(z: np.ndarray, seed: int, want: int, n: int = 4) -> list:
    """The first ``n`` counters at which token ``want`` wins the Gumbel-max over the WHOLE row ``z``: the draw
    without any cut."""
    found, c0, idx = [], 0, np.arange(len(z))
    while len(found) < n and c0 < 1 << 16:
        ctrs = np.arange(c0, c0 + 256, dtype=np.uint64)
        s = z[None, :] + gumbel64(seed, ctrs[:, None], idx[None, :]).astype(np.float32)
        found += [int(c) for c in ctrs[np.argmax(s, axis=1) == want]]
        c0 += 256
    assert len(found) >= n, "no such counters"
    return found[:n]


A, B_ID, C_ID = 700, 13, 401  # where the planted rows hold their three largest logits
BELOW_ONE_BF16 = 1.0 - 2.0 ** -8  # the bf16 neighbour below 1.0


def _planted_row(second: float, V: int = 1000) -> np.ndarray:
    """Logit 4 at id A, ``second`` at B_ID, -2 at C_ID, the rest at -30 and below (their mass is under e^-34)."""
    g = np.random.default_rng(4242)
    row = _bf16(-30.0 - 4.0 * g.random(V))
    row[A], row[B_ID], row[C_ID] = 4.0, second, -2.0
    return _bf16(row)


@functools.lru_cache(maxsize=None)
def planted_case() -> MinPCase:
    """Draws whose winner without the min_p cut is the second token (B_ID), the counters searched on the host.

    The logits are 4 at A and 1 at B_ID, so z_A - z_B = 3 / T, and min_p = exp(-3 / T) packs to the float32
    -3 / T exactly (T = 0.5, 1, 2): t = fl32(m - 3 / T) IS z_B, with no rounding anywhere.

    * rows "at": B_ID sits exactly at t; it stays and wins (4 counters per T);
    * rows "below": B_ID holds the bf16 neighbour below 1; it is dropped and never wins (4 counters per T);
    * rows "p<m" (T = 1): top-p keeps A and B_ID (p Z mid-way through B_ID's mass) and min_p = exp(-2) puts t = 2
      above B_ID: the winner sits between the top-p cut and the higher min_p cut, and is dropped;
    * rows "m<p" (T = 1): min_p = exp(-4) keeps A and B_ID (t = 0) and top-p keeps A alone (p Z mid-way through
      A's mass): the winner sits between the min_p cut and the higher top-p cut, and is dropped.

    B_ID's mass is 0.047 Z and A's 0.95 Z against a top-p band of 1e-4 Z: one cut, every draw decided."""
    rows, cols, tags = [], [], []
    at, below = _planted_row(1.0), _planted_row(BELOW_ONE_BF16)
    for ti, T in enumerate(T_LIST):
        mp, seed = math.exp(-3.0 / T), (1 << 62) + 31 * ti
        assert ops.pack_sampling(T, 0, 1.0, 0, 0, mp)[5] == ops.f32_bits(-3.0 / T)
        for row, tag in ((at, "at"), (below, "below")):
            z = row * (np.float32(1.0) / np.float32(T))
            for c in search_winner(z, seed, B_ID):
                rows.append(row)
                cols.append(ops.pack_sampling(T, 0, 1.0, seed, c, mp))
                tags.append(tag)
    mass = np.exp(at.astype(np.float64) - 4.0)
    Z = mass.sum()
    p_ab = float(np.float32((mass[A] + 0.5 * mass[B_ID]) / Z))  # keeps A and B_ID
    p_a = float(np.float32(0.5 * mass[A] / Z))  # keeps A alone
    for tag, p, mp, seed in (("p<m", p_ab, math.exp(-2.0), (1 << 62) + 977), ("m<p", p_a, math.exp(-4.0), 978)):
        for c in search_winner(at, seed, B_ID):
            rows.append(at)
            cols.append(ops.pack_sampling(1.0, 0, p, seed, c, mp))
            tags.append(tag)
    return MinPCase("planted-V1000", 1000, tuple(rows), _block(cols), planted=True, tags=tuple(tags))


CASES = {
    **{f"rows-V{V}": functools.partial(rows_case, V) for V in (32, 1000, 32000)},
    "rows-V128256": functools.partial(rows_case, 128256, 16),
    **{f"rows-V1000-B{B}": functools.partial(rows_case, 1000, B) for B in (1, 16, 17)},
    "special-V1000": special_case,
    "planted-V1000": planted_case,
}


@functools.lru_cache(maxsize=None)
def replay_case(name: str, variant: str | None = None) -> tuple:
    """The reference draws of a case, computed once and shared."""
    case = CASES[name]()
    return tuple(replay_minp(case.rows[r], case.col(r), variant) for r in range(case.B))
