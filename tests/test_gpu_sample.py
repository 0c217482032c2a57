"""The stochastic sampler (ops.sample_, sample.hip) replayed on the host, draw by draw.

``k_sample`` is deterministic given (seed, counter), so a test can say which
token a draw must return. ``replay`` is that reference, in numpy. It follows
what the kernel computes:

* noise: ``h = mix64(seed + mix64(ctr * 0x9E3779B97F4A7C15 + i + 1))`` in
  wrapping uint64, ``u = ((h >> 11) + 0.5) * 2^-53``, ``g_i = -log(-log u)`` in
  float64, rounded once to float32;
* ``z_i = fl32(logit_i * fl32(1 / T))`` (the division is correctly rounded on
  both sides; ``ops/build.py`` passes no fast-math flag);
* top-k: keep ``z >= k-th largest z``, ties kept, off for k <= 0 or k >= V.
  Exact: no tolerance;
* top-p over that set: masses ``exp(z_i - max z)`` in float64, the cut is the
  largest value at which the mass of all tokens >= it reaches ``p Z``; off
  unless 0 < p < 1;
* the winner: argmax of ``fl32(z_i + g_i)`` over the kept set, the lower id on
  equal scores; ``T >= 1e-4`` false (NaN included): ``ids[row]`` untouched.

The top-p band
--------------
The kernel sums the masses in fp32: ``Z~`` in registers, a wave tree and 16
serial adds; then, at each of four 8-bit levels of the radix select, per-bucket
totals by LDS float atomics in no fixed order, a prefix scan of the 256 totals,
and ``need -= above``. The reference therefore accepts a band of cuts: cut j
(distinct values, descending; C_j the mass of all tokens >= it, C_j - w_j the
mass strictly above it) is acceptable when

    C_j - w_j < p Z + tau Z   and   C_j >= p Z - tau Z.

tau (U = 2^-24; n the size of the top-k set; d_i = max z - z_i; p_i = mass
share) collects every error of the two sides of the kernel's comparison
"running total >= need", relative to Z:

* ``__expf(x)``: the device-library headers declare ``__ocml_native_exp_f32``
  and state no bound. Assumed here: it is ``v_exp_f32(x * log2(e))``, the
  instruction is good to 1 ulp = 2 U (the public CDNA ISA guide), the fp32
  constant and the product each round once (2 U |x| relative in the result),
  and x = fl32(z_i - m) carries U d_i: (2 + 3 d_i) U per mass. Weighted over a
  sum that is at most U (2 + 3 sum_i p_i d_i) <= U (2 + 3 ln n), as
  sum_i p_i d_i = H(p) - ln(Z) <= ln n (Z >= 1). It enters both sides:
  2 (2 + 3 ln n) U.
* In the pass that sums Z~ the compiler contracts the multiply and the
  subtraction into one fma (the generated code shows it; the histogram passes
  subtract separately), so there x is fl32(logit_i / T - m) without the inner
  rounding of z_i: up to U |z_i| in the exponent, at most U zmax over the sum
  (zmax: the largest finite |z_i| of the set).
* Z~: every term is positive, so an fp32 add costs at most U of the total;
  ceil(V / 1024) serial adds per thread, a tree of depth 6, 16 wave totals:
  (ceil(V / 1024) + 22) U; need = fl32(p Z~): U.
* the histograms: a sum of n_b positive terms in any order is within
  (n_b - 1) U of its value. The buckets that make up ``above`` over the four
  levels, and the last bucket, are disjoint sets of tokens: (n - 1) U in all.
* ``find_bucket``: 3 adds in the lane, 6 scan steps, excl = incl - s, and up to
  4 adds of the running total in the winning lane: 14 U per level, 56 U.
* ``need -= above``: one rounding per level, 4 U.
* masses below 2^-126 may flush: n 2^-126, the 1e-30.

    tau = U (n + ceil(V / 1024) + 88 + 6 ln n + zmax) (1 + 2^-10) + 1e-30

At n = V = 32000 that is 1.9e-3; at k = 50 about 1e-5. When ``find_bucket``
finds no bucket (a level's re-accumulated total falls short of the carried
``need``), the cut falls to the bottom of the enclosing bucket, which keeps
exactly that bucket's tokens: the cut whose C_j is within these roundings of
p Z, so it is inside the band (see the comment there in sample.hip).

The margin of the winner
------------------------
The hash and u are integer and exact-IEEE operations, identical on both sides.
The device's double ``log`` is not correctly rounded. With 2 ulp allowed for
each log on each side (the OpenCL accuracy the device library is built to is
1 ulp for double log; glibc documents 1 ulp), w = -log u carries 2^-51
relative, which the outer log turns into 2^-51 absolute, plus its own
2^-51 |g|: 2^-51 (1 + |g|) a side. So the two float64 values of g_i differ by
at most delta_i = 2^-49 (1 + |g_i|) (a factor of 2 to spare), and the fp32
g_i differ (by one ulp of g_i) only when the host's float64 value lies within
delta_i of an fp32 rounding boundary. The score fl32(z_i + g_i) is one
correctly rounded add of the same z_i (the generated code has a plain add
there, no fma), so it then moves by at most one ulp of the score, and not at
all otherwise. The margin is therefore not a constant: token i has the score
interval [fl32(z_i + g_i^-), fl32(z_i + g_i^+)] (g^-, g^+ the fp32 neighbours)
when its g sits on such a boundary, and the single value fl32(z_i + g_i) when
not. With L the largest lower end, every token whose upper end reaches L is a
possible winner. A draw is decided when there is one, or when all of them have
one and the same exact score (then the lowest id wins, a rule the cases test);
it is undecided otherwise, and also when the winner differs across the band.
For an undecided draw the device's id must be one of the possible winners.
A boundary is hit with probability about 2^-25 (1 + |g|) / ulp32(g) ~ 1e-6 per
token, so near-ties are rare: none in this module's cases.

(The engine test, which sees log-probabilities and not logits, uses a plain
margin instead: see ``test_engine_draws_replay``.)

No case may have more than 2 % of its draws undecided, the cut probes none:
``test_reference_decides_the_cases`` asserts that on the host.

Observed (MI355X; each GPU test prints its own): 755 kernel draws compared,
755 decided, largest undecided share of a case 0.0000, every id equal to the
reference's; engine: 24 draws, decided share 1.000. Three side builds of
sample.hip with one arithmetic slip each: ``need = k + 1`` fails 15 of the 18
kernel tests here (and one of the eight chi-square cases of test_gpu_ops.py,
through its kept-set assertion); ``i`` for ``i + 1`` in the hash fails 17 of 18
(the chi-square test passes all eight); ``incl > need`` in the float select
passes everything, here and there: it differs from the kernel only when a
running fp32 total equals ``need`` exactly, and a cut whose cumulative mass
equals p Z is the middle of the band, where either neighbour is acceptable.
"""
import functools
import math
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd import ops

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")

U = 2.0 ** -24
BF = torch.bfloat16
SENTINEL = -7
GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
UNDECIDED_CAP = 0.02
VARIANTS = ("k+1", "k-1", "tie_by_id", "p_excl_crossing", "p_before_k", "p_unscaled", "noise_i", "swap_seed_ctr",
            "no_ctr", "tie_high_id", "stride_B")


# ---------------------------------------------------------------- the reference of one draw
def mix64(z: np.ndarray) -> np.ndarray:
    """SplitMix64 finaliser on a uint64 array (numpy arrays wrap)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def gumbel64(seed, ctr, idx: np.ndarray, offset: int = 1) -> np.ndarray:
    """float64 Gumbel noise of tokens ``idx`` for draws ``ctr`` (a scalar, or an array that broadcasts)."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    inner = ctr * np.uint64(GOLD) + idx.astype(np.uint64) + np.uint64(offset)
    h = mix64(np.uint64(seed & M64) + mix64(inner))
    u = ((h >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    with np.errstate(divide="ignore"):
        return -np.log(-np.log(u))


def tau(n: int, V: int, zmax: float) -> float:
    return U * (n + math.ceil(V / 1024) + 88 + 6 * math.log(max(n, 1)) + zmax) * (1 + 2.0 ** -10) + 1e-30


@dataclass(frozen=True)
class Draw:
    winner: int | None  # None: a greedy row, ids[row] untouched
    possible: frozenset = frozenset()

    @property
    def decided(self):
        return self.winner is None or len(self.possible) == 1


def _f32(bits: int) -> np.float32:
    return np.array([bits & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0]


def _pick(z, idx, seed, ctr, variant):
    """(winner, possible winners) of the Gumbel-max over tokens ``idx``."""
    if variant == "swap_seed_ctr":
        seed, ctr = ctr, seed
    if variant == "no_ctr":
        ctr = 0
    g64 = gumbel64(seed, ctr, idx, 0 if variant == "noise_i" else 1)
    g = g64.astype(np.float32)
    with np.errstate(invalid="ignore"):
        s = z[idx] + g  # float32
        delta = 2.0 ** -49 * (1 + np.abs(g64))
        g_lo, g_hi = (g64 - delta).astype(np.float32), (g64 + delta).astype(np.float32)
        lo, hi = s, s
        if (g_lo != g_hi).any():  # some g within delta of an fp32 rounding boundary
            lo, hi = z[idx] + g_lo, z[idx] + g_hi
    L = lo.max()
    P = np.flatnonzero(hi >= L)
    if variant == "tie_high_id":
        return int(idx[P].max()), frozenset([int(idx[P].max())])
    if len(P) == 1 or (lo[P] == hi[P]).all():
        w = int(idx[P].min())
        return w, frozenset([w])
    exact = np.flatnonzero(s == s.max())
    return int(idx[exact].min()), frozenset(int(i) for i in idx[P])


def _top_p_cuts(z, keep, p32, V, src, band):
    """Acceptable top-p cut values over the set ``keep``, the exact one first."""
    idx = np.flatnonzero(keep)
    x = src[idx].astype(np.float64)
    mass = np.exp(x - x.max())
    vals, inv = np.unique(z[idx], return_inverse=True)
    w = np.bincount(inv, weights=mass, minlength=len(vals))[::-1]
    vals = vals[::-1]
    C = np.cumsum(w)
    Z = C[-1]
    target = float(p32) * Z
    exact = min(int(np.searchsorted(C, target, side="left")), len(vals) - 1)
    if not band:
        return [vals[exact]], exact, vals
    finite = np.abs(z[idx][np.isfinite(z[idx])])
    t = tau(len(idx), V, float(finite.max()) if len(finite) else 0.0) * Z
    js = np.flatnonzero((C - w < target + t) & (C >= target - t))
    assert exact in js
    return [vals[exact]] + [vals[j] for j in js if j != exact], exact, vals


def replay(logits: np.ndarray, col, variant: str | None = None) -> Draw:
    """One draw: ``logits`` the row as float32 (exact bf16 values), ``col`` the five int64 the kernel reads."""
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

    def top_k(zz):
        if k >= V:
            return np.ones(V, dtype=bool)
        kk = min(k + 1, V) if variant == "k+1" else max(k - 1, 1) if variant == "k-1" else k
        if variant == "tie_by_id":
            keep = np.zeros(V, dtype=bool)
            keep[np.lexsort((np.arange(V), -zz))[:kk]] = True
            return keep
        return zz >= np.partition(zz, V - kk)[V - kk]

    keep = top_k(z)
    cuts = [np.float32(-np.inf)]
    if p_on:
        src = logits if variant == "p_unscaled" else z
        over = np.ones(V, dtype=bool) if variant == "p_before_k" else keep
        cuts, exact, vals = _top_p_cuts(z, over, p, V, src, band=variant is None)
        if variant == "p_excl_crossing":
            if exact == 0:
                return Draw(-1, frozenset([-1]))  # nothing left to draw from
            cuts = [vals[exact - 1]]
    results = []
    for c in (min(cuts), max(cuts)) if len(cuts) > 1 else cuts:
        results.append(_pick(z, np.flatnonzero(keep & (z >= c)), seed, ctr, variant))
    if len(cuts) > 1:
        w_lo, P_lo = results[0]
        if all(z[i] >= max(cuts) for i in P_lo):  # the best of the largest set lies in every smaller one
            return Draw(w_lo, P_lo)
        every = [_pick(z, np.flatnonzero(keep & (z >= c)), seed, ctr, variant) for c in cuts]
        return Draw(every[0][0], frozenset().union(*(P for _, P in every)))
    return Draw(*results[0])


# ---------------------------------------------------------------- rows
KINDS = ("gauss0.5", "gauss2", "gauss4", "equal", "straddle", "neginf", "spike", "allneg")


@functools.lru_cache(maxsize=None)
def _row(kind: str, V: int) -> torch.Tensor:
    """A bf16 logits row."""
    if kind.startswith("probe"):
        return _probe_row(V, int(kind[5:]))
    g = torch.Generator().manual_seed(7000 + KINDS.index(kind) + V)
    if kind.startswith("gauss"):
        return (torch.randn(V, generator=g) * float(kind[5:])).to(BF)
    if kind == "equal":  # large enough that at T = 1e-4 the scores fall on a grid of 1/8: exact ties
        return torch.full((V,), 120.0).to(BF)
    if kind == "straddle":  # three distinct large values, then up to 100 equal ones on scattered ids
        z = torch.randn(V, generator=g).clamp_(max=2.0)
        perm = torch.randperm(V, generator=g)
        big = torch.tensor([9.0, 8.0, 7.0])[:min(3, V)]
        z[perm[:len(big)]] = big
        z[perm[3:3 + max(0, min(100, V - 3))]] = 5.0
        return z.to(BF)
    if kind == "neginf":  # -inf on half the entries (never all of them)
        z = torch.randn(V, generator=g)
        z[torch.randperm(V, generator=g)[:V // 2]] = -math.inf
        return z.to(BF)
    if kind == "spike":
        z = torch.full((V,), -80.0)
        z[min(V // 2 + 1, V - 1)] = 80.0
        return z.to(BF)
    if kind == "allneg":  # negative whatever T > 0: the sign branch of the order-preserving key
        return (-(torch.randn(V, generator=g).abs() * 2.0 + 1.0)).to(BF)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _row_np(kind: str, V: int) -> np.ndarray:
    return _row(kind, V).float().numpy()


def _probe_row(V: int, k: int) -> torch.Tensor:
    """A Gaussian row (clamped at 3) under k + 3 distinct values 6, 6 - 1/32, ... (exact in bf16) on scattered
    ids, so each cut of a probe falls between two tokens."""
    g = torch.Generator().manual_seed(9000 + V + k)
    row = torch.randn(V, generator=g).clamp_(max=3.0)
    row[torch.randperm(V, generator=g)[:k + 3]] = 6.0 - torch.arange(k + 3) / 32.0
    return row.to(BF)


# ---------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    name: str
    V: int
    kinds: tuple  # row -> kind
    block: tuple  # the params block, 5 tuples of ld ints
    probe: bool = False  # built for one specific cut: no draw may be undecided

    @property
    def B(self):
        return len(self.kinds)

    @property
    def ld(self):
        return len(self.block[0])

    def col(self, row: int, stride: int | None = None):
        flat = [v for line in self.block for v in line]
        stride = self.ld if stride is None else stride
        return tuple(flat[q * stride + row] for q in range(5))


def _case(name, V, kinds, cols, extra=(), probe=False):
    block = tuple(zip(*(list(cols) + list(extra))))
    return Case(name, V, tuple(kinds), block, probe)


BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))
P_LIST = (1e-9, 0.5, 0.9, BELOW_ONE, 1.0, 0.0, -1.0, math.nan)
T_LIST = (1e-4, 0.7, 1.0, 1.5)
T_GREEDY = (0.0, 9.9e-5, -1.0, math.nan)


def _seed(r: int) -> int:
    return ((1 << 62) if r % 2 else 0) + 0x1234567 * (r + 1)


def _ctr(r: int) -> int:
    return (0, (1 << 40) + r, r, 3 * r + 1)[r % 4]


def _main_case(V: int) -> Case:
    """64 rows: every row kind with every p, k and T (sampled and greedy) rotating against them."""
    k_list = (1, 2, V - 1, V, V + 1, -3, 1 << 40, 5, 50)
    kinds, cols = [], []
    for r in range(64):
        j = r // 8
        kinds.append(KINDS[r % 8])
        T = T_GREEDY[(r // 9) % 4] if r % 9 == 4 else T_LIST[(r + j) % 4]
        cols.append(ops.pack_sampling(T, k_list[(2 * r + j) % 9], P_LIST[(r + j) % 8], _seed(r), _ctr(r)))
    return _case(f"rows-V{V}", V, kinds, cols)


def _big_case() -> Case:
    V = 128256
    cols = [ops.pack_sampling(0.7, 50, 0.9, _seed(1), 1 << 40), ops.pack_sampling(1.0, 0, 1.0, _seed(2), 0)]
    return _case(f"rows-V{V}", V, ["gauss4", "gauss4"], cols)


def _layout_case() -> Case:
    """ld = 80 > B = 64; columns 64..79 look live, so that a stride of B changes the ids. Odd rows are greedy."""
    V, kinds, cols = 1000, [], []
    for r in range(64):
        kinds.append(KINDS[(r // 2) % 8])
        T = T_GREEDY[(r // 2) % 4] if r % 2 else T_LIST[1 + (r // 2) % 3]
        cols.append(ops.pack_sampling(T, (0, 40, 7)[r % 3], (1.0, 0.9, 0.6)[(r // 2) % 3], _seed(r + 100), _ctr(r)))
    extra = [ops.pack_sampling(1.0, 1, 1.0, 0x5EED0000 + c, c) for c in range(16)]
    return _case("layout-ld80", V, kinds, cols, extra)


def _search(z_top: np.ndarray, ids: np.ndarray, seed: int, upto: int, want: int, n: int = 8, start: int = 0):
    """The first ``n`` counters >= start at which token ``want`` (a rank) wins the Gumbel-max over ranks
    0..upto-1."""
    found, c0 = [], start
    while len(found) < n and c0 < start + (1 << 18):
        ctrs = np.arange(c0, c0 + 2048, dtype=np.uint64)
        g = gumbel64(seed, ctrs[:, None], ids[None, :upto]).astype(np.float32)
        s = z_top[None, :upto] + g
        found += [int(c) for c in ctrs[np.argmax(s, axis=1) == want]]
        c0 += 2048
    assert len(found) >= n, "no such counters"
    return found[:n]


@functools.lru_cache(maxsize=None)
def _probe_case(V: int, k: int) -> Case:
    """Draws on either side of the top-k cut and of the top-p cut of one row (T = 1, so z is the logit):

    * top-k: 8 counters at which rank k + 1 wins over the top k + 1 (the device must return the best of the top
      k), 8 at which rank k wins over the top k (the device must return it);
    * top-p inside the top k: p Z mid-gap between the cumulative masses before and after rank c = k // 2 + 1, a
      token far heavier than tau Z, so that the band holds one cut; 8 counters at which rank c wins over the top
      c, 8 at which rank c + 1 wins over the top c + 1."""
    kind = f"probe{k}"
    z = _row_np(kind, V)
    ids = np.argsort(-z, kind="stable")[:k + 2]
    zt = z[ids]
    seed = (1 << 62) + 1000003 * V + k
    cols = [ops.pack_sampling(1.0, k, 1.0, seed, c) for c in _search(zt, ids, seed, k + 1, k) +
            _search(zt, ids, seed, k, k - 1)]
    c = k // 2 + 1
    mass = np.exp(zt[:k].astype(np.float64) - float(zt[0]))
    C = np.cumsum(mass)
    p = float(np.float32((C[c - 1] - 0.5 * mass[c - 1]) / C[-1]))
    cols += [ops.pack_sampling(1.0, k, p, seed + 1, x) for x in _search(zt, ids, seed + 1, c, c - 1) +
             _search(zt, ids, seed + 1, c + 1, c)]
    return _case(f"probe-V{V}-k{k}", V, [kind] * len(cols), cols, probe=True)


@functools.lru_cache(maxsize=None)
def _tie_case() -> Case:
    """16 draws whose two best scores are equal in fp32: the all-equal row at T = 1e-4 has z = 1.2e6, where fp32
    steps by 1/8, and the counters are searched on the host. The lower id must win."""
    V, seed = 1025, (1 << 62) + 99
    z = _row_np("equal", V) * (np.float32(1.0) / np.float32(1e-4))
    found, c0 = [], 0
    while len(found) < 16 and c0 < 1 << 16:
        ctrs = np.arange(c0, c0 + 512, dtype=np.uint64)
        s = z[None, :] + gumbel64(seed, ctrs[:, None], np.arange(V)[None, :]).astype(np.float32)
        found += [int(c) for c in ctrs[(s == s.max(axis=1, keepdims=True)).sum(axis=1) >= 2]]
        c0 += 512
    cols = [ops.pack_sampling(1e-4, 0, 1.0, seed, c) for c in found[:16]]
    return _case("ties-V1025", V, ["equal"] * 16, cols, probe=True)


MAIN_V = (1, 2, 63, 64, 1023, 1024, 1025, 4096, 32000)
CASE_NAMES = tuple(f"rows-V{V}" for V in MAIN_V) + ("rows-V128256", "layout-ld80", "ties-V1025") + \
    tuple(f"probe-V{V}-k{k}" for V in (1000, 32000) for k in (2, 5, 50))


@functools.lru_cache(maxsize=None)
def _get(name: str) -> Case:
    if name.startswith("probe"):
        _, v, k = name.split("-")
        return _probe_case(int(v[1:]), int(k[1:]))
    if name == "layout-ld80":
        return _layout_case()
    if name == "ties-V1025":
        return _tie_case()
    if name == "rows-V128256":
        return _big_case()
    return _main_case(int(name[6:]))


@functools.lru_cache(maxsize=None)
def _replay_case(name: str, variant: str | None = None) -> tuple:
    """The reference draws of a case, computed once and shared."""
    case = _get(name)
    stride = case.B if variant == "stride_B" else None
    return tuple(replay(_row_np(case.kinds[r], case.V), case.col(r, stride), variant) for r in range(case.B))


# ---------------------------------------------------------------- host-only tests
def test_hash_and_noise_known_values():
    """SplitMix64's finaliser against its published first output (seed 0: the state after one step is the golden
    ratio constant), and the noise's range."""
    assert int(mix64(np.array([GOLD], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF
    g = gumbel64(1 << 62, 1 << 40, np.arange(100000))
    assert np.isfinite(g).all() and -3.7 < g.min() and g.max() < 37.5
    assert abs(g.mean() - 0.5772) < 0.02  # Euler's constant
    assert tau(32000, 32000, 10.0) < 2e-3 and tau(50, 32000, 10.0) < 2e-5


def test_reference_decides_the_cases():
    """The cap, on the reference alone: at most 2 % of a case's draws undecided, none in a cut probe."""
    for name in CASE_NAMES:
        case, ref = _get(name), _replay_case(name)
        sampled = [d for d in ref if d.winner is not None]
        undecided = sum(not d.decided for d in sampled)
        print(f"{name}: {len(ref)} rows, {len(sampled)} sampled, {undecided} undecided")
        assert undecided <= (0 if case.probe else UNDECIDED_CAP * len(ref)), name
        for r, d in enumerate(ref):  # a -inf token is never the reference's winner
            if d.winner is not None:
                assert all(math.isfinite(_row_np(case.kinds[r], case.V)[i]) for i in d.possible), (name, r)
    layout = _replay_case("layout-ld80")
    assert all((d.winner is None) == bool(r % 2) for r, d in enumerate(layout))  # greedy and sampled interleaved
    for name in CASE_NAMES:  # every probe case: 8 draws on each side of each cut
        if name.startswith("probe"):
            assert _get(name).B == 32
    ties = _get("ties-V1025")
    assert ties.B == 16
    for r, d in enumerate(_replay_case("ties-V1025")):  # two equal best scores, the lower id the winner
        hi = replay(_row_np("equal", ties.V), ties.col(r), "tie_high_id")
        assert hi.winner > d.winner, r


def test_probes_sit_on_their_cuts():
    """In a probe case rows 0..7 are won by a token that rank k + 1 would beat, rows 8..15 by rank k, rows 16..23
    by the top-p crossing token and rows 24..31 by a token that the one after the crossing token would beat."""
    for V in (1000, 32000):
        for k in (2, 5, 50):
            name = f"probe-V{V}-k{k}"
            z = _row_np(f"probe{k}", V)
            order = np.argsort(-z, kind="stable")
            ref = _replay_case(name)
            c = k // 2 + 1
            assert all(d.winner in order[:k] for d in ref[:8]) and all(d.winner == order[k - 1] for d in ref[8:16])
            assert all(d.winner == order[c - 1] for d in ref[16:24]) and all(d.winner in order[:c] for d in ref[24:])
            assert all(d.winner == order[k] for d in _replay_case(name, "k+1")[:8])
            assert all(d.winner != order[k - 1] for d in _replay_case(name, "k-1")[8:16])
            assert all(d.winner != order[c - 1] for d in _replay_case(name, "p_excl_crossing")[16:24])


def test_perturbed_reference_changes_decided_draws():
    """Each slip of the reference changes the winner of at least one decided draw of the module's cases: the
    cases can tell such a kernel from a right one."""
    for variant in VARIANTS:
        changed = total = 0
        for name in CASE_NAMES:
            for base, pert in zip(_replay_case(name), _replay_case(name, variant)):
                if base.winner is not None and base.decided:
                    total += 1
                    changed += pert.winner != base.winner
                elif base.winner is None and variant == "stride_B":
                    changed += pert.winner is not None
        print(f"{variant}: changes {changed} of {total} decided draws")
        assert changed >= 1, variant


# ---------------------------------------------------------------- GPU: the kernel
_tally = {"compared": 0, "decided": 0, "worst": 0.0}


def _check_case(name: str):
    case, ref = _get(name), _replay_case(name)
    logits = torch.stack([_row(kind, case.V) for kind in case.kinds]).cuda()
    ids = torch.full((case.B,), SENTINEL, dtype=torch.int64, device="cuda")
    params = torch.tensor(case.block, dtype=torch.int64, device="cuda")
    assert params.shape == (5, case.ld)
    ops.sample_(logits, ids, params)
    torch.cuda.synchronize()
    got = ids.cpu().tolist()
    sampled = undecided = 0
    for r, (d, g) in enumerate(zip(ref, got)):
        what = (name, r, case.kinds[r], case.col(r))
        if d.winner is None:
            assert g == SENTINEL, what  # a greedy row keeps what it held
            continue
        sampled += 1
        assert 0 <= g < case.V and math.isfinite(_row_np(case.kinds[r], case.V)[g]), what + (g,)
        if d.decided:
            assert g == d.winner, what + (g, d.winner)
        else:
            undecided += 1
            assert g in d.possible, what + (g, sorted(d.possible))
    share = undecided / max(len(ref), 1)
    _tally["compared"] += sampled
    _tally["decided"] += sampled - undecided
    _tally["worst"] = max(_tally["worst"], share)
    print(f"{name}: {sampled} draws compared, {sampled - undecided} decided, undecided share {share:.4f}; so far "
          f"{_tally['compared']} compared, {_tally['decided']} decided, largest share {_tally['worst']:.4f}")


@cuda
@pytest.mark.gpu
@pytest.mark.parametrize("V", MAIN_V + (128256,))
def test_rows_replay(V):
    _check_case(f"rows-V{V}")


@cuda
@pytest.mark.gpu
@pytest.mark.parametrize("V", (1000, 32000))
@pytest.mark.parametrize("k", (2, 5, 50))
def test_cut_probes_replay(V, k):
    _check_case(f"probe-V{V}-k{k}")


@cuda
@pytest.mark.gpu
def test_layout_replay():
    _check_case("layout-ld80")


@cuda
@pytest.mark.gpu
def test_equal_scores_replay():
    _check_case("ties-V1025")


# ---------------------------------------------------------------- GPU: the engine
def _lp_bound(V: int, lse: float, lp: float) -> float:
    """The log-probability kernel's error bound, as derived in tests/test_gpu_logprobs.py."""
    D = 8 * math.ceil(V / 8192) + 22
    return U * (6 + D + 7 * math.log(V) + abs(lse) + abs(lp)) * (1 + 2.0 ** -10) + 1e-30


@cuda
@pytest.mark.gpu
def test_engine_draws_replay():
    """Two sampled requests side by side (T = 1, top_k = 8, different seeds, logprobs = 20). A token's record
    holds the top 20 (id, logprob) of the very logits the sampler read, and logprob = logit - lse does not move an
    argmax, so the kept set is the ranks at or above the 8th value and the token must be the replayed Gumbel-max
    over it, at the counter the engine passes (the token's index).

    A draw is undecided when its two best scores are closer than 2 lp_bound (T = 1; |lse| <= 64 assumed, each
    unit of it is worth U) plus the fp32 margin: for each of the two tokens one ulp of g (the boundary case
    above, and this replay's unrounded g) and one ulp of the score, at |g| < 64 and |score| < 128:
    2 (2^-18 + 2^-17). The condition is that no draw is undecided."""
    from p2p_llm_tunnel_amd.models.server import Engine, Request, Sampling
    eng = Engine(device="cuda:0", config="micro", max_batch=4)
    try:
        V, n = eng.model.cfg.vocab, 12
        seeds = ((1 << 62) + 12345, 777)
        reqs = [eng.submit(Request(list(prompt), n, sampling=Sampling(temperature=1.0, top_k=8, seed=s), logprobs=20))
                for prompt, s in zip((b"replay a", b"another one"), seeds)]
        toks = [list(iter(r.out.get, None)) for r in reqs]
    finally:
        eng.stop()
    decided = total = 0
    for req, seq, seed in zip(reqs, toks, seeds):
        assert len(seq) == n and len(req.lp) == n
        for ctr, (tok, (_, top)) in enumerate(zip(seq, req.lp)):
            assert len(top) == 20
            ids = np.array([i for i, _ in top])
            lp = np.array([x for _, x in top], dtype=np.float64)
            assert lp[19] < lp[7], "the 8th value's ties run past the record"
            keep = lp >= lp[7]
            score = lp[keep] + gumbel64(seed, ctr, ids[keep])
            order = np.argsort(-score)
            margin = 2 * _lp_bound(V, 64.0, float(-lp[keep].min())) + 2 * (2.0 ** -18 + 2.0 ** -17)
            total += 1
            assert score[order[0]] - score[order[1]] > margin, ("undecided: change the seed", seed, ctr)
            decided += 1
            assert tok == int(ids[keep][order[0]]), (seed, ctr, tok, top)
    assert toks[0] != toks[1]
    print(f"engine: {total} draws compared, decided share {decided / total:.3f}")
