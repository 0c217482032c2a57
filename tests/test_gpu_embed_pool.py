"""``ops.embed_pool_`` (embed_pool.hip) against an fp64 reference computed from
the exact inputs the kernel read: the bf16 ``resid`` rows, the bf16 norm
weight ``g``, eps as the fp32 number it is passed as and, for a continued
piece, the exact fp32 ``acc`` row ("teacher forcing", as in
test_gpu_fused_stages.py). Because the inputs are exact, the allowed error is
a formula in the rows n of a job and dim, derived here from the operations the
kernel performs and not fitted to what it returns. U = 2^-24 is the fp32 unit
roundoff; second-order terms are covered by a factor 1.01 (the largest
first-order term, (dim / 2) U at dim 16384, is 5e-4, so (1 + e)^k <= 1 + 1.01 k e
holds with room); TINY = 2^-126 absorbs roundings below fp32's normal range.

Per row r, exact: Y_rc = x_rc g_c / sqrt(sum_c x_rc^2 / dim + eps).

* Sum of squares. A product of two bf16 values is exact in fp32. The terms are
  non-negative, so a sum with at most ``depth`` roundings on any path carries at
  most depth U relative: a lane adds 8 per 16-byte word it owns, then 6 levels
  across the wave (adding zeros is exact), depth <= dim. The mean, the eps add:
  U each; all under the square root, which halves them; rsqrtf <= 2 ulp = 4 U
  (no fast-math flag). 1/rms: <= (dim / 2 + 8) U relative, the figure
  test_gpu_fused_stages.py uses. (A row whose sum overflows fp32 is measured
  again on x 2^-96, an exact scaling: the same error.)
* Two products, (x inv) g: U each. So |y_rc - Y_rc| <= (dim / 2 + 10) U |Y_rc|.
* Additions. a = a0 + y_1 + ... + y_n, sequentially, r ascending: with a0 = 0
  ("first") the first add is exact, m = n - 1 roundings, otherwise m = n; each
  at most U times the partial sum, itself at most |a0| + S_c, S_c = sum_r |Y_rc|.

  E_a(c) = 1.01 U [(dim / 2 + 10) S_c + m (|a0_c| + S_c)] + TINY

  bounds |a_c - A_c| for what a piece writes to ``acc`` (A = a0 + sum_r Y_r).
* Final norm ("last"). O = A / ||A||. The kernel divides its own a by the fp32
  norm of a: |a_c / ||a|| - O_c| <= (E_a(c) + |O_c| ||E_a||_2) / ||A||, and the
  computed quotient differs from a_c / ||a|| by the squares (U), their sum
  (<= dim U, as above), both halved by sqrtf (correctly rounded, U), and the
  division (U): <= (dim / 2 + 4) U relative.

  E_o(c) = 1.01 [(E_a(c) + |O_c| ||E_a||_2) / ||A|| + (dim / 2 + 4) U |O_c|] + TINY

  A sequence whose A is exactly zero (all-zero rows) must give exact zeros.

The shapes are the smallest at which the kernel can go wrong: dim 8 (one
16-byte word, one lane), 264 (33 words: a partial wave), 1024, 5120 (640 words:
2.5 per lane of the 256) and 16384 (the limit); 1, 2, 17 and 64 rows; 1, 3 and 16
jobs with gaps between their rows; an all-zero row, a row of bf16 maxima (its
fp32 sum of squares overflows) and an all-zero sequence.

The CPU tests hold a plain fp32 numpy emulation of the kernel to the same
bounds on the same cases, and show that six one-line slips each break the bound
or the split invariance, so neither is loose enough to let them through."""
import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd import ops

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -126
EPS = 1e-5
DIMS = (8, 264, 1024, 5120, 16384)
N_ACC, N_OUT = 20, 18
POISON = np.uint32(0x7B7B7B7B)  # acc and out rows that must stay untouched hold this bit pattern
FIRST, LAST = 1, 2
BF16_MAX_BITS = 0x7F7F
F32_MAX = np.float32(3.4028234663852886e38)


# ---------------------------------------------------------------- inputs
def bf16_of(a):
    """float32 array -> (bf16 bit patterns uint16, their exact float32 values), round to nearest even."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return bits, (bits.astype(np.uint32) << 16).view(np.float32)


class Case:
    """Seeded inputs of one launch: ``jobs`` and every buffer the kernel reads."""

    def __init__(self, name, dim, rows, jobs, seed, zero_rows=(), max_rows=(), small_rows=()):
        self.name, self.dim, self.rows, self.jobs = name, dim, rows, jobs
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((rows, dim)).astype(np.float32) * np.float32(3.0)
        for r in small_rows:  # mean square near eps: eps decides 1/rms
            x[r] *= np.float32(1e-3)
        self.x_bits, self.x = bf16_of(x)
        for r in zero_rows:
            self.x_bits[r], self.x[r] = 0, 0.0
        for r in max_rows:  # +-bf16 max, alternating
            sign = (np.arange(dim) % 2).astype(np.uint16) << 15
            self.x_bits[r] = BF16_MAX_BITS | sign
            self.x[r] = (self.x_bits[r].astype(np.uint32) << 16).view(np.float32)
        self.g_bits, self.g = bf16_of(1.0 + 0.1 * rng.standard_normal(dim))
        self.acc = np.full((N_ACC, dim), POISON, dtype=np.uint32).view(np.float32)
        for _, n, a, flags, _ in jobs:
            if not flags & FIRST:  # a running sum, as an earlier piece of some length would have left it
                self.acc[a] = (rng.standard_normal(dim) * 3.0 * np.sqrt(rng.integers(1, 200))).astype(np.float32)


def _gapped(n_jobs, n, flags):
    """n_jobs jobs of n rows, one unused row between neighbours; acc and out rows in a scattered order."""
    return [(j * (n + 1), n, (7 * j + 3) % N_ACC, flags[j % len(flags)],
             (5 * j + 2) % N_OUT if flags[j % len(flags)] & LAST else -1) for j in range(n_jobs)]


def cases(dim):
    s = DIMS.index(dim) * 100
    return [
        Case("r1", dim, 1, [(0, 1, 0, 3, 0)], s + 1),
        Case("r2", dim, 2, [(0, 2, 5, 3, 17)], s + 2),
        Case("r2-continued", dim, 2, [(1, 1, 19, 2, 0)], s + 3),
        # 3 jobs with gaps (rows 5, 6 and 11 unused); row 2 all zero, row 8 of bf16 maxima, row 13 small
        Case("r17-j3", dim, 17, [(0, 5, 4, 3, 1), (7, 4, 0, 1, -1), (12, 5, 9, 2, 16)], s + 4,
             zero_rows=(2,), max_rows=(8,), small_rows=(13,)),
        # 16 jobs of 3 rows with gaps, every flag combination; job 4 (rows 16..18) is an all-zero sequence
        Case("r64-j16", dim, 64, _gapped(16, 3, (3, 1, 0, 2)), s + 5, zero_rows=(16, 17, 18), small_rows=(1, 30)),
        Case("r64-j1", dim, 64, [(0, 64, 11, 3, 9)], s + 6, zero_rows=(40,), small_rows=(63,)),
        Case("r64-j1-continued", dim, 64, [(0, 64, 2, 0, -1)], s + 7),
    ]


# ---------------------------------------------------------------- fp64 reference and bounds
def reference(case, job):
    """(what the job writes in fp64, the bound on each element's error, whether it goes to ``out``)."""
    row0, n, a, flags, _ = job
    dim = case.dim
    X = case.x[row0:row0 + n].astype(np.float64)
    g = case.g.astype(np.float64)
    inv = 1.0 / np.sqrt((X * X).mean(axis=1) + float(np.float32(EPS)))
    Y = X * inv[:, None] * g[None, :]
    a0 = np.zeros(dim) if flags & FIRST else case.acc[a].astype(np.float64)
    A = a0 + Y.sum(axis=0)
    S = np.abs(Y).sum(axis=0)
    m = n - 1 if flags & FIRST else n
    Ea = 1.01 * U * ((dim / 2 + 10) * S + m * (np.abs(a0) + S)) + TINY
    if not flags & LAST:
        return A, Ea, False
    norm = np.sqrt((A * A).sum())
    if norm == 0.0:
        return np.zeros(dim), np.zeros(dim), True  # exact zeros
    O = A / norm
    Eo = 1.01 * ((Ea + np.abs(O) * np.sqrt((Ea * Ea).sum())) / norm + (dim / 2 + 4) * U * np.abs(O)) + TINY
    return O, Eo, True


def check(case, acc, out):
    """``acc`` and ``out`` (float32 arrays) after the launch: every job inside its bound, nothing else touched."""
    worst = 0.0
    acc_written, out_written = set(), set()
    for job in case.jobs:
        want, bound, to_out = reference(case, job)
        got = (out[job[4]] if to_out else acc[job[2]]).astype(np.float64)
        (out_written if to_out else acc_written).add(job[4] if to_out else job[2])
        assert np.isfinite(got).all(), (case.name, job)
        err = np.abs(got - want)
        assert (err <= bound).all(), (case.name, job, float((err / np.maximum(bound, TINY)).max()))
        if bound.any():
            worst = max(worst, float((err / bound).max()))
    for r in range(N_ACC):  # rows no job names, and acc of jobs with "last"
        if r not in acc_written:
            assert np.array_equal(acc[r].view(np.uint32), case.acc[r].view(np.uint32)), (case.name, "acc", r)
    for r in range(N_OUT):
        if r not in out_written:
            assert (out[r].view(np.uint32) == POISON).all(), (case.name, "out", r)
    return worst


# ---------------------------------------------------------------- fp32 emulation (CPU)
def emulate(x, g, acc, out, jobs, eps=EPS, slip=None):
    """The kernel in plain fp32 numpy, in place on ``acc`` and ``out``. ``slip``: one arithmetic mistake."""
    f32 = np.float32
    dim = x.shape[1]
    with np.errstate(all="ignore"):
        for row0, n, a_i, flags, out_row in jobs:
            rows = x[row0:row0 + n]
            first = flags & FIRST and slip != "first_ignored"
            a = np.zeros(dim, dtype=f32) if first else acc[a_i].copy()
            order = range(n - 1, -1, -1) if slip == "rows_reversed" else range(n)
            for r in order:
                scale = f32(1.0)
                ss = np.sum(rows[r] * rows[r], dtype=f32)
                if not ss <= F32_MAX:
                    scale = f32(2.0 ** -96)
                    ss = np.sum((rows[r] * scale) * (rows[r] * scale), dtype=f32)
                e = f32(0.0) if slip == "eps_dropped" or scale != 1.0 else f32(eps)
                inv = f32(1.0) / np.sqrt(f32(ss / f32(n if slip == "mean_over_n" else dim)) + e, dtype=f32)
                y = (rows[r] * scale) * inv
                a = a + (y if slip == "g_skipped" else y * g)
            if flags & LAST or slip == "normalise_each_piece":
                total = np.sum(a * a, dtype=f32)
                res = a / np.sqrt(total, dtype=f32) if total > 0 and total <= F32_MAX else np.zeros(dim, dtype=f32)
                if flags & LAST:
                    out[out_row] = res
                else:
                    acc[a_i] = res
            else:
                acc[a_i] = a


SLIPS = ("eps_dropped", "mean_over_n", "g_skipped", "first_ignored", "rows_reversed", "normalise_each_piece")


def _emulated(case, slip=None):
    acc, out = case.acc.copy(), np.full((N_OUT, case.dim), POISON, dtype=np.uint32).view(np.float32)
    emulate(case.x, case.g, acc, out, case.jobs, slip=slip)
    return acc, out


def _split_runs(pool, dim, seed=77):
    """40 rows pooled in one launch, as 13 + 27 and as 40 single-row launches: the three ``out`` rows.
    ``pool(x_bits, x, g_bits, g, acc, out, jobs)`` runs one launch in place."""
    rng = np.random.default_rng(seed)
    x_bits, x = bf16_of(rng.standard_normal((40, dim)).astype(np.float32) * np.float32(3.0))
    g_bits, g = bf16_of(1.0 + 0.1 * rng.standard_normal(dim))
    plans = [[[(0, 40, 0, 3, 0)]],
             [[(0, 13, 0, 1, -1)], [(13, 27, 0, 2, 0)]],
             [[(r, 1, 0, (FIRST if r == 0 else 0) | (LAST if r == 39 else 0), 0 if r == 39 else -1)] for r in range(40)]]
    outs = []
    for launches in plans:
        acc = np.full((1, dim), POISON, dtype=np.uint32).view(np.float32)
        out = np.full((1, dim), POISON, dtype=np.uint32).view(np.float32)
        for jobs in launches:
            acc, out = pool(x_bits, x, g_bits, g, acc, out, jobs)
        outs.append(out[0].view(np.uint32).copy())
    return outs


def _cpu_pool(slip=None):
    def pool(x_bits, x, g_bits, g, acc, out, jobs):
        emulate(x, g, acc, out, jobs, slip=slip)
        return acc, out
    return pool


@pytest.mark.parametrize("dim", DIMS)
def test_fp32_emulation_is_inside_the_bounds(dim):
    for case in cases(dim):
        acc, out = _emulated(case)
        assert check(case, acc, out) <= 1.0


def test_fp32_emulation_is_split_invariant():
    one, two, forty = _split_runs(_cpu_pool(), 264)
    assert np.array_equal(one, two) and np.array_equal(one, forty)


@pytest.mark.parametrize("slip", SLIPS)
def test_a_slip_breaks_the_bound_or_the_split_invariance(slip):
    broke_bound = False
    for case in cases(264):
        acc, out = _emulated(case, slip)
        try:
            check(case, acc, out)
        except AssertionError:
            broke_bound = True
    one, two, forty = _split_runs(_cpu_pool(slip), 264)
    broke_split = not (np.array_equal(one, two) and np.array_equal(one, forty))
    assert broke_bound or broke_split, slip
    # which of the two each slip breaks, so that a change of the cases that lets one through shows here
    assert (broke_bound, broke_split) == {"eps_dropped": (True, False), "mean_over_n": (True, True),
                                          "g_skipped": (True, False), "first_ignored": (True, False),
                                          "rows_reversed": (False, True),
                                          "normalise_each_piece": (True, True)}[slip]


# ---------------------------------------------------------------- the kernel
def _dev(bits_or_f32, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(bits_or_f32))
    if dtype is torch.bfloat16:
        t = t.view(torch.int16).view(torch.bfloat16)
    return t.cuda()


def _gpu_pool(x_bits, x, g_bits, g, acc, out, jobs):
    d_acc, d_out = _dev(acc), _dev(out)
    ops.embed_pool_(_dev(x_bits.view(np.int16), torch.bfloat16), _dev(g_bits.view(np.int16), torch.bfloat16), d_acc,
                    d_out, jobs, EPS)
    torch.cuda.synchronize()
    return d_acc.cpu().numpy(), d_out.cpu().numpy()


@gpu
@cuda
@pytest.mark.parametrize("dim", DIMS)
def test_kernel_is_inside_the_bounds_and_writes_nothing_else(dim):
    for case in cases(dim):
        out0 = np.full((N_OUT, dim), POISON, dtype=np.uint32).view(np.float32)
        acc, out = _gpu_pool(case.x_bits, case.x, case.g_bits, case.g, case.acc, out0, case.jobs)
        worst = check(case, acc, out)
        print(f"embed_pool dim {dim} {case.name}: worst error / bound = {worst:.3f}")
        acc2, out2 = _gpu_pool(case.x_bits, case.x, case.g_bits, case.g, case.acc, out0, case.jobs)
        assert np.array_equal(acc.view(np.uint32), acc2.view(np.uint32))  # reruns are bit-identical
        assert np.array_equal(out.view(np.uint32), out2.view(np.uint32))


@gpu
@cuda
@pytest.mark.parametrize("dim", (264, 5120))
def test_kernel_is_split_invariant(dim):
    one, two, forty = (torch.from_numpy(o.view(np.int32)) for o in _split_runs(_gpu_pool, dim))
    assert torch.equal(one, two) and torch.equal(one, forty)
    assert not (one == int(POISON)).any()


@gpu
@cuda
def test_kernel_validates_before_launching():
    assert ops.MAX_EMBED_JOBS == 16 == ops.lib().p2pt_max_embed_jobs()
    dim = 264
    bf, f32 = torch.bfloat16, torch.float32
    x = torch.ones(17, dim, dtype=bf, device="cuda")
    g = torch.ones(dim, dtype=bf, device="cuda")
    poison = lambda n: torch.full((n, dim), int(POISON), dtype=torch.int32, device="cuda").view(f32)
    acc, out = poison(N_ACC), poison(N_OUT)
    ok = [(0, 4, 1, 3, 0)]
    wide = torch.ones(17, 2 * dim, dtype=bf, device="cuda")
    bad = [
        (x.float(), g, acc, out, ok), (x, g.float(), acc, out, ok), (x, g, acc.double(), out, ok),   # dtypes
        (x, g, acc, out.to(torch.float16), ok),
        (x.cpu(), g, acc, out, ok), (x, g.cpu(), acc, out, ok), (x, g, acc.cpu(), out, ok),          # devices
        (x, g, acc, out.cpu(), ok),
        (wide[:, ::2], g, acc, out, ok), (x, wide[0, ::2], acc, out, ok),                             # contiguity
        (x, g, poison(2 * N_ACC)[::2], out, ok), (x, g, acc, poison(2 * N_OUT)[::2], ok),
        (torch.ones(65, dim, dtype=bf, device="cuda"), g, acc, out, ok),                              # rows <= 64
        (x[0], g, acc, out, ok), (x[:0], g, acc, out, ok),                                            # [rows, dim]
        (torch.ones(4, 12, dtype=bf, device="cuda"), torch.ones(12, dtype=bf, device="cuda"),         # dim % 8
         torch.zeros(2, 12, device="cuda"), torch.zeros(2, 12, device="cuda"), ok),
        (x, torch.ones(dim + 8, dtype=bf, device="cuda"), acc, out, ok), (x, g[None], acc, out, ok),  # norm_weight (dim,)
        (x, g, poison(N_ACC)[:, :256].contiguous(), out, ok), (x, g, acc, out[0], ok),                # acc, out [n, dim]
        (x, g, acc, out, []), (x, g, acc, out, [(r, 1, r, 3, r) for r in range(17)]),                 # 1..16 jobs
        (x, g, acc, out, [(0, 4, 1, 3)]), (x, g, acc, out, [(0, 4, 1, 3, 0.0)]),                     # five plain ints
        (x, g, acc, out, [(0, 4, 1, True, 0)]), (x, g, acc, out, [5]),
        (x, g, acc, out, [(0, 0, 1, 3, 0)]), (x, g, acc, out, [(0, -1, 1, 3, 0)]),                   # n >= 1
        (x, g, acc, out, [(14, 4, 1, 3, 0)]), (x, g, acc, out, [(-1, 4, 1, 3, 0)]),                  # row0 + n <= rows
        (x, g, acc, out, [(17, 1, 1, 3, 0)]),
        (x, g, acc, out, [(0, 4, N_ACC, 3, 0)]), (x, g, acc, out, [(0, 4, -1, 3, 0)]),               # acc in range
        (x, g, acc, out, [(0, 4, 1, 3, N_OUT)]), (x, g, acc, out, [(0, 4, 1, 2, -1)]),               # out_row in range
        (x, g, acc, out, [(0, 4, 1, 4, 0)]), (x, g, acc, out, [(0, 4, 1, -1, 0)]),                   # flags
        (x, g, acc, out, [(0, 4, 1, 3, 0), (4, 4, 1, 3, 1)]),                                        # an acc row twice
        (x, g, acc, out, [(0, 4, 1, 3, 0), (4, 4, 2, 3, 0)]),                                        # an out row twice
        (x, g, acc, out, [(0, 4, 1, 1, 0)]), (x, g, acc, out, [(0, 4, 1, 0, 3)]),                    # no "last": out_row -1
    ]
    for n, (xx, gg, aa, oo, jobs) in enumerate(bad):
        with pytest.raises((TypeError, ValueError)):
            ops.embed_pool_(xx, gg, aa, oo, jobs, EPS)
            pytest.fail(f"bad call {n} was launched")
    for eps in (-1.0, float("nan"), float("inf"), "1e-5", None):
        with pytest.raises((TypeError, ValueError)):
            ops.embed_pool_(x, g, acc, out, ok, eps)
    torch.cuda.synchronize()
    assert (acc.view(torch.int32) == int(POISON)).all() and (out.view(torch.int32) == int(POISON)).all()
    ops.embed_pool_(x, g, acc, out, ok, EPS)  # and the good call does run
    torch.cuda.synchronize()
    assert torch.allclose(out[0], torch.full((dim,), dim ** -0.5, device="cuda"), rtol=1e-5, atol=0)
    assert (acc.view(torch.int32) == int(POISON)).all() and (out[1:].view(torch.int32) == int(POISON)).all()
