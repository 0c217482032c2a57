"""The fused decode step at the shapes of the checkpoints it serves, against fp64 (decode_fused.hip).

tests/test_gpu_fused_stages.py and its neighbours hold every kernel of the step to fp64 at vocab 512, hidden sizes up
to 2048 and ffn up to 2816. Llama-3.x (vocab 128256, dim 4096 / 8192, ffn 14336) and Qwen2.5 / Qwen3 (vocab 151936 /
152064, dim 3584 / 4096, ffn 18944) lie outside that range, and three code paths run only there. The helpers, the
references and the bounds are the stages file's (``gemm_ref``, ``rounded``, ``stage_lm_head``, ``stage_ratios``,
``first_argmax``, ``worst``); no tolerance is fixed here.

A. The LM head and ``k_argmax_merge`` at served vocabularies. A merge thread walks the per-block winners (one per
   32 columns) in trips of 8 * 256, so a second trip needs vocab > 65536 and a third vocab > 131072. One-layer
   models of the stages file's smallest shape (dim 256, ffn 512, 4/2 heads of 64) with ``wo`` and ``w_down`` zero:
   the final residual is then embed[token] exactly (bf(r + bf(0)) = r), the LM head's input is known before any
   launch, and only the vocabulary is large. 65568 is the smallest vocabulary with a second trip (2049 winners, the
   trip holds one); 128256, 151936 and 152064 are the served ones (4008, 4748 and 4752 winners; two, three and three
   trips). The LM head is random with planted rows, lm_head[t] = bf16(ALPHA * embed[token of row m]), written into
   the table the kernel reads: row m's logit at t is about 16, every other about N(0, 1), so the fp64 reference
   alone decides the id (asserted on the CPU). The targets sit at the trip edges (65535 | 65536, 131071 | 131072),
   the block edges (0, 31, 32, 65567, V - 32, V - 1) and, for tie rows, at t, t + 65536 and t + 131072 with one
   vector: bit-equal logits in different trips of the same merge thread, of which the lowest id must win. Every
   logit is judged, ids must equal the first maximum of the observed logits and the planted target, the
   per-block winners (am_val, am_idx) must be each block's first maximum, and rows past ``emit_rows`` keep their
   sentinels. FP8 weights with general row scales run at 65568 and 151936 (``wscale[n]`` up to n = 151935), judged
   as tests/test_gpu_weight_fp8.py's ``test_general_scales_match_fp64`` judges them: the stage bound as it stands on
   the weights q * s in fp64. CPU companions: an fp32 emulation of the two-stage argmax with the kernel's trip
   structure returns the targets, and five slips of it each change an id.

B. Weight byte offsets from 2^30 to the 2 GiB bound. ``k_skinny`` addresses its operands with 32-bit byte offsets;
   the LM heads of Qwen3-8B (151936 x 4096, 1.24e9 bytes) and Llama-3.x-70B (128256 x 8192, 2.10e9 bytes, 46 MB
   under the bound) are the served weights that reach them, so nothing smaller does. Built on the device, the layer
   kept small (4/2 heads of 64, ffn 512), the fp64 reference computed there in column blocks from the tensor the
   kernel read. Planted targets on either side of the first column at byte offset 2^30, and at V - 32 and V - 1.
   ``p2pt_skinny_gemm`` / ``ops.skinny_gemm`` had no such bound and now refuse an operand of 2 GiB or more.

C. One layer at Llama-3.1-8B's widths (dim 4096, ffn 14336, 32/8 heads of 128) and Qwen2.5-7B's (dim 3584, ffn
   18944, 28/4 heads of 128, QKV bias) at vocab 512, stage by stage with ``stage_ratios``, references on the device:
   grids of 224 to 448 column tiles, 448 sum-of-squares partials (dim 3584 in two K parts), wave shares of 37 k-steps
   (down at K 18944: nine load batches of 4 and one of 1), and the (K + 16) U bound at K 14336 and 18944. The layers
   are the models' own, so nothing smaller has these counts.

Largest |error| / bound seen on an MI355X (printed by each test as RATIO lines; three decimals; recorded here, the
tests assert <= 1.0). A: logits 0.978 .. 0.987 with bf16 weights, 0.978 .. 0.986 with FP8 weights, 0.970 on the
repeated head (E is ~1e-5 of a logit and the half ulp of the store ~4e-3, so an element next to a rounding tie sits
just under 1); every id, winner and sentinel exact. B: logits 0.583 / 0.815 at 151936 x 4096 (1 / 17 rows), 0.614 /
0.735 at 128256 x 8192, the standalone GEMM at 128256 x 8192 0.285 (E grows with K and widens the bound); planted
margins 11.0 .. 12.9. C, Llama-3.1-8B's layer (1, 17 rows): q 0.296, k 0.263, v 0.434, attn 0.870, o 1.000, h 0.656,
down 0.379, logits 0.433; Qwen2.5-7B's (1, 8, 9 rows): q 0.957, k 0.816, v 0.559, attn 0.835, o 1.000, h 0.634, down
0.286, logits 0.504 (o at 17, 8 and 9 rows rounds to 1.000 from below, as q and k do in the neighbours' records:
one element next to a rounding tie). Every GPU case takes under 1.5 s, most under 0.1 s; the CPU tests 12 s together.
"""
import functools
import math
from dataclasses import dataclass, replace
from types import SimpleNamespace

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig
import test_gpu_qwen2 as qw2
from test_gpu_fused_stages import (BF, F64, SENTINEL_BITS, SENTINEL_ID, Case, _cfg, first_argmax, gemm_ref,
                                   plan_strings, rounded, stage_lm_head, stage_ratios, step_plan, worst)

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu

TRIP = 8 * 256  # per-block winners one trip of k_argmax_merge covers: 256 threads x 8 loads
PART = 32  # columns per winner: the LM head's <4,2,ARGMAX,..> blocks hold two 16-column subtiles
NO_WINNER = 0x7FFFFFFF  # the index of a block (or a row) without a winner, and the merge's out-of-range filler
HIP_INVALID_VALUE = 1


def decided_by(ref, bound, plants):
    """The smallest margin over the rows by which the fp64 reference alone decides a planted row: the planted
    logit less its bound (the least over a tie row's ids) minus the largest of every other logit plus its bound.
    Positive: whatever the kernel computes inside the bounds, the planted id holds the row's maximum."""
    margins = []
    for m, ids in enumerate(plants):
        ids = list(ids)
        low = (ref[m, ids] - bound[m, ids]).min()
        rest = ref[m] + bound[m]
        rest[ids] = -math.inf
        margins.append(float(low - rest.max()))
    return min(margins)


def block_winners(logits):
    """(am_val, am_idx) [rows, V / 32] of logits [rows, V]: each 32-column block's maximum and its first index, as
    the LM head's epilogue leaves them (a NaN never wins; a block of NaN has -inf and NO_WINNER)."""
    l = logits.to(torch.float32)
    l = torch.where(torch.isnan(l), torch.full_like(l, -math.inf), l).view(l.shape[0], -1, PART)
    nan = torch.isnan(logits.to(torch.float32)).view(l.shape)
    val = l.amax(-1)
    col = torch.arange(l.shape[1] * PART).view(1, -1, PART).expand_as(l)
    idx = torch.where((l == val[..., None]) & ~nan, col, NO_WINNER).amin(-1)
    return val, idx


# ================================================================ A. the LM head at served vocabularies
ALPHA = 2.0 ** -4  # planted logit = ALPHA sqrt(256) |x| = about 16 for x ~ N(0, 1): see the module docstring
A_ROWS = 64
A_CFG = _cfg(256, 512, 4, 2, 64, 64)


@dataclass(frozen=True)
class HeadCase:
    vocab: int
    rows: int  # the case runs the first ``rows`` token rows of its vocabulary's 64
    emit_rows: int = 0
    fp8: bool = False
    dup: bool = False  # the LM head is 8 distinct rows repeated over the whole vocabulary (no planted rows)
    nan_row: int = -1  # this row's embedding row is NaN on the device

    @property
    def name(self):
        return (f"v{self.vocab}-r{self.rows}" + (f"-emit{self.emit_rows}" if self.emit_rows else "")
                + ("-fp8" if self.fp8 else "") + ("-dup" if self.dup else "") + ("-nan" if self.nan_row >= 0 else ""))

    @property
    def emit(self):
        return self.emit_rows or self.rows

    @property
    def cfg(self):
        return replace(A_CFG, vocab=self.vocab)

    @property
    def pos(self):
        return tuple((7 * r + 3) % 61 for r in range(self.rows))


def _head_cases():
    cs = []
    for vocab in (65568, 151936):
        for fp8 in (False, True):
            cs += [HeadCase(vocab, 1, fp8=fp8), HeadCase(vocab, 5, emit_rows=3, fp8=fp8), HeadCase(vocab, 17, fp8=fp8),
                   HeadCase(vocab, 64, fp8=fp8)]
    cs += [HeadCase(128256, 16), HeadCase(152064, 33)]
    cs += [HeadCase(151936, 5, dup=True), HeadCase(151936, 5, nan_row=3)]
    return cs


HEAD_CASES = _head_cases()
HEAD_IDS = [c.name for c in HEAD_CASES]


def plants(vocab):
    """The planted ids of the 64 token rows, one tuple per row (a tie row has two or three ids in different trips;
    its first, the lowest, is the target). The rows a small case runs come first: row 0 the first winner of trip
    two, row 1 the last of trip one, row 2 a tie across every trip, row 3 the last column."""
    def tie(t):
        return tuple(n for n in (t, t + 65536, t + 131072) if n < vocab)

    t1, t2 = (100, 40000) if vocab > 105536 else (7, 20)
    want = [(65536,), (65535,), tie(t1), (vocab - 1,), (0,), (31,), (32,), (65567,), (vocab - 32,)]
    if vocab > 131072:
        want += [(131071,), (131072,)]
    want.append(tie(t2))
    out, seen = [], set()
    for ids in want:
        if not seen & set(ids):
            out.append(ids)
            seen |= set(ids)
    g = torch.Generator().manual_seed(vocab)
    for n in torch.randperm(vocab, generator=g).tolist():  # the rest: anywhere, so in every trip
        if len(out) == A_ROWS:
            break
        if n not in seen:
            out.append((n,))
            seen.add(n)
    return out


@dataclass
class HeadInputs:
    tokens: torch.Tensor  # [64], distinct
    bf16: list  # the bf16 weight table (CPU)
    fp8: list | None  # the FP8 table with its scales behind it, at the vocabularies that run it
    plants: list


@functools.lru_cache(maxsize=None)
def head_inputs(vocab, dup=False) -> HeadInputs:
    """Seeded inputs of a vocabulary, made once and shared (never modified) by its cases: the tables are written
    directly in the fused layout (``FusedLlamaDecoder``), with wo and w_down zero and the norm slots, which the
    kernels do not read, ones."""
    g = torch.Generator().manual_seed(7 * vocab + dup)
    embed = torch.randn(vocab, 256, generator=g).to(BF)
    tokens = torch.randperm(vocab - 2, generator=g)[:A_ROWS] + 1
    tokens[0], tokens[1] = vocab - 1, 0  # the table's last row and its first
    lm = torch.randn(vocab, 256, generator=g) / 16
    planted = plants(vocab)
    if dup:
        lm = lm[:8].repeat(vocab // 8, 1).contiguous()
    else:
        x = embed[tokens].float()
        for m, ids in enumerate(planted):
            lm[list(ids)] = ALPHA * x[m]  # exact in bf16: ALPHA is a power of two
    ones = torch.ones(256, dtype=BF)
    wqkv, wgu = torch.randn(512, 256, generator=g) / 16, torch.randn(1024, 256, generator=g) / 16
    wo, wdown = torch.zeros(256, 256), torch.zeros(256, 512)
    gemms = (lm, wqkv, wo, wgu, wdown)
    table = [embed, ones, lm.to(BF), ones, wqkv.to(BF), wo.to(BF), ones, wgu.to(BF), wdown.to(BF)]
    f8 = None
    if vocab in (65568, 151936) and not dup:
        q = [ops.quantize_weight_fp8(w) for w in gemms]
        f8 = [embed, ones, q[0][0], ones, q[1][0], q[2][0], ones, q[3][0], q[4][0]] + [s for _, s in q]
    return HeadInputs(tokens, table, f8, planted)


def reference_head(vocab, fp8, dup=False):
    """The LM head as the references read it: the bf16 tensor, or q * s in fp64 (exact), which
    ``ops.dequantize_weight_fp8`` gives to within its one fp32 rounding."""
    inp = head_inputs(vocab, dup)
    if not fp8:
        return inp.bf16[2]
    q, s = inp.fp8[2], inp.fp8[9]
    return q.to(F64) * s.to(F64)[:, None]


@functools.lru_cache(maxsize=None)
def head_reference(vocab, fp8=False, dup=False):
    """``stage_lm_head``'s fp64 logits and bounds [rows, vocab] of the token rows the vocabulary's cases emit."""
    inp = head_inputs(vocab, dup)
    n = max(c.emit for c in HEAD_CASES if (c.vocab, c.fp8, c.dup) == (vocab, fp8, dup))
    case = Case("lm-head", replace(A_CFG, vocab=vocab), (0,) * n)
    return stage_lm_head(case, [None, None, reference_head(vocab, fp8, dup)], inp.bf16[0][inp.tokens[:n]])


@pytest.fixture(scope="module", autouse=True)
def _drop_the_tables_afterwards():
    yield
    head_inputs.cache_clear()
    head_reference.cache_clear()


def targets(case):
    return torch.tensor([ids[0] for ids in head_inputs(case.vocab).plants[:case.emit]])


def head_plan(case):
    c = case.cfg
    dims = ops.LlamaDims(vocab=c.vocab, dim=c.dim, n_layers=1, H=c.n_heads, Hkv=c.n_kv_heads, D=c.head_dim, ffn=c.ffn,
                         max_seq=c.max_seq, max_batch=case.rows + 1, eps=c.eps, theta=c.rope_theta)
    return dims, ops.step_plan(dims, case.rows, case.emit_rows)


def test_head_cases_reach_the_trips_they_claim():
    trips = {}
    for case in HEAD_CASES:
        _, p = head_plan(case)
        assert p.am_parts == p.lm_head.grid_x == case.vocab // PART and (p.lm_head.nw, p.lm_head.tn) == (4, 2)
        assert p.lm_head.grid_y == -(-case.emit // 16)
        trips[case.vocab] = (p.am_parts, -(-p.am_parts // TRIP))
    assert trips == {65568: (2049, 2), 128256: (4008, 2), 151936: (4748, 3), 152064: (4752, 3)}
    need = {0, 31, 32, 65535, 65536, 65567, 131071, 131072}
    seen, ties = set(), set()
    for case in HEAD_CASES:
        if case.dup:
            continue
        rows = [ids for m, ids in enumerate(head_inputs(case.vocab).plants[:case.emit]) if m != case.nan_row]
        seen |= {ids[0] for ids in rows} | {ids[0] - case.vocab for ids in rows}  # V - 32 and V - 1 as -32, -1
        ties |= {(case.vocab, len(ids)) for ids in rows if len(ids) > 1}  # a tie over two trips, or over three
        assert len({n for ids in rows for n in ids}) == sum(len(ids) for ids in rows)  # every row its own target
        assert all(b - a == 65536 for ids in rows for a, b in zip(ids, ids[1:]))
    assert need <= seen and {-32, -1} <= seen
    assert ties >= {(65568, 2), (128256, 2), (151936, 3), (152064, 3)}


def test_fp8_reference_is_the_dequantised_weight():
    for vocab in (65568, 151936):
        inp = head_inputs(vocab)
        exact = reference_head(vocab, True)
        deq = ops.dequantize_weight_fp8(inp.fp8[2], inp.fp8[9])
        assert bool(((deq.to(F64) - exact).abs() <= 2.0 ** -24 * exact.abs()).all())
        s = inp.fp8[9]
        assert s.shape == (vocab,) and not bool((torch.frexp(s)[0] == 0.5).all())  # general scales, no powers of two


@pytest.mark.parametrize("key", sorted({(c.vocab, c.fp8) for c in HEAD_CASES if not c.dup}))
def test_the_reference_alone_decides_every_planted_row(key):
    vocab, fp8 = key
    ref, bound = head_reference(vocab, fp8)
    margin = decided_by(ref, bound, head_inputs(vocab).plants[:ref.shape[0]])
    print("MARGIN", vocab, "fp8" if fp8 else "bf16", round(margin, 3))
    assert margin > 0


def emulate_argmax(logits, slip=None):
    """The two-stage argmax in fp32 with the kernels' structure: per-32-column winners (first index on ties), then
    per row 256 threads that each walk the winners 8 at a time, trip after trip, carrying (value, index), and the
    first-index maximum over the threads. ``slip`` names one mistake of the merge."""
    val, idx = block_winners(logits)
    R, parts = val.shape
    trips = -(-parts // TRIP)
    pad = trips * TRIP - parts
    val = torch.cat([val, torch.full((R, pad), -math.inf)], 1).view(R, trips, 8, 256)
    idx = torch.cat([idx, torch.full((R, pad), NO_WINNER)], 1).view(R, trips, 8, 256)
    b, i = torch.full((R, 256), -math.inf), torch.full((R, 256), NO_WINNER)
    for t in range(trips):
        if slip == "first_trip_only" and t > 0:
            break
        if slip == "partial_trip_skipped" and (t + 1) * TRIP > parts:
            break
        for j in range(8):
            pv, pi = val[:, t, j], idx[:, t, j]
            take = (pv > b) | ((pv == b) & (pi < i))
            if slip == "later_equal_replaces" and t > 0:
                take = pv >= b
            if slip == "index_in_16_bits":
                pi = pi & 0xFFFF
            b, i = torch.where(take, pv, b), torch.where(take, pi, i)
    top = b.amax(1, keepdim=True)
    i = torch.where(b == top, i, NO_WINNER).amin(1)
    return i if slip == "filler_index_wins" else torch.where(i == NO_WINNER, 0, i)


SLIPS = ("first_trip_only", "later_equal_replaces", "index_in_16_bits", "partial_trip_skipped", "filler_index_wins")


def emulated_logits(case):
    """The reference logits rounded to bf16, as fp32: what the argmax stages see (the NaN row as NaN)."""
    ref, _ = head_reference(case.vocab, case.fp8, case.dup)
    l = ref[:case.emit].to(BF).float()
    if 0 <= case.nan_row < case.emit:
        l[case.nan_row] = math.nan
    return l


def expected_ids(case):
    want = targets(case)
    if 0 <= case.nan_row < case.emit:
        want[case.nan_row] = 0
    return want


@pytest.mark.parametrize("case", HEAD_CASES, ids=HEAD_IDS)
def test_argmax_emulation_returns_the_targets(case):
    l = emulated_logits(case)
    ids = emulate_argmax(l)
    if case.dup:
        assert torch.equal(ids, first_argmax(l)) and int(ids.max()) < 8
    else:
        assert torch.equal(ids, expected_ids(case))


@pytest.mark.parametrize("slip", SLIPS)
def test_every_merge_slip_changes_an_id(slip):
    changed = {c.name for c in HEAD_CASES if not torch.equal(emulate_argmax(emulated_logits(c), slip),
                                                             emulate_argmax(emulated_logits(c)))}
    print("SLIP", slip, sorted(changed))
    assert changed
    planted = {c.name for c in HEAD_CASES if not c.dup}
    if slip in ("first_trip_only", "index_in_16_bits"):  # row 0's target is 65536 at every vocabulary
        assert changed >= planted
    if slip == "later_equal_replaces":  # the tie rows, and every row of the repeated head
        assert changed == {c.name for c in HEAD_CASES if c.emit >= 3}
    if slip == "partial_trip_skipped":  # the last trip is partial at every vocabulary
        assert {c.vocab for c in HEAD_CASES if c.name in changed} == {65568, 128256, 151936, 152064}
    if slip == "filler_index_wins":
        assert changed == {c.name for c in HEAD_CASES if c.nan_row >= 0}


def run_head(case):
    """One step of the case on the device: (logits, ids, final residual rows, am_val, am_idx) on the CPU, the last
    two [emit, parts]."""
    inp = head_inputs(case.vocab, case.dup)
    B = case.rows
    dims, plan = head_plan(case)
    table = [t.cuda() for t in (inp.fp8 if case.fp8 else inp.bf16)]
    tokens = inp.tokens[:B].cuda()
    if case.nan_row >= 0:
        table[0][tokens[case.nan_row]] = math.nan
    shape = (1, B + 1, case.cfg.max_seq, case.cfg.n_kv_heads, case.cfg.head_dim)
    kc, vc = torch.zeros(shape, dtype=BF, device="cuda"), torch.zeros(shape, dtype=BF, device="cuda")
    dec = ops.FusedLlamaDecoder(dims, table, kc, vc, weight_fp8=case.fp8)
    logits = torch.empty(B, case.vocab, dtype=BF, device="cuda")
    logits.view(torch.int16).fill_(SENTINEL_BITS)
    ids = torch.full((B,), SENTINEL_ID, dtype=torch.int64, device="cuda")
    dec.step(tokens, torch.tensor(case.pos, dtype=torch.int32, device="cuda"), logits, ids, None, case.emit_rows)
    torch.cuda.synchronize()
    views = dec.workspace_views()
    am = [views[k][:plan.am_parts, :case.emit].T.cpu() for k in ("am_val", "am_idx")]
    return logits.cpu(), ids.cpu(), views["resid"][:B].cpu(), am[0], am[1]


@cuda
@gpu
@pytest.mark.parametrize("case", HEAD_CASES, ids=HEAD_IDS)
def test_lm_head_and_merge_at_served_vocabularies(case):
    inp = head_inputs(case.vocab, case.dup)
    ref, bound = head_reference(case.vocab, case.fp8, case.dup)
    emit, nan = case.emit, case.nan_row
    logits, ids, resid, am_val, am_idx = run_head(case)
    fine = [m for m in range(emit) if m != nan]
    # The LM head's input is what the reference took: the final residual is embed[token], bit for bit.
    assert torch.equal(resid[fine].view(torch.int16), inp.bf16[0][inp.tokens[fine]].view(torch.int16))
    ratio = worst(logits[fine], (ref[fine], bound[fine]))  # every logit of every emitting row
    print("RATIO", case.name, round(ratio, 3))
    assert ratio <= 1.0
    assert torch.equal(ids[fine], first_argmax(logits[fine]))  # (a row of NaN has no first maximum: below)
    if case.dup:  # every maximum ties 18992 times over, in all three trips: the first is one of the 8 distinct rows
        assert int(ids[:emit].max()) < 8, ids
    else:
        assert torch.equal(ids[:emit], expected_ids(case)), (ids[:emit], expected_ids(case))
    if nan >= 0:  # the row of NaN has no winner, in any block or in the merge: id 0
        assert bool(torch.isnan(logits[nan].float()).all()) and int(ids[nan]) == 0
    want_val, want_idx = block_winners(logits[:emit])
    assert torch.equal(am_val, want_val) and torch.equal(am_idx, want_idx.to(torch.int32))
    # Rows at or past emit_rows keep what logits and ids held before the step.
    assert bool((logits[emit:].view(torch.int16) == SENTINEL_BITS).all())
    assert bool((ids[emit:] == SENTINEL_ID).all())


# ================================================================ B. byte offsets from 2^30 to the 2 GiB bound
@dataclass(frozen=True)
class WideHead:
    vocab: int
    dim: int
    rows: int

    @property
    def name(self):
        return f"v{self.vocab}-d{self.dim}-r{self.rows}"

    @property
    def cfg(self):
        return replace(_cfg(self.dim, 512, 4, 2, 64, 64), vocab=self.vocab)

    @property
    def first_past_2_30(self):  # the first LM-head row whose byte offset is >= 2^30
        return (1 << 30) // (2 * self.dim)

    @property
    def plants(self):
        n0, V = self.first_past_2_30, self.vocab
        edge = [n0, n0 - 1, V - 32, V - 1]
        rest = [(48271 * m + 11) % V for m in range(4, self.rows)]  # anywhere; distinct, and off the edges
        assert len(set(edge + rest)) == max(4, self.rows)
        return [(n,) for n in (edge + rest)[:self.rows]]


WIDE_HEADS = [WideHead(151936, 4096, 1), WideHead(151936, 4096, 17), WideHead(128256, 8192, 1),
              WideHead(128256, 8192, 17)]
WIDE_BYTES = {(151936, 4096): 1_244_659_712, (128256, 8192): 2_101_346_304}


def wide_dims(case):
    c = case.cfg
    return ops.LlamaDims(vocab=c.vocab, dim=c.dim, n_layers=1, H=c.n_heads, Hkv=c.n_kv_heads, D=c.head_dim, ffn=c.ffn,
                         max_seq=c.max_seq, max_batch=case.rows + 1, eps=c.eps, theta=c.rope_theta)


def test_wide_heads_are_the_served_ones_and_reach_2_30():
    for case in WIDE_HEADS:
        nbytes = case.vocab * case.dim * 2
        assert nbytes == WIDE_BYTES[case.vocab, case.dim] and 1 << 30 < nbytes < ops.GEMM_OPERAND_LIMIT
        n0 = case.first_past_2_30
        assert n0 == {4096: 131072, 8192: 65536}[case.dim] and n0 * case.dim * 2 == 1 << 30 and n0 < case.vocab - 32
        p = ops.step_plan(wide_dims(case), case.rows)
        assert p.lm_head.ss_in == p.down.grid_x == case.dim // 16  # 512 partials at 8192: the late loop from 128
        assert (p.lm_head.nw, p.lm_head.tn, p.lm_head.um, p.am_parts) == (4, 2, 4, case.vocab // PART)
    assert ops.GEMM_OPERAND_LIMIT - WIDE_BYTES[128256, 8192] < 47 << 20


def test_the_plan_stops_at_2_gib():
    def dims(vocab):
        return ops.LlamaDims(vocab=vocab, dim=8192, n_layers=1, H=4, Hkv=2, D=64, ffn=512, max_seq=64, max_batch=2,
                             eps=1e-5, theta=1e4)

    out = ops.StepPlan()
    assert 131040 * 8192 * 2 == (1 << 31) - 524288 and 131072 * 8192 * 2 == 1 << 31
    for vocab, ok in ((128256, True), (131040, True), (131072, False), (131104, False)):
        assert (ops.lib().p2pt_llama_plan(dims(vocab), 1, 0, out) == 0) == ok, vocab
        assert (ops.lib().p2pt_llama_ws_bytes(dims(vocab)) != 0) == ok, vocab
        if ok:
            assert ops.step_plan(dims(vocab), 1).lm_head.N == vocab
        else:
            with pytest.raises(ValueError):
                ops.step_plan(dims(vocab), 1)


def test_skinny_gemm_refuses_an_operand_of_2_gib_from_the_shapes_alone():
    # Tensors without storage: the refusal comes before anything looks at a device.
    meta = lambda *shape: torch.empty(*shape, dtype=BF, device="meta")
    with pytest.raises(ValueError, match="below 2 GiB"):
        ops.skinny_gemm(meta(3, 8192), meta(131072, 8192))  # w: exactly 2^31 bytes
    with pytest.raises(ValueError, match="below 2 GiB"):
        ops.skinny_gemm(meta(1, 4096), meta(1 << 20, 4096))  # 2^33: the 32-bit product would wrap to 0
    with pytest.raises(ValueError, match="below 2 GiB"):
        ops.skinny_gemm(meta(64, 1 << 24), meta(32, 1 << 24))  # x: 2^31 bytes
    with pytest.raises(ValueError, match="HIP device"):
        ops.skinny_gemm(meta(3, 8192), meta(131040, 8192))  # 2^31 - 524288 bytes pass the size check


def device_rng(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def device_randn(g, *shape, scale=1.0):
    """bf16 normal draws on the device, times a power of two (exact)."""
    return torch.randn(*shape, generator=g, device="cuda", dtype=BF) * scale


def blocked(fn, w, block=16384):
    """``fn(rows of w)`` -> (reference, bound), over blocks of w's rows (the outputs' columns): an fp64 copy of a
    whole 2 GB weight is never made."""
    parts = [fn(w[n:n + block]) for n in range(0, w.shape[0], block)]
    return torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)


@cuda
@gpu
@pytest.mark.parametrize("case", WIDE_HEADS, ids=[c.name for c in WIDE_HEADS])
def test_lm_head_with_byte_offsets_past_2_30(case):
    V, K, B = case.vocab, case.dim, case.rows
    g = device_rng(V + K + B)
    tokens = torch.tensor([V - 1, 0] + [(7919 * m + 5) % V for m in range(2, B)][:max(0, B - 2)],
                          device="cuda")[:B]
    assert len(set(tokens.tolist())) == B
    embed = torch.zeros(V, K, dtype=BF, device="cuda")  # full size; only the token rows are read
    x = device_randn(g, B, K)
    embed[tokens] = x
    lm = device_randn(g, V, K, scale=2.0 ** -6 if K == 4096 else 2.0 ** -7)
    planted = case.plants
    alpha = 16.0 / K  # a power of two: the planted logit is alpha sqrt(K) |x|, about 16
    for m, (t,) in enumerate(planted):
        lm[t] = x[m] * alpha
    ones = torch.ones(K, dtype=BF, device="cuda")
    zeros = lambda *s: torch.zeros(*s, dtype=BF, device="cuda")
    table = [embed, ones, lm, ones, device_randn(g, 512, K, scale=2.0 ** -6), zeros(K, 256), ones,
             device_randn(g, 1024, K, scale=2.0 ** -6), zeros(K, 512)]
    c = case.cfg
    ref, bound = blocked(lambda w: (lambda y, E: (y, rounded(y, E)))(*gemm_ref(x, w, c.eps)), lm)
    margin = decided_by(ref, bound, planted)  # before the kernel's output is looked at
    assert margin > 0, margin
    ref, bound = ref.cpu(), bound.cpu()

    shape = (1, B + 1, c.max_seq, c.n_kv_heads, c.head_dim)
    dec = ops.FusedLlamaDecoder(wide_dims(case), table, zeros(*shape), zeros(*shape))
    logits = torch.empty(B, V, dtype=BF, device="cuda")
    ids = torch.full((B,), SENTINEL_ID, dtype=torch.int64, device="cuda")
    pos = torch.tensor([(7 * r + 3) % 61 for r in range(B)], dtype=torch.int32, device="cuda")
    dec.step(tokens, pos, logits, ids)
    torch.cuda.synchronize()
    assert torch.equal(dec.workspace_views()["resid"][:B].view(torch.int16), x.view(torch.int16))
    logits, ids = logits.cpu(), ids.cpu()
    ratio = worst(logits, (ref, bound))  # every logit
    print("RATIO", case.name, round(ratio, 3), "margin", round(margin, 3))
    assert ratio <= 1.0
    assert torch.equal(ids, first_argmax(logits))
    assert ids.tolist() == [t for (t,) in planted]


@cuda
@gpu
def test_skinny_gemm_at_llama_70b_lm_head_matches_fp64():
    g = device_rng(70)
    x = device_randn(g, 3, 8192)
    w = device_randn(g, 128256, 8192, scale=2.0 ** -7)
    got = ops.skinny_gemm(x, w)
    ref, bound = blocked(lambda wb: (lambda y, E: (y, rounded(y, E)))(*gemm_ref(x, wb)), w)
    ratio = worst(got, (ref, bound))  # every output element
    print("RATIO skinny 128256x8192 r3", round(ratio, 3))
    assert got.shape == (3, 128256) and ratio <= 1.0


@cuda
@gpu
def test_skinny_gemm_refuses_a_2_gib_weight():
    w = torch.empty(131072, 8192, dtype=BF, device="cuda")  # uninitialised: it is never read
    x = torch.zeros(3, 8192, dtype=BF, device="cuda")
    with pytest.raises(ValueError, match="below 2 GiB"):
        ops.skinny_gemm(x, w)
    out = torch.zeros(3, 131072, dtype=BF, device="cuda")
    rc = ops.lib().p2pt_skinny_gemm(ops._p(x), ops._p(w), ops._p(out), 3, 131072, 8192, ops._stream(x))
    torch.cuda.synchronize()
    assert rc == HIP_INVALID_VALUE and not bool(out.any())  # refused by the library too, and nothing written
    # x of 2^31 bytes against a small weight: the same refusal, from the sizes alone (both pointers are w's)
    assert ops.lib().p2pt_skinny_gemm(ops._p(w), ops._p(w), ops._p(out), 64, 32, 1 << 24,
                                      ops._stream(x)) == HIP_INVALID_VALUE


# ================================================================ C. one layer at two served models' widths
LLAMA_8B = LlamaConfig(vocab=512, dim=4096, n_layers=1, n_heads=32, n_kv_heads=8, head_dim=128, ffn=14336,
                       max_seq=128, eps=1e-5, rope_theta=5e5)
QWEN_7B = LlamaConfig(vocab=512, dim=3584, n_layers=1, n_heads=28, n_kv_heads=4, head_dim=128, ffn=18944, max_seq=128,
                      eps=1e-6, rope_theta=1e6, qkv_bias=True)


def _ragged(rows):  # position 0, the cache's last position, and a spread between
    return tuple([0, 127, 64, 1, 100][:min(rows, 5)] + [(11 * r + 6) % 127 for r in range(5, rows)])


LAYER_CASES = [Case("llama-8b-r1", LLAMA_8B, (93,), seed=1), Case("llama-8b-r17", LLAMA_8B, _ragged(17), seed=2),
               Case("qwen-7b-r1", QWEN_7B, (127,), seed=3), Case("qwen-7b-r8", QWEN_7B, _ragged(8), seed=4),
               Case("qwen-7b-r9", QWEN_7B, _ragged(9), seed=5)]
LAYER_IDS = [c.name for c in LAYER_CASES]

# What each case launches (qkv, attn, o, gate_up, down, lm_head), recorded from ``ops.step_plan``.
_L = ("<8,1,ROPE,4>", "<8,1,RESID,4>", "<8,1,SILU,4>", "<8,1,RESID,4>", "<4,2,ARGMAX,4>")
_Q, _QK = "<8,1,ROPE_BIAS,4>", "<8,1,RESID,4> kp2"
EXPECTED_PLAN = {
    "llama-8b-r1": (_L[0], "k_attn<128,4> 2 slots", *_L[1:]),
    "llama-8b-r17": (_L[0], "k_attn<128,4> 1 slots", *_L[1:]),
    "qwen-7b-r1": (_Q, "k_attn<128,7> 2 slots", _QK, _L[2], _QK, _L[4]),
    "qwen-7b-r8": (_Q, "k_attn<128,7> 2 slots", _QK, _L[2], _QK, _L[4]),
    "qwen-7b-r9": (_Q, "k_attn<128,7> 2 slots", _L[1], _L[2], _L[3], _L[4]),
}


def test_plan_of_every_layer_case_is_the_recorded_one():
    assert set(EXPECTED_PLAN) == set(LAYER_IDS)
    plan = {c.name: step_plan(c) for c in LAYER_CASES}
    for name, p in plan.items():
        assert plan_strings(p) == EXPECTED_PLAN[name], name
    for name in ("qwen-7b-r1", "qwen-7b-r8"):  # two K parts on O and down: 448 column tiles of 8
        p = plan[name]
        assert (p.o.kpl, p.down.kpl) == (1, 1) and p.o.grid_x == p.down.grid_x == 448
        assert p.gate_up.ss_in == p.lm_head.ss_in == 448  # 8 waves hold 256 in registers; the late loop the rest
        # down, K 18944: 592 k-steps over 2 parts x 8 waves = 37 each, in load batches of 4: nine and one of 1
        assert (p.down.K, p.down.nw, p.down.um) == (18944, 8, 4) and 18944 // 32 // 2 // 8 == 37 == 9 * 4 + 1
    p = plan["qwen-7b-r9"]
    assert (p.o.kpl, p.down.kpl, p.gate_up.ss_in, p.down.grid_x) == (0, 0, 224, 224)
    for name in ("llama-8b-r1", "llama-8b-r17"):  # 256 column tiles of 16: one per CU, no K parts even at 1 row
        p = plan[name]
        assert (p.o.kpl, p.down.kpl, p.o.grid_x, p.gate_up.ss_in) == (0, 0, 256, 256)
        assert (p.gate_up.grid_x, p.down.K) == (2 * 14336 // 16, 14336)


def layer_table(case):
    """The fused weight table of the case's layer and its inputs, drawn on the device."""
    c = case.cfg
    g = device_rng(100 + case.seed)
    n_qkv, hd = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim, c.n_heads * c.head_dim
    ones = torch.ones(c.dim, dtype=BF, device="cuda")
    table = [device_randn(g, c.vocab, c.dim), ones, device_randn(g, c.vocab, c.dim, scale=2.0 ** -6), ones,
             device_randn(g, n_qkv, c.dim, scale=2.0 ** -6), device_randn(g, c.dim, hd, scale=2.0 ** -6), ones,
             device_randn(g, 2 * c.ffn, c.dim, scale=2.0 ** -6), device_randn(g, c.dim, c.ffn, scale=2.0 ** -7)]
    if c.qkv_bias:
        table.append(device_randn(g, n_qkv))
    shape = (case.rows + 1, c.max_seq, c.n_kv_heads, c.head_dim)
    kc0, vc0 = device_randn(g, *shape) * 2.5, device_randn(g, *shape)
    tokens = torch.randint(0, c.vocab, (case.rows,), generator=g, device="cuda")
    inp = SimpleNamespace(tokens=tokens, pos=torch.tensor(case.pos, dtype=torch.int32, device="cuda"), slots=None,
                          kc0=kc0, vc0=vc0)
    return table, inp


def observe_layer(case, table, inp):
    """tests/test_gpu_fused_stages.py's ``observe_gpu`` on device tensors: two passes of the step, the first with
    ``w_down`` zeroed, and every intermediate (copies, on the device)."""
    c, B = case.cfg, case.rows
    dims = ops.LlamaDims(vocab=c.vocab, dim=c.dim, n_layers=1, H=c.n_heads, Hkv=c.n_kv_heads, D=c.head_dim, ffn=c.ffn,
                         max_seq=c.max_seq, max_batch=B + 1, eps=c.eps, theta=c.rope_theta, qkv_bias=int(c.qkv_bias))
    kc, vc = inp.kc0[None].clone(), inp.vc0[None].clone()
    dec = ops.FusedLlamaDecoder(dims, table, kc, vc)
    views = dec.workspace_views()
    logits = torch.empty(B, c.vocab, dtype=BF, device="cuda")
    ids = torch.empty(B, dtype=torch.int64, device="cuda")

    def run():
        logits.view(torch.int16).fill_(SENTINEL_BITS)
        ids.fill_(SENTINEL_ID)
        dec.step(inp.tokens, inp.pos, logits, ids)
        torch.cuda.synchronize()
        return {k: views[k][:B].clone() for k in ("q", "attn", "h", "resid")}

    w_down = table[dec.table.index("w_down", 0)]
    saved = w_down.clone()
    w_down.zero_()
    first = run()
    w_down.copy_(saved)
    second = run()
    for k in ("q", "attn", "h"):
        assert torch.equal(first[k], second[k]), k
    return {"q": second["q"], "attn": second["attn"], "h": second["h"], "r1": first["resid"], "r2": second["resid"],
            "kc": kc[0], "vc": vc[0], "logits": logits, "ids": ids}


def qkv_stage_of(case):
    c = case.cfg
    if not c.qkv_bias:
        return {}
    return {"qkv_stage": lambda case, W, x0, pos, layer: qw2.stage_qkv_bias(c, W[4], W[9], x0, pos)}


@cuda
@gpu
@pytest.mark.parametrize("case", LAYER_CASES, ids=LAYER_IDS)
def test_served_layers_match_fp64(case):
    table, inp = layer_table(case)
    obs = observe_layer(case, table, inp)
    with torch.device("cuda"):  # the stage references make their index and frequency tensors where the data is
        ratios = stage_ratios(case, table, obs, inp=inp, **qkv_stage_of(case))
    print("RATIO", case.name, {k: round(v, 3) for k, v in ratios.items()}, "PLAN", plan_strings(step_plan(case)))
    assert max(ratios.values()) <= 1.0, ratios
    # The step appended exactly one K and one V row per token row and touched nothing else in the cache.
    rows, pos = torch.arange(case.rows, device="cuda"), inp.pos.long()
    for got, before in ((obs["kc"], inp.kc0), (obs["vc"], inp.vc0)):
        same = got.view(torch.int16) == before.view(torch.int16)
        assert not bool(same[rows, pos].all(-1).all(-1).any())  # every appended row was written
        same[rows, pos] = True
        assert bool(same.all())
    assert not bool((obs["ids"] == SENTINEL_ID).any())
