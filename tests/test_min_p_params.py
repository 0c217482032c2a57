"""min_p on the host: request parsing with and without the switch (``params.sampling_params``), the packing of
ln(min_p) (``ops.pack_sampling``), and the host replay of the ``MINP`` sampler (tests/min_p_ref.py) against
hand-built rows and against six one-line slips of itself."""
import math
import struct

import numpy as np
import pytest

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.params import Sampling, SamplingError, sampling_params
from tests import min_p_ref as R


def _f32(bits: int) -> float:
    return struct.unpack("<f", struct.pack("<I", bits))[0]


# ---------------------------------------------------------------- parsing
def test_switch_off_answers_as_before():
    for v in (0.05, 1, 0.5, True, "0.1", -0.1, 1.5):
        with pytest.raises(SamplingError, match="min_p=.* is not supported by this server"):
            sampling_params({"options": {"min_p": v}}, True)
    for v in (0, 0.0, None):  # the neutral values pass
        assert sampling_params({"options": {"min_p": v, "temperature": 0.7}}, True).min_p == 0.0
    for v in (0.05, 1.5, "x", True, None):  # not an OpenAI parameter: not looked at
        s = sampling_params({"min_p": v, "temperature": 0.7, "top_p": 0.9, "seed": 3}, False)
        assert (s.temperature, s.top_p, s.seed, s.min_p) == (0.7, 0.9, 3, 0.0)
    # the penalties switch does not take min_p
    with pytest.raises(SamplingError, match="min_p"):
        sampling_params({"options": {"min_p": 0.05}}, True, penalties=True, vocab=100)
    assert Sampling().min_p == 0.0 and len(Sampling(0.7).column(3)) == 5
    assert Sampling(0.7, 5, 0.9, 11).column(3) == ops.pack_sampling(0.7, 5, 0.9, 11, 3)


@pytest.mark.parametrize("ollama", (True, False))
def test_switch_on_takes_the_range(ollama):
    def parse(v, **more):
        src = {"min_p": v, "temperature": 0.8, **more}
        return sampling_params({"options": src} if ollama else src, ollama, min_p=True)
    for v in (0, 0.0, 1e-6, 0.05, 0.5, 1, 1.0):
        assert parse(v).min_p == float(v)
    assert parse(None).min_p == 0.0 and sampling_params({}, ollama, min_p=True).min_p == 0.0
    for v, text in ((True, "min_p must be a number, got True"), (False, "min_p must be a number, got False"),
                    ("0.1", "min_p must be a number, got '0.1'"), (-0.1, "min_p must be in [0.0, 1.0], got -0.1"),
                    (1.5, "min_p must be in [0.0, 1.0], got 1.5"), (math.nan, "min_p must be in [0.0, 1.0], got nan")):
        with pytest.raises(SamplingError) as e:
            parse(v)
        assert str(e.value) == text
    # the others stay refused with the switch on
    key = "typical_p" if ollama else "best_of"
    with pytest.raises(SamplingError, match=key):
        parse(0.05, **{key: 0.5 if ollama else 2})
    s = parse(0.3, top_k=7, top_p=0.9, seed=5)
    assert (s.temperature, s.top_k, s.top_p, s.seed, s.min_p) == (0.8, 7, 0.9, 5, 0.3)
    assert s.column(9, True) == ops.pack_sampling(0.8, 7, 0.9, 5, 9, 0.3) and len(s.column(9)) == 5


# ---------------------------------------------------------------- packing
def test_packing():
    five = ops.pack_sampling(0.7, 5, 0.9, 11, 3)
    assert len(five) == 5
    for mp in (0, 0.0, 1, 0.05, 1e-6):
        six = ops.pack_sampling(0.7, 5, 0.9, 11, 3, mp)
        assert six[:5] == five and len(six) == 6
    assert ops.pack_sampling(1, 0, 1, 0, 0, 0.0)[5] == 0xFF800000 and _f32(0xFF800000) == -math.inf
    assert ops.pack_sampling(1, 0, 1, 0, 0, 1.0)[5] == 0 and ops.pack_sampling(1, 0, 1, 0, 0, 1)[5] == 0
    want = np.float32(np.log(np.float64(0.05)))  # the fp32 nearest ln 0.05: fp64, rounded once
    assert ops.pack_sampling(1, 0, 1, 0, 0, 0.05)[5] == int(want.view(np.uint32))
    assert abs(_f32(ops.pack_sampling(1, 0, 1, 0, 0, 0.05)[5]) - math.log(0.05)) <= 2.0 ** -23  # half an ulp at 3
    for bad in (-0.1, 1.5, math.nan, math.inf, True, "0.5", -1e-9, 1.0000001):
        with pytest.raises(ValueError, match="min_p"):
            ops.pack_sampling(1, 0, 1, 0, 0, bad)
        with pytest.raises(ValueError, match="min_p"):
            Sampling(1.0, min_p=bad)


# ---------------------------------------------------------------- the replay
def _col(T, k, p, seed, ctr, mp):
    return ops.pack_sampling(T, k, p, seed, ctr, mp)


def test_replay_on_hand_built_rows():
    """Rows small enough to cut by hand. z = (2, 1, 0, -1) at T = 1: p_i / p_max = 1, e^-1, e^-2, e^-3."""
    row = np.array([2.0, 1.0, 0.0, -1.0], dtype=np.float32)
    idx = np.arange(4)

    def winners(mp, T=1.0, k=0, p=1.0, n=400):
        return [R.replay_minp(row, _col(T, k, p, 99, c, mp)).winner for c in range(n)]

    def unfiltered(T=1.0, n=400):
        z = row * (np.float32(1.0) / np.float32(T))
        return [int(np.argmax(z + R.gumbel64(99, c, idx).astype(np.float32))) for c in range(n)]

    assert winners(0.0) == unfiltered() and set(unfiltered()) == {0, 1, 2, 3}  # off: the plain Gumbel-max
    assert set(winners(1e-6)) == {0, 1, 2, 3}
    assert set(winners(0.2)) == {0, 1}  # e^-2 = 0.135 < 0.2 < e^-1
    assert set(winners(0.1)) == {0, 1, 2}  # e^-3 = 0.0498 < 0.1 < e^-2
    assert set(winners(0.5)) == {0} == set(winners(1.0))
    assert set(winners(0.2, T=2.0)) == {0, 1, 2, 3}  # z = logit / 2: ratios 1, .61, .37, .22
    assert set(winners(0.2, T=0.5)) == {0}  # z = 2 logit: ratios 1, .135, ...
    assert set(winners(0.1, k=2)) == {0, 1} and set(winners(0.2, k=3)) == {0, 1}  # the larger cut rules
    # top-p 0.5 keeps token 0 alone (its share is 0.64); min_p 0.1 alone would keep three
    assert set(winners(0.1, p=0.5)) == {0}
    # among the kept tokens the winner is the Gumbel-max over them, with the noise of their own ids
    for c, w in enumerate(winners(0.2, n=50)):
        z = row[:2]
        assert w == int(np.argmax(z + R.gumbel64(99, c, idx[:2]).astype(np.float32)))
    # a token exactly at t stays: exp(-1) packs to ln = -1 exactly, t = 2 - 1 = z_1
    assert ops.pack_sampling(1, 0, 1, 0, 0, math.exp(-1.0))[5] == ops.f32_bits(-1.0)
    assert set(winners(math.exp(-1.0))) == {0, 1}
    assert R.replay_minp(row, _col(0.0, 0, 1.0, 1, 1, 0.5)).winner is None  # greedy: ids stand
    assert R.replay_minp(row, _col(9e-5, 0, 1.0, 1, 1, 0.5)).winner is None
    # all equal: everything stays at min_p = 1; a row with -inf entries never returns one
    eq = np.full(6, 3.0, dtype=np.float32)
    assert set(R.replay_minp(eq, _col(1.0, 0, 1.0, 5, c, 1.0)).winner for c in range(200)) == set(range(6))
    half = np.array([1.0, -np.inf, 0.5, -np.inf], dtype=np.float32)
    assert set(R.replay_minp(half, _col(1.0, 0, 1.0, 5, c, 1e-6)).winner for c in range(200)) == {0, 2}


def test_reference_decides_the_cases():
    """No draw of the shared cases is undecided beyond test_gpu_sample's cap, none of a planted row; no kept set is
    empty; and the planted rows do what they were planted for."""
    for name in R.CASES:
        case, ref = R.CASES[name](), R.replay_case(name)
        assert case.ld == R.LD and all(len(line) == R.LD for line in case.block) and len(case.block) == 6
        sampled = [d for d in ref if d.winner is not None]
        undecided = sum(not d.decided for d in sampled)
        print(f"{name}: {len(ref)} rows, {len(sampled)} sampled, {undecided} undecided")
        assert undecided <= (0 if case.planted else 0.02 * len(ref)), name
        assert all(d.winner != -1 for d in sampled), name
        for r, d in enumerate(ref):
            if d.winner is not None:
                assert all(math.isfinite(case.rows[r][i]) for i in d.possible), (name, r)
    case, ref = R.planted_case(), R.replay_case("planted-V1000")
    assert [case.tags.count(t) for t in ("at", "below", "p<m", "m<p")] == [12, 12, 4, 4]
    for tag, d in zip(case.tags, ref):
        assert d.winner == (R.B_ID if tag == "at" else R.A), tag
    for r, tag in enumerate(case.tags):  # without the min_p cut: "at" / "below" rows are won by the second token
        col = case.col(r)
        off = R.replay_minp(case.rows[r], col[:5] + (ops.f32_bits(-math.inf),))
        assert off.winner == (R.A if tag == "m<p" else R.B_ID), (r, tag)  # ("m<p": top-p alone drops it already)
    special = R.replay_case("special-V1000")
    assert len({d.winner for d in special[:3]}) == 3  # all-equal rows: the draw moves with the seed
    assert all(d.winner == 501 for d in special[6:7])  # the spike at min_p = 1


def test_slips_of_the_replay_change_decided_draws():
    """Each one-line slip of the min_p cut changes the winner of at least one decided draw of the shared cases,
    and of the planted rows: the cases can tell such a kernel from a right one."""
    for variant in R.MINP_VARIANTS:
        changed = total = planted = 0
        for name in R.CASES:
            for base, pert in zip(R.replay_case(name), R.replay_case(name, variant)):
                if base.winner is not None and base.decided:
                    total += 1
                    changed += pert.winner != base.winner
                    planted += name.startswith("planted") and pert.winner != base.winner
        print(f"{variant}: changes {changed} of {total} decided draws ({planted} planted)")
        assert changed >= 1 and planted >= 1, variant
