"""Penalties and logit_bias on the GPU: ``ops.penalize_`` (penalty.hip) against
fp64 element by element, ``ops.penalty_reset_``, the host-side validation of
both, the engine with ``penalties=True`` against a CPU fp32 reference
generation, and the endpoint.

The op's bound is derived in ``utils/penalty_ref.exact`` and is per element:
the fp32 roundings of the kernel's own operations, 4 * 2^-24 of the term
magnitudes |x / rep| + |freq * count| + |pres|, plus half a bf16 ulp at the
result for the store; an element with a bias is stored twice, so it adds the
fp32 rounding of that sum and a second half ulp at the biased result. Nothing
is scaled by a maximum over the row. Elements no rule touches (off rows, ids
never seen and not biased) are compared bit for bit, NaN must stay NaN and
infinities must stay what they are.

Token equality and its margin (engine tests). The engine's logits are bf16 and
come from another schedule than the fp32 reference; the two agree within about
0.01 x max|logit| (test_gpu_model.py::test_chunked_prefill_matches_sequential).
The repetition penalty multiplies a logit, and so that error, by at most
max(rep, 1 / rep); frequency, presence and bias add exact amounts. The prompts
below come from fixed seeds, searched on the CPU so that AFTER the penalties the
reference's top-2 gap is at least 0.03 x max|logit| x max(rep, 1 / rep) at every
generated index (the "confident" margin of test_gpu_prefix_cache.py, scaled),
that each penalised completion differs from the unpenalised one, and that the
frequency case differs from what it would be with counts stuck at 1.
``test_fixed_inputs_are_confident`` (CPU) re-checks all of it from the seeds; the
GPU tests then demand equality at every index."""
import http.client
import json
import math
import random
from collections import Counter

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.server import Engine, Penalties, Request, Sampling, start_server
from p2p_llm_tunnel_amd.utils import penalty_ref as ref
from tests.penalty_cases import POISON, make_case

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu

V = 4096  # micro
N_NEW = 6
MARGIN = 0.03


def ids_of(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(V) for _ in range(n)]


# (a) frequency + presence (negative frequency: a generated token is favoured more with every repeat, so the
# counts decide), (b) repetition 1.3 over a long prompt, (c) a bias that bans the unpenalised completion's tokens.
PROMPT_A, PEN_A = ids_of(580, 40), dict(frequency=-2.0, presence=-2.0)
PROMPT_B, PEN_B = ids_of(998, 480), dict(repetition=1.3)
PROMPT_C = ids_of(14, 25)
# Unpenalised reference completions, then the penalised ones (margins 0.176, 0.045, 0.038).
PLAIN_A = [3742, 3530, 1958, 1331, 2560, 124]
PLAIN_B = [3801, 1776, 2755, 3780, 2370, 823]
PLAIN_C = [3019, 1180, 3224, 2617, 1730, 786]
REF_A = [3742, 3742, 3742, 3742, 3742, 3742]
REF_B = [3801, 1776, 2755, 3780, 1341, 1556]
REF_C = [3049, 412, 1102, 285, 368, 277]


def pen_c():
    return dict(logit_bias={t: -100.0 for t in PLAIN_C})


def ref_generate(model, prompt, pen: dict | None, n_new=N_NEW, cap=False, forced=None, stop_below=-1.0):
    """Greedy fp32 reference generation with the reference penalty (fp64 on the
    fp32 logits). Returns (tokens, smallest top-2 gap / (max|logit| * max(rep, 1 / rep)),
    per step (raw log-softmax row, max|logit|)). ``cap``: counts stuck at 1 (a deliberately wrong
    variant). ``forced``: follow these tokens instead of the argmax."""
    p = Penalties(**(pen or {}))
    seq, out, worst, rows = list(prompt), [], math.inf, []
    for k in range(n_new):
        lg = model.reference_logits(torch.tensor([seq]))[0].double()
        rows.append((torch.log_softmax(lg, 0), float(lg.abs().max())))
        x = lg.clone()
        seen = torch.tensor(sorted(set(prompt) | set(out)))
        x[seen] = torch.where(x[seen] > 0, x[seen] / p.repetition, x[seen] * p.repetition)
        for t, c in Counter(out).items():
            x[t] -= p.frequency * (1 if cap else c) + p.presence
        for t, b in p.logit_bias.items():
            x[t] += b
        top = x.topk(2).values
        worst = min(worst, float(top[0] - top[1]) / (float(lg.abs().max()) * max(p.repetition, 1 / p.repetition)))
        out.append(int(x.argmax()) if forced is None else forced[k])
        seq.append(out[-1])
        if worst < stop_below:  # (the seed search gives up on a candidate here)
            break
    return out, worst, rows


@pytest.fixture(scope="module")
def cpu_model():
    from p2p_llm_tunnel_amd.models.tiny_llm import TinyLlama
    return TinyLlama("micro", device="cpu", max_batch=1, seed=0)


def test_fixed_inputs_are_confident(cpu_model):
    assert cpu_model.cfg.vocab == V
    for prompt, pen, plain, want in ((PROMPT_A, PEN_A, PLAIN_A, REF_A), (PROMPT_B, PEN_B, PLAIN_B, REF_B),
                                     (PROMPT_C, pen_c(), PLAIN_C, REF_C)):
        out, worst, _ = ref_generate(cpu_model, prompt, None)
        assert out == plain and (worst >= MARGIN or prompt is PROMPT_A)  # PLAIN_A is compared with no GPU result
        out, worst, _ = ref_generate(cpu_model, prompt, pen)
        assert out == want and worst >= MARGIN, (out, worst)
        assert want != plain
    assert ref_generate(cpu_model, PROMPT_A, PEN_A, cap=True)[0] != REF_A  # the counts decide
    assert not set(REF_C) & set(PLAIN_C)


# ---------------------------------------------------------------- op
def _dev(case):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    B, V_, n_slots = case["B"], case["V"], case["n_slots"]
    d = {"logits": torch.from_numpy(case["logits"].view(np.int16)).cuda().view(torch.bfloat16),
         "ids": t(case["ids"], torch.int64), "tok": t(case["tok"], torch.int64), "dec": t(case["dec"], torch.int64),
         "slot": t(case["slot"], torch.int64), "state": t(case["state"], torch.int32),
         "params": torch.tensor([ops.pack_penalties(*p[:3], on=bool(p[3])) for p in case["params"]],
                                dtype=torch.int64).T.contiguous().cuda(),
         "work": torch.full((B, V_), 7.0, dtype=torch.bfloat16, device="cuda"),
         "bias_n": torch.zeros(n_slots, dtype=torch.int32), "bias_ids": torch.full((n_slots, 300), -5, dtype=torch.int32),
         "bias_val": torch.full((n_slots, 300), 1e9, dtype=torch.float32)}
    for s, lst in case["bias"].items():
        d["bias_n"][s] = len(lst)
        d["bias_ids"][s, :len(lst)] = torch.tensor([t_ for t_, _ in lst], dtype=torch.int32)
        d["bias_val"][s, :len(lst)] = torch.tensor([v for _, v in lst], dtype=torch.float32)
    for k in ("bias_n", "bias_ids", "bias_val"):
        d[k] = d[k].cuda()
    return d


def _call(d):
    ops.penalize_(d["logits"], d["work"], d["ids"], d["tok"], d["dec"], d["slot"], d["params"], d["state"],
                  d["bias_n"], d["bias_ids"], d["bias_val"])
    torch.cuda.synchronize()
    return d["work"].view(torch.int16).cpu().numpy().view(np.uint16), d["ids"].cpu().numpy(), d["state"].cpu().numpy()


def _hold(case, work, ids, state, logits=None, start_state=None, start_ids=None):
    logits = case["logits"] if logits is None else logits
    start_state = case["state"] if start_state is None else start_state
    start_ids = case["ids"] if start_ids is None else start_ids
    want, bound, touched, want_state = ref.exact(logits, case["tok"], case["dec"], case["slot"], case["params"],
                                                 start_state, case["bias"])
    excess = ref.check(work, logits, want, bound, touched)
    print(f"B={case['B']} V={case['V']}: worst |got - fp64| - bound = {excess:.3e} over {int(touched.sum())} touched")
    assert excess <= 0
    assert np.array_equal(state, want_state)  # whole: poison slots, untouched words, +1 at the decode tokens only
    for r in range(case["B"]):
        if r in case["on_rows"]:
            assert ids[r] == ref.argmax_rule(work[r]), r  # the argmax of what was stored
        else:
            assert ids[r] == start_ids[r] and np.array_equal(work[r], logits[r]), r
    return want_state


@gpu
@cuda
@pytest.mark.parametrize("V_", [32, 1000, 1001, 4096, 32000, 151936])
@pytest.mark.parametrize("B", [1, 16, 17, 64])
def test_penalize_against_fp64(B, V_):
    case = make_case(B, V_, seed=B * 1000 + V_ % 997)
    d = _dev(case)
    raw = d["logits"].clone()
    work, ids, state = _call(d)
    assert torch.equal(raw.view(torch.int16), d["logits"].view(torch.int16))  # the raw logits are never written
    mid = _hold(case, work, ids, state)
    used = {int(case["slot"][r]) for r in case["on_rows"]}
    assert all((state[s] == POISON).all() for s in range(case["n_slots"]) if s not in used)
    # A second call reads the words the first wrote back (and counts the decode tokens once more).
    work2, ids2, state2 = _call(d)
    _hold(case, work2, ids2, state2, start_state=mid, start_ids=ids)
    diff = state2.astype(np.int64) - case["state"]
    hits = {(int(case["slot"][r]), int(case["tok"][r])) for r in case["on_rows"] if case["dec"][r]}
    assert {(int(s), int(t)) for s, t in zip(*np.nonzero(diff))} == hits and set(diff[diff != 0]) <= {2}


def _plain(B, V_, x, on=True, rep=1.0, freq=0.0, pres=0.0):
    """A case of all-on rows (row r on slot r) over given fp32 logits, empty state."""
    return {"B": B, "V": V_, "logits": ref.f32_to_bf16(np.asarray(x, dtype=np.float32)), "ids": np.full(B, 5, np.int64),
            "tok": np.zeros(B, np.int64), "dec": np.zeros(B, np.int64), "slot": np.arange(B, dtype=np.int64),
            "params": [(rep, freq, pres, int(on))] * B, "state": np.zeros((B, V_), np.int32), "bias": {},
            "on_rows": list(range(B)) if on else [], "n_slots": B}


@gpu
@cuda
@pytest.mark.parametrize("V_", [32000, 1001])
def test_ties_nan_rows_and_deciding_biases(V_):
    """Row 0: the maximum planted on both sides of every seam (8-element vector,
    1024-lane pass = 8192 elements, 64-lane wave = 512 elements, the last
    element), lowest id wins. Row 1: all NaN -> id 0. Row 2: all -inf -> id 0.
    Row 3: +100 on one id decides. Row 4: -100 on the raw argmax removes it.
    Row 5: -inf everywhere but a NaN at id 0 and a tie at ids 9 and 20 -> 9.
    Row 6: like row 0, but the lowest tied id is penalised away (count 1)."""
    rng = np.random.default_rng(V_)
    B = 7
    x = (rng.standard_normal((B, V_)) * 2).astype(np.float32)
    seams = [p for p in (8200, 8191, 8192, 7, 8, 511, 512, 16384, 16383, V_ - 1, V_ - 9) if p < V_]
    x[0, seams] = x[6, seams] = 50.0
    x[1, :] = np.nan
    x[2, :] = -np.inf
    x[5, :] = -np.inf
    x[5, [0, 9, 20]] = (np.nan, 1.5, 1.5)
    case = _plain(B, V_, x, rep=1.3, freq=0.5, pres=1.0)
    case["state"][6, min(seams)] = 1
    hot = int(np.argmax(ref.bf16_to_f32(case["logits"][4])))
    case["bias"] = {3: [(V_ - 3, 100.0)], 4: [(hot, -100.0)], 0: [(3, 0.5)]}  # row 0: the tie survives a re-read
    work, ids, state = _call(_dev(case))
    _hold(case, work, ids, state)
    assert list(ids[:4]) == [min(seams), 0, 0, V_ - 3] and ids[4] != hot and ids[5] == 9
    assert ids[6] == sorted(seams)[1]
    assert np.isnan(ref.bf16_to_f32(work[1])).all() and (work[2] == 0xFF80).all()


@gpu
@cuda
def test_penalty_reset():
    V_, n_slots = 1000, 5
    state = torch.full((n_slots, V_), POISON, dtype=torch.int32, device="cuda")
    bias_n = torch.full((n_slots,), 77, dtype=torch.int32, device="cuda")
    bias_ids = torch.full((n_slots, 300), -9, dtype=torch.int32, device="cuda")
    bias_val = torch.full((n_slots, 300), 3.5, dtype=torch.float32, device="cuda")
    prompt = [3, 999, 3, 0, 512, 1000, -1, 7]  # a repeat, both ends, two ids outside the vocabulary
    vals = np.array([-100.0, 0.25, 100.0], dtype=np.float32)
    bias = torch.tensor([[5, 999, 17], vals.view(np.int32).tolist()], dtype=torch.int32, device="cuda")
    ops.penalty_reset_(state, 2, torch.tensor(prompt, dtype=torch.int32, device="cuda"), bias_n, bias_ids, bias_val, bias)
    ops.penalty_reset_(state, 4, torch.tensor([1] * 700, dtype=torch.int32, device="cuda"), bias_n, bias_ids, bias_val)
    torch.cuda.synchronize()
    want = np.full((n_slots, V_), POISON, dtype=np.int32)
    want[2] = want[4] = 0
    want[2, [3, 999, 0, 512, 7]] = ref.PROMPT_BIT
    want[4, 1] = ref.PROMPT_BIT
    assert np.array_equal(state.cpu().numpy(), want)
    assert bias_n.tolist() == [77, 77, 3, 77, 0]
    assert bias_ids[2, :3].tolist() == [5, 999, 17] and bias_val[2, :3].tolist() == vals.tolist()
    ids_rest = bias_ids.clone()
    ids_rest[2, :3] = -9
    vals_rest = bias_val.clone()
    vals_rest[2, :3] = 3.5
    assert (ids_rest == -9).all() and (vals_rest == 3.5).all()


@gpu
@cuda
def test_validation_raises_before_a_launch():
    case = make_case(4, 64, seed=1)
    good = _dev(case)
    order = ("logits", "work", "ids", "tok", "dec", "slot", "params", "state", "bias_n", "bias_ids", "bias_val")

    def bad(exc, **kw):
        with pytest.raises(exc):
            ops.penalize_(*[kw.get(k, good[k]) for k in order])

    for k in order:  # dtype, device
        wrong = good[k].to(torch.float64)
        bad(TypeError, **{k: wrong})
        bad(ValueError, **{k: good[k].cpu()})
    bad(ValueError, logits=good["logits"].T.contiguous().T)  # not contiguous
    bad(ValueError, work=good["work"][:3])
    bad(ValueError, work=good["logits"])  # in place: the raw logits are never written
    bad(ValueError, ids=good["ids"][:3])
    bad(ValueError, tok=good["tok"][:3])
    bad(ValueError, dec=good["dec"][:3])
    bad(ValueError, slot=good["slot"][:3])
    bad(ValueError, params=good["params"][:3])
    bad(ValueError, params=good["params"][:, :3].contiguous())
    bad(ValueError, state=good["state"][:, :32].contiguous())  # another vocabulary than the logits'
    bad(ValueError, state=torch.zeros((3, 16), dtype=torch.int32, device="cuda"))  # V < 32
    bad(ValueError, bias_n=good["bias_n"][:2])
    bad(ValueError, bias_ids=good["bias_ids"][:, :299].contiguous())
    bad(ValueError, bias_val=good["bias_val"][:2])
    odd = torch.zeros(4 * 64 + 8, dtype=torch.bfloat16, device="cuda")[1:4 * 64 + 1].view(4, 64)
    bad(ValueError, logits=odd)  # not 16-byte aligned
    before = good["state"].clone()
    torch.cuda.synchronize()
    assert torch.equal(good["state"], before) and (good["work"] == 7.0).all()  # nothing ran

    st, bn, bi, bv = good["state"], good["bias_n"], good["bias_ids"], good["bias_val"]
    prompt = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
    for args in ((st, st.shape[0], prompt, bn, bi, bv), (st, -1, prompt, bn, bi, bv), (st, True, prompt, bn, bi, bv),
                 (st, 0, prompt[:0], bn, bi, bv), (st, 0, prompt.view(1, 2), bn, bi, bv), (st, 0, prompt.cpu(), bn, bi, bv),
                 (st, 0, prompt, bn[:1], bi, bv),
                 (st, 0, prompt, bn, bi, bv, torch.zeros((2, 301), dtype=torch.int32, device="cuda")),
                 (st, 0, prompt, bn, bi, bv, torch.zeros((3, 4), dtype=torch.int32, device="cuda")),
                 (st, 0, prompt, bn, bi, bv, torch.zeros((2, 0), dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            ops.penalty_reset_(*args)
    for args in ((st, 0, prompt.long(), bn, bi, bv), (st.float(), 0, prompt, bn, bi, bv),
                 (st, 0, prompt, bn, bi, bv, torch.zeros((2, 3), dtype=torch.float32, device="cuda"))):
        with pytest.raises(TypeError):
            ops.penalty_reset_(*args)
    torch.cuda.synchronize()
    assert torch.equal(good["state"], before)


# ---------------------------------------------------------------- engine
def collect(req):
    out = []
    while (t := req.out.get(timeout=60)) is not None:
        out.append(t)
    return out


@pytest.fixture(scope="module")
def engines():
    on = Engine(device="cuda:0", config="micro", max_batch=4, seed=0, penalties=True)
    off = Engine(device="cuda:0", config="micro", max_batch=4, seed=0)
    yield on, off
    on.stop()
    off.stop()


def _cases():
    return [(PROMPT_A, PEN_A, REF_A, PLAIN_A), (PROMPT_B, PEN_B, REF_B, PLAIN_B), (PROMPT_C, pen_c(), REF_C, PLAIN_C)]


def _slot_state(eng, slot):
    torch.cuda.synchronize()
    st = eng._pen.state[slot].cpu().numpy()
    return ({int(t) for t in np.nonzero(st & ref.PROMPT_BIT)[0]},
            {int(t): int(st[t] & ref.COUNT_MASK) for t in np.nonzero(st & ref.COUNT_MASK)[0]})


@gpu
@cuda
def test_engine_graphs_and_unpenalised_requests(engines):
    on, off = engines
    assert len(on._graphs) == 16 and len(off._graphs) == 12
    assert on._bufs[16][0].h_in.shape[0] == 15 and off._bufs[16][0].h_in.shape[0] == 11
    assert off._pen is None
    for prompt, _, _, plain in _cases():
        got = [collect(e.submit(Request(list(prompt), N_NEW))) for e in (on, off)]
        assert got[0] == got[1]
        assert got[0] == plain or prompt is PROMPT_A  # (the unpenalised reference of A is not a confident one)
    with pytest.raises(ValueError, match="penalties=True"):
        off.submit(Request(list(PROMPT_A), 2, penalties=Penalties(**PEN_A)))
    with pytest.raises(ValueError, match="logit_bias ids"):
        on.submit(Request(list(PROMPT_A), 2, penalties=Penalties(logit_bias={V: 1.0})))


@gpu
@cuda
def test_engine_one_by_one_matches_the_reference_and_resets_the_slot(engines):
    """One at a time every request lands in slot 0, which the previous penalised
    request has just left: its counts and prompt bits must be gone."""
    on, _ = engines
    for prompt, pen, want, _ in _cases():
        out = collect(on.submit(Request(list(prompt), N_NEW, penalties=Penalties(**pen))))
        assert out == want
        bits, counts = _slot_state(on, 0)
        assert bits == set(prompt) and counts == dict(Counter(want[:-1]))  # the last token is never fed back
        assert on._pen.bias_n[0].item() == len(pen.get("logit_bias", {}))


@gpu
@cuda
def test_engine_batched_matches_one_by_one(engines):
    on, _ = engines
    for order in (_cases(), _cases()[::-1]):
        plain = on.submit(Request(list(PROMPT_C), N_NEW))  # an unpenalised neighbour in the same steps
        reqs = [on.submit(Request(list(p), N_NEW, penalties=Penalties(**pen))) for p, pen, _, _ in order]
        assert [collect(r) for r in reqs] == [want for _, _, want, _ in order]
        assert collect(plain) == PLAIN_C


@gpu
@cuda
def test_engine_one_token_requests_reuse_a_slot_back_to_back(engines):
    """max_new = 1 with a one-chunk prompt frees the slot at plan time, so the
    next admission into it comes before that step has drained: the two
    alternating stagings per slot are what keeps each reset's input intact."""
    on, _ = engines
    reqs = [on.submit(Request(list(p), 1, penalties=Penalties(**pen))) for _ in range(4) for p, pen, _, _ in _cases()]
    assert [collect(r) for r in reqs] == [want[:1] for _ in range(4) for _, _, want, _ in _cases()]
    out = collect(on.submit(Request(list(PROMPT_A), N_NEW, penalties=Penalties(**PEN_A))))
    assert out == REF_A


@gpu
@cuda
def test_engine_with_the_prefix_cache():
    eng = Engine(device="cuda:0", config="micro", max_batch=4, seed=0, penalties=True, prefix_cache=True)
    try:
        assert len(eng._graphs) == 16
        first = eng.submit(Request(list(PROMPT_B), N_NEW, penalties=Penalties(**PEN_B)))
        assert collect(first) == REF_B and first.cached_tokens == 0
        again = eng.submit(Request(list(PROMPT_B), N_NEW, penalties=Penalties(**PEN_B)))
        assert collect(again) == REF_B and again.cached_tokens == len(PROMPT_B) - 1  # in place: one row ran
        slot = next(i for i, s in enumerate(eng._kv) if s is again.kv)
        bits, counts = _slot_state(eng, slot)
        assert bits == set(PROMPT_B) and counts == dict(Counter(REF_B[:-1]))  # bits from the ids, not the rows run
    finally:
        eng.stop()


@gpu
@cuda
def test_sampled_request_reports_the_raw_distribution(engines, cpu_model):
    """A sampled request whose bias bans the unpenalised completion: it never
    draws a banned token, a fixed seed replays it, and its logprobs are the
    model's own softmax(logits): the banned raw argmax still leads the top list,
    and every chosen token's logprob is the reference's raw one, within twice
    the 0.01 x max|logit| the two sets of logits agree to (logit and lse)."""
    on, _ = engines
    runs = []
    for _ in range(2):
        r = on.submit(Request(list(PROMPT_C), N_NEW, sampling=Sampling(0.8, 0, 1.0, seed=11),
                              penalties=Penalties(**pen_c()), logprobs=3))
        runs.append((collect(r), r.lp))
    assert runs[0] == runs[1]
    out, lp = runs[0]
    assert len(out) == N_NEW and not set(out) & set(PLAIN_C)
    assert lp[0][1][0][0] == PLAIN_C[0]  # the banned token: still the raw distribution's first
    _, _, rows = ref_generate(cpu_model, PROMPT_C, None, forced=out)
    for k, (chosen, top) in enumerate(lp):
        row, scale = rows[k]
        assert abs(chosen - float(row[out[k]])) <= 0.02 * scale, (k, chosen, float(row[out[k]]))
        assert [a >= b for (_, a), (_, b) in zip(top, top[1:])] == [True] * 2


def _post(port, path, body):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    c.request("POST", path, body=json.dumps(body), headers={"content-type": "application/json"})
    r = c.getresponse()
    return r.status, json.loads(r.read())


@gpu
@cuda
def test_endpoint_with_and_without_the_switch(engines):
    on, off = engines
    text = "penalise me"
    bodies = [("/v1/completions", {"prompt": text, "max_tokens": 4, "frequency_penalty": 0.5, "presence_penalty": 0.5}),
              ("/v1/chat/completions", {"messages": [{"role": "user", "content": text}], "max_tokens": 4,
                                        "logit_bias": {"17": -100}, "repetition_penalty": 1.2}),
              ("/api/generate", {"prompt": text, "stream": False, "num_predict": 4,
                                 "options": {"repeat_penalty": 1.1, "repeat_last_n": -1}})]
    for eng, want in ((on, 200), (off, 400)):
        srv, port, _ = start_server(port=0, engine=eng, model_name="micro", penalties=eng.penalties)
        try:
            for path, body in bodies:
                status, out = _post(port, path, body)
                assert status == want, (path, out)
            status, out = _post(port, "/api/generate", {"prompt": text, "stream": False,
                                                        "options": {"repeat_penalty": 1.1, "repeat_last_n": 64}})
            assert status == 400 and ("repeat_last_n" if eng is on else "repeat_penalty") in out["error"]["message"]
            # A ban through the endpoint: the greedy completion's first token, then without it.
            status, out = _post(port, "/v1/completions", {"prompt": text, "max_tokens": 1})
            first = out["choices"][0]["text"]
            assert status == 200 and first.startswith(" t")
            if eng is on:
                status, out = _post(port, "/v1/completions", {"prompt": text, "max_tokens": 1,
                                                              "logit_bias": {first[2:]: -100}})
                assert status == 200 and out["choices"][0]["text"] != first
        finally:
            srv.shutdown()
            eng.deliver = None
