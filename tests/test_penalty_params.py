"""--penalties without a GPU: how the penalty parameters and logit_bias parse
with the switch off (refused, as before) and on, what the endpoint answers, that
an eager engine refuses, and the arithmetic of ``ops.penalize_`` as the fp32
NumPy emulation in ``utils/penalty_ref.py`` states it: same operation order,
same bf16 stores, the count-in-registers rule and ``state`` over several steps,
held to the fp64 bound derived in ``penalty_ref.exact``. One-line slips of that
arithmetic must each leave the bound or change an id."""
import http.client
import json

import numpy as np
import pytest

from p2p_llm_tunnel_amd.models.server import (Engine, Penalties, Request, SamplingError, penalty_params,
                                              sampling_params, start_server)
from p2p_llm_tunnel_amd.utils import penalty_ref as ref
from tests.penalty_cases import POISON, make_case
from tests.test_inference_server import FakeModel

OFF_CASES = [
    ({"presence_penalty": 0.5}, False), ({"frequency_penalty": -1}, False), ({"logit_bias": {"1": 5}}, False),
    ({"options": {"repeat_penalty": 1.1}}, True), ({"options": {"presence_penalty": 0.2}}, True),
    ({"options": {"frequency_penalty": 0.2}}, True),
]


@pytest.mark.parametrize("body,ollama", OFF_CASES)
def test_switch_off_refuses_as_before(body, ollama):
    with pytest.raises(SamplingError, match="is not supported by this server"):
        sampling_params(body, ollama)
    sampling_params(body, ollama, penalties=True, vocab=1000)  # the same body passes with the switch on
    assert penalty_params(body, ollama, 1000) is not None


def test_accepted_values():
    p = penalty_params({"presence_penalty": -2, "frequency_penalty": 2.0, "repetition_penalty": 10,
                        "logit_bias": {"0": -100, "999": 100, "17": 0.5}}, False, 1000)
    assert (p.presence, p.frequency, p.repetition) == (-2.0, 2.0, 10.0)
    assert p.logit_bias == {0: -100.0, 999: 100.0, 17: 0.5}
    p = penalty_params({"options": {"repeat_penalty": 1.1, "presence_penalty": 0.5, "frequency_penalty": -0.5,
                                    "repeat_last_n": -1}}, True, 1000)
    assert (p.repetition, p.presence, p.frequency, p.logit_bias) == (1.1, 0.5, -0.5, {})
    assert penalty_params({"options": {"repeat_penalty": 1.5, "repeat_last_n": 0}}, True, 1000) is None  # 0: off
    p = penalty_params({"options": {"repeat_penalty": 1.5, "repeat_last_n": 0, "presence_penalty": 1}}, True, 1000)
    assert (p.repetition, p.presence) == (1.0, 1.0)
    full = {str(i): 1 for i in range(300)}
    assert len(penalty_params({"logit_bias": full}, False, 1000).logit_bias) == 300
    # Neutral values are no penalties at all, on either setting.
    neutral = {"presence_penalty": 0, "frequency_penalty": 0.0, "repetition_penalty": 1, "logit_bias": {}}
    assert penalty_params(neutral, False, 1000) is None and penalty_params({"logit_bias": None}, False, 1000) is None
    assert penalty_params({"logit_bias": {"5": 0}}, False, 1000) is None
    assert penalty_params({"options": {"repeat_penalty": 1.0}}, True, 1000) is None
    assert penalty_params({"options": None}, True, 1000) is None
    sampling_params({k: v for k, v in neutral.items() if k != "repetition_penalty"}, False)
    sampling_params(neutral, False, penalties=True, vocab=1000)


@pytest.mark.parametrize("body,ollama,name", [
    ({"presence_penalty": 2.1}, False, "presence_penalty"), ({"presence_penalty": "x"}, False, "presence_penalty"),
    ({"frequency_penalty": -2.5}, False, "frequency_penalty"), ({"frequency_penalty": True}, False, "frequency_penalty"),
    ({"repetition_penalty": 0}, False, "repetition_penalty"), ({"repetition_penalty": 10.5}, False, "repetition_penalty"),
    ({"repetition_penalty": -1}, False, "repetition_penalty"),
    ({"logit_bias": [1, 2]}, False, "logit_bias"), ({"logit_bias": "5"}, False, "logit_bias"),
    ({"logit_bias": {"x": 1}}, False, "logit_bias"), ({"logit_bias": {"-1": 1}}, False, "logit_bias"),
    ({"logit_bias": {"1.0": 1}}, False, "logit_bias"), ({"logit_bias": {" 1": 1}}, False, "logit_bias"),
    ({"logit_bias": {"": 1}}, False, "logit_bias"), ({"logit_bias": {"1000": 1}}, False, "logit_bias"),
    ({"logit_bias": {"5": 100.5}}, False, "logit_bias"), ({"logit_bias": {"5": -101}}, False, "logit_bias"),
    ({"logit_bias": {"5": "1"}}, False, "logit_bias"), ({"logit_bias": {"5": True}}, False, "logit_bias"),
    ({"logit_bias": {"5": None}}, False, "logit_bias"),
    ({"logit_bias": {"5": 1, "05": 2}}, False, "token id 5 twice"),
    ({"logit_bias": {str(i): 1 for i in range(301)}}, False, "at most 300"),
    ({"options": {"repeat_penalty": 0}}, True, "repeat_penalty"), ({"options": {"repeat_penalty": 11}}, True, "repeat_penalty"),
    ({"options": {"presence_penalty": 3}}, True, "presence_penalty"),
    ({"options": {"frequency_penalty": -3}}, True, "frequency_penalty"),
    ({"options": {"repeat_last_n": 64}}, True, "repeat_last_n"), ({"options": {"repeat_last_n": 1}}, True, "repeat_last_n"),
    ({"options": {"repeat_last_n": -2}}, True, "repeat_last_n"), ({"options": {"repeat_last_n": 0.0}}, True, "repeat_last_n"),
    ({"options": {"repeat_last_n": True}}, True, "repeat_last_n"),
    # still refused, and out of scope
    ({"n": 2}, False, "n="), ({"best_of": 2}, False, "best_of"), ({"options": {"mirostat": 1}}, True, "mirostat"),
    ({"options": {"tfs_z": 0.5}}, True, "tfs_z"), ({"options": {"typical_p": 0.5}}, True, "typical_p"),
    ({"options": {"min_p": 0.1}}, True, "min_p"), ({"options": "x"}, True, "options"),
])
def test_switch_on_refuses(body, ollama, name):
    with pytest.raises(SamplingError, match=name):
        sampling_params(body, ollama, penalties=True, vocab=1000)


def test_repeat_last_n_message_says_why():
    with pytest.raises(SamplingError, match="covers the whole prompt and everything generated"):
        penalty_params({"options": {"repeat_last_n": 64}}, True, 1000)


def test_penalties_object():
    assert Penalties().neutral and Penalties(logit_bias={3: 0}).neutral and not Penalties(repetition=1.1).neutral
    for kw in ({"repetition": 0}, {"repetition": 11}, {"frequency": 2.5}, {"presence": -3}, {"presence": True},
               {"logit_bias": {"3": 1}}, {"logit_bias": {-1: 1}}, {"logit_bias": {3: 101}},
               {"logit_bias": {i: 1 for i in range(301)}}):
        with pytest.raises(ValueError):
            Penalties(**kw)
    assert Request([1], 1, penalties=Penalties()).penalties is None  # neutral: no penalties
    with pytest.raises(ValueError, match="embedding"):
        Request([1], 1, embed="mean", penalties=Penalties(presence=1))
    with pytest.raises(TypeError):
        Request([1], 1, penalties={"presence": 1})


def _post(port, path, body):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=10)
    c.request("POST", path, body=json.dumps(body))
    r = c.getresponse()
    return r.status, json.loads(r.read())


def test_http_400_names_the_parameter_and_eager_engine_refuses():
    with pytest.raises(ValueError, match="graph-captured"):
        Engine(max_batch=4, model=FakeModel(), penalties=True)
    eng = Engine(max_batch=4, model=FakeModel())
    assert not eng.penalties and len(eng._graphs) == 0
    with pytest.raises(ValueError, match="penalties=True"):
        eng.submit(Request([1, 2], 2, penalties=Penalties(frequency=0.5)))
    with pytest.raises(ValueError, match="built without them"):
        start_server(port=0, engine=eng, model_name="fake", penalties=True)
    srv, port, _ = start_server(port=0, engine=eng, model_name="fake")
    try:
        for path, body, name in (("/v1/chat/completions", {"messages": [], "frequency_penalty": 0.4}, "frequency_penalty"),
                                 ("/v1/completions", {"prompt": "a", "logit_bias": {"5": -100}}, "logit_bias"),
                                 ("/api/generate", {"prompt": "a", "options": {"repeat_penalty": 1.1}}, "repeat_penalty")):
            status, out = _post(port, path, body)
            assert status == 400 and name in out["error"]["message"] and "not supported" in out["error"]["message"]
        # The front end of an engine with the switch: the parse alone is exercised here (no GPU), through bodies
        # that never reach the engine.
        eng.penalties = True
        for path, body, name in (("/v1/chat/completions", {"messages": [], "frequency_penalty": 2.4}, "frequency_penalty"),
                                 ("/v1/completions", {"prompt": "a", "logit_bias": {"1000": 1}}, "logit_bias"),
                                 ("/v1/completions", {"prompt": "a", "logit_bias": {"5": 1, "005": 1}}, "twice"),
                                 ("/v1/completions", {"prompt": "a", "repetition_penalty": 0}, "repetition_penalty"),
                                 ("/api/generate", {"prompt": "a", "options": {"repeat_last_n": 64}}, "repeat_last_n"),
                                 ("/api/generate", {"prompt": "a", "options": {"mirostat": 2}}, "mirostat"),
                                 ("/v1/completions", {"prompt": "a", "n": 3}, "n=")):
            status, out = _post(port, path, body)
            assert status == 400 and name in out["error"]["message"], (body, out)
        eng.penalties = False
        status, out = _post(port, "/v1/completions", {"prompt": "a", "max_tokens": 2, "frequency_penalty": 0})
        assert status == 200
    finally:
        srv.shutdown()
        eng.stop()


# ---------------------------------------------------------------- the arithmetic
def _run(case, fn=ref.emulate):
    state = case["state"].copy()
    work, ids = fn(case["logits"], case["ids"], case["tok"], case["dec"], case["slot"], case["params"], state,
                   case["bias"])
    return work, ids, state


@pytest.mark.parametrize("B,V", [(1, 32), (5, 1000), (17, 4096), (3, 1001)])
def test_emulation_meets_the_fp64_bound(B, V):
    case = make_case(B, V, seed=100 + B)
    work, ids, state = _run(case)
    want, bound, touched, want_state = ref.exact(case["logits"], case["tok"], case["dec"], case["slot"],
                                                 case["params"], case["state"], case["bias"])
    assert ref.check(work, case["logits"], want, bound, touched) <= 0
    assert touched.any() and (bound[touched & np.isfinite(want)] > 0).all()
    assert np.array_equal(state, want_state)
    on = case["on_rows"]
    for r in range(B):
        if r in on:
            assert ids[r] == ref.argmax_rule(work[r])
        else:
            assert ids[r] == case["ids"][r] and np.array_equal(work[r], case["logits"][r])
    # state: poison everywhere no row owns, exactly +1 at the decode rows' tokens of the rows that are on
    diff = state.astype(np.int64) - case["state"]
    hits = {(int(case["slot"][r]), int(case["tok"][r])) for r in on if case["dec"][r]}
    assert {(int(s), int(t)) for s, t in zip(*np.nonzero(diff))} == hits and set(diff[diff != 0]) <= {1}
    used = {int(case["slot"][r]) for r in on}
    assert all((state[s] == POISON).all() for s in range(case["n_slots"]) if s not in used)


def test_state_over_several_steps():
    """A sequence of 6 steps on one slot: the prompt row counts nothing, every
    decode row counts its input token once, and the n-th repeat of a token is
    penalised by n * frequency: the count written back is the count read."""
    V, slot = 64, 2
    state = np.zeros((4, V), dtype=np.int32)
    state[slot, [3, 9]] = ref.PROMPT_BIT
    x = np.zeros(V, dtype=np.float32)
    x[[5, 9, 11]] = (8.0, 7.5, 6.0)
    logits = ref.f32_to_bf16(x)[None, :]
    params = [(1.0, 1.0, 0.25, 1)]
    out, tok, dec = [], 3, 0
    for _ in range(6):
        _, ids = ref.emulate(logits, [0], [tok], [dec], [slot], params, state, {})
        out.append(int(ids[0]))
        tok, dec = out[-1], 1
    # By hand, value = x - count - 0.25 once counted: step 1 (prompt row) 5 wins with 8; step 2 counts that 5:
    # 6.75 < 7.5 -> 9; step 3 counts the 9: 6.25 < 6.75 -> 5; step 4: 5 has 5.75, 9 has 6.25 -> 9; step 5: 9 has
    # 5.25, 5 has 5.75, 11 has 6 -> 11; step 6: 11 has 4.75 -> 5. The last token is never fed, so never counted.
    assert out == [5, 9, 5, 9, 11, 5]
    assert [int(state[slot, t]) for t in (5, 9, 11, 3)] == [2, ref.PROMPT_BIT + 2, 1, ref.PROMPT_BIT]
    assert int(np.count_nonzero(state)) == 4


SLIPS = ("unseen_penalised", "mul_positive", "freq_no_count", "pres_scaled", "bias_first", "token_not_counted",
         "prompt_row_counted", "prompt_bit_ignored", "argmax_raw")


def _slipped(slip):
    """``ref.emulate`` with one line wrong."""
    def fn(logits, ids, tok, dec, slot, params, state, bias):
        B, V = logits.shape
        work, ids = logits.copy(), np.array(ids, dtype=np.int64)
        f = np.float32
        with np.errstate(all="ignore"):
            for r in range(B):
                rep, freq, pres, on = params[r]
                if not on or not 0 <= slot[r] < state.shape[0]:
                    continue
                s = int(slot[r])
                d = {"token_not_counted": False, "prompt_row_counted": True}.get(slip, bool(dec[r]))
                cnt, prompt, state[s] = ref._counts(state[s], int(tok[r]), d, V)
                if slip == "prompt_bit_ignored":
                    prompt = np.zeros_like(prompt)
                x = ref.bf16_to_f32(logits[r])
                if slip == "bias_first":
                    for tid, val in bias.get(s, ()):
                        x[tid] = ref.bf16_to_f32(ref.f32_to_bf16(x[tid:tid + 1] + f(val)))[0]
                seen = ((cnt > 0) | prompt) & ~np.isnan(x)
                if slip == "unseen_penalised":
                    seen = ~np.isnan(x)
                y = np.where(x > 0, x * f(rep) if slip == "mul_positive" else x / f(rep), x * f(rep)).astype(f)
                y = (y - (f(freq) * (f(1) if slip == "freq_no_count" else cnt.astype(f))).astype(f)).astype(f)
                p = (f(pres) * cnt.astype(f)).astype(f) if slip == "pres_scaled" else f(pres)
                y = np.where(cnt > 0, (y - p).astype(f), y)
                work[r] = np.where(seen, ref.f32_to_bf16(y), logits[r] if slip != "bias_first" else ref.f32_to_bf16(x))
                if slip != "bias_first":
                    for tid, val in bias.get(s, ()):
                        work[r, tid] = ref.f32_to_bf16(ref.bf16_to_f32(work[r, tid:tid + 1]) + f(val))[0]
                ids[r] = ref.argmax_rule(logits[r] if slip == "argmax_raw" else work[r])
        return work, ids
    return fn


@pytest.mark.parametrize("slip", SLIPS)
def test_one_line_slips_are_caught(slip):
    case = make_case(17, 4096, seed=117)
    good_work, good_ids, good_state = _run(case)
    work, ids, state = _run(case, _slipped(slip))
    want, bound, touched, want_state = ref.exact(case["logits"], case["tok"], case["dec"], case["slot"],
                                                 case["params"], case["state"], case["bias"])
    caught = ref.check(work, case["logits"], want, bound, touched) > 0 or not np.array_equal(ids, good_ids) or \
        not np.array_equal(state, want_state)
    assert caught, slip
    assert np.array_equal(_run(case, _slipped(None))[0], good_work)  # without a slip it is the emulation
