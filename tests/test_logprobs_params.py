"""Log-probabilities of the inference endpoint (models/server.py), CPU side:
how the three endpoint kinds parse "logprobs" / "top_logprobs", the pure
rendering functions on synthetic records, and the eager engine's refusal.
The kernel, the engine's records and the HTTP responses are tested on the GPU
(tests/test_gpu_logprobs.py)."""
import http.client
import json
import math

import pytest

from p2p_llm_tunnel_amd.models.server import (Engine, Request, SamplingError, chat_logprob_entry, chat_logprobs,
                                              completion_logprobs, logprob_params, sampling_params, start_server)
from tests.test_inference_server import FakeModel


@pytest.mark.parametrize("body,kind,want", [
    # chat: a boolean plus top_logprobs 0..20
    ({}, "chat", None), ({"logprobs": None}, "chat", None), ({"logprobs": False}, "chat", None),
    ({"logprobs": False, "top_logprobs": 0}, "chat", None), ({"top_logprobs": 0}, "chat", None),
    ({"logprobs": 0}, "chat", None),  # the neutral value older clients send
    ({"logprobs": True}, "chat", 0), ({"logprobs": True, "top_logprobs": None}, "chat", 0),
    ({"logprobs": True, "top_logprobs": 0}, "chat", 0), ({"logprobs": True, "top_logprobs": 3}, "chat", 3),
    ({"logprobs": True, "top_logprobs": 20}, "chat", 20), ({"logprobs": True, "top_logprobs": 5.0}, "chat", 5),
    # completions: the legacy integer 1..5
    ({}, "text", None), ({"logprobs": None}, "text", None), ({"logprobs": False}, "text", None),
    ({"logprobs": 0}, "text", None), ({"logprobs": 1}, "text", 1), ({"logprobs": 5}, "text", 5),
    ({"logprobs": 2, "top_logprobs": 0}, "text", 2),
    # Ollama: none, whatever the body says
    ({}, "ollama", None), ({"logprobs": True, "top_logprobs": 99}, "ollama", None),
])
def test_logprob_params_accepts(body, kind, want):
    assert logprob_params(body, kind) == want


@pytest.mark.parametrize("body,kind,field", [
    ({"logprobs": True, "top_logprobs": 21}, "chat", "top_logprobs"),
    ({"logprobs": True, "top_logprobs": -1}, "chat", "top_logprobs"),
    ({"logprobs": True, "top_logprobs": 2.5}, "chat", "top_logprobs"),
    ({"logprobs": True, "top_logprobs": "3"}, "chat", "top_logprobs"),
    ({"logprobs": True, "top_logprobs": True}, "chat", "top_logprobs"),
    ({"top_logprobs": 2}, "chat", "top_logprobs"),
    ({"logprobs": False, "top_logprobs": 2}, "chat", "top_logprobs"),
    ({"top_logprobs": 21}, "chat", "top_logprobs"),
    ({"logprobs": 3}, "chat", "logprobs"), ({"logprobs": "yes"}, "chat", "logprobs"),
    ({"logprobs": 6}, "text", "logprobs"), ({"logprobs": -1}, "text", "logprobs"),
    ({"logprobs": True}, "text", "logprobs"), ({"logprobs": 1.5}, "text", "logprobs"),
    ({"logprobs": "2"}, "text", "logprobs"), ({"logprobs": 2, "top_logprobs": 2}, "text", "top_logprobs"),
])
def test_logprob_params_refuses_and_names_the_field(body, kind, field):
    with pytest.raises(SamplingError) as e:
        logprob_params(body, kind)
    assert field in str(e.value)


def test_sampling_params_still_refuses_both_keys():
    for body in ({"logprobs": True}, {"top_logprobs": 2}, {"logprobs": 2}):
        with pytest.raises(SamplingError):
            sampling_params(body, False)


def test_request_validates_logprobs():
    assert Request([1], 2).logprobs is None and Request([1], 2).lp == []
    assert Request([1], 2, logprobs=0).logprobs == 0 and Request([1], 2, logprobs=20).logprobs == 20
    for bad in (-1, 21, True, 2.0, "3"):
        with pytest.raises(ValueError):
            Request([1], 2, logprobs=bad)


# Synthetic records, as the engine appends them: (chosen_logprob, [(id, logprob), ...]).
_TEXT = {1: "Hello", 2: " wörld", 3: "", 4: "€", 5: "Hello"}  # 3: an empty piece; 5 shares 1's text
_RECORDS = [(-0.5, [(1, -0.5), (2, -1.25)]), (-2.0, [(4, -0.25), (2, -2.0)]), (-math.inf, [(1, -0.125), (3, -math.inf)]),
            (-0.75, [(1, -0.75), (5, -1.5)])]
_TOKENS = [1, 2, 3, 4]


def test_chat_rendering():
    out = chat_logprobs(_TOKENS, _RECORDS, _TEXT.__getitem__)
    assert list(out) == ["content"] and len(out["content"]) == 4
    e0, e1, e2, e3 = out["content"]
    assert e0 == {"token": "Hello", "logprob": -0.5, "bytes": list(b"Hello"), "top_logprobs": [
        {"token": "Hello", "logprob": -0.5, "bytes": list(b"Hello")},
        {"token": " wörld", "logprob": -1.25, "bytes": list(" wörld".encode())}]}
    assert e1["bytes"] == [0x20, 0x77, 0xC3, 0xB6, 0x72, 0x6C, 0x64]  # the multibyte token's UTF-8
    assert e1["top_logprobs"][0]["bytes"] == [0xE2, 0x82, 0xAC]
    assert e2["token"] == "" and e2["bytes"] == [] and e2["logprob"] == -9999.0  # empty piece; -inf clamped
    assert e2["top_logprobs"][1] == {"token": "", "logprob": -9999.0, "bytes": []}
    assert e3 == chat_logprob_entry(4, _RECORDS[3], _TEXT.__getitem__)
    json.loads(json.dumps(out, allow_nan=False))  # JSON-ready: nothing non-finite left
    assert chat_logprobs([], [], _TEXT.__getitem__) == {"content": []}
    assert chat_logprob_entry(1, (math.nan, []), _TEXT.__getitem__)["logprob"] == -9999.0


def test_completions_rendering():
    out = completion_logprobs(_TOKENS, _RECORDS, _TEXT.__getitem__)
    assert sorted(out) == ["text_offset", "token_logprobs", "tokens", "top_logprobs"]
    assert out["tokens"] == ["Hello", " wörld", "", "€"]
    assert out["token_logprobs"] == [-0.5, -2.0, -9999.0, -0.75]
    assert out["text_offset"] == [0, 5, 11, 11]  # characters, not bytes; the empty piece takes none
    assert out["top_logprobs"][0] == {"Hello": -0.5, " wörld": -1.25}
    assert out["top_logprobs"][2] == {"Hello": -0.125, "": -9999.0}
    assert out["top_logprobs"][3] == {"Hello": -0.75}  # two ids with one text: the more probable stays
    json.loads(json.dumps(out, allow_nan=False))
    one = completion_logprobs([2], [_RECORDS[1]], _TEXT.__getitem__, offset=5)  # a streamed chunk
    assert one["text_offset"] == [5] and one["tokens"] == [" wörld"]


def test_eager_engine_refuses_logprobs_with_400():
    """The eager engine (CPU stand-ins, injected models) has no logits: a
    logprobs request is refused, as sampling is, and the connection stays usable."""
    eng = Engine(max_batch=4, model=FakeModel())
    srv, port, _ = start_server(port=0, engine=eng, model_name="fake")
    try:
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=10)
        for path, body in (("/v1/chat/completions", {"messages": [], "logprobs": True, "top_logprobs": 2}),
                           ("/v1/chat/completions", {"messages": [], "logprobs": True}),
                           ("/v1/completions", {"prompt": "x", "logprobs": 2})):
            c.request("POST", path, body=json.dumps(dict(body, max_tokens=2)))
            r = c.getresponse()
            err = json.loads(r.read())
            assert r.status == 400 and "logprobs" in err["error"]["message"], (path, body, err)
        c.request("POST", "/v1/chat/completions", body=json.dumps({"messages": [], "max_tokens": 2,
                                                                   "logprobs": False, "top_logprobs": 0}))
        r = c.getresponse()
        out = json.loads(r.read())
        assert r.status == 200 and "logprobs" not in out["choices"][0]  # the connection stays usable
        with pytest.raises(ValueError):
            eng.submit(Request([1], 2, logprobs=1))
    finally:
        srv.shutdown()
        eng.stop()
