"""POST /api/chat (Ollama's chat route) on the CPU, over the stand-in model of tests/test_inference_server.py:
the streamed and the non-streamed shapes field by field, done_reason, equality with /v1/chat/completions, every
refusal, and a client that goes away mid-stream."""
import json
import re
import socket
import time

from p2p_llm_tunnel_amd.models.server import Engine, start_server
from tests.test_inference_server import FakeModel, _post, _server, expected

MSGS = [{"role": "system", "content": "be brief"}, {"role": "user", "content": "hello"},
        {"role": "assistant", "content": "hi"}, {"role": "user", "content": "again"}]
PROMPT = "\n".join(m["content"] for m in MSGS).encode()
FINAL_KEYS = {"model", "created_at", "message", "done", "done_reason", "total_duration", "prompt_eval_count",
              "prompt_eval_duration", "eval_count", "eval_duration"}


def _text(ids):
    return "".join(f" t{t}" for t in ids)


def _check_final(obj, content, reason, n_prompt, n_eval):
    assert set(obj) == FINAL_KEYS
    assert obj["model"] == "fake" and obj["done"] is True and obj["done_reason"] == reason
    assert obj["message"] == {"role": "assistant", "content": content}
    assert re.fullmatch(r"\d{4}-\d\d-\d\dT\d\d:\d\d:\d\d\.\d{6}Z", obj["created_at"])
    assert obj["prompt_eval_count"] == n_prompt and obj["eval_count"] == n_eval
    for k in ("total_duration", "prompt_eval_duration", "eval_duration"):
        assert type(obj[k]) is int and obj[k] >= 0, k
    assert obj["total_duration"] == obj["prompt_eval_duration"] + obj["eval_duration"] > 0


def test_streamed_and_non_streamed_shapes():
    srv, port, eng = _server()
    try:
        body = {"model": "fake", "messages": MSGS, "options": {"num_predict": 5}, "keep_alive": "5m"}
        st, ct, data, c = _post(port, "/api/chat", body)  # "stream" defaults to true
        assert st == 200 and ct == "application/x-ndjson"
        assert data.endswith(b"\n") and b"\n\n" not in data
        lines = [json.loads(l) for l in data.split(b"\n") if l]
        assert len(lines) == 6
        for o in lines[:-1]:
            assert set(o) == {"model", "created_at", "message", "done"}
            assert o["model"] == "fake" and o["done"] is False and o["created_at"] == lines[-1]["created_at"]
            assert set(o["message"]) == {"role", "content"} and o["message"]["role"] == "assistant"
        want = _text(expected(PROMPT, 5))
        assert "".join(o["message"]["content"] for o in lines) == want
        assert [o["message"]["content"] for o in lines[:-1]] == [f" t{t}" for t in expected(PROMPT, 5)]
        _check_final(lines[-1], "", "length", len(PROMPT), 5)
        # the same connection (keep-alive), not streamed: one object with the whole content
        st, ct, data, _ = _post(port, "/api/chat", dict(body, stream=False), c)
        assert st == 200 and ct == "application/json"
        _check_final(json.loads(data), want, "length", len(PROMPT), 5)
        # the same messages on /v1/chat/completions at temperature 0: the same content
        st, _, data, _ = _post(port, "/v1/chat/completions", {"messages": MSGS, "max_tokens": 5, "temperature": 0})
        assert st == 200 and json.loads(data)["choices"][0]["message"]["content"] == want
        # top-level num_predict, as /api/generate takes it; options.num_predict wins where both are given
        st, _, data, _ = _post(port, "/api/chat", {"messages": MSGS, "stream": False, "num_predict": 3})
        assert json.loads(data)["eval_count"] == 3
        st, _, data, _ = _post(port, "/api/chat", {"messages": MSGS, "stream": False, "num_predict": 3,
                                                   "options": {"num_predict": 2, "temperature": 0, "seed": 1}})
        assert json.loads(data)["message"]["content"] == _text(expected(PROMPT, 2))
        # empty tools / format and an empty images list are nothing to refuse
        st, _, data, _ = _post(port, "/api/chat", {"messages": [{"role": "user", "content": "x", "images": []}],
                                                   "tools": [], "format": "", "stream": False, "num_predict": 1})
        assert st == 200 and json.loads(data)["done"] is True
    finally:
        srv.shutdown()
        eng.stop()


def test_done_reason_stop_on_a_stop_string():
    srv, port, eng = _server()
    try:
        ids = expected(PROMPT, 8)
        stop = f" t{ids[3]}"
        whole = _text(ids)
        want = whole[:whole.index(stop)]
        for stream in (True, False):
            st, _, data, _ = _post(port, "/api/chat", {"messages": MSGS, "stream": stream,
                                                       "options": {"num_predict": 8, "stop": [stop]}})
            assert st == 200
            lines = [json.loads(l) for l in data.split(b"\n") if l]
            assert "".join(o["message"]["content"] for o in lines) == want
            assert lines[-1]["done_reason"] == "stop" and lines[-1]["done"] is True
            assert lines[-1]["eval_count"] == 4  # the tokens taken, the matched one included
    finally:
        srv.shutdown()
        eng.stop()


class _Tok:
    """A tokenizer's surface as the front end uses it, over bytes: ids render as " t<id>"; one id is EOS."""

    def __init__(self, eos):
        self.eos_ids = frozenset([eos])

    def chat(self, msgs, template_kwargs=None):
        return list("\n".join(m["content"] for m in msgs).encode())

    def encode(self, text):
        return list(text.encode())

    def decode(self, ids):
        return _text(ids)

    def detokenizer(self, prompt):
        tok = self

        class D:
            def push(self, t):
                return tok.decode([t])
        return D()


def test_done_reason_stop_on_eos():
    ids = expected(PROMPT, 8)
    eng = Engine(max_batch=4, model=FakeModel())
    srv, port, _ = start_server(port=0, engine=eng, model_name="fake", tokenizer=_Tok(ids[4]))
    try:
        for stream in (True, False):
            st, _, data, _ = _post(port, "/api/chat", {"messages": MSGS, "stream": stream,
                                                       "options": {"num_predict": 8}})
            assert st == 200
            lines = [json.loads(l) for l in data.split(b"\n") if l]
            assert "".join(o["message"]["content"] for o in lines) == _text(ids[:4])
            assert lines[-1]["done_reason"] == "stop" and lines[-1]["prompt_eval_count"] == len(PROMPT)
            assert lines[-1]["eval_count"] == 5  # four with text, and the EOS token
        st, _, data, _ = _post(port, "/api/chat", {"messages": MSGS, "stream": False, "options": {"num_predict": 3}})
        assert json.loads(data)["done_reason"] == "length"
    finally:
        srv.shutdown()
        eng.stop()


def test_every_refusal():
    srv, port, eng = _server()
    try:
        user = {"role": "user", "content": "x"}
        tool = {"type": "function", "function": {"name": "f"}}
        cases = [({"messages": [user], "tools": [tool]}, "tools"),
                 ({"messages": [user], "format": "json"}, "format"),
                 ({"messages": [user], "format": {"type": "object"}}, "format"),
                 ({"messages": [dict(user, images=["aGk="])]}, "messages[0].images"),
                 ({"messages": [user, {"role": "user", "content": ["x"]}]}, "messages[1].content"),
                 ({"messages": [{"role": "user", "content": None}]}, "messages[0].content"),
                 ({"messages": [{"role": "user"}]}, "messages[0].content"),
                 ({"messages": [{"role": "tool", "content": "x"}]}, "messages[0].role"),
                 ({"messages": [{"content": "x"}]}, "messages[0].role"),
                 ({"messages": ["x"]}, "messages[0]"),
                 ({"messages": []}, "messages"),
                 ({}, "messages"),
                 ({"messages": "hello"}, "messages"),
                 ({"messages": [user], "options": {"min_p": 0.05}}, "min_p"),  # no --min-p here
                 ({"messages": [user], "options": {"mirostat": 1}}, "mirostat"),
                 ({"messages": [user], "options": {"temperature": -1}}, "temperature"),
                 ({"messages": [user], "options": {"stop": [3]}}, "stop"),
                 ({"messages": [user], "options": {"num_predict": "many"}}, "max_tokens"),
                 ({"messages": [user], "options": {"temperature": 0.7}}, "eagerly")]  # the stand-in cannot sample
        for body, word in cases:
            st, ct, data, _ = _post(port, "/api/chat", body)
            assert st == 400 and ct == "application/json", (body, st, data)
            assert word in json.dumps(json.loads(data)["error"]), (body, data)
        assert not any(eng.slots) and eng.tokens_out == 0
    finally:
        srv.shutdown()
        eng.stop()


def test_client_disconnect_frees_the_slot():
    srv, port, eng = _server(delay_s=0.005)
    try:
        s = socket.create_connection(("127.0.0.1", port), timeout=10)
        body = json.dumps({"messages": MSGS, "options": {"num_predict": 1000}})
        s.sendall(b"POST /api/chat HTTP/1.1\r\nHost: x\r\nContent-Length: %d\r\n\r\n%s" % (len(body), body.encode()))
        got = b""
        while b'"done": false' not in got:  # mid-stream: a token line has arrived
            got += s.recv(4096)
        assert got.startswith(b"HTTP/1.1 200") and b"application/x-ndjson" in got
        s.close()
        deadline = time.time() + 10
        while any(eng.slots) and time.time() < deadline:
            time.sleep(0.02)
        assert not any(eng.slots)
        assert eng.tokens_out < 1000
        st, _, data, _ = _post(port, "/api/chat", {"messages": MSGS, "stream": False, "num_predict": 2})
        assert st == 200 and json.loads(data)["eval_count"] == 2
    finally:
        srv.shutdown()
        eng.stop()
