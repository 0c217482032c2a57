"""--prompt-logprobs without a GPU: what "echo" and "prompt_logprobs" parse to with the switch off (not looked at, as
before) and on, the response of lm-eval's log-likelihood call from a stubbed engine result, that --gpus passes the
flag on, and ``ops.lm_score_plan``'s grids (docs/PROMPT_LOGPROBS.md)."""
import http.client
import json

import pytest

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.params import SamplingError, prompt_logprob_params
from p2p_llm_tunnel_amd.models.server import Engine, Request, arg_parser, replica_cmd, start_server
from tests.test_inference_server import FakeModel


@pytest.mark.parametrize("body", [{"echo": True, "logprobs": 1}, {"prompt_logprobs": 5}, {"echo": "yes"}])
def test_switch_off_looks_at_nothing(body):
    assert prompt_logprob_params(body, "text", False) == (False, None, None)
    assert prompt_logprob_params(body, "ollama", True) == (False, None, None)


@pytest.mark.parametrize("body,kind,want", [
    ({"echo": True, "logprobs": 1}, "text", (True, 1, None)),
    ({"echo": True, "logprobs": 0}, "text", (True, 0, None)),
    ({"echo": True}, "text", (True, None, None)),
    ({"echo": False, "logprobs": 5}, "text", (False, None, None)),
    ({"prompt_logprobs": 1}, "chat", (False, None, 1)),
    ({"prompt_logprobs": 0, "echo": True, "logprobs": 1}, "text", (True, 1, 0)),
])
def test_switch_on_accepts(body, kind, want):
    assert prompt_logprob_params(body, kind, True) == want


@pytest.mark.parametrize("body,kind,name", [
    ({"echo": True, "logprobs": 2}, "text", "logprobs"), ({"prompt_logprobs": 2}, "text", "prompt_logprobs"),
    ({"prompt_logprobs": True}, "chat", "prompt_logprobs"), ({"prompt_logprobs": -1}, "chat", "prompt_logprobs"),
    ({"echo": 1}, "text", "echo"), ({"echo": True}, "chat", "echo"),
])
def test_switch_on_refuses(body, kind, name):
    with pytest.raises(SamplingError, match=name):
        prompt_logprob_params(body, kind, True)


def _post(port, path, body):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=10)
    c.request("POST", path, body=json.dumps(body))
    r = c.getresponse()
    return r.status, json.loads(r.read())


def test_http_routes_and_the_loglikelihood_call():
    with pytest.raises(ValueError, match="graph-captured"):
        Engine(max_batch=4, model=FakeModel(), prompt_logprobs=True)
    eng = Engine(max_batch=4, model=FakeModel())
    with pytest.raises(ValueError, match="prompt_logprobs=True"):
        eng.submit(Request([1, 2], 0, score=True))
    with pytest.raises(ValueError, match="built without it"):
        start_server(port=0, engine=eng, model_name="fake", prompt_logprobs=True)
    srv, port, _ = start_server(port=0, engine=eng, model_name="fake")
    try:
        # Off: both keys are ignored, the completion is what it is without them.
        base = _post(port, "/v1/completions", {"prompt": "ab", "max_tokens": 2})
        got = _post(port, "/v1/completions", {"prompt": "ab", "max_tokens": 2, "echo": True, "prompt_logprobs": 7})
        assert got[0] == base[0] == 200 and got[1]["choices"][0]["text"] == base[1]["choices"][0]["text"]
        assert "prompt_logprobs" not in got[1]["choices"][0]

        # On, with the engine's answer stubbed: three prompt tokens, the first without a record.
        seen = []

        def submit(req):
            seen.append(req)
            req.prompt_lp = [None] + [(-0.5 * p, 7, -0.25) for p in range(1, len(req.prompt))]
            batch = []
            if req.max_new:  # one generated token, with its record when the request has logprobs
                req.lp.append((-0.125, [(9, -0.125)][:req.logprobs or 0]))
                req.generated = 1
                batch.append((req, 9))
            eng.deliver(batch + [(req, None)])
            return req
        eng.prompt_logprobs, eng.use_graph, eng.submit = True, True, submit
        for body, name in (({"prompt": "a", "echo": True, "logprobs": 3}, "logprobs"),
                           ({"prompt": "a", "prompt_logprobs": 2}, "prompt_logprobs"),
                           ({"prompt": "a" * 5000, "echo": True, "logprobs": 1, "max_tokens": 0}, "context")):
            status, out = _post(port, "/v1/completions", body)
            assert status == 400 and name in out["error"]["message"], out
        status, out = _post(port, "/v1/completions", {"prompt": "abc", "echo": True, "logprobs": 1, "max_tokens": 0,
                                                      "prompt_logprobs": 0})
        assert status == 200 and seen[-1].score and seen[-1].max_new == 0 and seen[-1].logprobs == 1
        ids = seen[-1].prompt
        texts = [" t%d" % t for t in ids]
        choice = out["choices"][0]
        assert choice["text"] == "".join(texts)
        assert choice["logprobs"] == {
            "tokens": texts, "token_logprobs": [None] + [-0.5 * p for p in range(1, len(ids))],
            "top_logprobs": [None] + [{" t7": -0.25}] * (len(ids) - 1),
            "text_offset": [sum(len(t) for t in texts[:p]) for p in range(len(ids))]}
        assert choice["prompt_logprobs"] == [None] + [
            {str(ids[p]): {"logprob": -0.5 * p, "decoded_token": texts[p]}} for p in range(1, len(ids))]

        # The chat route, not streamed, with its own logprobs beside vLLM's field.
        status, out = _post(port, "/v1/chat/completions", {"messages": [{"role": "user", "content": "hi"}],
                                                           "max_tokens": 1, "logprobs": True, "top_logprobs": 1,
                                                           "prompt_logprobs": 1})
        assert status == 200 and seen[-1].score and seen[-1].max_new == 1
        ids, choice = seen[-1].prompt, out["choices"][0]
        assert [e["token"] for e in choice["logprobs"]["content"]] == [" t9"]
        assert choice["prompt_logprobs"][0] is None and len(choice["prompt_logprobs"]) == len(ids)
        assert choice["prompt_logprobs"][1][str(ids[1])]["logprob"] == -0.5
        assert choice["prompt_logprobs"][1]["7"]["rank"] == 1  # the top token's entry (the prompt token's own, if it is 7)

        # The completions route, streamed: the prompt's share is the first chunk, the token's offset follows it.
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=10)
        c.request("POST", "/v1/completions", body=json.dumps({"prompt": "abc", "echo": True, "logprobs": 0,
                                                              "max_tokens": 1, "stream": True}))
        chunks = [json.loads(line[6:]) for line in c.getresponse().read().decode().splitlines()
                  if line.startswith("data: {")]
        head, tok = chunks[0]["choices"][0], chunks[1]["choices"][0]
        texts = [" t%d" % t for t in seen[-1].prompt]
        assert head["text"] == "".join(texts) and head["logprobs"]["tokens"] == texts
        assert head["logprobs"]["top_logprobs"] == [None] + [{}] * (len(texts) - 1)
        assert tok["logprobs"] == {"tokens": [" t9"], "token_logprobs": [-0.125], "top_logprobs": [{}],
                                   "text_offset": [len(head["text"])]}
        assert chunks[-1]["choices"][0]["finish_reason"] == "length"

        # "echo" alone is no scoring request: it generates at least one token, and the fit check counts that token.
        n = eng.model.cfg.max_seq - 1
        status, out = _post(port, "/v1/completions", {"prompt": "a" * n, "echo": True, "max_tokens": 0})
        assert status == 400 and "context" in out["error"]["message"]
        status, out = _post(port, "/v1/completions", {"prompt": "a" * (n - 1), "echo": True, "max_tokens": 0})
        assert status == 200 and not seen[-1].score and seen[-1].max_new == 1 and len(seen[-1].prompt) == n - 1
    finally:
        srv.shutdown()
        eng.stop()


def test_gpus_passes_the_flag_on():
    on = arg_parser().parse_args(["--gpus", "2", "--prompt-logprobs"])
    off = arg_parser().parse_args(["--gpus", "2"])
    assert "--prompt-logprobs" in replica_cmd(on, 1) and "--prompt-logprobs" not in replica_cmd(off, 1)


@pytest.mark.parametrize("shape,grid", [((560, 64, 1), (3, 1)), ((560, 256, 17), (3, 2)), ((4112, 1024, 64), (17, 4))])
def test_lm_score_plan(shape, grid):
    p = ops.lm_score_plan(*shape)
    assert (p.slab, p.threads, (p.slabs, p.tiles), p.work_words) == (256, 256, grid, 5 * ops.MAX_ROWS * grid[0])
    with pytest.raises(ValueError):
        ops.lm_score_plan(shape[0], shape[1] + 8, shape[2])
    with pytest.raises(ValueError):
        ops.lm_score_plan(shape[0], shape[1], 65)
