"""Embedding requests (``Request(embed=)``) and the three embedding routes on
the CPU, with the stand-in model of test_prefix_cache.py grown an
``embed_pool``: the "final hidden state" of a row is a known integer vector
that depends on the row's token, its position and every earlier token of its
slot (through the stand-in's poisoned ``kv``), ``decode_step`` leaves one per
row of the step in ``resid`` (the rows past the step poisoned), and
``embed_pool`` sums and L2-normalises them as embed_pool.hip does (without the
RMSNorm, which the kernel's own tests cover), on a poisoned ``acc``. Expected
embeddings are computed from the request's token history alone
(``expect_embedding``). The HIP kernel is covered by test_gpu_embed_pool.py,
the GPU engine and endpoint by test_gpu_embeddings.py."""
import base64
import http.client
import json
import socket
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd.models.server import Engine, Request, start_server
from test_prefix_cache import POISON, MemModel, V, collect, expect, ids_of, wait_for

DIM = 8
ROWS = 64
COLS = np.arange(DIM, dtype=np.int64) + 3


def hidden(c, pos, token):
    """The stand-in's hidden state of a row: ``c`` = sum_{j <= pos} (j + 1) * kv[slot, j]."""
    return ((c * COLS + 17 * pos + token) % 101 - 50).astype(np.float64)


class EmbModel(MemModel):
    def __init__(self, max_batch=4, max_seq=256, delay_s=0.0):
        super().__init__(max_batch=max_batch, max_seq=max_seq, delay_s=delay_s)
        self.cfg.dim = DIM
        self.resid = np.full((ROWS, DIM), float(POISON))
        self.acc = np.full((max_batch + 1, DIM), float(POISON))
        self.pools = []  # one list of jobs per embed_pool call

    def decode_step(self, tokens, pos, pos_range, slots=None):
        out = super().decode_step(tokens, pos, pos_range, slots=slots)
        self.resid[:] = float(POISON)
        for r, (t, p, s) in enumerate(zip(tokens.tolist(), pos.tolist(), slots.tolist())):
            self.resid[r] = hidden(int((self.w[:p + 1] * self.kv[s, :p + 1]).sum()), p, t)
        self.n_rows = len(tokens)
        return out

    def embed_pool(self, jobs, out):
        jobs = [tuple(j) for j in jobs]
        assert 1 <= len(jobs) <= 16 and out.dtype == torch.float32 and out.shape[1] == DIM
        accs, outs = [j[2] for j in jobs], [j[4] for j in jobs if j[3] & 2]
        assert len(set(accs)) == len(accs) and len(set(outs)) == len(outs) and self.scratch_slot not in accs
        self.pools.append(jobs)
        for row0, n, acc, flags, out_row in jobs:
            assert n >= 1 and 0 <= row0 and row0 + n <= self.n_rows and 0 <= flags <= 3
            a = np.zeros(DIM) if flags & 1 else self.acc[acc].copy()
            for r in range(row0, row0 + n):
                a += self.resid[r]
            if flags & 2:
                assert 0 <= out_row < out.shape[0]
                norm = np.sqrt((a * a).sum())
                out[out_row] = torch.from_numpy((a / norm if norm > 0 else a * 0).astype(np.float32))
                self.acc[acc] = float(POISON)  # the kernel leaves it alone; nobody may rely on it
            else:
                assert out_row == -1
                self.acc[acc] = a


def expect_embedding(ids, pooling="mean", max_seq=256):
    """The embedding of a prompt from its token history alone."""
    ids = [t % V for t in ids[:max_seq - 1]]
    c, total = 0, np.zeros(DIM)
    for p, t in enumerate(ids):
        c += (p + 1) * t
        h = hidden(c, p, t)
        total = h if pooling == "last" else total + h
    return (total / np.sqrt((total * total).sum())).astype(np.float32)


def embed(eng, ids, pooling="mean"):
    req = eng.submit(Request(list(ids), 1, embed=pooling))
    assert collect(req) == []  # no token is ever delivered
    return req


def close(a, b):
    return a is not None and a.dtype == np.float32 and a.shape == (DIM,) and np.allclose(a, b, rtol=0, atol=2e-7)


@pytest.fixture
def engines():
    made = []

    def make(cache=False, **kw):
        made.append(Engine(model=EmbModel(**kw), prefix_cache=cache))
        return made[-1]
    yield make
    for e in made:
        e.model.gate.set()
        e.stop()


def test_stand_in_pool_shows_poison_and_order():
    m = EmbModel()
    step = lambda toks, p0, slot: m.decode_step(torch.tensor(toks), torch.arange(p0, p0 + len(toks), dtype=torch.int32),
                                                (0, 0), slots=torch.full((len(toks),), slot, dtype=torch.int32))
    out = torch.zeros(2, DIM)
    step([5, 9, 2], 0, 1)
    m.embed_pool([(0, 3, 1, 3, 0)], out)
    assert close(out[0].numpy(), expect_embedding([5, 9, 2]))
    m.embed_pool([(0, 3, 1, 2, 1)], out)  # "first" not set: the poisoned acc shows
    assert not close(out[1].numpy(), expect_embedding([5, 9, 2]))
    m.embed_pool([(2, 1, 1, 3, 1)], out)
    assert close(out[1].numpy(), expect_embedding([5, 9, 2], "last"))


def test_single_chunk_prompt(engines):
    eng = engines()
    P = ids_of(1, 10)
    r = embed(eng, P)
    assert close(r.embedding, expect_embedding(P))
    assert eng.model.pools == [[(0, 10, 0, 3, 0)]] and eng.embeddings == 1
    assert eng.tokens_out == 0 and not any(eng.slots)
    assert sorted(eng.model.log) == [(0, p) for p in range(10)]  # the slot was freed with its last prompt row


def test_prompt_of_three_steps(engines):
    eng = engines()
    P = ids_of(2, 150)
    r = embed(eng, P)
    assert close(r.embedding, expect_embedding(P))
    assert eng.model.pools == [[(0, 64, 0, 1, -1)], [(0, 64, 0, 0, -1)], [(0, 22, 0, 2, 0)]] and eng.steps == 3


def test_last_pooling(engines):
    eng = engines()
    for n in (2, 10, 150):
        P = ids_of(3 + n, n)
        r = embed(eng, P, "last")
        assert close(r.embedding, expect_embedding(P, "last")) and not close(r.embedding, expect_embedding(P))
    assert [len(c) for c in eng.model.pools] == [1, 1, 1]  # one row each, in the step of the last prompt row
    assert eng.model.pools[-1] == [(21, 1, 0, 3, 0)]


def test_slot_reuse_and_hand_over(engines):
    eng = engines(max_batch=4)
    prompts = [ids_of(10 + i, n) for i, n in enumerate((5, 70, 1, 33, 129, 64, 65, 2))]  # 2 x max_batch, back to back
    reqs = [eng.submit(Request(list(p), 1, embed="mean")) for p in prompts]
    for p, r in zip(prompts, reqs):
        assert collect(r) == [] and close(r.embedding, expect_embedding(p))
    assert eng.embeddings == 8 and eng.model.scratch_slot not in {s for s, _ in eng.model.log}


def test_more_than_sixteen_jobs_take_two_launches(engines):
    eng = engines(max_batch=20)
    eng.model.gate.clear()
    first = eng.submit(Request(ids_of(30, 3), 1, embed="mean"))
    assert eng.model.blocked.wait(10)  # the engine sits in decode_step: the next twenty arrive in one pass
    prompts = [ids_of(31 + i, 1 + i % 3) for i in range(20)]
    reqs = [eng.submit(Request(list(p), 1, embed="mean")) for p in prompts]
    eng.model.gate.set()
    assert collect(first) == [] and close(first.embedding, expect_embedding(ids_of(30, 3)))
    for p, r in zip(prompts, reqs):
        assert collect(r) == [] and close(r.embedding, expect_embedding(p))
    assert [len(c) for c in eng.model.pools] == [1, 16, 4]


def test_embeds_between_generating_chats(engines):
    eng = engines(delay_s=0.001)
    chats = [(ids_of(50 + i, 20 + 30 * i), 25) for i in range(3)]
    creqs = [eng.submit(Request(list(p), n)) for p, n in chats]
    firsts = [r.out.get(timeout=20) for r in creqs]  # all three are generating
    prompts = [ids_of(60 + i, n) for i, n in enumerate((7, 150, 40, 64, 3))]
    ereqs = [eng.submit(Request(list(p), 1, embed="mean")) for p in prompts]
    late = eng.submit(Request(ids_of(70, 90), 12))  # a chat that prefills next to the embeds
    for p, r in zip(prompts, ereqs):
        assert collect(r) == [] and close(r.embedding, expect_embedding(p))
    for (p, n), r, f in zip(chats, creqs, firsts):
        assert [f] + collect(r) == expect(p, n)
    assert collect(late) == expect(ids_of(70, 90), 12)
    assert eng.tokens_out == 3 * 25 + 12


def test_cancelled_embed_frees_its_slot(engines):
    eng = engines(max_batch=1)
    eng.model.gate.clear()
    P = ids_of(80, 150)
    r = eng.submit(Request(list(P), 1, embed="mean"))
    assert eng.model.blocked.wait(10)  # its first 64 rows are running
    r.cancelled = True
    eng.model.gate.set()
    assert collect(r) == [] and r.embedding is None
    wait_for(lambda: not any(eng.slots), "the cancelled embed request keeps its slot")
    assert len(eng.model.log) < 150 and eng.embeddings == 0
    Q = ids_of(81, 70)  # the same slot and acc row, which hold the cancelled request's partial sum
    assert close(embed(eng, Q).embedding, expect_embedding(Q))


def test_truncation_keeps_the_head(engines):
    eng = engines(max_seq=64)
    P = ids_of(90, 100)
    r = embed(eng, P)
    assert close(r.embedding, expect_embedding(P, max_seq=64)) and len(eng.model.log) == 63
    assert not close(r.embedding, expect_embedding(P[-63:], max_seq=64))


def test_prefix_cache_embed_takes_no_prefix_and_leaves_its_rows(engines):
    on = engines(cache=True)
    P = ids_of(100, 40)
    _, out = (lambda r: (r, collect(r)))(on.submit(Request(list(P), 4)))
    assert out == expect(P, 4)
    mark = len(on.model.log)
    r = embed(on, P + out[:2])  # 41 of its rows are resident: it runs all the same
    assert r.cached_tokens == 0 and close(r.embedding, expect_embedding(P + out[:2]))
    assert sorted(p for _, p in on.model.log[mark:]) == list(range(42))
    Q = ids_of(101, 50)
    e = embed(on, Q)
    assert close(e.embedding, expect_embedding(Q)) and on.prefix_hits == 0
    chat = on.submit(Request(list(Q) + [7, 8], 5))  # the same text, as a chat: the embed request's rows are resident
    assert collect(chat) == expect(Q + [7, 8], 5) and chat.cached_tokens == 50 > 0
    assert on.model.copies == []


def test_model_without_embed_pool_is_refused():
    from test_inference_server import FakeModel
    eng = Engine(max_batch=4, model=FakeModel())
    try:
        assert eng.can_embed is False
        with pytest.raises(ValueError, match="embed_pool"):
            eng.submit(Request([1, 2, 3], 1, embed="mean"))
        with pytest.raises(ValueError, match="embed"):
            Request([1], 1, embed="max")
        assert Request([1], 1).embed is None
    finally:
        eng.stop()


# ---------------------------------------------------------------- HTTP
@pytest.fixture
def server():
    made = []

    def make(pooling="mean", **kw):
        eng = Engine(model=EmbModel(**kw))
        srv, port, _ = start_server(port=0, engine=eng, model_name="emb", embed_pooling=pooling)
        made.append((srv, eng))
        return port, eng
    yield make
    for srv, eng in made:
        srv.shutdown()
        eng.stop()


def post(port, path, body, conn=None):
    c = conn or http.client.HTTPConnection("127.0.0.1", port, timeout=20)
    c.request("POST", path, body=json.dumps(body), headers={"content-type": "application/json"})
    r = c.getresponse()
    return r.status, json.loads(r.read()), c


def vec(x):
    return np.asarray(x, dtype=np.float32)


TEXTS = ["a first sentence", "b", "the third one is longer than one step of sixty-four rows " * 2, "ünïcode too"]


def test_openai_route(server):
    port, eng = server()
    for path in ("/v1/embeddings", "/embeddings"):
        st, j, _ = post(port, path, {"input": TEXTS[0], "model": "whatever"})
        assert st == 200 and j["object"] == "list" and j["model"] == "emb"
        assert [(d["object"], d["index"]) for d in j["data"]] == [("embedding", 0)]
        assert close(vec(j["data"][0]["embedding"]), expect_embedding(TEXTS[0].encode()))
        assert j["usage"] == {"prompt_tokens": len(TEXTS[0]), "total_tokens": len(TEXTS[0])}
    st, j, _ = post(port, "/v1/embeddings", {"input": TEXTS})  # a batch, answered in input order
    assert st == 200 and [d["index"] for d in j["data"]] == [0, 1, 2, 3]
    for d, t in zip(j["data"], TEXTS):
        assert close(vec(d["embedding"]), expect_embedding(t.encode()))
    n_tok = sum(len(t.encode()) for t in TEXTS)
    assert j["usage"] == {"prompt_tokens": n_tok, "total_tokens": n_tok}
    st, jb, _ = post(port, "/v1/embeddings", {"input": TEXTS, "encoding_format": "base64"})
    assert st == 200
    for d, f in zip(jb["data"], j["data"]):  # little-endian float32 bytes of the float answer
        raw = base64.b64decode(d["embedding"])
        assert len(raw) == 4 * DIM and np.array_equal(np.frombuffer(raw, dtype="<f4"), vec(f["embedding"]))
    ids = ids_of(5, 30)
    st, j, _ = post(port, "/v1/embeddings", {"input": ids, "dimensions": DIM})  # token ids
    assert st == 200 and len(j["data"]) == 1 and close(vec(j["data"][0]["embedding"]), expect_embedding(ids))
    st, j, _ = post(port, "/v1/embeddings", {"input": [ids, ids[:3]]})
    assert st == 200 and close(vec(j["data"][1]["embedding"]), expect_embedding(ids[:3]))
    assert j["usage"]["prompt_tokens"] == 33


def test_ollama_routes(server):
    port, eng = server(max_seq=64)
    st, j, _ = post(port, "/api/embed", {"model": "m", "input": TEXTS[:2]})
    assert st == 200 and j["model"] == "emb" and j["prompt_eval_count"] == len(TEXTS[0]) + 1
    assert isinstance(j["total_duration"], int) and j["total_duration"] > 0
    assert [close(vec(e), expect_embedding(t.encode())) for e, t in zip(j["embeddings"], TEXTS)] == [True, True]
    st, j, _ = post(port, "/api/embed", {"input": TEXTS[0]})
    assert st == 200 and len(j["embeddings"]) == 1
    long = TEXTS[2]
    assert len(long) > 63
    st, j, _ = post(port, "/api/embed", {"input": long})  # truncate defaults to true: the first max_seq - 1 tokens
    assert st == 200 and j["prompt_eval_count"] == 63
    assert close(vec(j["embeddings"][0]), expect_embedding(long.encode(), max_seq=64))
    st, j, _ = post(port, "/api/embed", {"input": ["ok", long], "truncate": False})
    assert st == 400 and "input[1]" in j["error"]["message"]
    st, j, _ = post(port, "/api/embeddings", {"model": "m", "prompt": TEXTS[1]})  # legacy
    assert st == 200 and set(j) == {"embedding"} and close(vec(j["embedding"]), expect_embedding(TEXTS[1].encode()))


def test_last_pooling_route(server):
    port, eng = server("last")
    st, j, _ = post(port, "/v1/embeddings", {"input": TEXTS[2]})
    assert st == 200 and close(vec(j["data"][0]["embedding"]), expect_embedding(TEXTS[2].encode(), "last"))
    with pytest.raises(ValueError, match="embed_pooling"):
        start_server(port=0, engine=eng, embed_pooling="max")


def test_bad_requests_get_400_and_the_connection_lives(server):
    port, eng = server(max_seq=64)
    bad = [
        ({"input": ""}, "input is empty"), ({"input": ["ok", ""]}, "input[1]"), ({"input": []}, "input"),
        ({"input": [[]]}, "input[0]"), ({}, "input"), ({"input": 5}, "input"), ({"input": ["ok", 5]}, "input[1]"),
        ({"input": ["x"] * 257}, "256"), ({"input": "x" * 64}, "at most 63"), ({"input": ["ok", "y" * 100]}, "input[1]"),
        ({"input": [1, 2, V]}, "token ids"), ({"input": "ok", "dimensions": DIM + 1}, "dimensions"),
        ({"input": "ok", "encoding_format": "hex"}, "encoding_format"),
    ]
    conn = None
    for body, what in bad:
        st, j, conn = post(port, "/v1/embeddings", body, conn)  # one connection throughout: keep-alive after a 400
        assert st == 400 and what in j["error"]["message"], (body, j)
    st, j, conn = post(port, "/v1/embeddings", {"input": "x" * 63}, conn)
    assert st == 200 and close(vec(j["data"][0]["embedding"]), expect_embedding(b"x" * 63, max_seq=64))
    for path, body in (("/api/embed", {"input": [1, 2]}), ("/api/embed", {"input": "a", "truncate": "no"}),
                       ("/api/embeddings", {"prompt": ""}), ("/api/embeddings", {"input": "a"})):
        st, j, conn = post(port, path, body, conn)
        assert st == 400, (path, body)
    conn.request("POST", "/v1/embeddings", body=b"{not json", headers={"content-type": "application/json"})
    r = conn.getresponse()
    assert r.status == 400 and r.read()
    conn.request("GET", "/v1/embeddings")
    r = conn.getresponse()
    assert r.status == 404 and r.read()
    assert eng.embeddings == 1 and eng.thread.is_alive()


def test_engine_without_embed_pool_answers_400():
    from test_inference_server import FakeModel
    eng = Engine(max_batch=4, model=FakeModel())
    srv, port, _ = start_server(port=0, engine=eng, model_name="fake")
    try:
        st, j, _ = post(port, "/v1/embeddings", {"input": "hello"})
        assert st == 400 and "embed_pool" in j["error"]["message"]
    finally:
        srv.shutdown()
        eng.stop()


def test_disconnect_cancels_outstanding_items(server):
    port, eng = server(delay_s=0.01, max_batch=2)
    body = json.dumps({"input": ["z" * 200] * 12}).encode()
    s = socket.create_connection(("127.0.0.1", port), timeout=10)
    s.sendall(b"POST /v1/embeddings HTTP/1.1\r\nHost: x\r\nContent-Length: %d\r\n\r\n%s" % (len(body), body))
    wait_for(lambda: eng.steps >= 1, "the engine never started")
    s.close()
    wait_for(lambda: not any(eng.slots) and eng.pending.empty() and eng.steps >= 4, "items were left running")
    assert eng.embeddings < 12
    st, j, _ = post(port, "/v1/embeddings", {"input": "still there"})
    assert st == 200 and close(vec(j["data"][0]["embedding"]), expect_embedding(b"still there"))


def test_cli_flag_reaches_the_children(monkeypatch):
    import subprocess

    from p2p_llm_tunnel_amd.models import server as srv_mod
    cmds = []

    class _P:
        def __init__(self, cmd):
            cmds.append(cmd)

        def poll(self):
            return 0

        def terminate(self):
            pass
    monkeypatch.setattr(subprocess, "Popen", _P)
    a = SimpleNamespace(port=9000, gpus=2, host="127.0.0.1", config="micro", max_batch=4, checkpoint=None, max_seq=None,
                        default_temperature=0.0, prefix_cache=False, prefix_min=16, embed_pooling="last")
    assert srv_mod._replicas(a) == 0
    assert len(cmds) == 2 and all(c[-2:] == ["--embed-pooling", "last"] for c in cmds)
    cmds.clear()
    a.embed_pooling = "mean"
    srv_mod._replicas(a)
    assert all("--embed-pooling" not in c for c in cmds)
