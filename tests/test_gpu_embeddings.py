"""The embedding routes on the GPU: the ``micro`` engine (max_batch 4) behind
the endpoint, compared with ``TinyLlama.reference_hidden`` (fp32, CPU, the same
seeded weights) pooled in fp64: the mean over all positions, L2-normalised.
The comparison is the cosine distance 1 - cos(a, b) <= DELTA.

DELTA is the model's error, not the pooling kernel's (test_gpu_embed_pool.py
holds that to a few fp32 roundings): the fused step keeps its activations in
bf16 and splits its sums by row count, so its final residual differs from the
fp32 reference's. That error was measured on the MI355X on these five prompts
without the new kernel: one ``decode_step`` per chunk of up to 64 rows, the
step's own ``resid`` rows read back through ``workspace_views()``, normalised
and pooled in fp64, against the fp32 reference pooled the same way:

    tokens             5        16        17        64       150
    1 - cos    2.198e-05 1.220e-05 1.742e-05 2.145e-05 1.178e-05

DELTA = 4 x the largest, the allowance for batching-dependent attention splits
(a request's rows run in other row counts next to other requests).

The chats that run next to the embedding requests use the prompts of
test_gpu_prefix_cache.py, whose fp32 top-2 margins are re-checked on the CPU
there, so their greedy tokens are compared for equality."""
import http.client
import json
import os
import random

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd.models.server import Request, start_server
from test_gpu_prefix_cache import N_NEW, TAILS

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu

V, DIM = 4096, 256  # micro
LENGTHS = (5, 16, 17, 64, 150)
DELTA = 4 * 2.198e-05


def prompt(n):
    rng = random.Random(4000 + n)
    return [rng.randrange(V) for _ in range(n)]


def cos_dist(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 1.0 - float(a @ b) / float(np.sqrt(a @ a) * np.sqrt(b @ b))


@pytest.fixture(scope="module")
def references():
    """fp32 reference hidden states of the prompts, mean-pooled and normalised in fp64 (computed once)."""
    from p2p_llm_tunnel_amd.models.tiny_llm import TinyLlama
    m = TinyLlama("micro", device="cpu", max_batch=1, seed=0)
    assert (m.cfg.vocab, m.cfg.dim) == (V, DIM)
    refs = {}
    for n in LENGTHS:
        h = m.reference_hidden(torch.tensor([prompt(n)]))[0].double().numpy()
        pooled = h.mean(axis=0)
        refs[n] = pooled / np.sqrt(pooled @ pooled)
    return refs


@pytest.fixture(scope="module")
def endpoint():
    srv, port, eng = start_server(device="cuda:0", config="micro", max_batch=4)
    yield port, eng
    eng.stop()
    srv.shutdown()


def post(port, path, body):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    c.request("POST", path, body=json.dumps(body), headers={"content-type": "application/json"})
    r = c.getresponse()
    data = r.read()
    assert r.status == 200, data
    return json.loads(data)


def embedding(port, ids):
    j = post(port, "/v1/embeddings", {"input": ids})
    assert j["usage"]["prompt_tokens"] == len(ids) and len(j["data"]) == 1
    e = np.asarray(j["data"][0]["embedding"], dtype=np.float32)
    assert e.shape == (DIM,) and abs(float(np.sqrt(e.astype(np.float64) @ e)) - 1.0) < 1e-5
    return e


def collect(req):
    out = []
    while (t := req.out.get(timeout=60)) is not None:
        out.append(t)
    return out


@gpu
@cuda
def test_embeddings_match_the_fp32_reference(endpoint, references):
    port, eng = endpoint
    assert len(eng._graphs) == 12  # the pooling launch is never captured
    before = eng.embeddings
    j = post(port, "/v1/embeddings", {"input": [prompt(n) for n in LENGTHS]})  # one batch: 5 items on 4 slots
    assert [d["index"] for d in j["data"]] == list(range(len(LENGTHS)))
    for n, d in zip(LENGTHS, j["data"]):
        alone = embedding(port, prompt(n))
        for what, e in (("alone", alone), ("batched", np.asarray(d["embedding"], dtype=np.float32))):
            dist = cos_dist(e, references[n])
            print(f"embedding of {n} tokens, {what}: 1 - cos = {dist:.3e}")
            assert dist <= DELTA, (n, what, dist)
    assert len(eng._graphs) == 12 and eng.embeddings - before == 2 * len(LENGTHS)


@gpu
@cuda
def test_embedding_next_to_generating_chats(endpoint, references):
    port, eng = endpoint
    quiet = [collect(eng.submit(Request(list(t), N_NEW))) for t in TAILS]  # the chats without embeds, one by one
    assert all(len(q) == N_NEW for q in quiet)
    alone = embedding(port, prompt(150))
    chats = [eng.submit(Request(list(t), N_NEW)) for t in TAILS]  # three chats and the embed share the steps
    emb = eng.submit(Request(prompt(150), 1, embed="mean"))
    assert collect(emb) == [] and [collect(r) for r in chats] == quiet
    assert emb.embedding.dtype == np.float32 and emb.embedding.shape == (DIM,)
    dist = cos_dist(emb.embedding, alone)
    print(f"150 tokens next to three chats against alone: 1 - cos = {dist:.3e}")
    assert dist <= DELTA and cos_dist(emb.embedding, references[150]) <= DELTA
    assert len(eng._graphs) == 12


@gpu
@cuda
def test_last_pooling_and_the_ollama_routes(endpoint, references):
    port, eng = endpoint
    text = "".join(chr(32 + t % 90) for t in prompt(64))  # byte-level tokens: 64 of them
    ids = list(text.encode())
    want = embedding(port, ids)
    j = post(port, "/api/embed", {"model": "micro", "input": [text, text[:5]]})
    assert j["prompt_eval_count"] == 69 and len(j["embeddings"]) == 2
    assert cos_dist(j["embeddings"][0], want) <= DELTA
    assert cos_dist(post(port, "/api/embeddings", {"prompt": text})["embedding"], want) <= DELTA
    # "last" pooling is the same kernel on one row: of a one-token prompt it is the mean, bit for bit, and of a
    # longer one it is a unit vector that is not the mean (the stand-in of test_embeddings.py checks which row).
    one = [eng.submit(Request(prompt(5)[:1], 1, embed=mode)) for mode in ("last", "mean")]
    assert [collect(r) for r in one] == [[], []] and np.array_equal(one[0].embedding, one[1].embedding)
    last = eng.submit(Request(prompt(17), 1, embed="last"))
    assert collect(last) == []
    assert abs(float(np.sqrt(last.embedding.astype(np.float64) @ last.embedding)) - 1.0) < 1e-5
    assert cos_dist(last.embedding, references[17]) > 100 * DELTA


@gpu
@cuda
def test_embeddings_through_the_tunnel(endpoint, references):
    from p2p_llm_tunnel_amd.utils.procs import Tunnel
    port, eng = endpoint
    text = "an embedding request through the tunnel"
    direct = embedding(port, list(text.encode()))
    with Tunnel(f"http://127.0.0.1:{port}", transport=os.environ.get("P2PT_TRANSPORT", "webrtc")) as t:
        j = post(t.proxy_port, "/v1/embeddings", {"input": [text, prompt(150)], "encoding_format": "base64"})
        import base64
        got = [np.frombuffer(base64.b64decode(d["embedding"]), dtype="<f4") for d in j["data"]]
        assert got[0].shape == (DIM,) and cos_dist(got[0], direct) <= DELTA
        assert cos_dist(got[1], references[150]) <= DELTA
        assert cos_dist(post(t.proxy_port, "/api/embed", {"input": text})["embeddings"][0], direct) <= DELTA
        assert cos_dist(post(t.proxy_port, "/api/embeddings", {"prompt": text})["embedding"], direct) <= DELTA
