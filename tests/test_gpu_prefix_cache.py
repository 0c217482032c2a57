"""The prefix cache on the GPU: ``ops.kv_copy_`` (kv_copy.hip) bit for bit
against torch indexing, its host-side validation, the engine with
``prefix_cache=True`` against the same engine with it off, and the endpoint.

Token equality and its margin. A reused K/V row was computed by another graph
(a 16-row decode step, or another request's prefill chunking) than the row it
replaces, and schedules only agree within about 0.01 x max|logit|
(test_gpu_model.py::test_chunked_prefill_matches_sequential). Tokens are
therefore compared only where the fp32 reference decides clearly: the prompts
below come from fixed seeds, searched on the CPU so that
``TinyLlama.reference_logits`` has a top-2 gap of at least 0.03 x max|logit|
(the "confident" margin of test_fused_prefill_sized_steps_match_unfused) at
EVERY generated index of every compared request. About one candidate in 30
qualifies for 6 tokens. ``test_fixed_inputs_are_confident`` (CPU) re-checks the
condition and the reference tokens from the seeds; with such inputs the GPU
tests demand equality at every index, nothing skipped or cut short.

The 8-job kernel case runs on a third cache shape with 10 slots: 8 jobs with
distinct destinations and disjoint sources need at least 9, and the two
prescribed shapes have 5 and 4 (they take the largest legal mixed sets)."""
import http.client
import json
import random

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.server import Engine, Request, start_server

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu

V = 4096  # micro
N_NEW = 6
MARGIN = 0.03


def ids_of(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(V) for _ in range(n)]


def words(seed, n):
    rng = random.Random(seed)
    return " ".join("".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randrange(2, 9)))
                    for _ in range(n))


# Scenario 1: a two-turn conversation; the first prompt has 130 tokens.
TURN1 = ids_of(1058, 130)
REF_TURN1 = [3873, 3049, 434, 3033, 192, 523]
TURN2 = TURN1 + REF_TURN1 + ids_of(2013, 7)
REF_TURN2 = [1104, 940, 1678, 532, 4042, 136]
# Scenario 2: three requests share the 70-token prefix of a fourth that is generating.
SHARED = ids_of(3000, 70)
TAILS = [SHARED + ids_of(s, 4 + s % 7) for s in (3128, 3129, 3138)]
REF_TAILS = [[867, 1505, 274, 2002, 810, 987], [1407, 405, 3263, 2374, 19, 5], [475, 2467, 1907, 3546, 2840, 3835]]
BACKGROUND = SHARED + ids_of(3001, 9)  # generates throughout; not compared
# Endpoint: two chat turns (byte-level prompts; generated ids render as " t<id>").
CHAT1 = words(573, 12)
REF_CHAT1 = [1940, 3619, 2708, 329, 2622, 4030]
CHAT2 = words(917, 4)
REF_CHAT2 = [996, 3331, 1302, 3571, 3014, 2480]


def render(ids):
    return "".join(f" t{t}" for t in ids)


def chat_text(turn):
    return "\n".join([CHAT1, render(REF_CHAT1), CHAT2][:1 if turn == 1 else 3])


def test_fixed_inputs_are_confident():
    from p2p_llm_tunnel_amd.models.tiny_llm import TinyLlama
    m = TinyLlama("micro", device="cpu", max_batch=1, seed=0)
    assert m.cfg.vocab == V and TURN2[:135] == TURN1 + REF_TURN1[:5]
    cases = [(TURN1, REF_TURN1), (TURN2, REF_TURN2), *zip(TAILS, REF_TAILS),
             (list(chat_text(1).encode()), REF_CHAT1), (list(chat_text(2).encode()), REF_CHAT2)]
    for prompt, want in cases:
        seq = list(prompt)
        for k in range(N_NEW):
            lg = m.reference_logits(torch.tensor([seq]))[0]
            top = lg.topk(2).values
            gap, scale = float(top[0] - top[1]), float(lg.abs().max())
            assert gap >= MARGIN * scale, (len(prompt), k, gap / scale)
            assert int(lg.argmax()) == want[k]
            seq.append(want[k])
    assert all(len(t) > 70 and t[:70] == SHARED and t[70] != BACKGROUND[70] for t in TAILS)
    assert len({t[70] for t in TAILS}) == 3  # the common prefix of any two is exactly the shared 70


# ---------------------------------------------------------------- kernel
SHAPES = [(2, 5, 96, 2, 64), (3, 4, 40, 4, 128), (2, 10, 24, 2, 64)]


def _caches(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    mk = lambda: torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int16).cuda().view(torch.bfloat16)
    return mk(), mk()  # every 16-bit pattern: NaNs and infs included


def _job_sets(shape):
    n_slots, S = shape[1], shape[2]
    sets = [[(1, 3, 1)], [(0, 2, 17)], [(n_slots - 1, 0, S)], [(2, 1, 0)]]
    lens = [S, 0, 5, 17, 1, S - 1, 2, 33 % S]
    if n_slots >= 10:  # 8 jobs, two sources, mixed lengths, one of 0
        sets.append([(8 + d % 2, d, lens[d]) for d in range(8)])
    else:  # the most this shape allows: every other slot from one source
        sets.append([(n_slots - 1, d, lens[d]) for d in range(n_slots - 1)])
    return sets


@gpu
@cuda
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kv_copy_is_exact_and_writes_nothing_else(shape):
    for n, jobs in enumerate(_job_sets(shape)):
        k, v = _caches(shape, 7 * n + shape[1])
        want_k, want_v = k.clone().view(torch.int16), v.clone().view(torch.int16)
        for src, dst, rows in jobs:
            want_k[:, dst, :rows] = want_k[:, src, :rows]
            want_v[:, dst, :rows] = want_v[:, src, :rows]
        ops.kv_copy_(k, v, jobs)
        torch.cuda.synchronize()
        assert torch.equal(k.view(torch.int16), want_k), jobs  # the whole cache: a stray byte anywhere fails
        assert torch.equal(v.view(torch.int16), want_v), jobs


@gpu
@cuda
def test_kv_copy_validates_before_launching():
    assert ops.MAX_KV_COPY_JOBS == 8
    shape = (2, 10, 24, 2, 64)
    k, v = _caches(shape, 1)
    k0, v0 = k.clone().view(torch.int16), v.clone().view(torch.int16)
    ok = [(0, 1, 4)]
    narrow_k, narrow_v = _caches((1, 3, 8, 1, 4), 2)  # rows of 8 bytes
    bad = [
        (k.to(torch.float16), v, ok), (k, v.to(torch.float16), ok),            # dtype
        (k, v.cpu(), ok), (k.cpu(), v.cpu(), ok),                               # device
        (k.transpose(1, 2), v.transpose(1, 2), ok), (k, v[:, :, ::2], ok),      # contiguity
        (k[0], v[0], ok),                                                       # 5-D
        (k, v[:, :9].contiguous(), ok),                                         # equal shapes
        (k, v, []), (k, v, [(0, d, 1) for d in range(1, 10)]),                  # 1..8 jobs
        (k, v, [(-1, 1, 4)]), (k, v, [(0, 10, 4)]), (k, v, [(10, 0, 4)]),       # slots in range
        (k, v, [(0, 1, -1)]), (k, v, [(0, 1, 25)]),                             # 0 <= n <= max_seq
        (k, v, [(3, 3, 4)]),                                                    # src != dst
        (k, v, [(0, 1, 4), (1, 2, 4)]), (k, v, [(1, 2, 4), (0, 1, 4)]),         # source and destination
        (k, v, [(0, 2, 1), (1, 2, 1)]),                                         # a destination twice
        (narrow_k, narrow_v, [(0, 1, 4)]),                                      # rows a multiple of 16 bytes
    ]
    n0 = narrow_k.clone().view(torch.int16)
    for kk, vv, jobs in bad:
        with pytest.raises((TypeError, ValueError)):
            ops.kv_copy_(kk, vv, jobs)
    torch.cuda.synchronize()
    assert torch.equal(k.view(torch.int16), k0) and torch.equal(v.view(torch.int16), v0)
    assert torch.equal(narrow_k.view(torch.int16), n0)


# ---------------------------------------------------------------- engine
def collect(req):
    out = []
    while (t := req.out.get(timeout=60)) is not None:
        out.append(t)
    return out


@pytest.fixture(scope="module")
def pair():
    on = Engine(device="cuda:0", config="micro", max_batch=4, seed=0, prefix_cache=True)
    off = Engine(device="cuda:0", config="micro", max_batch=4, seed=0)
    yield on, off
    on.stop()
    off.stop()


def _slot(eng, req):
    return next(i for i, s in enumerate(eng._kv) if s is req.kv)


@gpu
@cuda
def test_engine_two_turns_reuse_the_slot(pair):
    on, off = pair
    assert len(on._graphs) == 12 == len(off._graphs)  # the copy is never captured
    hits, copies = on.prefix_hits, on.kv_copies
    outs = {}
    for eng in (on, off):
        r1 = eng.submit(Request(list(TURN1), N_NEW))
        out1 = collect(r1)
        r2 = eng.submit(Request(TURN1 + out1 + TURN2[136:], N_NEW))
        outs[eng] = (out1, collect(r2), r1.cached_tokens, r2.cached_tokens)
    assert outs[off][0] == REF_TURN1  # margin 0.076: the turn-2 prompt is the one the margins were checked for
    assert outs[on][:2] == outs[off][:2]
    assert outs[on][2:] == (0, 135) and outs[off][2:] == (0, 0)  # 130 prompt rows + 5 fed outputs
    assert (on.prefix_hits - hits, on.kv_copies - copies) == (1, 0)


@gpu
@cuda
def test_engine_copies_a_shared_prefix_from_a_busy_slot(pair):
    on, off = pair
    copies, cached = on.kv_copies, on.cached_tokens
    outs = {}
    for eng in (on, off):
        bg = eng.submit(Request(list(BACKGROUND), 160))
        bg.out.get(timeout=60)  # every prompt row of the background request is launched
        reqs = [eng.submit(Request(list(t), N_NEW)) for t in TAILS]
        outs[eng] = [collect(r) for r in reqs]
        if eng is on:
            assert not bg.cancelled and eng.slots[_slot(eng, bg)] is bg.kv  # it was generating throughout
            assert [r.cached_tokens for r in reqs] == [70, 70, 70]
            torch.cuda.synchronize()
            src = _slot(eng, bg)
            m = eng.model
            for r in reqs:  # copied from the busy slot, or admitted in place into a slot that was
                dst = _slot(eng, r)
                assert dst != src
                assert torch.equal(m.k_cache[:, dst, :70].view(torch.int16), m.k_cache[:, src, :70].view(torch.int16))
                assert torch.equal(m.v_cache[:, dst, :70].view(torch.int16), m.v_cache[:, src, :70].view(torch.int16))
        bg.cancelled = True
    assert outs[on] == outs[off]
    assert 1 <= on.kv_copies - copies <= 3  # the first of the three can only have been copied
    assert on.cached_tokens - cached == 210 and off.cached_tokens == 0


# ---------------------------------------------------------------- endpoint
def _chat(port, messages):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    c.request("POST", "/v1/chat/completions", body=json.dumps({"messages": messages, "max_tokens": N_NEW}),
              headers={"content-type": "application/json"})
    r = c.getresponse()
    assert r.status == 200
    return json.loads(r.read())


@gpu
@cuda
def test_endpoint_reports_cached_tokens():
    got = {}
    for cache in (True, False):
        srv, port, eng = start_server(device="cuda:0", config="micro", max_batch=4, prefix_cache=cache)
        try:
            first = {"role": "user", "content": CHAT1}
            j1 = _chat(port, [first])
            reply = j1["choices"][0]["message"]["content"]
            j2 = _chat(port, [first, {"role": "assistant", "content": reply}, {"role": "user", "content": CHAT2}])
            got[cache] = (reply, j2["choices"][0]["message"]["content"], j1["usage"], j2["usage"])
        finally:
            eng.stop()
            srv.shutdown()
    assert got[False][0] == render(REF_CHAT1)  # margin 0.057: the second prompt is the one that was checked
    assert got[True][:2] == got[False][:2]
    assert got[True][2]["prompt_tokens_details"] == {"cached_tokens": 0}
    assert got[True][3]["prompt_tokens_details"]["cached_tokens"] >= len(CHAT1.encode())
    assert "prompt_tokens_details" not in got[False][2] and "prompt_tokens_details" not in got[False][3]
