"""The engine's prefix cache (``Engine(prefix_cache=True)``) on the CPU, with
a stand-in model that has memory: ``decode_step`` writes ``kv[slot, pos] =
token`` and returns ``(7 + 31 * sum_{j <= pos} (j + 1) * kv[slot, j]) % vocab``,
so a token depends on every row of its slot up to its position, and ``kv``
starts out poisoned: a row read before it was written (or copied) changes the
output. The expected completion is computed from the token history alone
(``expect``); every case is compared with it and with an engine built with the
cache off. The HIP copy kernel and the GPU engine are covered by
tests/test_gpu_prefix_cache.py."""
import http.client
import json
import random
import threading
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd.models.server import Engine, Request, start_server

V = 1009  # prime: no weight (j + 1) <= max_seq and no poison multiple vanishes mod V
POISON = 123457


class MemModel:
    def __init__(self, max_batch=4, vocab=V, max_seq=256, delay_s=0.0):
        self.cfg = SimpleNamespace(vocab=vocab, max_seq=max_seq)
        self.device = torch.device("cpu")
        self.max_batch = max_batch
        self.scratch_slot = max_batch
        self.delay_s = delay_s
        self.kv = np.full((max_batch + 1, max_seq), POISON, dtype=np.int64)
        self.w = np.arange(1, max_seq + 1, dtype=np.int64)
        self.log = []  # (slot, pos) of every row run
        self.copies = []  # one list of jobs per kv_copy call
        self.gate = threading.Event()  # cleared: the next decode_step blocks
        self.gate.set()
        self.blocked = threading.Event()

    def decode_step(self, tokens, pos, pos_range, slots=None):
        if not self.gate.is_set():
            self.blocked.set()
            self.gate.wait(20)
        if self.delay_s:
            time.sleep(self.delay_s)
        t, p, s = tokens.tolist(), pos.tolist(), slots.tolist()
        for tok, pp, ss in zip(t, p, s):
            self.kv[ss, pp] = tok
        self.log += list(zip(s, p))
        out = [(7 + 31 * int((self.w[:pp + 1] * self.kv[ss, :pp + 1]).sum())) % self.cfg.vocab for pp, ss in zip(p, s)]
        return torch.tensor(out, dtype=torch.int64)

    def kv_copy(self, jobs):
        jobs = [tuple(j) for j in jobs]
        assert 1 <= len(jobs) <= 8
        srcs, dsts = {j[0] for j in jobs}, [j[1] for j in jobs]
        assert not srcs & set(dsts) and len(set(dsts)) == len(dsts) and self.scratch_slot not in srcs | set(dsts)
        self.copies.append(jobs)
        for src, dst, n in jobs:
            self.kv[dst, :n] = self.kv[src, :n]


def expect(ids, n, vocab=V):
    """``n`` tokens after ``ids`` from the token history alone."""
    hist = [t % vocab for t in ids]
    acc = sum((j + 1) * t for j, t in enumerate(hist))
    out = []
    for _ in range(n):
        tok = (7 + 31 * acc) % vocab
        out.append(tok)
        acc += (len(hist) + 1) * tok
        hist.append(tok)
    return out


def ids_of(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(V) for _ in range(n)]


def collect(req, timeout=20):
    out = []
    while (t := req.out.get(timeout=timeout)) is not None:
        out.append(t)
    return out


def run(eng, prompt, max_new):
    req = eng.submit(Request(list(prompt), max_new))
    return req, collect(req)


def engine(cache=True, cls=Engine, **model_kw):
    return cls(model=MemModel(**model_kw), prefix_cache=cache)


def wait_for(cond, what, timeout=10):
    deadline = time.time() + timeout
    while not cond():
        assert time.time() < deadline, what
        time.sleep(0.002)


@pytest.fixture
def engines():
    made = []

    def make(*a, **kw):
        made.append(engine(*a, **kw))
        return made[-1]
    yield make
    for e in made:
        e.model.gate.set()
        e.stop()


def test_stand_in_has_memory():
    m = MemModel()
    tok = lambda t, p, s: int(m.decode_step(torch.tensor([t]), torch.tensor([p], dtype=torch.int32), (p, p),
                                            slots=torch.tensor([s], dtype=torch.int32))[0])
    assert [tok(5, 0, 0), tok(9, 1, 0)] == [(7 + 31 * 5) % V, (7 + 31 * (5 + 18)) % V]
    assert tok(9, 1, 1) != tok(9, 1, 0)  # row 0 of slot 1 was never written: the poison shows
    m.kv_copy([(0, 1, 1)])
    assert tok(9, 1, 1) == tok(9, 1, 0)


def test_multi_turn_is_admitted_in_place(engines):
    on, off = engines(True), engines(False)
    P = ids_of(1, 40)
    r1, out1 = run(on, P, 6)
    assert out1 == expect(P, 6) == run(off, P, 6)[1] and r1.cached_tokens == 0
    turn2 = P + out1 + ids_of(2, 7)
    mark, pre = len(on.model.log), on.prefill_tokens
    r2, out2 = run(on, turn2, 5)
    assert out2 == expect(turn2, 5) == run(off, turn2, 5)[1]
    assert r2.cached_tokens == 45  # the 6th output was never fed back: not resident
    rows = on.model.log[mark:]
    prompt_rows = [p for _, p in rows if p < len(turn2)]
    assert sorted(prompt_rows) == list(range(45, len(turn2)))  # exactly len(turn2) - 45 prompt rows ran
    assert len({s for s, _ in rows}) == 1 and rows[0][0] == on.model.log[0][0]  # in the slot turn 1 left
    assert on.prefill_tokens - pre == len(turn2) - 45 - 1
    assert on.model.copies == [] and on.kv_copies == 0
    assert (on.prefix_hits, on.cached_tokens) == (1, 45)
    assert (off.prefix_hits, off.cached_tokens, off.kv_copies) == (0, 0, 0)


def test_shared_prefix_is_copied_from_a_busy_slot(engines):
    on, off = engines(True, delay_s=0.003), engines(False)
    system = ids_of(3, 32)
    A, B = system + [1] + ids_of(4, 9), system + [2] + ids_of(5, 7)
    ra = on.submit(Request(A, 60))
    first = ra.out.get(timeout=20)
    rb, out_b = run(on, B, 5)
    out_a = [first] + collect(ra)
    slot_a, slot_b = on.model.log[0][0], next(s for s, _ in on.model.log if s != on.model.log[0][0])
    assert on.model.copies == [[(slot_a, slot_b, 32)]] and on.kv_copies == 1
    assert rb.cached_tokens == 32 and min(p for s, p in on.model.log if s == slot_b) == 32
    assert out_b == expect(B, 5) == run(off, B, 5)[1]
    assert out_a == expect(A, 60) == run(off, A, 60)[1]  # A is unaffected


def test_same_prompt_twice(engines):
    on = engines(True)
    P = ids_of(6, 50)
    assert run(on, P, 4)[1] == expect(P, 4)
    r, out = run(on, P, 4)
    assert out == expect(P, 4) and r.cached_tokens == len(P) - 1  # the last prompt token still runs, to sample


def test_below_the_minimum_nothing_is_reused(engines):
    on = engines(True)
    assert on.prefix_min == 16
    P = ids_of(7, 40)
    Q = P[:15] + [(P[15] + 1) % V] + ids_of(8, 20)
    run(on, P, 3)
    r, out = run(on, Q, 3)
    assert out == expect(Q, 3) and r.cached_tokens == 0 and on.prefix_hits == 0
    R = P[:16] + [(P[16] + 1) % V] + ids_of(9, 20)  # one more common id: reused
    r, out = run(on, R, 3)
    assert out == expect(R, 3) and r.cached_tokens == 16


def test_least_recently_freed_slot_is_overwritten(engines):
    on = engines(True, max_batch=2)
    convs = [ids_of(10 + i, 30) for i in range(3)]
    outs, slots = [], []
    for c in convs:
        mark = len(on.model.log)
        outs.append(run(on, c, 4)[1])
        assert outs[-1] == expect(c, 4)
        slots.append(on.model.log[mark][0])
    assert slots[0] != slots[1] and slots[2] == slots[0]  # the third overwrote the oldest residency
    follow = lambda i: convs[i] + outs[i] + ids_of(20 + i, 5)
    r, out = run(on, follow(1), 3)  # kept
    assert out == expect(follow(1), 3) and r.cached_tokens == 33
    r, out = run(on, follow(0), 3)  # evicted
    assert out == expect(follow(0), 3) and r.cached_tokens == 0


def test_truncated_prompt_matches_on_its_kept_tail(engines):
    on, off = engines(True, max_seq=64), engines(False, max_seq=64)
    P = ids_of(30, 100)
    kept = P[-(64 - 6 - 1):]
    r, out = run(on, P, 6)
    assert out == expect(kept, 6) == run(off, P, 6)[1] and r.cached_tokens == 0
    r, out = run(on, P, 6)
    assert out == expect(kept, 6) and r.cached_tokens == len(kept) - 1
    Q = ids_of(31, 3) + P  # another head, the same kept tail
    r, out = run(on, Q, 6)
    assert out == expect(kept, 6) and r.cached_tokens == len(kept) - 1
    shifted = P + out + ids_of(32, 4)  # its tail starts elsewhere: no row is at its old position
    r, out2 = run(on, shifted, 6)
    assert out2 == expect(shifted[-57:], 6) == run(off, shifted, 6)[1] and r.cached_tokens == 0


def test_cancelled_request_leaves_its_launched_rows(engines):
    on = engines(True, delay_s=0.002)
    P = ids_of(40, 20)
    r = on.submit(Request(P, 100))
    got = [r.out.get(timeout=20) for _ in range(5)]
    r.cancelled = True
    wait_for(lambda: not any(on.slots), "the cancelled request keeps its slot")
    launched = r.kv["pos"]
    assert 20 + 4 <= launched < 120 and got == expect(P, 5)
    wait_for(lambda: len(r.kv["known"]) > launched, "launched steps never drained")
    full = P + expect(P, launched - len(P) + 1)  # every token a launched step sampled; the last was never fed
    assert r.kv["known"] == full and on._resident(r.kv) == full[:launched]
    follow = full + ids_of(41, 5)
    r2, out = run(on, follow, 4)
    assert out == expect(follow, 4) and r2.cached_tokens == launched
    assert on.model.copies == []


def test_nine_hits_in_one_pass_take_two_launches(engines):
    on = engines(True, max_batch=10, delay_s=0.001)
    system = ids_of(50, 32)
    ra = on.submit(Request(system + [0] + ids_of(51, 7), 200))
    ra.out.get(timeout=20)
    on.model.gate.clear()
    assert on.model.blocked.wait(10)  # the engine thread sits in decode_step: the nine arrive in one pass
    prompts = [system + [i + 1] + ids_of(60 + i, 3 + i) for i in range(9)]
    reqs = [on.submit(Request(p, 3)) for p in prompts]
    on.model.gate.set()
    for p, r in zip(prompts, reqs):
        assert collect(r) == expect(p, 3) and r.cached_tokens == 32
    src = on.model.log[0][0]
    assert [len(c) for c in on.model.copies] == [8, 1] and on.kv_copies == 9 and on.prefix_hits == 9
    assert all(j[0] == src and j[2] == 32 for c in on.model.copies for j in c)
    assert len({j[1] for c in on.model.copies for j in c}) == 9
    ra.cancelled = True


def test_a_destination_that_becomes_a_source_splits_the_launches(engines):
    """Slot 0 and slot 2 are free with old residencies, slot 1 is busy with the
    shared prefix. Two requests with that prefix arrive in one pass: the first is
    copied 1 -> 0 (least recently freed); for the second, slot 0 (now busy, the
    copied rows resident) ties with slot 1 and comes first, so its job 0 -> 2
    reads what the first job writes and must go into a later launch."""
    on = engines(True, max_batch=3, delay_s=0.001)
    run(on, ids_of(70, 20), 2)  # slot 0
    system = ids_of(71, 32)
    ra = on.submit(Request(system + [0] + ids_of(72, 7), 200))  # slot 1: never used comes first
    ra.out.get(timeout=20)
    run(on, ids_of(73, 20), 2)  # slot 2
    assert [on.model.log[0][0], on.model.log[20 + 1][0]] == [0, 1] and on.model.log[-1][0] in (1, 2)
    on.model.gate.clear()
    assert on.model.blocked.wait(10)
    B = system + [1] + ids_of(74, 5)
    rb, rc = on.submit(Request(B, 3)), on.submit(Request(B, 3))
    on.model.gate.set()
    assert collect(rb) == expect(B, 3) == collect(rc)
    assert (rb.cached_tokens, rc.cached_tokens) == (32, 32)  # B's own rows past 32 were not launched yet
    assert on.model.copies == [[(1, 0, 32)], [(0, 2, 32)]] and on.kv_copies == 2
    ra.cancelled = True


def test_model_without_kv_copy_is_refused():
    from test_inference_server import FakeModel
    with pytest.raises(ValueError, match="kv_copy"):
        Engine(max_batch=4, model=FakeModel(), prefix_cache=True)


def test_default_engine_is_unchanged():
    from test_inference_server import FakeModel, expected
    eng = Engine(max_batch=4, model=FakeModel())
    try:
        assert eng.prefix_cache is False
        for _ in range(2):
            r = eng.submit(Request(list(b"x" * 40), 5))
            assert collect(r) == expected(b"x" * 40, 5) and r.cached_tokens == 0
        assert (eng.prefix_hits, eng.cached_tokens, eng.kv_copies) == (0, 0, 0)
        assert eng.prefill_tokens == 2 * 39
    finally:
        eng.stop()


def test_soak(engines):
    on = engines(True, max_batch=3)
    rng = random.Random(99)
    prefixes = [ids_of(80 + i, rng.randrange(20, 61)) for i in range(5)]
    work = []
    for i in range(200):
        p = rng.choice(prefixes)
        p = p[:rng.randrange(18, len(p) + 1)] + [rng.randrange(V) for _ in range(rng.randrange(0, 31))]
        work.append((p, rng.randrange(1, 13), rng.random() < 0.06))
    reqs = [on.submit(Request(p, n)) for p, n, _ in work]
    finished = 0
    for (p, n, cancel), r in zip(work, reqs):
        if cancel:  # after its first token; what it launched stays resident
            assert r.out.get(timeout=20) == expect(p, 1)[0]
            r.cancelled = True
        else:
            assert collect(r) == expect(p, n)
            finished += 1
    assert finished > 150 and on.prefix_hits > 0
    assert on.cached_tokens == sum(r.cached_tokens for r in reqs)
    assert on.kv_copies == sum(len(c) for c in on.model.copies)
    assert on.model.scratch_slot not in {s for s, _ in on.model.log}


def _chat(port, messages, n):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=20)
    c.request("POST", "/v1/chat/completions", body=json.dumps({"messages": messages, "max_tokens": n}),
              headers={"content-type": "application/json"})
    r = c.getresponse()
    assert r.status == 200
    return json.loads(r.read())


@pytest.mark.parametrize("cache", [True, False])
def test_http_reports_cached_tokens(cache):
    eng = engine(cache)
    srv, port, _ = start_server(port=0, engine=eng, model_name="mem", prefix_cache=cache)
    try:
        first = {"role": "user", "content": "a question of forty bytes, more or less."}
        text1 = "\n".join([first["content"]])
        j1 = _chat(port, [first], 5)
        reply = j1["choices"][0]["message"]["content"]
        assert reply == "".join(f" t{t}" for t in expect(text1.encode(), 5))
        msgs = [first, {"role": "assistant", "content": reply}, {"role": "user", "content": "and then?"}]
        j2 = _chat(port, msgs, 5)
        text2 = "\n".join(m["content"] for m in msgs)
        assert j2["choices"][0]["message"]["content"] == "".join(f" t{t}" for t in expect(text2.encode(), 5))
        if cache:
            assert j1["usage"]["prompt_tokens_details"] == {"cached_tokens": 0}
            assert j2["usage"]["prompt_tokens_details"] == {"cached_tokens": len(text1.encode())} and eng.prefix_hits == 1
        else:
            assert "prompt_tokens_details" not in j1["usage"] and "prompt_tokens_details" not in j2["usage"]
            assert set(j2["usage"]) == {"prompt_tokens", "completion_tokens", "total_tokens"}
    finally:
        srv.shutdown()
        eng.stop()


def test_start_server_refuses_a_contradicting_engine():
    eng = engine(False)
    try:
        with pytest.raises(ValueError, match="prefix_cache"):
            start_server(port=0, engine=eng, prefix_cache=True)
    finally:
        eng.stop()


class _CountsTheLastToken(Engine):
    """The slip: the last generated token, drained but never fed back, counted as resident."""

    @staticmethod
    def _resident(s):
        return list(s["known"])


def test_stand_in_catches_a_residency_slip(engines):
    bad = engines(True, cls=_CountsTheLastToken)
    P = ids_of(1, 40)
    _, out1 = run(bad, P, 6)
    assert out1 == expect(P, 6)
    turn2 = P + out1 + ids_of(2, 7)
    r, out2 = run(bad, turn2, 5)
    assert r.cached_tokens == 46 and out2 != expect(turn2, 5)  # row 45 was never written: the poison shows


def test_cli_flags_reach_the_children(monkeypatch):
    from p2p_llm_tunnel_amd.models import server
    cmds = []

    class _P:
        def __init__(self, cmd):
            cmds.append(cmd)

        def poll(self):
            return 0

        def terminate(self):
            pass
    import subprocess
    monkeypatch.setattr(subprocess, "Popen", _P)
    a = SimpleNamespace(port=9000, gpus=2, host="127.0.0.1", config="micro", max_batch=4, checkpoint=None, max_seq=None,
                        default_temperature=0.0, prefix_cache=True, prefix_min=24)
    assert server._replicas(a) == 0
    assert len(cmds) == 2 and all(c[-3:] == ["--prefix-cache", "--prefix-min", "24"] for c in cmds)
    cmds.clear()
    a.prefix_cache = False
    server._replicas(a)
    assert all("--prefix-cache" not in c and "--prefix-min" not in c for c in cmds)
