"""Guided decoding on the GPU: ``ops.guide_`` (guide.hip) bit for bit against
its NumPy emulation, ``ops.guide_reset_``, the host-side validation of both, a
captured replay, the sampler on masked rows, the engine with ``guided=True``
(properties on ``tiny``, equality with a CPU reference generation on ``micro``)
and the endpoint on a synthetic checkpoint.

The kernel makes no rounding decision, so every comparison of its outputs is
exact. Token equality with the CPU reference (engine tests) needs a margin: the
engine's logits are bf16 and agree with the fp32 reference within about 0.01 x
max|logit| (test_gpu_model.py::test_chunked_prefill_matches_sequential). The
prompts below come from fixed seeds, searched on the CPU so that AFTER the mask
the reference's two largest allowed logits lie at least 0.03 x max|logit| apart
at every generated index; ``test_fixed_inputs_are_confident`` (CPU) re-checks
that from the seeds, and the GPU tests then demand equality at every index."""
import http.client
import json
import queue
import random
import re

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.guided import compile_guide
from p2p_llm_tunnel_amd.models.server import Engine, Penalties, Request, Sampling, start_server
from tests.guided_cases import completion, random_case, ref_generate, synthetic_vocab

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu

PATTERNS = [r"(yes|no|maybe)", r"[0-9]{3}-[0-9]{4}", r"-?[1-9][0-9]*(\.[0-9]+)?"]
MICRO_V, N_NEW, MARGIN = 4096, 8, 0.03
SEEDS = [1, 16, 11]  # per pattern: the prompt's seed
REFS = [[110, 111, 284, 284, 284, 284, 284, 284], [53, 49, 54, 45, 263, 54, 49, 284],
        [264, 46, 50, 56, 49, 262, 54, 49]]


def ids_of(seed, n, V=MICRO_V):
    rng = random.Random(seed)
    return [rng.randrange(V) for _ in range(n)]


@pytest.fixture(scope="module")
def micro_guides():
    tb, eos = synthetic_vocab(MICRO_V)
    return [compile_guide("regex", p, tb, eos, 64) for p in PATTERNS], tb, eos


def test_fixed_inputs_are_confident(micro_guides):
    from p2p_llm_tunnel_amd.models.tiny_llm import TinyLlama
    model = TinyLlama("micro", device="cpu", max_batch=1, seed=0)
    guides, tb, eos = micro_guides
    for g, seed, want in zip(guides, SEEDS, REFS):
        out, worst = ref_generate(model, ids_of(seed, 40), g, N_NEW)
        assert out == want and worst >= MARGIN, (out, worst)
        text, ended = completion(out, tb, eos)
        assert g.matches(text) if ended else g.viable(text)
        assert ref_generate(model, ids_of(seed, 40), None, N_NEW)[0] != want  # the guide decides


# ---------------------------------------------------------------- op
ORDER = ("x", "work", "ids", "tok", "dec", "slot", "base", "cur", "arena")


def _dev(case, in_place=False):
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in case.items() if k not in ("want", "x")}
    d["x"] = torch.from_numpy(case["x"].view(np.int16)).cuda().view(torch.bfloat16)
    d["work"] = d["x"] if in_place else torch.full_like(d["x"], 7.0)
    return d


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _check(d, case, what):
    torch.cuda.synchronize()
    work, ids, cur = case["want"]
    assert np.array_equal(_bits(d["work"]), work), what
    assert np.array_equal(d["ids"].cpu().numpy(), ids), what
    assert np.array_equal(d["cur"].cpu().numpy(), cur), what
    assert np.array_equal(d["base"].cpu().numpy(), case["base"]), what
    assert np.array_equal(d["arena"].cpu().numpy(), case["arena"]), what


@gpu
@cuda
@pytest.mark.parametrize("V", [32, 1000, 32000, 151936])
def test_kernel_bit_for_bit(V):
    for R in (1, 3, 16, 64):
        case = random_case(R, V, seed=R + V)
        work, ids, cur = case["want"]
        if R >= 16:  # the case moves something of every kind
            assert (work != case["x"]).any() and (ids != case["ids"]).any() and (cur != case["cur"]).any()
            assert (work[1] == case["x"][1]).all() and ids[1] == case["ids"][1]
        for in_place in (False, True):
            d = _dev(case, in_place)
            out = ops.guide_(*[d[k] for k in ORDER])
            assert out is d["work"]
            _check(d, case, (V, R, in_place))
            if not in_place:
                assert np.array_equal(_bits(d["x"]), case["x"])  # never written


@gpu
@cuda
def test_captured_replay_gives_the_same_bytes():
    from p2p_llm_tunnel_amd.models.tiny_llm import capture
    case = random_case(16, 32000, seed=5)
    d = _dev(case)
    keep = {k: d[k].clone() for k in ("ids", "cur")}
    graph, _ = capture(lambda: ops.guide_(*[d[k] for k in ORDER]), torch.device("cuda:0"))
    for _ in range(2):  # warm-up and capture ran the kernel: put the inputs it changes back, then replay
        d["ids"].copy_(keep["ids"])
        d["cur"].copy_(keep["cur"])
        d["work"].fill_(7.0)
        graph.replay()
        _check(d, case, "replay")


@gpu
@cuda
def test_guide_reset():
    arena = torch.full((50, 64), -1, dtype=torch.int16, device="cuda")
    base = torch.full((5,), 9, dtype=torch.int32, device="cuda")
    cur = torch.full((5,), 4, dtype=torch.int32, device="cuda")
    ops.guide_reset_(base, cur, arena, 2, 17)
    ops.guide_reset_(base, cur, arena, 4, -1)
    ops.guide_reset_(base, cur, arena, 0, 49)
    torch.cuda.synchronize()
    assert base.tolist() == [49, 9, 17, 9, -1] and cur.tolist() == [0, 4, 0, 4, 0]
    assert (arena == -1).all()


@gpu
@cuda
def test_validation_raises_before_a_launch():
    case = random_case(4, 64, seed=1)
    good = _dev(case)

    def bad(exc, **kw):
        with pytest.raises(exc):
            ops.guide_(*[kw.get(k, good[k]) for k in ORDER])

    for k in ORDER:  # dtype, device
        bad(TypeError, **{k: good[k].to(torch.float64)})
        bad(ValueError, **{k: good[k].cpu()})
    bad(ValueError, x=good["x"].T.contiguous().T)  # not contiguous
    bad(ValueError, work=good["work"][:3])
    bad(ValueError, work=good["x"].view(-1)[8:8 + 3 * 64].view(3, 64), x=good["x"][:3])  # overlaps, not the same
    bad(ValueError, ids=good["ids"][:3])
    bad(ValueError, tok=good["tok"][:3])
    bad(ValueError, dec=good["dec"][:3])
    bad(ValueError, slot=good["slot"][:3])
    bad(ValueError, slot=good["slot"].view(2, 4))
    bad(ValueError, cur=good["cur"][:5])
    bad(ValueError, base=good["base"].view(2, -1))
    bad(ValueError, arena=good["arena"][:, :32].contiguous())  # another vocabulary than the logits'
    bad(ValueError, arena=torch.zeros((3, 16), dtype=torch.int16, device="cuda"))  # V < 32
    bad(ValueError, arena=good["arena"].view(-1))
    odd = torch.zeros(4 * 64 + 8, dtype=torch.bfloat16, device="cuda")[1:4 * 64 + 1].view(4, 64)
    bad(ValueError, x=odd)  # not 16-byte aligned
    odd_arena = torch.zeros(96 * 64 + 8, dtype=torch.int16, device="cuda")[1:96 * 64 + 1].view(96, 64)
    bad(ValueError, arena=odd_arena)
    base, cur, arena = good["base"], good["cur"], good["arena"]
    for args in ((base, cur, arena, base.shape[0], 0), (base, cur, arena, -1, 0), (base, cur, arena, True, 0),
                 (base, cur, arena, 0, arena.shape[0]), (base, cur, arena, 0, -2), (base, cur, arena, 0, 1.0),
                 (base, cur[:3], arena, 0, 0), (base.cpu(), cur, arena, 0, 0)):
        with pytest.raises(ValueError):
            ops.guide_reset_(*args)
    with pytest.raises(TypeError):
        ops.guide_reset_(base.long(), cur, arena, 0, 0)
    torch.cuda.synchronize()
    assert (good["work"] == 7.0).all() and np.array_equal(good["cur"].cpu().numpy(), case["cur"])  # nothing ran
    assert np.array_equal(good["base"].cpu().numpy(), case["base"])


@gpu
@cuda
def test_sampler_never_draws_a_masked_id():
    """``sample_`` on rows ``guide_`` masked: temperature 1.5, a top-k larger
    than the allowed set and top-p < 1, 2,000 draws."""
    V, R, allowed = 32000, 50, [3, 700, 701, 15999, 31999]
    rng = np.random.default_rng(2)
    arena = np.full((2, V), -1, dtype=np.int16)
    arena[1, allowed] = 1
    x = torch.from_numpy(np.float32(rng.standard_normal((R, V)) * 3)).cuda().to(torch.bfloat16)
    work = torch.empty_like(x)
    ids = torch.zeros(R, dtype=torch.int64, device="cuda")
    zeros = torch.zeros(R, dtype=torch.int64, device="cuda")
    slot = torch.arange(R, dtype=torch.int64, device="cuda")
    base = torch.zeros(R, dtype=torch.int32, device="cuda")
    cur = torch.ones(R, dtype=torch.int32, device="cuda")
    ops.guide_(x, work, ids, zeros, zeros, slot, base, cur, torch.from_numpy(arena).cuda())
    assert set(ids.tolist()) <= set(allowed)
    seen = set()
    for ctr in range(40):
        params = torch.tensor([ops.pack_sampling(1.5, 50, 0.9, 1234 + r, ctr) for r in range(R)],
                              dtype=torch.int64).T.contiguous().cuda()
        drawn = ids.clone()
        ops.sample_(work, drawn, params)
        got = set(drawn.tolist())
        assert got <= set(allowed), got - set(allowed)
        seen |= got
    assert len(seen) >= 3  # it does sample


# ---------------------------------------------------------------- engine
def collect(req):
    out = []
    while (t := req.out.get(timeout=60)) is not None:
        out.append(t)
    return out


@gpu
@cuda
def test_engine_on_tiny_keeps_every_completion_inside_its_pattern():
    tb, eos = synthetic_vocab(32000)
    guides = [compile_guide("regex", p, tb, eos, 256) for p in PATTERNS]
    on = Engine(device="cuda:0", config="tiny", max_batch=4, seed=0, guided=True, guided_states=64)
    off = Engine(device="cuda:0", config="tiny", max_batch=4, seed=0)
    try:
        assert len(on._graphs) == 16 and len(off._graphs) == 12 and off._gd is None
        assert on._bufs[16][0].h_in.shape[0] == off._bufs[16][0].h_in.shape[0] == 11
        plain_prompt = ids_of(99, 100, 32000)
        want_plain = collect(off.submit(Request(list(plain_prompt), 10)))
        for pi, (g, pattern) in enumerate(zip(guides, PATTERNS)):
            plain = on.submit(Request(list(plain_prompt), 10))  # an unguided neighbour in the same steps
            reqs = [on.submit(Request(ids_of(7 + pi, 100, 32000), 12, guide=g,  # 100 rows: two prefill chunks
                                      sampling=None if s is None else Sampling(1.0, 0, 1.0, seed=s)))
                    for s in (None, 1, 2, 3)]
            outs = [collect(r) for r in reqs]
            assert collect(plain) == want_plain
            for out in outs:
                text, ended = completion(out, tb, eos)
                if ended:
                    assert re.fullmatch(pattern, text.decode()), (pattern, text)
                else:
                    assert len(out) == 12 and g.viable(text), (pattern, text)
            assert any(completion(o, tb, eos)[1] for o in outs) or pi == 2
        assert on.guide_uploads == 3 and on.guide_shared == 9  # one table per pattern, shared by its four requests
        # A table larger than the arena, another vocabulary, and an engine without the switch.
        with pytest.raises(ValueError, match="the arena holds 64"):
            on.submit(Request([1], 2, guide=compile_guide("regex", "[a-c]{70}", tb, eos, 256)))
        with pytest.raises(ValueError, match="vocabulary of 4096"):
            on.submit(Request([1], 2, guide=compile_guide("regex", "a", *synthetic_vocab(4096), 8)))
        with pytest.raises(ValueError, match="guided=True"):
            off.submit(Request([1], 2, guide=guides[0]))
        # More states than fit at once: the requests wait for room, take it in turn and all finish.
        big = [compile_guide("regex", "[a-c]{%d}" % n, tb, eos, 256) for n in (40, 41, 42)]
        reqs = [on.submit(Request(ids_of(3, 20, 32000), 50, guide=g)) for g in big]
        for g, r in zip(big, reqs):
            text, ended = completion(collect(r), tb, eos)
            assert ended and g.matches(text)
    finally:
        on.stop()
        off.stop()


@pytest.fixture(scope="module")
def micro_engine():
    eng = Engine(device="cuda:0", config="micro", max_batch=4, seed=0, guided=True, guided_states=64, penalties=True,
                 prefix_cache=True)
    yield eng
    eng.stop()


@gpu
@cuda
def test_engine_matches_the_cpu_reference(micro_engine, micro_guides):
    eng = micro_engine
    guides, tb, eos = micro_guides
    assert len(eng._graphs) == 20 and eng._bufs[16][0].h_in.shape[0] == 15
    reqs = [eng.submit(Request(ids_of(seed, 40), N_NEW, guide=g)) for g, seed in zip(guides, SEEDS)]
    assert [collect(r) for r in reqs] == REFS
    for g, seed, want in zip(guides, SEEDS, REFS):  # one by one: each lands in a slot another guide has just left
        assert collect(eng.submit(Request(ids_of(seed, 40), N_NEW, guide=g))) == want


@gpu
@cuda
def test_engine_with_penalties_and_the_prefix_cache(micro_engine, micro_guides):
    eng = micro_engine
    guides, tb, eos = micro_guides
    g, prompt, want = guides[1], ids_of(SEEDS[1], 40), REFS[1]
    first = eng.submit(Request(list(prompt), N_NEW, guide=g))
    assert collect(first) == want
    again = eng.submit(Request(list(prompt), N_NEW, guide=g))  # admitted in place on the cached rows
    assert collect(again) == want and again.cached_tokens == len(prompt) - 1
    # Guided and penalised: the reference's first token is banned, the completion still matches the pattern.
    ban = Penalties(logit_bias={want[0]: -100.0})
    out = collect(eng.submit(Request(list(prompt), N_NEW, guide=g, penalties=ban, logprobs=2)))
    text, ended = completion(out, tb, eos)
    assert want[0] not in out and len(out) == N_NEW
    assert g.matches(text) if ended else g.viable(text)
    # ... and an unguided request into a slot a guided one has left is not masked.
    plain = collect(eng.submit(Request(list(prompt), N_NEW)))
    assert plain != want and not g.viable(completion(plain, tb, eos)[0])


class _LoggedQueue(queue.Queue):
    """A request's output queue that also notes every put in a list shared by
    several requests: the engine thread makes all of them, so the list is the
    order in which their tokens arrived."""

    def __init__(self, log, name):
        super().__init__()
        self.log, self.name = log, name

    def put(self, item, *a, **kw):
        self.log.append((self.name, item))
        super().put(item, *a, **kw)


@gpu
@cuda
def test_a_guided_request_without_room_waits_at_the_head_of_the_queue():
    """The arena holds either table, not both: B waits for A's table to be given
    back, and C, unguided and queued behind B, does not overtake it although
    slots are free all the time."""
    tb, eos = synthetic_vocab(MICRO_V)
    ga, gb = compile_guide("regex", "[a-c]{20}", tb, eos, 64), compile_guide("regex", PATTERNS[1], tb, eos, 64)
    S = max(ga.n_states, gb.n_states)
    assert S < ga.n_states + gb.n_states
    eng = Engine(device="cuda:0", config="micro", max_batch=4, seed=0, guided=True, guided_states=S)
    try:
        log = []
        reqs = {"A": Request(ids_of(1, 20), 30, guide=ga), "B": Request(ids_of(2, 20), 12, guide=gb),
                "C": Request(ids_of(3, 20), 4)}
        for name, r in reqs.items():
            r.out = _LoggedQueue(log, name)
        for r in reqs.values():  # in this order
            eng.submit(r)
        outs = {name: collect(r) for name, r in reqs.items()}
        assert [len(outs[k]) for k in "ABC"] == [30, 12, 4]
        for g, out in ((ga, outs["A"]), (gb, outs["B"])):
            text, ended = completion(out, tb, eos)
            assert g.matches(text) if ended else g.viable(text), text
        assert eng.guide_uploads == 2 and eng.guide_shared == 0
        first = {k: next(i for i, (name, t) in enumerate(log) if name == k and t is not None) for k in "ABC"}
        last_a = max(i for i, (name, t) in enumerate(log) if name == "A" and t is not None)
        assert first["B"] > last_a  # B was admitted only once A had left
        # C came after B: its prompt is as long as B's and it sits in a higher slot, so its first token
        # follows B's in the step that runs both; admitted ahead of B it would have come during A.
        assert first["C"] > first["B"]
    finally:
        eng.stop()


def _post(port, path, body):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    c.request("POST", path, body=json.dumps(body), headers={"content-type": "application/json"})
    r = c.getresponse()
    return r.status, r.read()


@gpu
@cuda
def test_served_checkpoint_takes_guided_choice_over_http(tmp_path):
    from tests.test_checkpoint import _hf_checkpoint, _tokenizer_dir
    _hf_checkpoint(str(tmp_path))
    _tokenizer_dir(str(tmp_path))
    srv, port, eng = start_server(port=0, device="cuda:0", max_batch=2, checkpoint=str(tmp_path), max_seq=256,
                                  guided=True, guided_states=128)
    try:
        assert len(eng._graphs) == 16
        choices = ["hello world", "tunnel", "ünïcödé"]
        msgs = [{"role": "user", "content": "hello world"}]
        for key in ({"guided_choice": choices}, {"structured_outputs": {"choice": choices}},
                    {"guided_regex": "(hello world|tunnel|ünïcödé)"}):
            status, data = _post(port, "/v1/chat/completions", {"messages": msgs, "max_tokens": 24, **key})
            j = json.loads(data)
            assert status == 200 and j["choices"][0]["message"]["content"] in choices, j
            assert j["choices"][0]["finish_reason"] == "stop"
            status, data = _post(port, "/v1/chat/completions", {"messages": msgs, "max_tokens": 24, "stream": True,
                                                                "temperature": 1.0, "seed": 3, **key})
            objs = [json.loads(l[6:]) for l in data.split(b"\n") if l.startswith(b"data: {")]
            text = "".join(o["choices"][0]["delta"].get("content", "") for o in objs)
            assert status == 200 and text in choices and objs[-1]["choices"][0]["finish_reason"] == "stop"
        status, data = _post(port, "/v1/completions", {"prompt": "hello", "max_tokens": 3, "guided_regex": "[a-z]{9}"})
        j = json.loads(data)
        assert status == 200 and j["choices"][0]["finish_reason"] == "length"  # cut: a prefix of a match
        assert re.fullmatch("[a-z]{1,9}", j["choices"][0]["text"])
        assert eng.guide_uploads == 2 and len(srv._guides) == 3  # the choice list and its regex share one table
        for body, reason in (({"guided_regex": "(a"}, "missing"), ({"guided_regex": "a", "guided_choice": ["a"]}, "combined"),
                             ({"guided_choice": []}, "non-empty"), ({"guided_regex": "[a-c]{200}"}, "max_states")):
            status, data = _post(port, "/v1/completions", {"prompt": "hello", "max_tokens": 3, **body})
            assert status == 400 and reason in json.loads(data)["error"]["message"], data
    finally:
        srv.shutdown()
        eng.stop()
