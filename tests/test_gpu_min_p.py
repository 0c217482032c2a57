"""min_p on the GPU: ``ops.sample_minp_`` (sample.hip's ``MINP`` instantiation) against the host replay of
tests/min_p_ref.py, id for id; the engine built with ``min_p=True``; and /api/chat with ``options.min_p``.

The min_p cut is ``okey(z_i) >= okey(fl32(m + lnp))``: one IEEE add of two values both sides hold bit for bit
(m is a maximum of the same z_i; lnp travels as bits), so the cut has no band and the ids are compared exactly. The
top-p cut keeps its band (tests/test_gpu_sample.py); a draw it leaves undecided must be one of the possible
winners, and tests/test_min_p_params.py asserts on the host that the cases have none.

The planted rows are what fails without the cut: their counters were searched so that the draw without min_p
returns a token that min_p must drop (or, sitting exactly at t, must be able to return)."""
import http.client
import json
import math

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd import ops
from tests import min_p_ref as R
from tests.test_gpu_prefix_cache import CHAT1, MARGIN, N_NEW, REF_CHAT1, render
from tests.test_gpu_sample import SENTINEL, U, _lp_bound, _row

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
gpu = pytest.mark.gpu
BF = torch.bfloat16


# ---------------------------------------------------------------- the kernel
def _run(case):
    logits = torch.from_numpy(np.stack(case.rows)).to(BF).cuda()
    assert torch.equal(logits.float().cpu(), torch.from_numpy(np.stack(case.rows)))  # the rows are exact bf16 values
    ids = torch.full((case.B,), SENTINEL, dtype=torch.int64, device="cuda")
    params = torch.tensor(case.block, dtype=torch.int64, device="cuda")
    assert params.shape == (6, R.LD)
    ops.sample_minp_(logits, ids, params)
    torch.cuda.synchronize()
    return ids.cpu().tolist()


def _check_case(name: str):
    case, ref = R.CASES[name](), R.replay_case(name)
    got = _run(case)
    sampled = undecided = 0
    for r, (d, g) in enumerate(zip(ref, got)):
        what = (name, r, case.col(r))
        if d.winner is None:
            assert g == SENTINEL, what  # a greedy row (T = 0) keeps what it held
            continue
        sampled += 1
        assert 0 <= g < case.V and math.isfinite(case.rows[r][g]), what + (g,)
        if d.decided:
            assert g == d.winner, what + (g, d.winner)
        else:
            undecided += 1
            assert g in d.possible, what + (g, sorted(d.possible))
    print(f"{name}: {sampled} draws compared, {sampled - undecided} decided by the reference, every id equal")
    return got


@cuda
@gpu
@pytest.mark.parametrize("V", (32, 1000, 32000, 128256))
def test_rows_replay(V):
    _check_case(f"rows-V{V}")


@cuda
@gpu
@pytest.mark.parametrize("B", (1, 16, 17))
def test_row_counts_replay(B):
    _check_case(f"rows-V1000-B{B}")


@cuda
@gpu
def test_special_rows_replay():
    got = _check_case("special-V1000")
    case = R.special_case()
    assert len(set(got[:3])) == 3  # all-equal rows: every token stays, the draw moves with the seed
    assert got[6] == int(np.argmax(case.rows[6]))  # the spike at min_p = 1


@cuda
@gpu
def test_planted_rows_replay():
    """The rows that fail without the cut: see ``min_p_ref.planted_case``."""
    got = _check_case("planted-V1000")
    case = R.planted_case()
    for tag, g in zip(case.tags, got):
        assert g == (R.B_ID if tag == "at" else R.A), (tag, g)
    # the same draws through the plain sampler: the second token wins wherever top-p alone does not drop it
    logits = torch.from_numpy(np.stack(case.rows)).to(BF).cuda()
    ids = torch.full((case.B,), SENTINEL, dtype=torch.int64, device="cuda")
    ops.sample_(logits, ids, torch.tensor(case.block[:5], dtype=torch.int64, device="cuda"))
    for tag, g in zip(case.tags, ids.cpu().tolist()):
        assert g == (R.A if tag == "m<p" else R.B_ID), (tag, g)


@cuda
@gpu
def test_off_is_the_plain_sampler():
    """``sample_`` with [5, ld] params and ``sample_minp_`` with row 5 = -inf return the same ids on 64 random rows
    (and on the greedy ones leave the same ids alone)."""
    case = R.rows_case(32000)
    logits = torch.stack([_row(("gauss0.5", "gauss2", "gauss4")[r % 3], case.V).roll(131 * r) for r in range(64)]).cuda()
    five = torch.tensor(case.block[:5], dtype=torch.int64, device="cuda")
    six = torch.cat([five, torch.full((1, R.LD), ops.f32_bits(-math.inf), dtype=torch.int64, device="cuda")])
    a = torch.full((64,), SENTINEL, dtype=torch.int64, device="cuda")
    b = a.clone()
    ops.sample_(logits, a, five)
    ops.sample_minp_(logits, b, six)
    assert torch.equal(a, b)
    a, T = a.cpu(), [R._f32(t) for t in case.block[0][:64]]
    assert all((x == SENTINEL) == (not t >= 1e-4) for x, t in zip(a.tolist(), T))
    assert len(set(a.tolist())) > 32


@cuda
@gpu
def test_validation_raises_before_a_launch():
    logits = torch.zeros((4, 64), dtype=BF, device="cuda")
    ids = torch.full((4,), SENTINEL, dtype=torch.int64, device="cuda")
    six = torch.tensor([ops.pack_sampling(1.0, 0, 1.0, 1, 0, 0.5)] * 8, dtype=torch.int64, device="cuda").T.contiguous()
    assert six.shape == (6, 8)
    bad = [
        (ValueError, dict(params=six[:5].contiguous())),  # [5, ld] belongs to sample_
        (ValueError, dict(params=torch.cat([six, six[:1]]))),  # [7, ld]
        (ValueError, dict(params=six[:, :3].contiguous())),  # ld < B
        (ValueError, dict(params=six.reshape(-1))),
        (ValueError, dict(params=six.T)),  # [8, 6] and not contiguous
        (TypeError, dict(params=six.to(torch.int32))),
        (ValueError, dict(params=six.cpu())),
        (ValueError, dict(params=torch.cat([six, six], dim=1)[:, :8])),  # not contiguous
        (TypeError, dict(logits=logits.float())),
        (ValueError, dict(logits=logits[0])),
        (ValueError, dict(ids=ids[:3])),
        (TypeError, dict(ids=ids.to(torch.int32))),
        (RuntimeError, dict(logits=logits[:0], ids=ids[:0])),  # B = 0: the entry point's own check
        (RuntimeError, dict(logits=logits[:, :0].contiguous())),  # V = 0
    ]
    for exc, kw in bad:
        args = dict(logits=logits, ids=ids, params=six)
        args.update(kw)
        with pytest.raises(exc):
            ops.sample_minp_(args["logits"], args["ids"], args["params"])
    with pytest.raises(ValueError):
        ops.sample_(logits, ids, six)  # and [6, ld] does not pass as the plain sampler's block
    lib = ops.lib()
    for B, ld, V in ((0, 8, 64), (4, 3, 64), (4, 8, 0), (-1, 8, 64)):
        assert lib.p2pt_sample_minp(logits.data_ptr(), ids.data_ptr(), six.data_ptr(), B, ld, V, None) != 0
    torch.cuda.synchronize()
    assert ids.cpu().tolist() == [SENTINEL] * 4  # nothing ran
    ops.sample_minp_(logits, ids, six)
    torch.cuda.synchronize()
    assert all(0 <= t < 64 for t in ids.cpu().tolist())


# ---------------------------------------------------------------- the engine
def _collect(req):
    out = []
    while (t := req.out.get(timeout=60)) is not None:
        out.append(t)
    return out


MIN_P, T_ENG, N_ENG = 0.3, 1.5, 8


@cuda
@gpu
def test_engine_min_p_batch():
    """Two sampled requests in one batch on ``Engine(min_p=True)``: the first with min_p = 0.3 and one top
    log-probability, the second without min_p. The same two, the first without its min_p, run on an engine without
    the switch.

    The first request's bound. The kernel keeps token i iff z_i >= t, with z_i = fl32(l_i fl32(1 / T)),
    t = fl32(m + lnp), m = max z and lnp = fl32(ln 0.3); the l_i are the bf16 logits, which both kernels read
    exactly. With U = 2^-24: |z_i - l_i / T| <= 2 U |l_i| / T (1 + U), |t - (m + lnp)| <= U |t| and
    |lnp - ln 0.3| <= U |ln 0.3|, so a kept token has

        (l_tok - l_max) / T >= ln 0.3 - U (4 L / T + L / T + 2 |ln 0.3|),   L >= max |l_i|.

    The record holds lp_i = l_i - lse from logprobs.hip, each within ``_lp_bound`` (tests/test_gpu_logprobs.py's
    bound, as tests/test_gpu_sample.py states it) of that, and the top-1 entry is the largest logit's, so
    l_tok - l_max = lp_token - lp_top1 to within 2 lp_bound. With L = 64 and |lse| <= 64 assumed, as there:

        slack = (2 lp_bound(V, 64, |lp_token|) / T + U (5 * 64 / T + 2 |ln 0.3|)) (1 + 2^-10),

    about 3e-5 at V = 4096. The same request without min_p on the other engine must break the bound somewhere
    (random-init logits: most of the mass lies below 0.3 p_max), or the bound would show nothing.

    The second request's tokens are those of the same request on the engine without the switch (same seed; its rows
    sit beside a request of the same length there too). Both engines hold 12 graphs."""
    from p2p_llm_tunnel_amd.models.server import Engine, Request, Sampling
    seeds = ((1 << 62) + 4321, 99)
    prompts = (b"min_p on", b"min_p off")
    runs = {}
    for on in (True, False):
        eng = Engine(device="cuda:0", config="micro", max_batch=4, seed=0, min_p=on)
        try:
            assert len(eng._graphs) == 12 and eng.min_p is on
            first = Sampling(temperature=T_ENG, seed=seeds[0], min_p=MIN_P if on else 0.0)
            second = Sampling(temperature=T_ENG, top_k=40, top_p=0.95, seed=seeds[1])
            reqs = [eng.submit(Request(list(p), N_ENG, sampling=s, logprobs=1))
                    for p, s in zip(prompts, (first, second))]
            runs[on] = [(_collect(r), r.lp) for r in reqs]
            V = eng.model.cfg.vocab
            if not on:
                with pytest.raises(ValueError, match="min_p"):
                    eng.submit(Request(list(prompts[0]), 2, sampling=Sampling(temperature=1.0, min_p=0.1)))
        finally:
            eng.stop()

    def worst(tokens, records):
        out = []
        for tok, (lp_tok, top) in zip(tokens, records):
            assert len(top) == 1 and top[0][1] >= lp_tok - 2 * _lp_bound(V, 64.0, abs(lp_tok))
            slack = (2 * _lp_bound(V, 64.0, abs(lp_tok)) / T_ENG +
                     U * (5 * 64.0 / T_ENG + 2 * abs(math.log(MIN_P)))) * (1 + 2.0 ** -10)
            out.append(((lp_tok - top[0][1]) / T_ENG - math.log(MIN_P), slack))
        return out

    with_cut, without = worst(*runs[True][0]), worst(*runs[False][0])
    print("min_p = 0.3: (lp_token - lp_top1) / T - ln 0.3 per token:", [round(x, 4) for x, _ in with_cut],
          "slack", max(s for _, s in with_cut), "; without the cut:", [round(x, 4) for x, _ in without])
    assert len(with_cut) == N_ENG == len(without)
    for x, slack in with_cut:
        assert x >= -slack, (x, slack)
    assert any(x < -slack for x, slack in without)
    assert runs[True][1][0] == runs[False][1][0] and len(runs[True][1][0]) == N_ENG
    assert runs[True][0][0] != runs[False][0][0]


@cuda
@gpu
def test_engine_min_p_beside_penalties_and_guide():
    """With penalties and the guide the staging block has every row group, and the penalty rows sit one further
    down: 20 graphs as without min_p, and a penalised request (greedy, and sampled without min_p) returns the tokens
    of an engine with penalties alone."""
    from p2p_llm_tunnel_amd.models.server import Engine, Penalties, Request, Sampling
    outs = {}
    for on in (True, False):
        eng = Engine(device="cuda:0", config="micro", max_batch=4, seed=0, penalties=True, guided=on, min_p=on)
        try:
            assert len(eng._graphs) == (20 if on else 16)
            pen = Penalties(repetition=1.3, frequency=0.5, presence=0.2)
            reqs = [eng.submit(Request(list(b"again and again and again"), N_ENG, penalties=pen, sampling=s))
                    for s in (Sampling(), Sampling(temperature=0.8, top_k=20, seed=5))]
            outs[on] = [_collect(r) for r in reqs]
        finally:
            eng.stop()
    assert outs[True] == outs[False] and all(len(o) == N_ENG for o in outs[True])


# ---------------------------------------------------------------- the endpoint
def test_chat_prompt_is_confident():
    """CPU: the fp32 reference decides every token of the endpoint test's completion with a top-2 gap of at least
    0.03 x max|logit|, as tests/test_gpu_prefix_cache.py requires of it: no two bf16 logits tie at the maximum, so
    min_p = 1 leaves one token."""
    from p2p_llm_tunnel_amd.models.tiny_llm import TinyLlama
    m = TinyLlama("micro", device="cpu", max_batch=1, seed=0)
    seq = list(CHAT1.encode())
    for k in range(N_NEW):
        lg = m.reference_logits(torch.tensor([seq]))[0]
        top = lg.topk(2).values
        assert float(top[0] - top[1]) >= MARGIN * float(lg.abs().max()), k
        assert int(lg.argmax()) == REF_CHAT1[k]
        seq.append(REF_CHAT1[k])


def _api_chat(port, options, stream=False):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    c.request("POST", "/api/chat", body=json.dumps({"model": "m", "messages": [{"role": "user", "content": CHAT1}],
                                                    "stream": stream, "options": options}),
              headers={"content-type": "application/json"})
    r = c.getresponse()
    return r.status, r


@cuda
@gpu
def test_endpoint_min_p_one_is_greedy_and_streams_through_the_tunnel():
    from p2p_llm_tunnel_amd.models.server import start_server
    from p2p_llm_tunnel_amd.utils.procs import Tunnel
    srv, port, eng = start_server(device="cuda:0", config="micro", max_batch=4, min_p=True)
    try:
        st, r = _api_chat(port, {"temperature": 1, "min_p": 1.0, "seed": 7, "num_predict": N_NEW})
        obj = json.loads(r.read())
        assert st == 200 and obj["message"]["content"] == render(REF_CHAT1), obj
        assert obj["done_reason"] == "length" and obj["eval_count"] == N_NEW
        st, r = _api_chat(port, {"temperature": 1, "min_p": 0, "seed": 7, "num_predict": N_NEW})
        assert st == 200 and json.loads(r.read())["message"]["content"] != render(REF_CHAT1)  # it was the cut
        for bad in (1.5, True, "0.5"):
            st, r = _api_chat(port, {"temperature": 1, "min_p": bad})
            assert st == 400 and "min_p" in json.loads(r.read())["error"]["message"]
        with Tunnel(f"http://127.0.0.1:{port}", transport="tcp") as t:
            st, r = _api_chat(t.proxy_port, {"temperature": 1, "min_p": 1.0, "seed": 7, "num_predict": N_NEW}, True)
            assert st == 200 and r.getheader("content-type") == "application/x-ndjson"
            lines = []
            while (line := r.readline()):
                assert line.endswith(b"\n") and line.count(b"\n") == 1
                lines.append(json.loads(line))
        assert len(lines) == N_NEW + 1 and [o["done"] for o in lines] == [False] * N_NEW + [True]
        assert "".join(o["message"]["content"] for o in lines) == render(REF_CHAT1)
        assert lines[-1]["done_reason"] == "length" and lines[-1]["eval_count"] == N_NEW
    finally:
        eng.stop()
        srv.shutdown()
