"""On-device token log-probabilities: the kernel (ops.logprobs_, logprobs.hip)
against fp64, the engine's records, and the OpenAI responses.

Reference: ``torch.log_softmax`` of the same bf16 logits in float64, and the
order ``sorted(range(V), key=lambda i: (-z[i], i))``. Returned ids must match
the reference exactly; a logprob may differ from it by ``lp_bound``, derived
here from what the kernel computes (U = 2^-24, the fp32 unit roundoff; V the
row length; d_i = m - z_i >= 0; p_i = softmax_i):

* exp: the kernel calls the precise ``expf`` (ops/build.py compiles without
  fast-math), for which the OpenCL accuracy the device library is built to is
  <= 3 ulp = 6 U relative. Its argument fl(z_i - m) carries U d_i absolute,
  which is U d_i relative in the term. Over the sum that weighs as
  U sum_i p_i d_i = U (H(p) - log S) <= U log V, as S = sum_i exp(-d_i) >= 1.
  Terms that underflow (d_i > 87) change S by less than V 2^-126 (the +1e-30).
* the sum: every term is positive, so each fp32 add costs at most U relative
  to the total. A thread adds its 8 * ceil(V / 8192) terms serially, a wave
  reduces in a tree of depth 6, and the 16 wave totals are added serially:
  D = 8 ceil(V / 8192) + 22 adds deep, D U relative.
  So S carries (6 + log V + D) U relative, which is the same absolute in log S.
* log: precise ``logf``, <= 3 ulp = 6 U |log S| <= 6 U log V.
* one rounding of m + log S: U |lse|; one rounding of z - lse: U |logprob|.

  lp_bound = U (6 + D + 7 log V + |lse| + |logprob|) (1 + 2^-10) + 1e-30

(1 + 2^-10 covers the second-order terms.) At V = 128256 that is about 270 U =
1.6e-5 for a logprob near -12. -inf logits must give exactly -inf.

Largest observed error over the bound (MI355X): kernel cases 0.127 (5.6e-7
against a bound of 4.4e-6, a Gaussian row at V = 32), engine chosen logprobs
against a replay 3.8e-5 of its bound (see ``test_engine_records``).
"""
import functools
import http.client
import json
import math

import pytest
import torch

from p2p_llm_tunnel_amd import ops

pytestmark = pytest.mark.gpu
cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")

U = 2.0 ** -24
BF = torch.bfloat16
TOP = ops.MAX_TOP_LOGPROBS


def lp_bound(V: int, lse: float, lp: float) -> float:
    D = 8 * math.ceil(V / 8192) + 22
    return U * (6 + D + 7 * math.log(V) + abs(lse) + abs(lp)) * (1 + 2.0 ** -10) + 1e-30


# ---------------------------------------------------------------- kernel cases
ROW_KINDS = ("gauss0", "gauss1", "gauss2", "gauss3", "equal", "straddle5", "straddle20", "neginf", "spike")


def _row(kind: str, V: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(1000 + ROW_KINDS.index(kind) + V)
    if kind.startswith("gauss"):  # these tie naturally in bf16
        return (torch.randn(V, generator=g) * (1.0 + ROW_KINDS.index(kind))).to(BF)
    if kind == "equal":  # ids 0..N-1, each -log V
        return torch.full((V,), 1.5).to(BF)
    if kind.startswith("straddle"):
        # Three distinct large values, then equal values straddling rank N (100 of them where the row is long
        # enough), scattered over the row: of the equal ones the lowest ids win.
        z = torch.randn(V, generator=g).clamp_(max=2.0)
        perm = torch.randperm(V, generator=g)
        n_eq = min(100, V - 3)
        z[perm[:3]] = torch.tensor([9.0, 8.0, 7.0])
        z[perm[3:3 + n_eq]] = 5.0
        return z.to(BF)
    if kind == "neginf":  # -inf on half the entries
        z = torch.randn(V, generator=g)
        z[torch.randperm(V, generator=g)[:V // 2]] = -math.inf
        return z.to(BF)
    if kind == "spike":  # one logit far above the rest: 0 for it, a finite -160 for the others
        z = torch.full((V,), -80.0)
        z[V // 2 + 1] = 80.0
        return z.to(BF)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _reference(kind: str, V: int):
    """(bf16 row, fp64 log_softmax as a list, the first 20 ids of the reference order, lse)."""
    row = _row(kind, V)
    z = row.to(torch.float64)
    ref = torch.log_softmax(z, 0)
    zl = z.tolist()
    order = sorted(range(V), key=lambda i: (-zl[i], i))[:TOP]
    return row, ref.tolist(), order, float(torch.logsumexp(z, 0))


def _launch(V, kinds, wants, chosen):
    """One launch over ``kinds`` (a row each); returns (out_lp, out_ids) on the host. Outputs are prefilled with
    NaN / -1 so that untouched rows and columns show."""
    B = len(kinds)
    logits = torch.stack([_reference(k, V)[0] for k in kinds]).cuda()
    ids = torch.tensor(chosen, dtype=torch.int64, device="cuda")
    want = torch.tensor(list(wants) + [7, 7], dtype=torch.int64, device="cuda")  # [>= B]
    out_lp = torch.full((B, TOP + 1), math.nan, dtype=torch.float32, device="cuda")
    out_ids = torch.full((B, TOP), -1, dtype=torch.int32, device="cuda")
    ops.logprobs_(logits, ids, want, out_lp, out_ids)
    torch.cuda.synchronize()
    return out_lp.cpu(), out_ids.cpu()


_worst = {"ratio": 0.0}


def _check_close(got: float, ref: float, V: int, lse: float, what):
    if ref == -math.inf:
        assert got == -math.inf, (what, got)
        return
    bound = lp_bound(V, lse, ref)
    err = abs(got - ref)
    if err / bound > _worst["ratio"]:
        _worst["ratio"] = err / bound
        print(f"  {what}: error {err:.3e} / bound {bound:.3e}")
    assert err <= bound, (what, got, ref, err, bound)


def _check_launch(V, kinds, wants, chosen):
    out_lp, out_ids = _launch(V, kinds, wants, chosen)
    for r, (kind, w, c) in enumerate(zip(kinds, wants, chosen)):
        what = (V, kind, w)
        if w == 0:  # a row that is off keeps what it held
            assert torch.isnan(out_lp[r]).all() and (out_ids[r] == -1).all(), what
            continue
        N = w - 1
        _, ref, order, lse = _reference(kind, V)
        _check_close(out_lp[r, 0].item(), ref[c], V, lse, what + ("chosen", c))
        assert out_ids[r, :N].tolist() == order[:N], what
        for j in range(N):
            _check_close(out_lp[r, 1 + j].item(), ref[order[j]], V, lse, what + (j,))
        assert torch.isnan(out_lp[r, 1 + N:]).all() and (out_ids[r, N:] == -1).all(), what  # columns past N untouched


def _chosen(kind, V, r):
    if kind == "spike" and r % 2 == 0:
        return V // 2 + 1  # the maximum itself: logprob 0
    return (7 * r + V // 3) % V  # a non-maximal token


@cuda
@pytest.mark.parametrize("V", [32, 4096, 32000, 128256])
def test_kernel_single_rows(V):
    """B = 1: every row kind with every N."""
    for k, kind in enumerate(ROW_KINDS):
        for N in (0, 1, 5, 20):
            _check_launch(V, [kind], [1 + N], [_chosen(kind, V, k + N)])
    print(f"V={V}: largest error / bound so far = {_worst['ratio']:.3e}")


@cuda
@pytest.mark.parametrize("V", [32, 4096, 32000, 128256])
def test_kernel_mixed_launches(V):
    """B = 5: N in {0, 1, 5, 20} mixed within one launch, rows that are off between active rows."""
    launches = [
        (["gauss0", "equal", "gauss1", "straddle5", "gauss2"], [1 + 20, 1 + 5, 0, 1 + 5, 1 + 0]),
        (["neginf", "gauss2", "spike", "gauss3", "straddle20"], [1 + 1, 0, 1 + 5, 1 + 1, 1 + 20]),
        (["spike", "gauss1", "equal", "neginf", "gauss0"], [0, 1 + 20, 1 + 20, 1 + 20, 0]),
        (["equal", "straddle20", "gauss3", "gauss1", "neginf"], [1 + 0, 1 + 1, 1 + 20, 0, 1 + 5]),
    ]
    for kinds, wants in launches:
        _check_launch(V, kinds, wants, [_chosen(k, V, r) for r, k in enumerate(kinds)])
    print(f"V={V}: largest error / bound so far = {_worst['ratio']:.3e}")


@cuda
def test_kernel_expected_values_and_checks():
    V = 4096
    out_lp, out_ids = _launch(V, ["equal", "spike", "straddle5"], [1 + 20, 1 + 1, 1 + 5], [5, V // 2 + 1, 0])
    assert out_ids[0].tolist() == list(range(20))  # all equal: the lowest ids, each -log V
    assert all(abs(x + math.log(V)) <= lp_bound(V, 1.5 + math.log(V), math.log(V)) for x in out_lp[0].tolist())
    assert out_lp[1, 0].item() == 0.0 and out_lp[1, 1].item() == 0.0 and out_ids[1, 0].item() == V // 2 + 1
    row = _reference("straddle5", V)[0].float()
    eq = sorted((row == 5.0).nonzero().flatten().tolist())
    assert out_ids[2, 3:5].tolist() == eq[:2] and out_lp[2, 4].item() == out_lp[2, 5].item()
    # host-side validation: nothing is launched on mismatched tensors
    lg = torch.zeros(2, 64, dtype=BF, device="cuda")
    ids = torch.zeros(2, dtype=torch.int64, device="cuda")
    want = torch.ones(2, dtype=torch.int64, device="cuda")
    lp = torch.zeros(2, TOP + 1, device="cuda")
    oi = torch.zeros(2, TOP, dtype=torch.int32, device="cuda")
    ops.logprobs_(lg, ids, want, lp, oi)
    for bad in ((lg.float(), ids, want, lp, oi), (lg, ids.int(), want, lp, oi), (lg, ids, want[:1], lp, oi),
                (lg, ids, want, lp[:, :TOP], oi), (lg, ids, want, lp, oi.long()), (lg[:, :16], ids, want, lp, oi),
                (lg.cpu(), ids, want, lp, oi), (lg, ids[:1], want, lp, oi)):
        with pytest.raises((TypeError, ValueError)):
            ops.logprobs_(*bad)


# ---------------------------------------------------------------- engine
def _run(eng, prompt, n, **kw):
    from p2p_llm_tunnel_amd.models.server import Request
    r = eng.submit(Request(prompt, n, **kw))
    return list(iter(r.out.get, None)), r.lp


@cuda
def test_engine_records():
    """Engine(micro): one record per token, ordered and consistent; the same
    records beside a sampled neighbour and from a seeded sampled request run
    twice; chosen logprobs against a replay of the tokens through a second
    model with the same weights.

    The replay feeds one token per eager step, the engine chunked prefill in a
    captured graph, so a logit may differ by what tests/test_gpu_model.py
    allows between those: 1e-2 (graph vs eager) plus 1e-6 + 0.01 max|logit|
    (chunked vs sequential), together ``d``. A logprob z_c - lse then moves by
    at most 2 d (lse is 1-Lipschitz in the largest logit change), plus the
    kernel's own bound. Observed on an MI355X: at most 3.8e-5 of that (the
    replay's logits were equal to the engine's, or nearly)."""
    from p2p_llm_tunnel_amd.models.server import Engine, Request, Sampling
    from p2p_llm_tunnel_amd.models.tiny_llm import TinyLlama
    eng = Engine(device="cuda:0", config="micro", max_batch=4)
    try:
        prompt, n = list(b"logpr"), 12
        V = eng.model.cfg.vocab
        plain, none = _run(eng, prompt, n)
        toks, recs = _run(eng, prompt, n, logprobs=5)
        assert none == [] and toks == plain and len(recs) == n  # same tokens; one record per token
        slack = lp_bound(V, 20.0, 20.0)
        for t, (chosen, top) in zip(toks, recs):
            assert len(top) == 5
            for (ia, la), (ib, lb) in zip(top, top[1:]):
                assert la > lb or (la == lb and ia < ib), top  # non-increasing, ids ascending inside equal values
            assert chosen <= top[0][1]
            assert sum(math.exp(lp) for _, lp in top) <= 1 + 5 * slack
            listed = dict(top)
            if t in listed:
                assert listed[t] == chosen
        # beside a sampled neighbour (both prompts fit the 16-row graph, as alone)
        a = eng.submit(Request(prompt, n, logprobs=5))
        b = eng.submit(Request(list(b"other"), n, sampling=Sampling(temperature=1.0, seed=11)))
        ta, tb = list(iter(a.out.get, None)), list(iter(b.out.get, None))
        assert ta == toks and a.lp == recs and b.lp == [] and len(tb) == n
        # the request itself sampled, twice with one seed
        s1 = _run(eng, prompt, n, logprobs=5, sampling=Sampling(temperature=1.0, seed=42))
        s2 = _run(eng, prompt, n, logprobs=5, sampling=Sampling(temperature=1.0, seed=42))
        assert s1 == s2 and s1[0] != toks and len(s1[1]) == n
        # logprobs 0: the chosen token alone
        t0, r0 = _run(eng, prompt, n, logprobs=0)
        assert t0 == toks and r0 == [(c, []) for c, _ in recs]
    finally:
        eng.stop()
    # ground truth: replay prompt + generated tokens, one per step
    m = TinyLlama("micro", device="cuda", max_batch=1, seed=0)
    worst = 0.0
    for run_toks, run_recs in ((toks, recs), s1):
        seq = prompt + run_toks
        for p, tok in enumerate(seq[:-1]):
            _, logits = m.decode_step(torch.tensor([tok], device="cuda"), torch.tensor([p], dtype=torch.int32,
                                                                                        device="cuda"),
                                      (p, p), return_logits=True)
            k = p - (len(prompt) - 1)
            if k < 0:
                continue
            z = logits[0].to(torch.float64)
            ref = torch.log_softmax(z, 0)[seq[p + 1]].item()
            d = 1e-2 + 1e-6 + 0.01 * z.abs().max().item()
            bound = 2 * d + lp_bound(V, float(torch.logsumexp(z, 0)), ref)
            err = abs(run_recs[k][0] - ref)
            worst = max(worst, err / bound)
            assert err <= bound, (k, run_recs[k][0], ref, err, bound)
    print(f"engine chosen logprobs vs replay: largest error / bound = {worst:.3e}")


# ---------------------------------------------------------------- HTTP
@cuda
def test_http_logprobs():
    from p2p_llm_tunnel_amd.models.server import start_server
    srv, port, engine = start_server(device="cuda:0", config="micro", max_batch=4)
    try:
        conn = http.client.HTTPConnection("127.0.0.1", port, timeout=60)

        def post(path, body):
            conn.request("POST", path, body=json.dumps(body), headers={"content-type": "application/json"})
            r = conn.getresponse()
            return r.status, r.read()

        chat = {"max_tokens": 9, "messages": [{"role": "user", "content": "hi"}]}
        st, plain = post("/v1/chat/completions", chat)
        assert st == 200
        plain = json.loads(plain)
        assert "logprobs" not in plain["choices"][0]
        st, full = post("/v1/chat/completions", dict(chat, logprobs=True, top_logprobs=3))
        assert st == 200
        full = json.loads(full)
        assert full["choices"][0]["message"]["content"] == plain["choices"][0]["message"]["content"]
        entries = full["choices"][0]["logprobs"]["content"]
        assert len(entries) == full["usage"]["completion_tokens"] == 9
        assert all(len(e["top_logprobs"]) == 3 for e in entries)
        assert all(bytes(e["bytes"]).decode() == e["token"] and e["logprob"] <= 0 for e in entries)
        assert "".join(e["token"] for e in entries) == full["choices"][0]["message"]["content"]
        st, sse = post("/v1/chat/completions", dict(chat, logprobs=True, top_logprobs=3, stream=True))
        assert st == 200
        events = [l[6:] for l in sse.split(b"\n") if l.startswith(b"data: ")]
        assert events[-1] == b"[DONE]"
        chunks = [json.loads(e)["choices"][0] for e in events[:-1]]
        tokens = [c for c in chunks if c["finish_reason"] is None]
        assert len(tokens) == 9  # exactly one chunk per token
        assert all(len(c["logprobs"]["content"]) == 1 for c in tokens)
        assert [c["logprobs"]["content"][0] for c in tokens] == entries  # streamed == non-streamed (greedy)
        assert "".join(c["delta"]["content"] for c in tokens) == plain["choices"][0]["message"]["content"]
        # a matched stop sequence: its tokens keep their entries, the text is cut
        second = entries[1]["token"]
        st, cut = post("/v1/chat/completions", dict(chat, logprobs=True, stop=second.strip()))
        cut = json.loads(cut)["choices"][0]
        assert st == 200 and cut["finish_reason"] == "stop" and cut["message"]["content"] == entries[0]["token"] + " "
        assert [e["token"] for e in cut["logprobs"]["content"]] == [entries[0]["token"], second]
        assert cut["logprobs"]["content"][0]["top_logprobs"] == []
        # legacy completions
        st, legacy = post("/v1/completions", {"prompt": "hi", "max_tokens": 7, "logprobs": 2})
        assert st == 200
        choice = json.loads(legacy)["choices"][0]
        lp = choice["logprobs"]
        assert sorted(lp) == ["text_offset", "token_logprobs", "tokens", "top_logprobs"]
        assert all(len(lp[k]) == 7 for k in lp)
        assert "".join(lp["tokens"]) == choice["text"] and all(len(t) == 2 for t in lp["top_logprobs"])
        assert lp["text_offset"] == [sum(len(t) for t in lp["tokens"][:k]) for k in range(7)]
        # refused, each naming its field
        for path, bad, field in (("/v1/chat/completions", dict(chat, logprobs=True, top_logprobs=21), "top_logprobs"),
                                 ("/v1/chat/completions", dict(chat, top_logprobs=2), "top_logprobs"),
                                 ("/v1/completions", {"prompt": "hi", "logprobs": 6}, "logprobs")):
            st, body = post(path, bad)
            assert st == 400 and field in json.loads(body)["error"]["message"], (bad, body)
        # the same connection, without logprobs, afterwards
        st, again = post("/v1/chat/completions", chat)
        assert st == 200
        assert json.loads(again)["choices"][0]["message"]["content"] == plain["choices"][0]["message"]["content"]
    finally:
        engine.stop()
        srv.shutdown()
