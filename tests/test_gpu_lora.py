"""LoRA adapters on the GPU (docs/LORA.md): ``ops.lora_delta`` against fp64, the fused step with adapters (what stays
bit-identical to the base step; every stage of layers 0 and 1 against the unrounded effective weight W' + B'A' with
tests/test_gpu_fused_stages.py's references and bounds), and the engine and endpoint."""
import functools

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig, TinyLlama, capture
import test_gpu_fused_stages as stages
from test_gpu_fused_stages import BF, F64, U, Case, Inputs, cuda, rounded, stage_ratios, worst

N_ADAPTERS = 3


def delta_ref(x, A, B, aid):
    """delta = B'_a (A'_a x) per row in fp64, nothing rounded, and the bound on the kernel's fp32 value.

    The shrink sums K exact bf16 products in fp32 through the MFMA chain and the 4-wave split: t is within
    E_t = (K + 16) U sum_k |x_k||A'_rk| of its fp64 value (``gemm_ref``'s recursive-sum bound). The kernel then rounds
    t to bf16 once, as PEFT's bf16 forward does, so the expand's operand is within D_t = E_t + ulp(|t| + E_t) / 2 of t
    (``rounded``). The expand sums R exact products of B' and that operand in fp32: sum_r |B'_nr| D_t[r] for the
    operand's error, and (R + 16) U sum_r |B'_nr| (|t_r| + D_t[r]) for its own sum. A row without an adapter has
    reference 0 and bound 0: exactly 0.0."""
    M, K = x.shape
    n, R, _ = A.shape
    ref = torch.zeros(M, B.shape[1], dtype=F64)
    bound = torch.zeros_like(ref)
    xd = x.to(F64)
    for a in range(n):
        rows = (aid == a).nonzero().flatten()
        if not len(rows):
            continue
        Ad, Bd = A[a].to(F64), B[a].to(F64)
        t = xd[rows] @ Ad.T
        Dt = rounded(t, (K + 16) * U * (xd[rows].abs() @ Ad.abs().T))
        ref[rows] = t @ Bd.T
        bound[rows] = Dt @ Bd.abs().T + (R + 16) * U * ((t.abs() + Dt) @ Bd.abs().T)
    return ref, bound


AID_PATTERNS = {
    "one": lambda rows: torch.full((rows,), 1),                                   # every row on one adapter
    "mixed": lambda rows: torch.arange(rows) % 4 - 1,                             # -1, 0, 1, 2 inside every tile
    "tile": lambda rows: torch.where(torch.arange(rows) < 16, -1, 2),             # a whole tile without an adapter
}


@functools.lru_cache(maxsize=None)
def op_inputs(K, R):
    g = torch.Generator().manual_seed(K + R)
    x = torch.randn(40, K, generator=g).to(BF)
    A = (torch.randn(N_ADAPTERS, R, K, generator=g) * K ** -0.5).to(BF)
    B = torch.randn(N_ADAPTERS, 512, R, generator=g).to(BF)
    return x, A, B


@cuda
@pytest.mark.gpu
@pytest.mark.parametrize("pattern", AID_PATTERNS)
@pytest.mark.parametrize("rows", (1, 17, 40))
@pytest.mark.parametrize("R", (16, 192))
@pytest.mark.parametrize("K", (256, 2048))
def test_lora_delta_matches_fp64(K, R, rows, pattern):
    x, A, B = op_inputs(K, R)
    x = x[:rows].contiguous()
    aid = AID_PATTERNS[pattern](rows).to(torch.int32)
    got = ops.lora_delta(x.cuda(), A.cuda(), B.cuda(), aid.cuda()).cpu()
    ratio = worst(got, delta_ref(x, A, B, aid))
    print("RATIO lora_delta", K, R, rows, pattern, round(ratio, 3))
    assert ratio <= 1.0
    assert not bool(got[aid < 0].any())
    assert bool(got[aid >= 0].any()) == bool((aid >= 0).any())  # at one row, two of the patterns name no adapter


# ---------------------------------------------------------------- the step
def _cfg(n_layers):
    # ffn 352: gate/up's 704 columns are no multiple of k_lora_delta's 256 per workgroup, down's K has 11 k-steps.
    return LlamaConfig(vocab=stages.VOCAB, dim=256, n_layers=n_layers, n_heads=4, n_kv_heads=2, head_dim=64, ffn=352,
                       max_seq=64)


def make_lora(cfg, b_scale=0.25, seed=3):
    """``N_ADAPTERS`` random rank-8 adapters on every module as ``ops.pack_lora`` packs them with the norm weights of
    ``TinyLlama(cfg, seed)`` (CPU tensors). ``b_scale`` is large enough to move the outputs by many bf16 ulps."""
    m = TinyLlama(cfg, device="cpu", max_batch=1, seed=seed)
    g = torch.Generator().manual_seed(77 + seed)

    def stacked(name, sizes, K, norm):
        packed = [ops.pack_lora(cfg, name, [torch.randn(8, K, generator=g) * K ** -0.5 for _ in sizes],
                                [torch.randn(n, 8, generator=g) * b_scale for n in sizes], 0.5, norm)
                  for _ in range(N_ADAPTERS)]
        return tuple(torch.stack(t) for t in zip(*packed))
    return [{name: stacked(name, sizes, K, L.get({"wqkv": "attn_norm", "w_gate_up": "ffn_norm"}.get(name)))
             for name, (sizes, K) in ops.lora_shapes(cfg).items()} for L in m.layers]


class Step:
    """One step of ``TinyLlama(cfg, seed 3)`` on ``rows`` rows, row b on slot b, with ``lora`` or without."""

    def __init__(self, cfg, rows, kv_dtype="bf16", lora=None):
        self.m = m = TinyLlama(cfg, device="cuda", max_batch=rows, seed=3, kv_dtype=kv_dtype)
        self.dec = m.fused_decoder() if lora is None else ops.FusedLlamaDecoder(
            m.dims(), m.fused_weights(), m.k_cache, m.v_cache,
            lora=[{k: (A.cuda(), B.cuda()) for k, (A, B) in layer.items()} for layer in lora])
        self.tokens = torch.randint(0, cfg.vocab, (rows,), generator=torch.Generator().manual_seed(3)).cuda()
        self.pos = torch.tensor([(7 * r + 3) % 61 for r in range(rows)], dtype=torch.int32).cuda()
        self.logits = torch.empty(rows, cfg.vocab, dtype=BF, device="cuda")
        self.ids = torch.empty(rows, dtype=torch.int64, device="cuda")

    def run(self, adapters=None, zeroed=()):
        """The step (``zeroed`` tensors held at zero during it) and ``state()``."""
        saved = [w.clone() for w in zeroed]
        for w in zeroed:
            w.zero_()
        self.step(adapters)
        return self.state(zip(zeroed, saved))

    def step(self, adapters=None):  # the launch alone: capturable
        self.dec.step(self.tokens, self.pos, self.logits, self.ids, **({} if adapters is None else {"adapters": adapters}))

    def state(self, restore=()):  # every per-row workspace buffer, the cache rows appended, logits and ids (CPU)
        torch.cuda.synchronize()
        for w, s0 in restore:
            w.copy_(s0)
        rows = torch.arange(len(self.ids), device="cuda")
        out = {"logits": self.logits.cpu(), "ids": self.ids.cpu(),
               "kc": self.m.k_cache[:, rows, self.pos.long()].float().cpu().transpose(0, 1),
               "vc": self.m.v_cache[:, rows, self.pos.long()].float().cpu().transpose(0, 1)}
        for k, v in self.dec.workspace_views().items():
            if k not in ("delta", "counters", "qkv"):  # [parts, 64] or [64, ...] -> rows first
                out[k] = (v.T if k in ("ss", "am_val", "am_idx") else v)[:len(self.ids)].cpu()
        return out


def differ(a, b, rows=slice(None)):
    return [k for k in a if not torch.equal(a[k][rows], b[k][rows])]


@cuda
@pytest.mark.gpu
@pytest.mark.parametrize("kv_dtype", ("bf16", "fp8"))
@pytest.mark.parametrize("rows", (1, 17, 40))
def test_rows_without_an_adapter_are_the_base_step(rows, kv_dtype):
    cfg = _cfg(2)
    want = Step(cfg, rows, kv_dtype).run()
    # Adapters 0, 1, 2, none repeating (the one row of a 1-row step, whose O projection runs in K parts, is on 0).
    lo = Step(cfg, rows, kv_dtype, make_lora(cfg))
    aid = ((torch.arange(rows) + 1) % 4 - 1).to(torch.int32)
    aid_d = aid.cuda()
    got = lo.run(aid_d)
    assert differ(got, want, aid < 0) == []
    assert not torch.equal(got["resid"][aid >= 0], want["resid"][aid >= 0])  # a dropped delta would leave them equal
    graph, _ = capture(lambda: lo.step(aid_d), "cuda")  # three replays of the captured step are the eager call
    for _ in range(3):
        lo.logits.zero_()
        graph.replay()
        assert differ(lo.state(), got) == []
    # adapters=None on the same decoder, and every row on an adapter whose B' is zero: the base step.
    assert differ(lo.run(), want) == []
    zero = Step(cfg, rows, kv_dtype, make_lora(cfg, b_scale=0.0))
    assert differ(zero.run(torch.ones(rows, dtype=torch.int32, device="cuda")), want) == []


def gemm_ref_lora(x, w, eps=None, *, adapters, aid):
    """``gemm_ref`` on the effective weight W' + B'_a A'_a of each row's adapter, in fp64 and not rounded:
    y = x W'^T + B'(A' x), and to the accumulator's E the delta's bound (``delta_ref``) and the one fp32 add that joins
    the two, U |y|, ahead of the 1/rms factor's own error. ``adapters``: id(weight of the table) -> (A', B')."""
    if id(w) not in adapters:
        return GEMM_REF(x, w, eps)
    (y, E), (d, Ed) = GEMM_REF(x, w), delta_ref(x, *adapters[id(w)], aid)
    y = y + d
    E = E + Ed + U * y.abs()
    if eps is not None:
        rs = torch.rsqrt(x.to(F64).pow(2).mean(1, keepdim=True) + eps)
        y, E = y * rs, E * rs + (x.shape[1] / 2 + 8) * U * (y * rs).abs()
    return y, E


GEMM_REF = stages.gemm_ref


@cuda
@pytest.mark.gpu
@pytest.mark.parametrize("rows", (1, 3, 17))
@pytest.mark.parametrize("layer", (0, 1))
def test_lora_stages_match_fp64(layer, rows, monkeypatch):
    """Every stage of ``layer`` (the last of layer + 1) from its own observed inputs, adapters 0 and 1 alternating; at
    1 and 3 rows O adds its delta on the K-parts path. Three passes as in tests/test_gpu_fused_layers.py."""
    cfg = _cfg(layer + 1)
    assert (ops.step_plan(stages.llama_dims(cfg, rows + 1), rows).o.kpl > 0) == (rows <= 4)
    lora = make_lora(cfg)
    st = Step(cfg, rows, lora=lora)
    aid = (torch.arange(rows) % 2).to(torch.int32)
    wo, w_down = (stages.layer_w(cfg, st.dec.weights, layer, n) for n in ("wo", "w_down"))
    bo, bdown = st.dec.lora[layer]["wo"][1], st.dec.lora[layer]["w_down"][1]
    p1, p2, p3 = (st.run(aid.cuda(), z) for z in ([wo, w_down, bo, bdown], [w_down, bdown], []))
    assert differ({k: p1[k] for k in ("q", "attn")}, p3) == [] and torch.equal(p2["h"], p3["h"])
    obs = {"x0": p1["resid"], "q": p3["q"], "attn": p3["attn"], "h": p3["h"], "r1": p2["resid"], "r2": p3["resid"],
           "kc": st.m.k_cache[layer].cpu(), "vc": st.m.v_cache[layer].cpu(), "logits": p3["logits"], "ids": p3["ids"]}
    assert not torch.equal(Step(cfg, rows).run()["resid"], p3["resid"])  # the adapters move the step

    W = [w.cpu() for w in st.dec.weights]
    adapters = {id(stages.layer_w(cfg, W, layer, name)): lora[layer][name] for name in ops.LAYER_GEMMS}
    monkeypatch.setattr(stages, "gemm_ref", functools.partial(gemm_ref_lora, adapters=adapters, aid=aid))
    ratios = stage_ratios(Case("lora", cfg, tuple(st.pos.tolist())), W, obs, layer=layer,
                          inp=Inputs(None, W, st.tokens.cpu(), st.pos.cpu(), None, None, None))
    print("RATIO lora step layer", layer, "rows", rows, {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios


@cuda
@pytest.mark.gpu
def test_engine_and_endpoint_serve_an_adapter(tmp_path):
    """``tiny``, one synthetic adapter, prefix cache: batched == alone != base; a base request reuses no adapter rows;
    every HTTP route with model = NAME returns the engine's own tokens under the adapter."""
    import http.client
    import json
    from p2p_llm_tunnel_amd.models.engine import Request
    from p2p_llm_tunnel_amd.models.server import start_server
    from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS
    from test_lora import write_adapter
    write_adapter(tmp_path, CONFIGS["tiny"], b_scale=0.5)
    srv, port, eng = start_server(device="cuda:0", config="tiny", max_batch=4, loras={"ad": str(tmp_path)},
                                  prefix_cache=True, prefix_min=4)
    try:
        assert len(eng._lora_graphs) == len(eng._graphs) > 0

        def gen(adapter, prompt, others=0):
            reqs = [Request(prompt, 8, adapter=adapter)] + [Request([9, 8, 7, 6 + i], 8) for i in range(others)]
            for r in reqs:
                eng.submit(r)
            return [list(iter(lambda r=r: r.out.get(timeout=60), None)) for r in reqs][0], reqs[0]

        alone, _ = gen("ad", list(range(40, 70)))
        again, r_ad = gen("ad", list(range(40, 70)), others=2)
        base, r_base = gen(None, list(range(40, 70)))
        assert len(alone) == 8 and again == alone and base != alone
        assert r_ad.cached_tokens > 0 and r_base.cached_tokens == 0  # the adapter's rows serve the adapter only
        with pytest.raises(ValueError, match="adapter"):
            eng.submit(Request([1, 2, 3], 2, adapter="other"))

        c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        c.request("GET", "/v1/models")
        assert [m["id"] for m in json.loads(c.getresponse().read())["data"]] == ["p2pt-tiny", "ad"]
        want = {m: "".join(" t%d" % t for t in gen(a, list(b"hello"))[0]) for m, a in (("ad", "ad"), ("p2pt-tiny", None))}
        assert want["ad"] != want["p2pt-tiny"]
        text = {"/v1/chat/completions": lambda o: o["choices"][0]["message"]["content"],
                "/v1/completions": lambda o: o["choices"][0]["text"], "/api/generate": lambda o: o["response"],
                "/api/chat": lambda o: o["message"]["content"]}
        for route, model in ((r, m) for r in text for m in want):
            body = {"model": model, "stream": False, "max_tokens": 8, "options": {"num_predict": 8},
                    **({"messages": [{"role": "user", "content": "hello"}]} if "chat" in route else {"prompt": "hello"})}
            c.request("POST", route, body=json.dumps(body), headers={"content-type": "application/json"})
            assert text[route](json.loads(c.getresponse().read())) == want[model], (route, model)
    finally:
        eng.stop()
        srv.shutdown()
