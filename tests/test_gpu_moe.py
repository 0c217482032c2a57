"""The routed-expert FFN kernels (docs/MOE.md) on the GPU: ``ops.moe_ffn`` and the last MoE layer of real fused steps
against fp64, stage by stage. Every stage's reference is computed from what that stage's kernel read (the bf16 inputs
and the previous kernel's own outputs), so the bounds do not compound. u = 2^-24 (fp32), v = 2^-8 (one bf16 rounding).

router   |dl| <= Lb = (K + ss_u) u rs sum|x w|: the fp32 chain over K = dim, and ss_u units for 1/rms (the sum of
         `parts` partials, fma, rsqrtf) and the last product. Ids are compared exactly, so every fp64 gap among a
         row's first top_k + 1 logits must exceed 2 Lb (asserted on the reference alone: 0 undecided rows).
route_w  relative 4 Lb + 2 (range + 1) 2^-22 + (E + 4) u: the argument of __expf, __expf itself, the sum, the division.
moe_h    dg <= (K + 4) u rs sum|x w| + v |g|, up likewise; df <= 1.1 dg (|up| + dup) + |silu(g)| dup
         + (|g| + 4) 2^-22 |f| for the fp32 SiLU; the store adds v (|f| + df).
moe_part (K + 4) u |w| sum|h wd| over K = ffn_e.    resid  (top_k + 2) u (|resid| + sum|part|) + v |r|.
ss       (cb_cols + 2) u of the partial's value.

Shapes: dim 256, ffn_e 128; one case at dim 2048 / ffn_e 1024 takes the 8-wave kernels and the 8-column combine. Rows
1, 16, 17, 40, 64 cross 1 to 4 row tiles and RT = 1, 2, 4; at 1 row the combine has 4 columns, from 16 rows on 16.
Not covered: in a 2-layer step the first layer's MoE buffers are checked only through the second layer's input, and
only norm_topk = True runs through the step (the op covers both).
"""
import ctypes
import itertools

import pytest
import torch

from p2p_llm_tunnel_amd import ops

pytestmark = pytest.mark.gpu
U, V = 2.0 ** -24, 2.0 ** -8


def make_inputs(E, rows, dim=256, ffn=128, seed=0, plant=None):
    """bf16 inputs on the CPU. ``plant``: {row: [experts, most probable first]}: a signal of 8, 7, ... in column e of
    the row against a router whose first E columns are the identity, so the route is decided by design."""
    g = torch.Generator().manual_seed(1000 * E + rows + seed)
    x = torch.randn(64, dim, generator=g)
    router = torch.randn(E, dim, generator=g) * (2.0 / dim ** 0.5)
    if plant is not None:
        x[:, :E] = 0.0
        router[:, :E] = torch.eye(E) * 2.0
        router[:, E:] *= 0.1  # the other columns' share of a logit stays well below the signals' spacing
        for b, experts in plant.items():
            for j, e in enumerate(experts):
                x[b, e] = 8.0 - j
    wgu = torch.randn(E, 2 * ffn, dim, generator=g) / dim ** 0.5
    wd = torch.randn(E, dim, ffn, generator=g) / ffn ** 0.5
    x = x.to(torch.bfloat16)
    # The partial sums of squares as a producer with 16-column tiles leaves them.
    ss = x.double().pow(2).view(64, dim // 16, 16).sum(-1).T.contiguous().float()
    return x, ss, router.to(torch.bfloat16), wgu.to(torch.bfloat16), wd.to(torch.bfloat16)


def router_reference(x, ss, router, rows, top_k, norm_topk, eps, ss_u=None):
    """fp64 logits, their bound Lb, the route and the undecided-row count, from the inputs alone."""
    K = x.shape[1]
    ss_u = ss.shape[0] + 16 if ss_u is None else ss_u  # the units of u that 1/rms and the last product carry
    rs = (ss.double().sum(0)[:rows] / K + eps).rsqrt()
    xd, rd = x[:rows].double(), router.double()
    logit = rs[:, None] * (xd @ rd.T)
    Lb = (K + ss_u) * U * rs[:, None] * (xd.abs() @ rd.abs().T)
    order = torch.sort(logit, dim=1, descending=True, stable=True)
    ids = order.indices[:, :top_k]
    E = router.shape[0]
    undecided = 0
    if top_k < E:
        gap = order.values[:, top_k - 1] - order.values[:, top_k]
        undecided = int((gap <= 2 * Lb.max(1).values).sum())
    inner = order.values[:, : top_k - 1] - order.values[:, 1:top_k]
    undecided += int((inner <= 2 * Lb.max(1, keepdim=True).values).any(1).sum()) if top_k > 1 else 0
    e = (logit - logit.max(1, keepdim=True).values).exp()
    sel = e.gather(1, ids)
    w = sel / (sel.sum(1, keepdim=True) if norm_topk else e.sum(1, keepdim=True))
    rng = (logit.max(1).values - logit.min(1).values)[:, None]
    w_bound = w * (4 * Lb.max(1, keepdim=True).values + 2 * (rng + 1) * 2.0 ** -22 + (E + 4) * U)
    return rs, ids, w, w_bound, undecided


def hold_stages(x, rs_ref, ids_ref, w_ref, w_bound, rs_u, wgu, wd, got, resid, ss_new, plan):
    """One MoE layer against fp64: ``x`` the rows it read, ``got`` its buffers, ``resid`` / ``ss_new`` what it left."""
    rows, top_k = ids_ref.shape
    dim, ffn = x.shape[1], wd.shape[2]

    def hold(stage, value, ref, bound):
        assert torch.isfinite(value).all(), f"{stage}: a slot a pair owns was not written"
        ratio = ((value.double() - ref).abs() / bound).max().item()
        print(f"  {stage}: max error / bound = {ratio:.3f}")
        assert ratio <= 1.0, stage

    assert torch.equal(got["route_id"].long(), ids_ref), "route_id"
    hold("route_w", got["route_w"], w_ref, w_bound)
    hold("route_rs", got["route_rs"], rs_ref, rs_u * U * rs_ref)
    ids, rs = got["route_id"].long(), got["route_rs"].double()
    xd = x[:rows].double()
    wsel = wgu.double()[ids]  # [rows, top_k, 2 ffn, dim], rows interleaved (gate_j, up_j)
    acc = torch.einsum("bk,bjnk->bjn", xd, wsel) * rs[:, None, None]
    mag = torch.einsum("bk,bjnk->bjn", xd.abs(), wsel.abs()) * rs[:, None, None]
    g, up = acc[..., 0::2], acc[..., 1::2]
    dg, du = (dim + 4) * U * mag[..., 0::2] + V * g.abs(), (dim + 4) * U * mag[..., 1::2] + V * up.abs()
    silu = g * torch.sigmoid(g)
    f = silu * up
    df = 1.1 * dg * (up.abs() + du) + silu.abs() * du + (g.abs() + 4) * 2.0 ** -22 * f.abs()
    hold("moe_h", got["moe_h"].view(rows, top_k, ffn), f, df + V * (f.abs() + df) + 1e-30)
    h, w = got["moe_h"].double().view(rows, top_k, ffn), got["route_w"].double()
    dsel = wd.double()[ids]  # [rows, top_k, dim, ffn]
    y = torch.einsum("bjf,bjdf->bjd", h, dsel) * w[..., None]
    ymag = torch.einsum("bjf,bjdf->bjd", h.abs(), dsel.abs()) * w[..., None]
    hold("moe_part", got["moe_part"], y, (ffn + 4) * U * ymag + 1e-30)
    part = got["moe_part"].double()
    r = xd + part.sum(1)
    hold("resid", resid[:rows], r, (top_k + 2) * U * (xd.abs() + part.abs().sum(1)) + V * r.abs() + 1e-30)
    sq = resid[:rows].double().pow(2).view(rows, plan.cb_grid, plan.cb_cols).sum(-1).T
    hold("ss", ss_new[: plan.cb_grid, :rows], sq, (plan.cb_cols + 2) * U * sq + 1e-30)


def check_moe_ffn(x, ss, router, wgu, wd, rows, top_k, norm_topk, eps=1e-5):
    """Run ``ops.moe_ffn`` on poisoned outputs and hold every stage to fp64."""
    dev = torch.device("cuda")
    E, dim, ffn = router.shape[0], x.shape[1], wd.shape[2]
    rs_ref, ids_ref, w_ref, w_bound, undecided = router_reference(x, ss, router, rows, top_k, norm_topk, eps)
    assert undecided == 0, f"{undecided} rows of the inputs are undecided: choose another seed"
    full = x.clone().to(dev)  # 64 rows: those past `rows` are the guard
    # The producer's partials, then poison up to the most partials the combine may leave (4-column workgroups).
    ss_d = torch.cat([ss, torch.full((dim // 4 - ss.shape[0], 64), float("nan"))]).to(dev)
    nan = lambda *shape, dtype=torch.float32: torch.full(shape, float("nan"), dtype=dtype, device=dev)  # noqa: E731
    out = {"route_id": torch.full((rows, top_k), -7, dtype=torch.int32, device=dev), "route_w": nan(rows, top_k),
           "route_rs": nan(rows), "moe_h": nan(rows * top_k, ffn, dtype=torch.bfloat16),
           "moe_part": nan(rows, top_k, dim)}
    ops.moe_ffn(full[:rows], ss_d, router.to(dev), wgu.to(dev), wd.to(dev), top_k, norm_topk, eps, out=out,
                ss_in=ss.shape[0])
    torch.cuda.synchronize()
    hold_stages(x, rs_ref, ids_ref, w_ref, w_bound, ss.shape[0] + 8, wgu, wd, {k: t.cpu() for k, t in out.items()},
                full.cpu(), ss_d.cpu(), ops.moe_ffn_plan(rows, dim, ffn, ops.MoeDims(E, top_k, int(norm_topk))))
    assert torch.equal(full.cpu()[rows:], x[rows:]), "a row past the step's rows moved"


# (E, top_k, norm_topk, rows, input seed): the seed is 0 except where that draw leaves a row undecided at some top_k
# (a gap below 2 Lb among 128 logits); those two were chosen on the CPU from the fp64 reference alone.
CASES = [(E, k, n, rows, {(128, 40): 31676, (128, 64): 63352}.get((E, rows), 0))
         for E, k, n, rows in itertools.product((4, 8, 128), (1, 2, 8), (True, False), (1, 16, 17, 40, 64)) if k <= E]


@pytest.mark.parametrize("E,top_k,norm_topk,rows,seed", CASES)
def test_moe_ffn_against_fp64(E, top_k, norm_topk, rows, seed):
    check_moe_ffn(*make_inputs(E, rows, seed=seed), rows, top_k, norm_topk)


PLANTED = {  # name: (E, top_k, rows, the planted experts of each row or None, shape)
    "one_expert_gets_all_four_row_tiles": (8, 1, 64, {b: [5] for b in range(64)}, {}),
    "16_pairs_17_pairs_and_none": (4, 1, 64, {b: [1 if b < 16 else 2 if b < 33 else 3] for b in range(64)}, {}),
    "top2_with_one_expert_empty": (8, 2, 64, {b: [b % 6, 7] for b in range(64)}, {}),
    "wide_model_8_waves_8_column_combine": (4, 2, 8, None, {"dim": 2048, "ffn": 1024}),
}


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_moe_ffn_planted_routes_and_the_wide_shape(name):
    E, top_k, rows, plant, shape = PLANTED[name]
    x, ss, router, wgu, wd = make_inputs(E, rows, plant=plant, **shape)
    if plant:  # the reference routes as planted
        assert router_reference(x, ss, router, 64, top_k, True, 1e-5)[1].tolist() == [plant[b] for b in range(64)]
    else:
        plan = ops.moe_ffn_plan(rows, 2048, 1024, ops.MoeDims(E, top_k, 1))
        assert (plan.gu_nw, plan.dn_nw, plan.cb_cols) == (8, 8, 8)
    check_moe_ffn(x, ss, router, wgu, wd, rows, top_k, True)


# ------------------------------------------------------------------ the fused step
def moe_model(n_layers, kv_dtype="bf16", seed=3, zero_last_down=False):
    from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig, TinyLlama
    cfg = LlamaConfig(vocab=512, dim=256, n_layers=n_layers, n_heads=4, n_kv_heads=2, head_dim=64, ffn=128,
                      max_seq=64, n_experts=8, top_k=2)
    m = TinyLlama(cfg, device="cuda", max_batch=40, seed=seed, kv_dtype=kv_dtype)
    if zero_last_down:  # the last layer's experts then add exactly 0: the step leaves that layer's input in resid
        m.layers[-1]["w_down"].zero_()
    return m


def step_inputs(rows, chunk, g):
    """The first ``chunk`` rows a prefill chunk of slot 0 at positions 0.., the others one row per slot."""
    tokens = torch.randint(0, 512, (rows,), generator=g)
    pos = torch.tensor(list(range(chunk)) + [int(p) for p in torch.randint(0, 8, (rows - chunk,), generator=g)],
                       dtype=torch.int32)
    slots = torch.tensor([0] * chunk + list(range(1, rows - chunk + 1)), dtype=torch.int32)
    return tokens.cuda(), pos.cuda(), slots.cuda()


@pytest.mark.parametrize("n_layers,kv_dtype", [(1, "bf16"), (1, "fp8"), (2, "bf16"), (2, "fp8")])
@pytest.mark.parametrize("rows", [1, 17, 40])
def test_fused_step_stages_against_fp64_and_graph_replay(n_layers, kv_dtype, rows):
    """The last layer's MoE buffers of a real step (the attention kernels' residual and partials, a second layer, an
    FP8 cache) held to the bounds above. The rows that layer read are what a twin model whose last down projection
    is zero leaves in resid, bit for bit: bf16(x + 0) = x, and every kernel before it is the same. The buffers the
    unchanged kernels write (q, attn, part_o, ...) are test_gpu_fused_stages.py's. Then graph replay == eager.
    Model seed 3, except where its last layer's input has an undecided row (asserted below, on the reference)."""
    seed = 4 if (n_layers, kv_dtype, rows) == (2, "fp8", 40) else 3
    m, twin = moe_model(n_layers, kv_dtype, seed), moe_model(n_layers, kv_dtype, seed, zero_last_down=True)
    tokens, pos, slots = step_inputs(rows, min(rows, 5), torch.Generator().manual_seed(rows))
    twin.step_rows(tokens, pos, slots)
    x = twin.fused_decoder().workspace_views()["resid"].cpu()
    ids, logits = m.step_rows(tokens, pos, slots)
    dec = m.fused_decoder()
    views = {k: v.clone() for k, v in dec.workspace_views().items()}
    torch.cuda.synchronize()
    c = m.cfg
    router, wgu, wd = (dec.weights[dec.table.index(n, n_layers - 1)].cpu() for n in ("router", "w_gate_up", "w_down"))
    parts = ops.step_plan(dec.dims, rows).gate_up.ss_in  # the O projection's partials, fp32 sums of <= 16 squares:
    ss_exact = x.double().pow(2).sum(1)[None, :].float().double()  # 18 u more than the op's exact partials
    rs_ref, ids_ref, w_ref, w_bound, undecided = router_reference(x, ss_exact, router, rows, c.top_k, True, c.eps,
                                                                  ss_u=parts + 34)
    assert undecided == 0, f"{undecided} undecided rows: choose another model seed"
    got = {k: views[k][: rows * (c.top_k if k == "moe_h" else 1)].cpu()
           for k in ("route_id", "route_w", "route_rs", "moe_h", "moe_part")}
    hold_stages(x, rs_ref, ids_ref, w_ref, w_bound, parts + 26, wgu, wd, got, views["resid"].cpu(),
                views["ss"].cpu(), ops.moe_plan(dec.dims, c.moe, rows))
    m.capture_graph(rows)
    for _ in range(3):  # several replays against the eager result
        g_ids, g_logits = m.graph_step(tokens, pos, slots, return_logits=True)
        torch.cuda.synchronize()
        assert torch.equal(g_ids, ids) and torch.equal(g_logits, logits)
        after = dec.workspace_views()
        for name, v in got.items():
            assert torch.equal(after[name][: len(v)].cpu(), v), name
        assert torch.equal(after["resid"][:rows], views["resid"][:rows])


def test_permuting_the_rows_permutes_the_residual_bit_for_bit():
    m, g = moe_model(1), torch.Generator().manual_seed(5)
    tokens, pos, slots = step_inputs(40, 0, g)
    m.step_rows(tokens, pos, slots)
    first = m.fused_decoder().workspace_views()["resid"][:40].clone()
    perm = torch.randperm(40, generator=g).cuda()
    m.step_rows(tokens[perm], pos[perm], slots[perm])
    torch.cuda.synchronize()
    assert torch.equal(m.fused_decoder().workspace_views()["resid"][:40], first[perm])


def test_a_dense_step_through_the_moe_entry_point_is_the_old_one():
    """``p2pt_llama_decode_moe`` with moe = nullptr against ``p2pt_llama_decode_chunk``: logits, ids, the K cache and
    every workspace byte."""
    from p2p_llm_tunnel_amd.models.tiny_llm import TinyLlama
    m = TinyLlama("micro", device="cuda", max_batch=20)
    dec = m.fused_decoder()
    tokens, pos, slots = step_inputs(17, 4, torch.Generator().manual_seed(2))
    results = []
    for fn, extra in ((ops.lib().p2pt_llama_decode_chunk, []), (ops.lib().p2pt_llama_decode_moe, [None])):
        dec.ws.zero_(), m.k_cache.zero_(), m.v_cache.zero_()
        logits = torch.empty(17, m.cfg.vocab, dtype=torch.bfloat16, device="cuda")
        ids = torch.empty(17, dtype=torch.int64, device="cuda")
        assert fn(ctypes.byref(dec.dims), ctypes.byref(dec.weight_format), None, None, dec._wptr, ops._p(m.k_cache),
                  ops._p(m.v_cache), ops._p(tokens), ops._p(pos), ops._p(slots), 17, 0, ops._p(dec.ws), dec.ws.numel(),
                  ops._p(logits), ops._p(ids), ops._stream(tokens), 0, *extra) == 0
        torch.cuda.synchronize()
        results.append((logits, ids, dec.ws.clone(), m.k_cache.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*results))


def test_engine_serves_tiny_moe_with_the_reference_greedy_tokens():
    """``tiny-moe`` through ``Engine`` (12 graphs as for a dense model): requests alone and sharing steps both give
    the fp32 reference's greedy tokens, on prompts whose margins test_moe.py re-checks on the CPU."""
    from test_moe import CONFIDENT
    from p2p_llm_tunnel_amd.models.engine import Engine, Request
    eng = Engine(device="cuda:0", config="tiny-moe", max_batch=4, seed=0)
    try:
        assert len(eng._graphs) == 12
        want = [ref for _, ref in CONFIDENT]
        alone = [list(iter(eng.submit(Request(list(p), len(ref))).out.get, None)) for p, ref in CONFIDENT]
        reqs = [eng.submit(Request(list(p), len(ref))) for p, ref in CONFIDENT]
        assert alone == want and [list(iter(r.out.get, None)) for r in reqs] == want
    finally:
        eng.stop()


def test_endpoint_serves_a_synthetic_mixtral_checkpoint(tmp_path):
    import http.client
    import json
    from test_moe import mixtral_checkpoint
    from p2p_llm_tunnel_amd.models.server import start_server, weights_line
    mixtral_checkpoint(str(tmp_path), tie=False)
    srv, port, eng = start_server(port=0, device="cuda:0", max_batch=2, checkpoint=str(tmp_path), max_seq=128)
    try:
        c = eng.model.cfg
        assert eng.use_graph and len(eng._graphs) == 12 and (c.n_experts, c.top_k) == (4, 2)
        assert "MoE: 4 experts, top-2" in weights_line(eng.model, "bf16")
        conn = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        conn.request("POST", "/v1/chat/completions", body=json.dumps(
            {"max_tokens": 5, "messages": [{"role": "user", "content": "hi"}]}))
        r = conn.getresponse()
        body = json.loads(r.read())
        assert r.status == 200 and body["choices"][0]["finish_reason"] == "length"
        assert body["usage"]["completion_tokens"] == 5
    finally:
        srv.shutdown()
        eng.stop()
