"""FP8 expert weights on the GPU (docs/MOE_FP8.md), against the bf16 kernels bit for bit where the K split is theirs and
against fp64 everywhere.

Bit-exactness: planted e4m3 bytes below 0.5 with power-of-two row scales 2^-3 .. 2^2 decode to exact bf16 weights
w = q s. Where NW divides K / 64, a wave's pairs of k-steps are the bf16 kernel's k-steps and its MFMAs come in the
same order, so its fp32 sum is the bf16 kernel's divided by s exactly (a power of two commutes with every rounding; no
value here comes near fp32's subnormals), and (v s) rs = (v s) rs, rw (v s) likewise: every buffer must be equal.

fp64: the stage bounds of test_gpu_moe.py, from the weights q s in fp64 and the inputs each kernel read. The FP8 kernels
add one fp32 rounding, of v s: u |acc| <= u sum|x w| more in moe_h and moe_part, i.e. (K + 5) u where those bounds say
(K + 4) u. ``hold_stages`` is used as it is, so the test holds the kernels to the tighter, unwidened bound.
"""
import itertools
import json
import signal
import subprocess
import sys

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig, TinyLlama, fused_row_perm
from test_gpu_moe import PLANTED, hold_stages, make_inputs, router_reference, step_inputs
from test_moe import MIXTRAL, mixtral_checkpoint
from test_moe_fp8 import FP8_CONFIDENT

pytestmark = pytest.mark.gpu
EXACT = [(E, k, rows, None, 256, 256) for E, k, rows in itertools.product((4, 8), (1, 2), (1, 16, 17, 40, 64))] + \
    [(*PLANTED[n][:4], 256, 256) for n in sorted(PLANTED) if PLANTED[n][3]]
SPLIT = [(4, 2, 17, None, 256, 128), (8, 2, 40, None, 256, 192), (4, 2, 8, None, 2048, 1024)]


def planted_experts(shape, g):
    """Random e4m3 bytes of magnitude below 0.5 (no NaN byte), power-of-two row scales, and their exact bf16 product."""
    q = (torch.randint(0, 0x30, shape, generator=g) | (torch.randint(0, 2, shape, generator=g) << 7)).to(torch.uint8)
    s = torch.exp2(torch.randint(-3, 3, shape[:2], generator=g).float())
    return q, s, (q.view(torch.float8_e4m3fn).float() * s[..., None]).to(torch.bfloat16)


@pytest.mark.parametrize("E,top_k,rows,plant,dim,ffn", EXACT + SPLIT)
def test_moe_ffn_with_fp8_experts(E, top_k, rows, plant, dim, ffn):
    x, ss, router, wgu, wd = make_inputs(E, rows, dim=dim, ffn=ffn, plant=plant)
    plan, exact = ops.moe_ffn_plan(rows, dim, ffn, ops.MoeDims(E, top_k, 1)), (E, top_k, rows, plant, dim, ffn) in EXACT
    divides = (dim // 64) % plan.gu_nw == 0 and (ffn // 64) % plan.dn_nw == 0
    assert divides == (exact or dim == 2048)  # the wide case runs the quantiser's scales: fp64 alone
    assert (plan.gu_nw, plan.dn_nw) == ((8, 8) if dim == 2048 else (4, 4))
    if exact:  # planted bytes; else the quantiser's own bytes and scales
        g = torch.Generator().manual_seed(rows)
        (qgu, sgu, wgu), (qd, sd, wd) = planted_experts(wgu.shape, g), planted_experts(wd.shape, g)
    else:
        (qgu, sgu), (qd, sd) = ([torch.stack(t) for t in zip(*(ops.quantize_weight_fp8(w.float()) for w in stack))]
                                for stack in (wgu, wd))
    rs_ref, ids_ref, w_ref, w_bound, undecided = router_reference(x, ss, router, rows, top_k, True, 1e-5)
    assert undecided == 0
    dev, runs = torch.device("cuda"), []
    for fp8 in (True, False) if exact else (True,):
        full = x.clone().to(dev)
        ss_d = torch.cat([ss, torch.full((dim // 4 - ss.shape[0], 64), float("nan"))]).to(dev)
        nan = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), dtype=dtype, device=dev)  # noqa: E731
        out = {"route_id": torch.full((rows, top_k), -7, dtype=torch.int32, device=dev), "route_w": nan(rows, top_k),
               "route_rs": nan(rows), "moe_h": nan(rows * top_k, ffn, dtype=torch.bfloat16),
               "moe_part": nan(rows, top_k, dim)}
        if fp8:
            ops.moe_ffn(full[:rows], ss_d, router.to(dev), ops.block_expert_fp8(qgu).to(dev),
                        ops.block_expert_fp8(qd).to(dev), top_k, True, out=out, ss_in=ss.shape[0],
                        gate_up_scale=sgu.to(dev), down_scale=sd.to(dev))
        else:
            ops.moe_ffn(full[:rows], ss_d, router.to(dev), wgu.to(dev), wd.to(dev), top_k, True, out=out,
                        ss_in=ss.shape[0])
        torch.cuda.synchronize()
        runs.append({**{k: t.cpu() for k, t in out.items()}, "resid": full.cpu(), "ss": ss_d.cpu()[: plan.cb_grid, :rows]})
    got = runs[0]
    deq = lambda q, s: q.view(torch.float8_e4m3fn).double() * s.double()[..., None]  # noqa: E731
    hold_stages(x, rs_ref, ids_ref, w_ref, w_bound, ss.shape[0] + 8, deq(qgu, sgu), deq(qd, sd), got, got["resid"],
                torch.cat([got["ss"], torch.zeros(plan.cb_grid, 64 - rows)], 1), plan)
    assert torch.equal(got["resid"][rows:], x[rows:]), "a row past the step's rows moved"
    for name in got if exact else ():
        assert torch.equal(got[name], runs[1][name]), name


@pytest.mark.parametrize("n_layers,kv_dtype", [(1, "bf16"), (1, "fp8"), (2, "bf16"), (2, "fp8")])
@pytest.mark.parametrize("rows", [1, 17, 40])
def test_the_fused_step_with_fp8_experts_is_the_bf16_step_bit_for_bit(n_layers, kv_dtype, rows):
    cfg = LlamaConfig(vocab=512, dim=256, n_layers=n_layers, n_heads=4, n_kv_heads=2, head_dim=64, ffn=256, max_seq=64,
                      n_experts=8, top_k=2)
    base, g = TinyLlama(cfg, device="cpu", max_batch=1, seed=3), torch.Generator().manual_seed(7)
    back = torch.argsort(fused_row_perm(cfg, "w_gate_up", "cpu"))  # the fused table's row order -> the plain one
    fp8_layers, bf16_layers = [], []
    for L in base.layers:  # an FFN norm of one, so that the fold is exact and both tables hold the same weights
        L = {k: t.cuda() for k, t in L.items() if k not in ("w_gate_up", "w_down")} | {"ffn_norm": torch.ones(256).bfloat16().cuda()}
        (qgu, sgu, wgu), (qd, sd, wd) = planted_experts((8, 512, 256), g), planted_experts((8, 256, 256), g)
        fp8_layers.append(L | {"w_gate_up_q": qgu.cuda(), "w_gate_up_s": sgu.cuda(), "w_down_q": qd.cuda(), "w_down_s": sd.cuda()})
        bf16_layers.append(L | {"w_gate_up": wgu[:, back].contiguous().cuda(), "w_down": wd.cuda()})
    top = {k: getattr(base, k).cuda() for k in ("embed", "final_norm", "lm_head")}
    tokens, pos, slots = step_inputs(rows, min(rows, 5), torch.Generator().manual_seed(rows))
    results = []
    for layers, fmt in ((fp8_layers, "fp8"), (bf16_layers, "bf16")):
        m = TinyLlama(cfg, device="cuda", max_batch=40, weights={**top, "layers": layers}, kv_dtype=kv_dtype, expert_dtype=fmt)
        ids, logits = m.step_rows(tokens, pos, slots)
        torch.cuda.synchronize()
        results.append((ids, logits, m.k_cache.view(torch.uint8), m.v_cache.view(torch.uint8), m.fused_decoder().ws.clone()))
    assert m.fused_decoder().workspace_views()["moe_part"][:rows].abs().sum() > 0
    for name, a, b in zip(("ids", "logits", "k_cache", "v_cache", "workspace"), *results):
        assert torch.equal(a, b), name
    m = TinyLlama(cfg, device="cuda", max_batch=40, weights={**top, "layers": fp8_layers}, kv_dtype=kv_dtype, expert_dtype="fp8")
    m.capture_graph(rows)
    for _ in range(3):  # several replays against the eager result
        g_ids, g_logits = m.graph_step(tokens, pos, slots, return_logits=True)
        torch.cuda.synchronize()
        assert torch.equal(g_ids, results[0][0]) and torch.equal(g_logits, results[0][1])
        assert torch.equal(m.fused_decoder().ws, results[0][4])


def test_engine_serves_tiny_moe_with_fp8_experts_and_the_reference_greedy_tokens():
    from p2p_llm_tunnel_amd.models.engine import Engine, Request
    eng = Engine(device="cuda:0", config="tiny-moe", max_batch=4, seed=0, expert_dtype="fp8")
    try:
        assert len(eng._graphs) == 12 and eng.model.expert_dtype == "fp8"
        want = [ref for _, ref in FP8_CONFIDENT]
        alone = [list(iter(eng.submit(Request(list(p), len(ref))).out.get, None)) for p, ref in FP8_CONFIDENT]
        reqs = [eng.submit(Request(list(p), len(ref))) for p, ref in FP8_CONFIDENT]
        assert alone == want and [list(iter(r.out.get, None)) for r in reqs] == want
    finally:
        eng.stop()


@pytest.mark.parametrize("gpus", [0, 1])
def test_endpoint_serves_a_synthetic_mixtral_checkpoint_with_fp8_experts(tmp_path, monkeypatch, gpus):
    import http.client
    from p2p_llm_tunnel_amd.models.server import start_server, weights_line
    from p2p_llm_tunnel_amd.utils.procs import free_port
    monkeypatch.setitem(MIXTRAL, "intermediate_size", 128)  # test_moe.py's checkpoint at an expert size that blocks
    mixtral_checkpoint(str(tmp_path), tie=False)
    if gpus:  # the switch through --gpus 1: a parent that starts one replica, which prints its start-up lines
        port = free_port()
        proc = subprocess.Popen([sys.executable, "-m", "p2p_llm_tunnel_amd.models.server", "--gpus", "1", "--port", str(port),
                                 "--checkpoint", str(tmp_path), "--max-seq", "128", "--max-batch", "2", "--expert-dtype",
                                 "fp8"], stdout=subprocess.PIPE, text=True)
        lines = list(iter(lambda: (lambda l: l if l and "inference endpoint on" not in l else "")(proc.stdout.readline()), ""))
        stop = lambda: (proc.send_signal(signal.SIGINT), proc.wait(60))  # noqa: E731
    else:
        srv, port, eng = start_server(port=0, device="cuda:0", max_batch=2, checkpoint=str(tmp_path), max_seq=128,
                                      expert_dtype="fp8")
        lines = [weights_line(eng.model, "bf16")]
        stop = lambda: (srv.shutdown(), eng.stop())  # noqa: E731
    try:
        assert any("fp8 experts" in l and "MoE: 4 experts, top-2" in l for l in lines), lines
        conn = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        conn.request("POST", "/v1/chat/completions", body=json.dumps(
            {"max_tokens": 5, "messages": [{"role": "user", "content": "hi"}]}))
        r = conn.getresponse()
        body = json.loads(r.read())
        assert r.status == 200 and body["usage"]["completion_tokens"] == 5
    finally:
        stop()
