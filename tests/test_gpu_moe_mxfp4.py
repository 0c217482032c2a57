"""MXFP4 expert weights on the GPU (docs/MOE_MXFP4.md), against the bf16 kernels bit for bit where the K split is theirs
and against fp64 where it differs.

Bit-exactness: every MXFP4 value e2m1 * 2^(E - 127) with E in the quantiser's range is a bf16 number, so the dequantised
experts are exact bf16 weights, and the kernel has no scale of its own. Where NW divides K / 128 a wave's quads of
k-steps are the bf16 kernel's k-steps and its MFMAs come in the same order on the same operands: every buffer is equal.

fp64: the stage bounds of test_gpu_moe.py from the dequantised weights in fp64, unwidened: there is no extra rounding.
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
from test_moe_mxfp4 import confident_prompts

pytestmark = pytest.mark.gpu
EXACT = [(E, k, rows, None, 512, 512) for (E, k), rows in itertools.product(((4, 1), (8, 2)), (1, 17, 40, 64))] + \
    [(*PLANTED[n][:4], 512, 512) for n in sorted(PLANTED) if PLANTED[n][3]] + [(8, 2, 17, None, 1024, 1024)]
SPLIT = [(4, 2, 17, None, 256, 128), (8, 2, 40, None, 384, 640)]  # idle waves; 3 quads on 4 waves, 5 on 8


def mxfp4_experts(w, g, plant=True):
    """A stack ``[E, N, K]`` through the quantiser: nibble bytes, e8m0 bytes and the dequantised stack in fp32.
    ``plant``: block exponents 2^-12 .. 2^4 that differ per block, and all 16 nibble codes in every row's first 8 bytes."""
    q, ex = (torch.stack(t) for t in zip(*(ops.quantize_weight_mxfp4(e.float()) for e in w)))
    if plant:
        ex = (127 + torch.randint(-12, 5, ex.shape, generator=g)).to(torch.uint8)
        q[..., :8] = torch.tensor([0x10 * (2 * i + 1) + 2 * i for i in range(8)], dtype=torch.uint8)
    return q, ex, torch.stack([ops.dequantize_weight_mxfp4(a, b) for a, b in zip(q, ex)])


@pytest.mark.parametrize("E,top_k,rows,plant,dim,ffn", EXACT + SPLIT)
def test_moe_ffn_with_mxfp4_experts(E, top_k, rows, plant, dim, ffn):
    x, ss, router, wgu, wd = make_inputs(E, rows, dim=dim, ffn=ffn, plant=plant)
    plan, exact = ops.moe_ffn_plan(rows, dim, ffn, ops.MoeDims(E, top_k, 1)), (E, top_k, rows, plant, dim, ffn) in EXACT
    assert ((dim // 128) % plan.gu_nw == 0 and (ffn // 128) % plan.dn_nw == 0) == exact
    assert (plan.gu_nw, plan.dn_nw) == {512: (4, 4), 1024: (8, 8), 256: (4, 4), 384: (4, 8)}[dim]
    g = torch.Generator().manual_seed(rows)
    (qgu, egu, dgu), (qd, ed, dd) = mxfp4_experts(wgu, g, exact), mxfp4_experts(wd, g, exact)
    assert not exact or len({int(c) for b in qgu[0, 0, :8] for c in (b & 15, b >> 4)}) == 16
    assert torch.equal(dgu.bfloat16().float(), dgu) and torch.equal(dd.bfloat16().float(), dd)
    rs_ref, ids_ref, w_ref, w_bound, undecided = router_reference(x, ss, router, rows, top_k, True, 1e-5)
    assert undecided == 0
    dev, runs = torch.device("cuda"), []
    for mxfp4 in (True, False) if exact else (True,):
        full = x.clone().to(dev)
        ss_d = torch.cat([ss, torch.full((dim // 4 - ss.shape[0], 64), float("nan"))]).to(dev)
        nan = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), dtype=dtype, device=dev)  # noqa: E731
        out = {"route_id": torch.full((rows, top_k), -7, dtype=torch.int32, device=dev), "route_w": nan(rows, top_k),
               "route_rs": nan(rows), "moe_h": nan(rows * top_k, ffn, dtype=torch.bfloat16),
               "moe_part": nan(rows, top_k, dim)}
        if mxfp4:
            ops.moe_ffn(full[:rows], ss_d, router.to(dev), ops.block_expert_mxfp4(qgu).to(dev),
                        ops.block_expert_mxfp4(qd).to(dev), top_k, True, out=out, ss_in=ss.shape[0],
                        gate_up_exp=egu.to(dev), down_exp=ed.to(dev))
        else:
            ops.moe_ffn(full[:rows], ss_d, router.to(dev), dgu.bfloat16().to(dev), dd.bfloat16().to(dev), top_k, True,
                        out=out, ss_in=ss.shape[0])
        torch.cuda.synchronize()
        runs.append({**{k: t.cpu() for k, t in out.items()}, "resid": full.cpu(), "ss": ss_d.cpu()[: plan.cb_grid, :rows]})
    got = runs[0]
    hold_stages(x, rs_ref, ids_ref, w_ref, w_bound, ss.shape[0] + 8, dgu.double(), dd.double(), got, got["resid"],
                torch.cat([got["ss"], torch.zeros(plan.cb_grid, 64 - rows)], 1), plan)
    assert torch.equal(got["resid"][rows:], x[rows:]), "a row past the step's rows moved"
    for name in got if exact else ():
        assert torch.equal(got[name], runs[1][name]), name


@pytest.mark.parametrize("n_layers,kv_dtype", [(1, "bf16"), (1, "fp8"), (2, "bf16"), (2, "fp8")])
@pytest.mark.parametrize("rows", [1, 17, 40])
def test_the_fused_step_with_mxfp4_experts_is_the_bf16_step_bit_for_bit(n_layers, kv_dtype, rows):
    cfg = LlamaConfig(vocab=512, dim=512, n_layers=n_layers, n_heads=8, n_kv_heads=2, head_dim=64, ffn=512, max_seq=64,
                      n_experts=8, top_k=2)
    base, g = TinyLlama(cfg, device="cpu", max_batch=1, seed=3), torch.Generator().manual_seed(7)
    back = torch.argsort(fused_row_perm(cfg, "w_gate_up", "cpu"))  # the fused table's row order -> the plain one
    mx_layers, bf16_layers = [], []
    for L in base.layers:  # an FFN norm of one, so that the fold is exact and both tables hold the same weights
        (qgu, egu, dgu), (qd, ed, dd) = mxfp4_experts(L["w_gate_up"], g), mxfp4_experts(L["w_down"], g)
        L = {k: t.cuda() for k, t in L.items() if k not in ("w_gate_up", "w_down")} | {"ffn_norm": torch.ones(512).bfloat16().cuda()}
        mx_layers.append(L | {"w_gate_up_q": qgu.cuda(), "w_gate_up_e": egu.cuda(), "w_down_q": qd.cuda(), "w_down_e": ed.cuda()})
        bf16_layers.append(L | {"w_gate_up": dgu[:, back].bfloat16().contiguous().cuda(), "w_down": dd.bfloat16().cuda()})
    top = {k: getattr(base, k).cuda() for k in ("embed", "final_norm", "lm_head")}
    tokens, pos, slots = step_inputs(rows, min(rows, 5), torch.Generator().manual_seed(rows))
    results = []
    for layers, fmt in ((mx_layers, "mxfp4"), (bf16_layers, "bf16")):
        m = TinyLlama(cfg, device="cuda", max_batch=40, weights={**top, "layers": layers}, kv_dtype=kv_dtype, expert_dtype=fmt)
        ids, logits = m.step_rows(tokens, pos, slots)
        torch.cuda.synchronize()
        results.append((ids, logits, m.k_cache.view(torch.uint8), m.v_cache.view(torch.uint8), m.fused_decoder().ws.clone()))
    assert m.fused_decoder().workspace_views()["moe_part"][:rows].abs().sum() > 0
    for name, a, b in zip(("ids", "logits", "k_cache", "v_cache", "workspace"), *results):
        assert torch.equal(a, b), name
    m = TinyLlama(cfg, device="cuda", max_batch=40, weights={**top, "layers": mx_layers}, kv_dtype=kv_dtype, expert_dtype="mxfp4")
    m.capture_graph(rows)
    for _ in range(3):  # several replays against the eager result
        g_ids, g_logits = m.graph_step(tokens, pos, slots, return_logits=True)
        torch.cuda.synchronize()
        assert torch.equal(g_ids, results[0][0]) and torch.equal(g_logits, results[0][1])
        assert torch.equal(m.fused_decoder().ws, results[0][4])


def test_engine_serves_tiny_moe_with_mxfp4_experts_and_the_reference_greedy_tokens():
    from p2p_llm_tunnel_amd.models.engine import Engine, Request
    prompts = confident_prompts()  # on the CPU, before anything runs on the GPU
    assert len(prompts) >= 4
    eng = Engine(device="cuda:0", config="tiny-moe", max_batch=4, seed=0, expert_dtype="mxfp4")
    try:
        assert len(eng._graphs) == 12 and eng.model.expert_dtype == "mxfp4"
        want = [ref for _, ref in prompts]
        alone = [list(iter(eng.submit(Request(list(p), len(ref))).out.get, None)) for p, ref in prompts]
        reqs = [eng.submit(Request(list(p), len(ref))) for p, ref in prompts[:4]]
        assert alone == want and [list(iter(r.out.get, None)) for r in reqs] == want[:4]
    finally:
        eng.stop()


@pytest.mark.parametrize("gpus", [0, 1])
def test_endpoint_serves_a_synthetic_mixtral_checkpoint_with_mxfp4_experts(tmp_path, monkeypatch, gpus):
    import http.client
    from p2p_llm_tunnel_amd.models.server import start_server, weights_line
    from p2p_llm_tunnel_amd.utils.procs import free_port
    mixtral_checkpoint(str(tmp_path), tie=False)  # test_moe.py's checkpoint: a per-expert size of 96 does not block
    with pytest.raises(ValueError, match="multiples of 128, got dim 128, ffn 96"):
        start_server(port=0, device="cuda:0", max_batch=2, checkpoint=str(tmp_path), max_seq=128, expert_dtype="mxfp4")
    monkeypatch.setitem(MIXTRAL, "intermediate_size", 256)  # and at one that does
    mixtral_checkpoint(str(tmp_path), tie=False)
    if gpus:  # the switch through --gpus 1: a parent that starts one replica, which prints its start-up lines
        port = free_port()
        proc = subprocess.Popen([sys.executable, "-m", "p2p_llm_tunnel_amd.models.server", "--gpus", "1", "--port", str(port),
                                 "--checkpoint", str(tmp_path), "--max-seq", "128", "--max-batch", "2", "--expert-dtype",
                                 "mxfp4"], stdout=subprocess.PIPE, text=True)
        lines = list(iter(lambda: (lambda l: l if l and "inference endpoint on" not in l else "")(proc.stdout.readline()), ""))
        stop = lambda: (proc.send_signal(signal.SIGINT), proc.wait(60))  # noqa: E731
    else:
        srv, port, eng = start_server(port=0, device="cuda:0", max_batch=2, checkpoint=str(tmp_path), max_seq=128,
                                      expert_dtype="mxfp4")
        lines = [weights_line(eng.model, "bf16")]
        stop = lambda: (srv.shutdown(), eng.stop())  # noqa: E731
    try:
        assert any("mxfp4 experts" in l and "MoE: 4 experts, top-2" in l for l in lines), lines
        conn = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        conn.request("POST", "/v1/chat/completions", body=json.dumps(
            {"max_tokens": 5, "messages": [{"role": "user", "content": "hi"}]}))
        r = conn.getresponse()
        body = json.loads(r.read())
        assert r.status == 200 and body["usage"]["completion_tokens"] == 5
    finally:
        stop()
