"""``p2pt_llama_step`` against each entry point from before ``StepOptions`` that tests and scripts still call, on the
GPU: the same step through both must leave the same logits, ids, workspace and caches, bit for bit. 17 rows with a
4-row prefill chunk among them: two row tiles, so chunk attention runs where it is on and the 16 / 17 tile edge is
crossed; emit_rows = 0 is every row. The options whose own entry point is gone (KV scales, FP8 and MXFP4 experts, LoRA)
reach the step through ``FusedLlamaDecoder.step`` alone, and test_gpu_kv_scale.py, test_gpu_moe_fp8.py,
test_gpu_moe_mxfp4.py and test_gpu_lora.py hold them.
"""
import ctypes

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from test_gpu_moe import step_inputs

pytestmark = pytest.mark.gpu
ROWS = 17

# name -> (model config, its keywords, the options beside the model's own, the old entry point, its arguments between
# dims and the weight table as a function of the decoder, its arguments after the stream)
CASES = {
    "bf16": ("micro", {}, {}, "p2pt_llama_decode", lambda dec, w: [], []),
    "fp8": ("micro", {"weight_dtype": "fp8"}, {}, "p2pt_llama_decode_w", lambda dec, w: [ops.WeightPlan(w8=1)], []),
    "windows": ("micro", {}, {"windows": (0, 3)}, "p2pt_llama_decode_win",
                lambda dec, w: [ops.WeightPlan(w8=0), None, w], []),
    "mxfp4": ("micro", {"weight_dtype": "mxfp4"}, {}, "p2pt_llama_decode_fmt",
              lambda dec, w: [dec.weight_format, None, None], []),
    "chunk": ("micro", {}, {"chunk_attn": True}, "p2pt_llama_decode_chunk",
              lambda dec, w: [dec.weight_format, None, None], [1]),
    "moe": ("tiny-moe", {}, {}, "p2pt_llama_decode_moe", lambda dec, w: [dec.weight_format, None, None],
            lambda dec: [0, dec.moe]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_step_through_the_options_is_the_old_entry_point_bit_for_bit(case):
    from p2p_llm_tunnel_amd.models.tiny_llm import TinyLlama
    config, keywords, beside, name, head, tail = CASES[case]
    m = TinyLlama(config, device="cuda", max_batch=20, **keywords)
    dec = m.fused_decoder()
    windows = beside.get("windows")
    opts = ops.step_options(dec.weight_format, None, windows, beside.get("chunk_attn", False), dec.moe)
    # Neither windows nor chunk attention changes the workspace: the decoder's own serves both calls.
    assert ops.workspace_layout(dec.dims, opts)[0] == dec.ws.numel()
    assert (dec.weight_format.layers, dec.moe is not None) == {"fp8": (1, False), "mxfp4": (2, False),
                                                               "moe": (0, True)}.get(case, (0, False))
    tokens, pos, slots = step_inputs(ROWS, 4, torch.Generator().manual_seed(2))
    warr = (ctypes.c_int * len(windows))(*windows) if windows else None
    old = [ctypes.byref(dec.dims), *head(dec, warr)], (tail(dec) if callable(tail) else tail)
    new = [ctypes.byref(dec.dims), ctypes.byref(opts)], [None]  # no adapters
    results = []
    for fn, (first, last) in ((getattr(ops.lib(), name), old), (ops.lib().p2pt_llama_step, new)):
        dec.ws.zero_(), m.k_cache.zero_(), m.v_cache.zero_()
        logits = torch.empty(ROWS, m.cfg.vocab, dtype=torch.bfloat16, device="cuda")
        ids = torch.empty(ROWS, dtype=torch.int64, device="cuda")
        assert fn(*first, dec._wptr, ops._p(m.k_cache), ops._p(m.v_cache), ops._p(tokens), ops._p(pos), ops._p(slots),
                  ROWS, 0, ops._p(dec.ws), dec.ws.numel(), ops._p(logits), ops._p(ids), ops._stream(tokens), *last) == 0
        torch.cuda.synchronize()
        results.append((logits, ids, dec.ws.clone(), m.k_cache.clone(), m.v_cache.clone()))
    for what, a, b in zip(("logits", "ids", "workspace", "k_cache", "v_cache"), *results):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), what
    assert bool(results[0][3].view(torch.uint8).any()) and bool(results[0][1].ge(0).all())  # the step did run
