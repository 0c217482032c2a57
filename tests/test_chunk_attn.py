"""Chunk attention without a GPU (docs/CHUNK_ATTN.md): the plan, the kernel table, the refusals and the default path."""
import ctypes

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models import server
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, TinyLlama, llama_dims


def dims_of(D, G, max_seq=4096, Hkv=2, kv8=0):
    return ops.LlamaDims(vocab=512, dim=256, n_layers=2, H=Hkv * G, Hkv=Hkv, D=D, ffn=256, max_seq=max_seq,
                         max_batch=6, eps=1e-5, theta=1e4, kv_fp8=kv8)


@pytest.mark.parametrize("B", (1, 16, 17, 33, 64))
@pytest.mark.parametrize("max_seq,Hkv", ((512, 2), (4096, 4), (32768, 8), (100, 1)))
def test_chunk_plan_follows_the_span_rules(B, max_seq, Hkv):
    d = dims_of(128, 4, max_seq, Hkv)
    p, tiles = ops.chunk_plan(d, B), (B + 15) // 16
    assert (p.D, p.G, p.tiles, p.grid_y, p.waves) == (128, 4, tiles, tiles * Hkv, 4)
    # attn_slots on the tile count in place of the row count, and k_attn's stride: the library's own, for `tiles` rows
    assert (p.slots, p.stride) == (ops.step_plan(d, tiles).attn.slots, ops.step_plan(d, B).attn.stride)
    # every span of the longest row is a whole number of 32-token pieces, at least 64 tokens, and fits the slots
    span = ops.attn_span(max_seq, p.slots)
    assert span % 32 == 0 and span >= 64 and -(-max_seq // span) <= p.slots <= p.stride
    assert p.grid_y <= ops.MAX_ROWS * d.H  # the tickets fit the workspace's counters


@pytest.mark.parametrize("kv8", (0, 1))
@pytest.mark.parametrize("G", (1, 2, 4, 5, 6, 7, 8))
@pytest.mark.parametrize("D", (64, 128))
def test_every_table_entry_has_its_chunk_kernel(D, G, kv8):
    d = dims_of(D, G, kv8=kv8)
    assert ops.chunk_plan(d, 64).waves == (4 if G <= 4 else 8)
    for B in (16, 17, 64):
        assert ops.plan_kernels_ok(d, B, chunk_attn=True)
        assert ops.plan_kernels_ok(d, B, chunk_attn=True, windows=(0, 128), weight_format="mxfp4")
    with pytest.raises(ValueError):
        ops.plan_kernels_ok(dims_of(D, 3), 64, chunk_attn=True)  # no G = 3 in the table, with or without the flag


def test_the_flag_is_no_part_of_a_plan():
    # step_plan and the workspace take no flag: there is no second plan to compare, and today's bytes are pinned by the
    # earlier families' plan and ws_layout tests. This only checks that planning the chunk kernel leaves no state behind.
    d = llama_dims(CONFIGS["small"], 9, False)
    before = [bytes(ops.step_plan(d, B)) for B in (16, 64)], ops.lib().p2pt_llama_ws_bytes(ctypes.byref(d))
    assert ops.chunk_plan(d, 64).tiles == 4 and ops.plan_kernels_ok(d, 64, chunk_attn=True)
    assert ([bytes(ops.step_plan(d, B)) for B in (16, 64)], ops.lib().p2pt_llama_ws_bytes(ctypes.byref(d))) == before
    with pytest.raises(TypeError, match="chunk_attn must be a bool"):
        ops.FusedLlamaDecoder(d, [], torch.empty(0), torch.empty(0), chunk_attn=1)


def test_the_eager_engine_and_the_unfused_path_refuse_the_flag():
    m = TinyLlama("micro", device="cpu", max_batch=2, chunk_attn=True)
    with pytest.raises(ValueError, match="chunk_attn needs the graph-captured HIP step"):
        server.Engine(model=m)
    plain = TinyLlama("micro", device="cpu", max_batch=2)
    with pytest.raises(ValueError, match="injected model was built without it"):
        server.Engine(model=plain, chunk_attn=True)
    with pytest.raises(ValueError, match="injected engine was built without it"):
        server.start_server(chunk_attn=True, engine=server.Engine(model=plain))
    with pytest.raises(ValueError, match="chunk_attn runs the fused step only"):
        TinyLlama("micro", device="cpu", max_batch=2, chunk_attn=True, fused=False)
    with pytest.raises(ValueError, match="chunk_attn runs the fused step only"):  # more rows than a fused step takes
        m.step_rows(torch.zeros(65, dtype=torch.int64), torch.zeros(65, dtype=torch.int32))
    # the CLI flag, passed on by --gpus
    a, off = server.arg_parser().parse_args(["--chunk-attn", "--gpus", "2"]), server.arg_parser().parse_args([])
    assert a.chunk_attn and "--chunk-attn" in server.replica_cmd(a, 1)
    assert not off.chunk_attn and "--chunk-attn" not in server.replica_cmd(off, 0)
