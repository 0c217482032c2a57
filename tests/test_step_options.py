"""``StepOptions``: the one struct the fused step's options travel in. The four exports that take it
(``p2pt_llama_step``, ``_step_kernels``, ``_step_ws``, ``_step_weights``) against the entry points from before it that
tests and scripts still call, over every option, and the refusals ``options_ok`` holds for all four. Host only: the
library, no device. No call here can reach a kernel launch: the one call of ``p2pt_llama_step`` passes a workspace of
0 bytes, which the step refuses after the options and ahead of its first launch.
"""
import collections
import ctypes
import itertools

import pytest
import torch

from p2p_llm_tunnel_amd import ops
from test_moe import ROLES  # decode_fused.hip's enum Role, R_ROUTER last

INT, SIZE = ctypes.c_int, ctypes.c_size_t
INVALID = 1  # hipErrorInvalidValue
FAMILIES = {"plain": {}, "bias": {"qkv_bias": 1}, "qk_norm": {"qk_norm": 1}, "table": {"rope_table": 1},
            "kv_fp8": {"kv_fp8": 1}}
ROWS = (1, 16, 17, 64)
DENSE_KEYS = ["resid", "q", "attn", "h", "ss", "part_o", "part_ml", "am_val", "am_idx", "counters", "qkv"]
MOE_KEYS = ["route_id", "route_w", "route_rs", "moe_h", "moe_part"]

Config = collections.namedtuple("Config", "fmt windows chunk moe experts lora", defaults=("bf16", False, False, False,
                                                                                        "bf16", False))
# Each weight format, MoE x each expert format and LoRA, each with and without windows and chunk attention.
ON_OFF = list(itertools.product((False, True), repeat=2))
GRID = [Config(fmt=f, windows=w, chunk=c) for f in ops.WEIGHT_FORMATS for w, c in ON_OFF]
GRID += [Config(moe=True, experts=e, windows=w, chunk=c) for e in ops.EXPERT_FORMATS for w, c in ON_OFF]
GRID += [Config(lora=True, windows=w, chunk=c) for w, c in ON_OFF]


def dims(**kw):
    # dim, H * D and ffn are whole groups of 128, so grouped int4 layers and MXFP4 experts are served.
    base = dict(vocab=512, dim=256, n_layers=2, H=4, Hkv=2, D=64, ffn=256, max_seq=64, max_batch=5, eps=1e-5, theta=1e4)
    base.update(kw)
    return ops.LlamaDims(**base)


def pieces(c: Config):
    """The options of ``c`` one by one, as the entry points from before ``StepOptions`` take them."""
    fmt = ops.as_weight_format(weight_format=c.fmt)
    windows = (0, 3) if c.windows else None
    moe = ops.MoeDims(4, 2, 1) if c.moe else None
    experts = ops.ExpertFormat(ops.EXPERT_FORMATS[c.experts]) if c.moe else None
    lora = ops.LoraTable(n_adapters=2, rank=(INT * 4)(16, 16, 32, 16)) if c.lora else None
    return fmt, windows, moe, experts, lora


def options(c: Config, kv_scales=None):
    fmt, windows, moe, experts, lora = pieces(c)
    return ops.step_options(fmt, kv_scales, windows, c.chunk, moe, experts, lora)


def ref(x):
    return ctypes.byref(x) if x is not None else None


def served(c: Config, family: str) -> bool:
    return not (c.lora and family == "qk_norm")  # the one combination of the grid that the step refuses


def test_the_mirror_is_the_struct():
    assert [n for n, _ in ops.StepOptions._fields_] == ["fmt", "kv_scales", "windows", "chunk_attn", "moe", "experts",
                                                        "lora"]
    assert ctypes.sizeof(ops.StepOptions) == 56 and ops.StepOptions.chunk_attn.offset == 24
    assert bytes(ops.step_options(ops.WeightFormat(0, 0))) == bytes(56)  # all zero: the bf16 dense step
    o = options(Config("mxfp4", True, True, True, "fp8", True))
    assert (o.fmt.layers, o.fmt.lm_head, o.chunk_attn, list(o.windows[:2])) == (2, 1, 1, [0, 3])
    assert (o.moe.contents.top_k, o.experts.contents.w8, list(o.lora.contents.rank)) == (2, 1, [16, 16, 32, 16])
    for name in ("p2pt_llama_step", "p2pt_llama_step_kernels", "p2pt_llama_step_ws", "p2pt_llama_step_weights"):
        assert getattr(ops.lib(), name).argtypes[1] == ctypes.POINTER(ops.StepOptions)
    assert len(ops.lib().p2pt_llama_step.argtypes) == 16 and ops.lib().p2pt_llama_step_ws.restype is SIZE


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_kernel_lookup_is_the_old_entry_points(family):
    lib, d = ops.lib(), dims(**FAMILIES[family])
    for c, B in itertools.product(GRID, ROWS):
        fmt, windows, moe, experts, lora = pieces(c)
        got = lib.p2pt_llama_step_kernels(d, options(c), B, 0)
        if c.lora:  # its own export is gone: the variants exist for every row count of a dense bf16 model without QK-norm
            assert got == (0 if served(c, family) else -1), (c, B)
            continue
        warr = (INT * 2)(*windows) if windows else None
        assert got == lib.p2pt_llama_plan_kernels_experts(d, B, 0, fmt, warr, int(c.chunk), ref(moe), ref(experts)) == 0
        if not c.moe and not c.chunk:
            assert got == lib.p2pt_llama_plan_kernels_fmt(d, B, 0, fmt, warr)
        if not c.moe and not c.chunk and c.fmt in ("bf16", "fp8"):
            wp = ops.WeightPlan(w8=fmt.layers)
            assert got == lib.p2pt_llama_plan_kernels_win(d, B, 0, wp, warr)
            if not c.windows:
                assert got == lib.p2pt_llama_plan_kernels_w(d, B, 0, wp)
        if c == Config():
            assert got == lib.p2pt_llama_plan_kernels(d, B, 0)
        assert ops.plan_kernels_ok(d, B, windows=windows, weight_format=fmt, chunk_attn=c.chunk, moe=moe,
                                   expert_format=experts)
    for B in (0, 65):
        assert lib.p2pt_llama_step_kernels(d, options(Config()), B, 0) == -1


def old_workspace(lib, d, c):
    """What each entry point from before ``StepOptions`` that can say ``c`` reports: (bytes, {index in WsBuf order:
    (offset, count)}). A buffer it does not report is empty in a configuration it can say."""
    fmt, _, moe, _, _ = pieces(c)
    off, cnt, out = (SIZE * 16)(), (SIZE * 16)(), []
    if c.fmt != "int4g128":
        assert lib.p2pt_llama_ws_layout_moe(d, ref(moe), off, cnt, 16) == 16
        out.append((lib.p2pt_llama_ws_bytes_moe(d, ref(moe)), {i: (off[i], cnt[i]) for i in range(16)}))
    if not c.moe:  # xg is the twelfth buffer there and the seventeenth of WsBuf
        assert lib.p2pt_llama_ws_layout_fmt(d, fmt, off, cnt, 12) == 12
        out.append((lib.p2pt_llama_ws_bytes_fmt(d, fmt), {(16 if i == 11 else i): (off[i], cnt[i]) for i in range(12)}))
    if not c.moe and c.fmt != "int4g128":
        assert lib.p2pt_llama_ws_layout(d, off, cnt, 11) == 11
        out.append((lib.p2pt_llama_ws_bytes(d), {i: (off[i], cnt[i]) for i in range(11)}))
    return out


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_workspace_is_the_old_entry_points_buffer_for_buffer(family):
    lib, d = ops.lib(), dims(**FAMILIES[family])
    n = len(ops.WS_BUFFERS)
    dense = lib.p2pt_llama_ws_bytes(d)
    for c in GRID:
        off, cnt = (SIZE * n)(), (SIZE * n)()
        nbytes = lib.p2pt_llama_step_ws(d, options(c), off, cnt, n)
        if not served(c, family):
            assert nbytes == 0 and not any(off) and not any(cnt)
            continue
        assert nbytes == lib.p2pt_llama_step_ws(d, options(c), None, None, 0) > 0
        used = [i for i in range(n) if cnt[i]]
        if c.lora:  # its own exports are gone: the dense workspace and delta, fp32 [64][widest projection], after it
            assert all((off[i], cnt[i]) == at for i, at in old_workspace(lib, d, Config())[-1][1].items())
            assert off[17] == dense
            assert cnt[17] == 64 * max((d.H + 2 * d.Hkv) * d.D, d.dim, 2 * d.ffn) and nbytes == dense + 4 * cnt[17]
            assert [i for i in used if i > 10] == [17]
            continue
        for old_bytes, reported in old_workspace(lib, d, c):
            assert nbytes == old_bytes
            for i in range(n):
                assert (off[i], cnt[i]) == reported[i] if i in reported else cnt[i] == 0, (c, i)
        assert [i for i in used if i > 10] == ([11, 12, 13, 14, 15] if c.moe else []) + ([16] if c.fmt == "int4g128" else [])
    short = (SIZE * n)()
    assert lib.p2pt_llama_step_ws(d, options(Config()), short, short, n - 1) == dense and not any(short)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_weight_layout_is_the_old_entry_points_and_pythons(family):
    lib, d = ops.lib(), dims(**FAMILIES[family])
    R, L = len(ROLES), d.n_layers
    for c in GRID:
        fmt, _, moe, experts, _ = pieces(c)
        at, sc = (INT * (R * L))(), (INT * (R * L))()
        size = lib.p2pt_llama_step_weights(d, options(c), at, sc, R * L)
        if not served(c, family):
            assert size == -1
            continue
        assert lib.p2pt_llama_step_weights(d, options(c), at, sc, R * L - 1) == -1
        table = ops.WeightTable(d, weight_format=fmt, moe=moe, expert_format=experts)
        key = lambda j: (ROLES[j % R], None if j % R < 4 else j // R)  # noqa: E731
        assert size == len(table)
        assert {key(j): at[j] for j in range(R * L) if at[j] >= 0} == \
            {(e.name, e.layer): i for i, e in enumerate(table) if not e.name.endswith(" scale")}
        assert {key(j): sc[j] for j in range(R * L) if sc[j] >= 0} == \
            {(e.name[:-len(" scale")], e.layer): i for i, e in enumerate(table) if e.name.endswith(" scale")}
        if c.moe:
            old, old_sc, plain = (INT * (R * L))(), (INT * (R * L))(), (INT * (R * L))()
            assert lib.p2pt_llama_weight_layout_experts(d, moe, experts, old, old_sc, R * L) == size
            assert list(old) == list(at) and list(old_sc) == list(sc)
            assert lib.p2pt_llama_weight_layout_moe(d, moe, plain, R * L) == size - (2 * L if experts.w8 else 0)
            assert list(plain) == list(at)
            continue
        assert all(at[j * R + R - 1] == -1 for j in range(L))  # no router
        old, old_sc = (INT * (13 * L))(), (INT * (13 * L))()
        assert lib.p2pt_llama_weight_layout_fmt(d, fmt, old, old_sc, 13 * L) == size
        thirteen = [j for j in range(R * L) if j % R != R - 1]
        assert list(old) == [at[j] for j in thirteen] and list(old_sc) == [sc[j] for j in thirteen]
        if c.fmt in ("bf16", "fp8"):
            again, again_sc = (INT * (13 * L))(), (INT * (13 * L))()
            assert lib.p2pt_llama_weight_layout(d, ops.WeightPlan(w8=fmt.layers), again, again_sc, 13 * L) == size
            assert list(again) == list(old) and list(again_sc) == list(old_sc)


def refused():
    """name -> (dims, options): each invalid in one way; the same with that one thing put right is served."""
    moe, scales = ops.MoeDims(4, 2, 1), torch.ones(4, 2, 2)
    lora = ops.LoraTable(n_adapters=1, rank=(INT * 4)(16, 16, 16, 16))
    bf16, fp8 = ops.WeightFormat(0, 0), ops.WeightFormat(1, 1)
    return {
        "an unsupported format pair": (dims(), ops.step_options(ops.WeightFormat(2, 2))),
        "a negative window": (dims(), ops.step_options(bf16, windows=(0, -1))),
        "experts without moe": (dims(), ops.step_options(bf16, experts=ops.ExpertFormat(1))),
        "moe with FP8 layers": (dims(), ops.step_options(fp8, moe=moe)),
        "LoRA with MoE": (dims(), ops.step_options(bf16, moe=moe, lora=lora)),
        "LoRA with an FP8 LM head": (dims(), ops.step_options(fp8, lora=lora)),
        "LoRA with QK-norm": (dims(qk_norm=1), ops.step_options(bf16, lora=lora)),
        "kv_scales without kv_fp8": (dims(), ops.step_options(bf16, kv_scales=scales)),
    }, scales  # the tensor outlives the options that point into it


@pytest.mark.parametrize("what", sorted(refused()[0]))
def test_an_invalid_option_is_refused_by_all_four(what):
    lib = ops.lib()
    cases, _keep = refused()
    d, o = cases[what]
    n, R = len(ops.WS_BUFFERS), len(ROLES)
    off, cnt, at, sc = (SIZE * n)(), (SIZE * n)(), (INT * (R * 2))(), (INT * (R * 2))()
    assert lib.p2pt_llama_step_kernels(d, o, 1, 0) == -1
    assert lib.p2pt_llama_step_ws(d, o, off, cnt, n) == 0 and not any(off) and not any(cnt)
    assert lib.p2pt_llama_step_weights(d, o, at, sc, R * 2) == -1
    assert lib.p2pt_llama_step(d, o, None, None, None, None, None, None, 1, 0, None, 0, None, None, None, None) == INVALID


def test_each_refusal_is_that_options_alone():
    # Every case of refused() with its one fault put right is served by the three host-only exports.
    lib, moe, scales = ops.lib(), ops.MoeDims(4, 2, 1), torch.ones(4, 2, 2)
    lora = ops.LoraTable(n_adapters=1, rank=(INT * 4)(16, 16, 16, 16))
    bf16 = ops.WeightFormat(0, 0)
    for d, o in ((dims(), ops.step_options(ops.WeightFormat(2, 1))), (dims(), ops.step_options(bf16, windows=(0, 1))),
                 (dims(), ops.step_options(bf16, moe=moe, experts=ops.ExpertFormat(1))),
                 (dims(), ops.step_options(bf16, moe=moe)), (dims(), ops.step_options(bf16, lora=lora)),
                 (dims(kv_fp8=1), ops.step_options(bf16, kv_scales=scales))):
        assert lib.p2pt_llama_step_kernels(d, o, 1, 0) == 0
        assert lib.p2pt_llama_step_ws(d, o, None, None, 0) > 0 and lib.p2pt_llama_step_weights(d, o, None, None, 0) == -1
        at = (INT * (len(ROLES) * 2))()
        assert lib.p2pt_llama_step_weights(d, o, at, None, len(ROLES) * 2) > 0


@pytest.mark.parametrize("name,d,c,keys", [
    ("dense", dims(), Config(), DENSE_KEYS),
    ("qk_norm", dims(qk_norm=1), Config(), DENSE_KEYS),
    ("moe", dims(), Config(moe=True), DENSE_KEYS + MOE_KEYS),
    ("int4", dims(), Config("int4g128"), DENSE_KEYS + ["xg"]),
    ("lora", dims(), Config(lora=True), DENSE_KEYS + ["delta"]),
])
def test_the_workspace_keys_are_what_they_were(name, d, c, keys):
    nbytes, layout = ops.workspace_layout(d, options(c))
    assert list(layout) == keys
    assert (layout["qkv"][2] > 0) == (name == "qk_norm")  # empty, and still a key, without QK-norm
    assert all(layout[k][2] > 0 for k in keys if k != "qkv")
    for (dtype, off, count) in layout.values():
        assert off % 256 == 0 and off + count * dtype.itemsize <= nbytes
    assert [n for n, _ in ops.FusedLlamaDecoder._WS_BUFFERS] == DENSE_KEYS == [n for n, _ in ops.WS_BUFFERS[:ops.WS_DENSE]]
