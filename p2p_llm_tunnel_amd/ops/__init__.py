"""Python front-end for the gfx950 HIP kernels (``kernels.hip``, ``decode_fused.hip``, ``sample.hip``,
``logprobs.hip``, ``kv_copy.hip``, ``embed_pool.hip``, ``penalty.hip``, ``guide.hip``).

The kernels are compiled in-tree into ``_hip_ops.so`` (see ``build.py``) and
called through ctypes on the current torch stream. Every wrapper validates
shapes, dtypes, devices and contiguity on the host *before* launching, so a
mismatched tensor raises instead of faulting the GPU. There is no silent
PyTorch fallback: if the library is missing on a GPU host, ``lib()`` raises.
"""
from __future__ import annotations

import collections
import ctypes
import math
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class LlamaDims(ctypes.Structure):
    """Mirror of ``LlamaDims`` in decode_fused.hip."""
    _fields_ = [(n, ctypes.c_int) for n in ("vocab", "dim", "n_layers", "H", "Hkv", "D", "ffn", "max_seq",
                                           "max_batch")] + [("eps", ctypes.c_float), ("theta", ctypes.c_float),
                                                            ("kv_fp8", ctypes.c_int), ("rope_table", ctypes.c_int),
                                                            ("qk_norm", ctypes.c_int), ("qkv_bias", ctypes.c_int)]


_INT = ctypes.c_int


class GemmPlan(ctypes.Structure):
    """Mirror of ``GemmPlan`` in decode_fused.hip: ``k_skinny<nw, tn, epi, um>`` with ``1 << kpl`` K parts on a
    ``grid_x`` x ``grid_y`` grid, reading ``ss_in`` sum-of-squares partials (0: no norm)."""
    _fields_ = [(n, _INT) for n in ("epi", "nw", "tn", "um", "kpl", "grid_x", "grid_y", "ss_in", "M", "N", "K")]


class AttnPlan(ctypes.Structure):
    """Mirror of ``AttnPlan``: ``k_attn<D, G>`` on ``slots`` x ``grid_y`` workgroups; ``stride`` partial slots per
    head in part_o / part_ml."""
    _fields_ = [(n, _INT) for n in ("D", "G", "slots", "stride", "grid_y")]


class StepPlan(ctypes.Structure):
    """Mirror of ``StepPlan``: what one fused step launches (``qkv_first``: layer 0; ``qk_norm_grid``:
    ``k_qknorm_rope``'s gridDim.x, 0 when the model has no QK-norm and the kernel is not launched;
    ``qk_norm_table``: 1 when that kernel is the variant that reads the RoPE frequencies from a table)."""
    _fields_ = ([("rows", _INT), ("emit_rows", _INT)] +
                [(n, GemmPlan) for n in ("qkv_first", "qkv", "o", "gate_up", "down", "lm_head")] +
                [("attn", AttnPlan), ("am_parts", _INT), ("qk_norm_grid", _INT), ("qk_norm_table", _INT)])


class KvPlan(ctypes.Structure):
    """Mirror of ``KvPlan``: the FP8-cache variants a step launches beside its ``StepPlan`` (``dims.kv_fp8``):
    ``attn_kv8``: 1 for ``k_attn<D, G, true>``, which reads an e4m3 cache; ``qk_norm_kv8``: 1 when
    ``k_qknorm_rope`` is the variant that appends k and v as e4m3. The _KV8 epilogue shows in ``StepPlan.qkv.epi``."""
    _fields_ = [("attn_kv8", _INT), ("qk_norm_kv8", _INT)]


class WeightPlan(ctypes.Structure):
    """Mirror of ``WeightPlan``: the weight format of a step, beside its ``StepPlan`` as ``KvPlan`` is. ``w8``: 1
    when the five GEMM weights (wqkv, wo, w_gate_up, w_down, lm_head) are e4m3 bytes with one fp32 scale per
    output row and every ``k_skinny`` is its FP8-weight instantiation (docs/WEIGHT_FP8.md); 0: bf16."""
    _fields_ = [("w8", _INT)]


class WeightFormat(ctypes.Structure):
    """Mirror of ``WeightFormat``: the weight formats of a step, beside its ``StepPlan`` as ``WeightPlan`` is, and what
    the ``_fmt`` entry points take. ``layers``: the format of a layer's four GEMM weights (wqkv, wo, w_gate_up,
    w_down); ``lm_head``: the LM head's. 0 bf16, 1 FP8 (docs/WEIGHT_FP8.md), 2 MXFP4 (docs/WEIGHT_MXFP4.md: the layers
    only, with an FP8 LM head). The supported pairs are ``WEIGHT_FORMATS``' values."""
    _fields_ = [("layers", _INT), ("lm_head", _INT)]

    def __repr__(self):
        return f"WeightFormat(layers={self.layers}, lm_head={self.lm_head})"


WEIGHT_FORMATS = {"bf16": (0, 0), "fp8": (1, 1), "mxfp4": (2, 1)}  # weight dtype -> (layers, lm_head) of WeightFormat


def as_weight_format(weight_fp8: bool = False, weight_format=None) -> WeightFormat:
    """The ``WeightFormat`` a caller means: ``weight_format`` (a ``WeightFormat``, or one of "bf16", "fp8", "mxfp4")
    where given, else FP8 throughout for ``weight_fp8`` and bf16 without. Both at once, an unknown name or a pair of
    formats the step does not run are refused (host only: no library)."""
    if weight_format is None:
        return WeightFormat(*WEIGHT_FORMATS["fp8" if weight_fp8 else "bf16"])
    if weight_fp8:
        raise ValueError("give weight_fp8 or weight_format, not both")
    if isinstance(weight_format, str):
        if weight_format not in WEIGHT_FORMATS:
            raise ValueError(f"weight_format must be one of {sorted(WEIGHT_FORMATS)}, got {weight_format!r}")
        return WeightFormat(*WEIGHT_FORMATS[weight_format])
    if not isinstance(weight_format, WeightFormat) or \
            (weight_format.layers, weight_format.lm_head) not in WEIGHT_FORMATS.values():
        raise ValueError(f"weight_format must be a WeightFormat of (layers, lm_head) in "
                         f"{sorted(WEIGHT_FORMATS.values())} or one of {sorted(WEIGHT_FORMATS)}, got {weight_format!r}")
    return WeightFormat(weight_format.layers, weight_format.lm_head)


class WindowPlan(ctypes.Structure):
    """Mirror of ``WindowPlan``: what one layer's sliding window changes of a step, beside its ``StepPlan`` as
    ``KvPlan`` and ``WeightPlan`` are (docs/SLIDING_WINDOW.md). ``win``: 1 for ``k_attn<D, G, KV8, true>``;
    ``window``: its launch argument; ``slots``: its gridDim.x, the span slots of a cache of ``min(max_seq, window)``
    rows. A layer without a window has ``win`` 0, ``window`` 0 and ``StepPlan.attn.slots``."""
    _fields_ = [("win", _INT), ("window", _INT), ("slots", _INT)]


def _signatures() -> dict:
    """Every symbol ``lib()`` binds -> its argtypes. The restype is ``c_int`` unless ``_RESTYPES`` names another."""
    vp, i, f, sz, ptr = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.POINTER
    dims, wp, ip, szp, wf = ptr(LlamaDims), ptr(WeightPlan), ptr(i), ptr(sz), ptr(WeightFormat)
    return {
        "p2pt_rmsnorm": [vp, vp, vp, vp, vp, i, i, f, vp],
        "p2pt_silu_mul": [vp, vp, i, i, vp],
        "p2pt_rope_qkv_cache": [vp, vp, vp, vp, vp, i, i, i, i, i, f, vp, vp],
        "p2pt_qk_norm_rope_cache": [vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, f, f, vp, vp],
        "p2pt_decode_attention": [vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, f, vp],
        "p2pt_argmax": [vp, vp, i, i, vp],
        "p2pt_skinny_gemm": [vp, vp, vp, i, i, i, vp],
        "p2pt_sample": [vp, vp, vp, i, i, i, vp],
        "p2pt_sample_minp": [vp, vp, vp, i, i, i, vp],
        "p2pt_logprobs": [vp, vp, vp, vp, vp, i, i, vp],
        "p2pt_kv_copy": [vp, vp, i, i, i, i, i, ip, vp],
        "p2pt_max_kv_copy_jobs": [],
        "p2pt_embed_pool": [vp, i, i, vp, vp, i, vp, i, f, i, ip, vp],
        "p2pt_max_embed_jobs": [],
        "p2pt_penalize": [vp, vp, vp, vp, vp, vp, vp, i, vp, i, vp, vp, vp, i, i, vp],
        "p2pt_penalty_reset": [vp, i, i, i, vp, i, vp, vp, vp, vp, i, vp],
        "p2pt_max_logit_bias": [],
        "p2pt_guide": [vp, vp, vp, vp, vp, vp, vp, vp, i, vp, i, i, i, vp],
        "p2pt_guide_reset": [vp, vp, i, i, i, i, vp],
        "p2pt_llama_ws_bytes": [dims],
        "p2pt_llama_ws_layout": [dims, szp, szp, i],
        "p2pt_llama_decode": [dims, ptr(vp), vp, vp, vp, vp, vp, i, i, vp, sz, vp, vp, vp],
        "p2pt_llama_plan": [dims, i, i, ptr(StepPlan)],
        "p2pt_llama_kv_plan": [dims, ptr(KvPlan)],
        "p2pt_llama_plan_kernels": [dims, i, i],
        "p2pt_llama_weight_plan": [dims, i, wp],
        "p2pt_llama_plan_kernels_w": [dims, i, i, wp],
        "p2pt_llama_decode_w": [dims, wp, ptr(vp), vp, vp, vp, vp, vp, i, i, vp, sz, vp, vp, vp],
        "p2pt_llama_decode_kv": [dims, wp, vp, ptr(vp), vp, vp, vp, vp, vp, i, i, vp, sz, vp, vp, vp],
        "p2pt_llama_weight_layout": [dims, wp, ip, ip, i],
        "p2pt_llama_window_plan": [dims, i, i, ptr(WindowPlan)],
        "p2pt_llama_plan_kernels_win": [dims, i, i, wp, ip],
        "p2pt_llama_decode_win": [dims, wp, vp, ip, ptr(vp), vp, vp, vp, vp, vp, i, i, vp, sz, vp, vp, vp],
        "p2pt_llama_weight_format": [dims, i, i, wf],
        "p2pt_llama_plan_kernels_fmt": [dims, i, i, wf, ip],
        "p2pt_llama_weight_layout_fmt": [dims, wf, ip, ip, i],
        "p2pt_llama_decode_fmt": [dims, wf, vp, ip, ptr(vp), vp, vp, vp, vp, vp, i, i, vp, sz, vp, vp, vp],
        "p2pt_attn_span": [i, i],
        "p2pt_max_rows": [],
        "p2pt_skinny_bench": [vp, vp, vp, i, i, i, i, i, i, vp],  # microbenchmark hooks (scripts/bench_skinny.py)
        "p2pt_attn_bench": [vp, vp, vp, vp, i, i, i, i, i, vp, vp, vp, vp, i, vp],
    }


_RESTYPES = {"p2pt_llama_ws_bytes": ctypes.c_size_t}


def lib() -> ctypes.CDLL:
    global _LIB
    if _LIB is None:
        # P2PT_HIP_OPS_LIB: another in-tree build of the same kernels (A/B runs on one box).
        path = os.path.join(HERE, os.environ.get("P2PT_HIP_OPS_LIB", "_hip_ops.so"))
        if not os.path.exists(path):
            from . import build as _b
            _b.build()
        _LIB = ctypes.CDLL(path)
        for name, argtypes in _signatures().items():
            fn = getattr(_LIB, name)
            fn.argtypes, fn.restype = argtypes, _RESTYPES.get(name, ctypes.c_int)
        if _LIB.p2pt_max_rows() != MAX_ROWS:
            raise RuntimeError(f"MAX_ROWS = {MAX_ROWS}, but {path} was built for {_LIB.p2pt_max_rows()} rows")
        if _LIB.p2pt_max_kv_copy_jobs() != MAX_KV_COPY_JOBS:
            raise RuntimeError(f"MAX_KV_COPY_JOBS = {MAX_KV_COPY_JOBS}, but {path} was built for "
                               f"{_LIB.p2pt_max_kv_copy_jobs()} jobs")
        if _LIB.p2pt_max_embed_jobs() != MAX_EMBED_JOBS:
            raise RuntimeError(f"MAX_EMBED_JOBS = {MAX_EMBED_JOBS}, but {path} was built for "
                               f"{_LIB.p2pt_max_embed_jobs()} jobs")
        if _LIB.p2pt_max_logit_bias() != MAX_LOGIT_BIAS:
            raise RuntimeError(f"MAX_LOGIT_BIAS = {MAX_LOGIT_BIAS}, but {path} was built for "
                               f"{_LIB.p2pt_max_logit_bias()} entries")
    return _LIB


MAX_ROWS = 64  # token rows per fused step; lib() checks it against decode_fused.hip's kMaxM
MAX_KV_COPY_JOBS = 8  # jobs per launch of kv_copy_ (kv_copy.hip's kMaxJobs: they travel in the kernel arguments)
MAX_EMBED_JOBS = 16  # jobs per launch of embed_pool_ (embed_pool.hip's kMaxJobs: in the kernel arguments too)
MAX_LOGIT_BIAS = 300  # entries of a slot's logit_bias list (penalty.hip's kMaxBias; the OpenAI API's limit)
KV_FP8_DTYPES = (torch.float8_e4m3fn, torch.uint8)  # cache dtypes of a decoder with dims.kv_fp8 (the same bytes)
WEIGHT_FP8_DTYPES = KV_FP8_DTYPES  # GEMM-weight dtypes of a decoder with weight_fp8 (the same bytes)
GEMM_OPERAND_LIMIT = 1 << 31  # bytes: every k_skinny operand stays below it (decode_fused_kernels.h's kOob)
E4M3_MAX = 448.0  # the largest finite e4m3fn value: a row's largest magnitude quantises to it
MXFP4_BLOCK = 32  # K elements per MXFP4 block: one e8m0 scale byte each (one k-step of k_skinny)
MXFP4_EXP_MIN, MXFP4_EXP_MAX = 2, 252  # the e8m0 bytes quantize_weight_mxfp4 emits (its docstring derives them)
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # the magnitudes of an e2m1 nibble's low three bits; bit 3: sign
MAX_TOP_LOGPROBS = 20  # top (id, logprob) pairs per row of logprobs_ (logprobs.hip's kMaxTop; the OpenAI API's limit)


def step_plan(dims: LlamaDims, B: int, emit_rows: int = 0) -> StepPlan:
    """What ``p2pt_llama_decode`` launches for B rows: the kernel variant, grid and partial counts of every
    stage, from the library's own planning function (host only: needs the library, not a GPU)."""
    plan = StepPlan()
    if lib().p2pt_llama_plan(ctypes.byref(dims), B, emit_rows, ctypes.byref(plan)) != 0:
        raise ValueError("dims or row count not supported by the fused decode kernels")
    return plan


def kv_plan(dims: LlamaDims) -> KvPlan:
    """The FP8-cache variants ``p2pt_llama_decode`` launches for ``dims`` (host only); both 0 without ``kv_fp8``."""
    plan = KvPlan()
    if lib().p2pt_llama_kv_plan(ctypes.byref(dims), ctypes.byref(plan)) != 0:
        raise ValueError("dims not supported by the fused decode kernels")
    return plan


def weight_plan(dims: LlamaDims, weight_fp8: bool = False, weight_format=None):
    """The weight format ``p2pt_llama_decode_w`` launches for (host only): ``w8`` 1 with FP8 weights, 0 without.
    ``step_plan(dims, B)`` is the same either way: the format changes no grid, wave count or load batch.
    With ``weight_format`` (see ``as_weight_format``) the answer is the library's ``WeightFormat`` instead, which an
    MXFP4 model needs: its layers and its LM head differ."""
    if weight_format is not None:
        f, out = as_weight_format(weight_fp8, weight_format), WeightFormat()
        if lib().p2pt_llama_weight_format(ctypes.byref(dims), f.layers, f.lm_head, ctypes.byref(out)) != 0:
            raise ValueError("dims not supported by the fused decode kernels")
        return out
    plan = WeightPlan()
    if lib().p2pt_llama_weight_plan(ctypes.byref(dims), int(bool(weight_fp8)), ctypes.byref(plan)) != 0:
        raise ValueError("dims not supported by the fused decode kernels")
    return plan


def check_windows(windows, n_layers: int) -> tuple | None:
    """``windows`` as the fused step takes them: None, or one int per layer, 0 for full attention and W >= 1 for a
    sliding window of W positions. Returns None when no layer has a window (None and all zeros alike)."""
    if windows is None:
        return None
    windows = tuple(windows)
    if len(windows) != n_layers:
        raise ValueError(f"windows must hold one entry per layer ({n_layers}), got {len(windows)}")
    for L, w in enumerate(windows):
        if not _int_in(w, 0, 1 << 31):
            raise ValueError(f"layer {L}: a window must be an int >= 0 (0: full attention), got {w!r}")
    return windows if any(windows) else None


def window_plan(dims: LlamaDims, B: int, window: int) -> WindowPlan:
    """What a layer with sliding window ``window`` (0: none) launches for attention at B rows, beside
    ``step_plan(dims, B)`` (host only): the ``k_attn`` variant, its window argument and its span slots. The
    partials' stride is ``step_plan(dims, B).attn.stride`` for every layer."""
    plan = WindowPlan()
    if not _int_in(window, 0, 1 << 31) or \
            lib().p2pt_llama_window_plan(ctypes.byref(dims), B, window, ctypes.byref(plan)) != 0:
        raise ValueError("dims, row count or window not supported by the fused decode kernels")
    return plan


def plan_kernels_ok(dims: LlamaDims, B: int, emit_rows: int = 0, weight_fp8: bool = False, windows=None,
                    weight_format=None) -> bool:
    """Whether every stage of ``step_plan(dims, B, emit_rows)``, ``kv_plan(dims)`` and
    ``weight_plan(dims, weight_fp8)`` names a kernel the library instantiates, by the lookups its launchers use
    (host only). ``windows``: the per-layer sliding windows (``check_windows``); every layer's ``window_plan`` is
    then looked up too. ``weight_format`` (see ``as_weight_format``): the formats instead of ``weight_fp8``."""
    windows = check_windows(windows, dims.n_layers)
    if weight_format is not None:
        f = as_weight_format(weight_fp8, weight_format)
        rc = lib().p2pt_llama_plan_kernels_fmt(ctypes.byref(dims), B, emit_rows, ctypes.byref(f),
                                               (ctypes.c_int * len(windows))(*windows) if windows is not None else None)
    elif windows is not None:
        wp = WeightPlan(w8=int(bool(weight_fp8)))
        rc = lib().p2pt_llama_plan_kernels_win(ctypes.byref(dims), B, emit_rows, ctypes.byref(wp),
                                               (ctypes.c_int * len(windows))(*windows))
    elif weight_fp8:
        wp = WeightPlan(w8=1)
        rc = lib().p2pt_llama_plan_kernels_w(ctypes.byref(dims), B, emit_rows, ctypes.byref(wp))
    else:
        rc = lib().p2pt_llama_plan_kernels(ctypes.byref(dims), B, emit_rows)
    if rc < 0:
        raise ValueError("dims or row count not supported by the fused decode kernels")
    return rc == 0


WeightEntry = collections.namedtuple("WeightEntry", "name layer dtypes shape align")  # layer None: global; align: bytes
LAYER_GEMMS = ("wqkv", "wo", "w_gate_up", "w_down")  # a layer's GEMM weights, in the order of their scales


class WeightTable(list):
    """The fused step's weight table for ``(dims, weight_fp8)``: its ``WeightEntry`` list, in order (host only: no
    device, no library). The one Python statement of the layout; decode_fused.hip's ``WeightTable`` is the C one,
    and ``p2pt_llama_weight_layout`` reports that for comparison (tests/test_weight_table.py).

    embed, final_norm, lm_head; inv_freq (fp32 (D / 2,), 8-byte aligned) with ``dims.rope_table``; then per layer
    attn_norm, wqkv, wo, ffn_norm, w_gate_up, w_down, plus q_norm, k_norm with ``dims.qk_norm`` or bqkv with
    ``dims.qkv_bias``. With ``weight_fp8`` the five GEMM weights are e4m3 (or uint8) bytes, 8-byte aligned (a lane
    loads 8 bytes at a multiple of 8 from the base), and their fp32 row scales follow the table: lm_head's, then
    each layer's four, named ``"<weight> scale"``.

    ``weight_format`` (``as_weight_format``) in place of ``weight_fp8``; "mxfp4" (docs/WEIGHT_MXFP4.md) is the FP8
    table with each layer's four GEMM weights as uint8 ``(N, K / 2)`` and, where the FP8 table has their row scales,
    their e8m0 block scales, uint8 ``(N, K / 32)``: byte ``[n][b]`` is the scale of elements ``32 b .. 32 b + 31`` of
    row n. The physical byte order of an MXFP4 row is the natural one, stated here once: byte ``[n][j]`` holds
    elements ``k = 2 j`` (low nibble, bits 0..3) and ``k = 2 j + 1`` (high nibble), rows in the row order of the
    weight. A lane of ``k_skinny<.., W8 = 2>`` loads its 8 k-values of a k-step as the 4 bytes at
    ``n K / 2 + 16 s + 4 (lane >> 4)`` and the block's scale as the byte at ``n K / 32 + s``, so a weight is 4-byte
    aligned and its scales need no alignment. ``pack_weight_mxfp4`` makes this order from nibble codes ``[N][K]``,
    ``unpack_weight_mxfp4`` undoes it, and decode_fused.hip's accessor and the kernel's offsets mirror it."""

    def __init__(self, dims: LlamaDims, weight_fp8: bool = False, weight_format=None):
        self.format = fmt = as_weight_format(weight_fp8, weight_format)
        d, bf, f32, u8 = dims, (torch.bfloat16,), (torch.float32,), (torch.uint8,)
        gemm, ga = (WEIGHT_FP8_DTYPES, 8) if fmt.lm_head else (bf, 2)
        n_qkv, norm = (d.H + 2 * d.Hkv) * d.D, (bf, (d.dim,), 2)
        top = {"embed": (bf, (d.vocab, d.dim), 2), "final_norm": norm, "lm_head": (gemm, (d.vocab, d.dim), ga)}
        if d.rope_table:
            top["inv_freq"] = (f32, (d.D // 2,), 8)
        shapes = {"wqkv": (n_qkv, d.dim), "wo": (d.dim, d.H * d.D), "w_gate_up": (2 * d.ffn, d.dim),
                  "w_down": (d.dim, d.ffn)}
        if fmt.layers == 2:  # nibbles, two to a byte
            lg = {n: (u8, (N, K // 2), 4) for n, (N, K) in shapes.items()}
        else:
            lg = {n: (gemm, shape, ga) for n, shape in shapes.items()}
        layer = {"attn_norm": norm, "wqkv": lg["wqkv"], "wo": lg["wo"], "ffn_norm": norm, "w_gate_up": lg["w_gate_up"],
                 "w_down": lg["w_down"]}
        if d.qk_norm:
            layer.update(q_norm=(bf, (d.D,), 2), k_norm=(bf, (d.D,), 2))
        elif d.qkv_bias:
            layer["bqkv"] = (bf, (n_qkv,), 2)
        groups = [(None, top)] + [(L, layer) for L in range(d.n_layers)]
        super().__init__(WeightEntry(n, L, *v) for L, group in groups for n, v in group.items())
        if fmt.lm_head:  # the scales, in the order of their weights: fp32 per row, or MXFP4's e8m0 byte per block
            self += [WeightEntry(n + " scale", L, u8, (shapes[n][0], shapes[n][1] // MXFP4_BLOCK), 1)
                     if L is not None and fmt.layers == 2 else WeightEntry(n + " scale", L, f32, v[1][:1], 4)
                     for L, group in groups for n, v in group.items() if n == "lm_head" or n in LAYER_GEMMS]
        self.per_layer = len(layer)
        self._at = {(e.name, e.layer): i for i, e in enumerate(self)}

    def index(self, name: str, layer: int | None = None) -> int:
        """Where ``name`` (of ``layer``; None for a global entry) sits; a role this table lacks is a KeyError."""
        if (name, layer) not in self._at:
            raise KeyError(f"this weight table has no {label(name, layer)}")
        return self._at[name, layer]

    def scale_index(self, name: str, layer: int | None = None) -> int:
        """Where the scales of GEMM weight ``name`` sit (FP8 and MXFP4 tables only): fp32 row scales, or the e8m0
        block scales of an MXFP4 weight."""
        return self.index(name + " scale", layer)


def label(name: str, layer: int | None) -> str:
    """How messages name a table entry: ``lm_head``, ``layer 1: bqkv``."""
    return name if layer is None else f"layer {layer}: {name}"


def attn_span(length: int, slots: int) -> int:
    """Tokens per span slot of ``k_attn`` for a row of ``length`` tokens on ``slots`` slots (host only)."""
    return lib().p2pt_attn_span(length, slots)


def loaded_path() -> str:
    """Path of the library ``lib()`` opened (``P2PT_HIP_OPS_LIB`` honoured)."""
    return lib()._name


def _stream(t: torch.Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _check(t: torch.Tensor, dtype, name: str, device=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name} must be on a HIP device")
    if device is not None and t.device != device:
        raise ValueError(f"{name} on {t.device}, expected {device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _int_in(v, lo, hi) -> bool:
    """``v`` is an int, no bool, with lo <= v < hi."""
    return isinstance(v, int) and not isinstance(v, bool) and lo <= v < hi


def _ok(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: HIP launch failed (hipError {rc})")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, residual: torch.Tensor | None = None):
    """out = rmsnorm(x [+ residual]) * weight. With a residual, returns (out, x + residual)."""
    _check(x, torch.bfloat16, "x")
    _check(weight, torch.bfloat16, "weight", x.device)
    hidden = x.shape[-1]
    if weight.shape != (hidden,):
        raise ValueError(f"weight shape {tuple(weight.shape)} != ({hidden},)")
    if hidden % 8 or hidden > 16384:
        raise ValueError("hidden must be a multiple of 8 and <= 16384")
    rows = x.numel() // hidden
    out = torch.empty_like(x)
    res_out = None
    if residual is not None:
        _check(residual, torch.bfloat16, "residual", x.device)
        if residual.shape != x.shape:
            raise ValueError("residual shape mismatch")
        res_out = torch.empty_like(x)
    _ok(lib().p2pt_rmsnorm(_p(x), _p(residual), _p(res_out), _p(weight), _p(out), rows, hidden, eps, _stream(x)),
        "rmsnorm")
    return out if residual is None else (out, res_out)


def silu_mul(gate_up: torch.Tensor) -> torch.Tensor:
    """[..., 2F] -> silu(gate) * up, [..., F]."""
    _check(gate_up, torch.bfloat16, "gate_up")
    two_f = gate_up.shape[-1]
    if two_f % 16:
        raise ValueError("last dim must be 2*F with F % 8 == 0")
    F = two_f // 2
    rows = gate_up.numel() // two_f
    out = torch.empty(*gate_up.shape[:-1], F, dtype=gate_up.dtype, device=gate_up.device)
    _ok(lib().p2pt_silu_mul(_p(gate_up), _p(out), rows, F, _stream(gate_up)), "silu_mul")
    return out


def _check_inv_freq(inv_freq: torch.Tensor, head_dim: int, device, values: bool = True) -> None:
    """A RoPE frequency table for the kernels that take one: fp32, contiguous, (head_dim / 2,), on ``device``,
    8-byte aligned (``k_qknorm_rope`` reads it in pairs), every entry finite and > 0. ``values``: read the table
    back (a sync) for the last of these; a per-step caller that made and checked its table once passes False and
    keeps the host-side checks alone."""
    _check(inv_freq, torch.float32, "inv_freq", device)
    if inv_freq.shape != (head_dim // 2,):
        raise ValueError(f"inv_freq shape {tuple(inv_freq.shape)} != ({head_dim // 2},)")
    if inv_freq.data_ptr() % 8:
        raise ValueError("inv_freq must be 8-byte aligned")
    if values and not bool((torch.isfinite(inv_freq) & (inv_freq > 0)).all().item()):
        raise ValueError("inv_freq entries must be finite and > 0")


def rope_qkv_cache(qkv: torch.Tensor, pos: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                   n_heads: int, n_kv_heads: int, head_dim: int, theta: float = 10000.0,
                   pos_range: tuple[int, int] | None = None, inv_freq: torch.Tensor | None = None,
                   inv_freq_checked: bool = False) -> torch.Tensor:
    """Apply RoPE to q and k of one new token per sequence and append k, v to the caches.

    qkv: [B, (H + 2*Hkv) * D]; pos: int32 [B]; caches: [B, Smax, Hkv, D]. Returns q [B, H, D].
    ``pos_range`` = host-known (min, max) of ``pos``; without it the bounds are
    read back from the device (a sync) before launch. ``inv_freq``: fp32 (head_dim / 2,) RoPE frequencies
    (scaled RoPE: ``models.rope.inv_freq``), used instead of theta's own. Its entries are read back (a sync) and
    checked unless ``inv_freq_checked`` says the caller has done so (``models.rope.inv_freq`` does, on the host):
    with it and ``pos_range`` the call syncs nothing and can be captured into a hipGraph.
    """
    _check(qkv, torch.bfloat16, "qkv")
    _check(pos, torch.int32, "pos", qkv.device)
    _check(k_cache, torch.bfloat16, "k_cache", qkv.device)
    _check(v_cache, torch.bfloat16, "v_cache", qkv.device)
    B = qkv.shape[0]
    if qkv.shape != (B, (n_heads + 2 * n_kv_heads) * head_dim):
        raise ValueError(f"qkv shape {tuple(qkv.shape)} inconsistent with heads")
    if pos.shape != (B,):
        raise ValueError("pos must be [B]")
    Smax = k_cache.shape[1]
    if k_cache.shape != (B, Smax, n_kv_heads, head_dim) or v_cache.shape != k_cache.shape:
        raise ValueError(f"cache shape {tuple(k_cache.shape)} != ({B}, Smax, {n_kv_heads}, {head_dim})")
    if n_heads % n_kv_heads or head_dim % 2:
        raise ValueError("bad head config")
    pmin, pmax = pos_range if pos_range is not None else (int(pos.min().item()), int(pos.max().item()))
    if pmin < 0 or pmax >= Smax:
        raise ValueError(f"positions out of cache range [0, {Smax})")
    if inv_freq is not None:
        _check_inv_freq(inv_freq, head_dim, qkv.device, values=not inv_freq_checked)
    q = torch.empty(B, n_heads, head_dim, dtype=qkv.dtype, device=qkv.device)
    _ok(lib().p2pt_rope_qkv_cache(_p(qkv), _p(pos), _p(q), _p(k_cache), _p(v_cache), B, n_heads, n_kv_heads,
                                  head_dim, Smax, theta, _p(inv_freq), _stream(qkv)), "rope_qkv_cache")
    return q


def qk_norm_rope_cache(qkv: torch.Tensor, pos: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                       q_weight: torch.Tensor, k_weight: torch.Tensor, n_heads: int, n_kv_heads: int, head_dim: int,
                       eps: float, theta: float, slots: torch.Tensor | None = None,
                       pos_range: tuple[int, int] | None = None, inv_freq: torch.Tensor | None = None,
                       inv_freq_checked: bool = False) -> torch.Tensor:
    """Per-head RMSNorm of q and k (QK-norm models: Qwen3), then RoPE and the cache append: the kernel the
    fused step of such a model launches after its QKV GEMM (``k_qknorm_rope``), on caller tensors.

    qkv: [B <= 64, (H + 2*Hkv) * D] in plain head order; pos: int32 [B]; caches: [n_slots, Smax, Hkv, D];
    q_weight, k_weight: (D,), D in {64, 128}. Every q and k head becomes x * rsqrt(mean(x^2) + eps) * weight in
    fp32, is rotated (rotate-half) at ``pos[b]`` and rounded to bf16 once; v is copied bit for bit. Row b goes
    to cache slot ``slots[b]`` (int32 [B]; default: slot b, so B <= n_slots). Returns q [B, H, D]. ``pos_range``
    = host-known (min, max) of ``pos``; without it the bounds are read back from the device (a sync) before
    launch, as those of ``slots`` always are. ``inv_freq``: fp32 (D / 2,) RoPE frequencies (scaled RoPE), used
    instead of theta's own: the ``k_qknorm_rope<D, true>`` variant; ``inv_freq_checked`` skips the readback of its
    entries, as in ``rope_qkv_cache``."""
    _check(qkv, torch.bfloat16, "qkv")
    dev = qkv.device
    _check(pos, torch.int32, "pos", dev)
    _check(k_cache, torch.bfloat16, "k_cache", dev)
    _check(v_cache, torch.bfloat16, "v_cache", dev)
    _check(q_weight, torch.bfloat16, "q_weight", dev)
    _check(k_weight, torch.bfloat16, "k_weight", dev)
    for name, v in (("n_heads", n_heads), ("n_kv_heads", n_kv_heads), ("head_dim", head_dim)):
        if not _int_in(v, 1, math.inf):
            raise ValueError(f"{name} must be a positive int, got {v!r}")
    if head_dim not in (64, 128):
        raise ValueError("head_dim must be 64 or 128")
    if n_heads % n_kv_heads:
        raise ValueError("n_heads must be a multiple of n_kv_heads")
    if qkv.dim() != 2 or qkv.shape[1] != (n_heads + 2 * n_kv_heads) * head_dim:
        raise ValueError(f"qkv shape {tuple(qkv.shape)} inconsistent with heads")
    B = qkv.shape[0]
    if not 1 <= B <= MAX_ROWS:
        raise ValueError(f"rows must be 1..{MAX_ROWS}")
    if pos.shape != (B,):
        raise ValueError("pos must be [B]")
    if k_cache.dim() != 4 or k_cache.shape[2:] != (n_kv_heads, head_dim) or v_cache.shape != k_cache.shape or \
            k_cache.shape[0] < 1 or k_cache.shape[1] < 1:
        raise ValueError(f"cache shape {tuple(k_cache.shape)} != (n_slots, Smax, {n_kv_heads}, {head_dim})")
    n_slots, Smax = k_cache.shape[0], k_cache.shape[1]
    for name, wgt in (("q_weight", q_weight), ("k_weight", k_weight)):
        if wgt.shape != (head_dim,):
            raise ValueError(f"{name} shape {tuple(wgt.shape)} != ({head_dim},)")
    if any(t.data_ptr() % 4 for t in (qkv, k_cache, v_cache, q_weight, k_weight)):
        raise ValueError("qkv, the caches and the weights must be 4-byte aligned")
    if not (math.isfinite(eps) and eps >= 0.0) or not (math.isfinite(theta) and theta > 0.0):
        raise ValueError("eps must be finite and >= 0, theta finite and > 0")
    if slots is not None:
        _check(slots, torch.int32, "slots", dev)
        if slots.shape != (B,):
            raise ValueError("slots must be [B]")
        if int(slots.min().item()) < 0 or int(slots.max().item()) >= n_slots:
            raise ValueError(f"slots out of range [0, {n_slots})")
    elif B > n_slots:
        raise ValueError(f"{B} rows but {n_slots} cache slots: pass slots")
    pmin, pmax = pos_range if pos_range is not None else (int(pos.min().item()), int(pos.max().item()))
    if pmin < 0 or pmax >= Smax:
        raise ValueError(f"positions out of cache range [0, {Smax})")
    if inv_freq is not None:
        _check_inv_freq(inv_freq, head_dim, dev, values=not inv_freq_checked)
    q = torch.empty(B, n_heads, head_dim, dtype=qkv.dtype, device=dev)
    _ok(lib().p2pt_qk_norm_rope_cache(_p(qkv), _p(pos), _p(slots), _p(q_weight), _p(k_weight), _p(q), _p(k_cache),
                                      _p(v_cache), B, n_heads, n_kv_heads, head_dim, Smax, n_slots, float(eps),
                                      float(theta), _p(inv_freq), _stream(qkv)), "qk_norm_rope_cache")
    return q


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, lens: torch.Tensor,
                     chunk: int = 64, max_len: int | None = None, scale: float | None = None) -> torch.Tensor:
    """Single-token GQA attention over the KV cache. q: [B, H, D]; lens: int32 [B] (>= 1).

    The sequence is split into `chunk`-token pieces, one workgroup each
    (B * Hkv * ceil(max_len / chunk) workgroups), so even batch-1 decode
    fills the 256 CUs. Splits past a sequence's length exit immediately, which
    lets a captured graph use max_len = cache capacity for every step.
    """
    _check(q, torch.bfloat16, "q")
    _check(k_cache, torch.bfloat16, "k_cache", q.device)
    _check(v_cache, torch.bfloat16, "v_cache", q.device)
    _check(lens, torch.int32, "lens", q.device)
    B, H, D = q.shape
    Smax, Hkv = k_cache.shape[1], k_cache.shape[2]
    if k_cache.shape != (B, Smax, Hkv, D) or v_cache.shape != k_cache.shape:
        raise ValueError("cache shape mismatch")
    if D not in (64, 128):
        raise ValueError("head_dim must be 64 or 128")
    if H % Hkv or H // Hkv > 8:
        raise ValueError("n_heads / n_kv_heads must be an integer <= 8")
    if lens.shape != (B,):
        raise ValueError("lens must be [B]")
    if not _int_in(chunk, 1, math.inf):
        raise ValueError(f"chunk must be a positive int, got {chunk!r}")
    if max_len is None:
        max_len = int(lens.max().item())
        if int(lens.min().item()) < 1:
            raise ValueError("every sequence needs at least one cached token")
    if max_len > Smax:
        raise ValueError("lens exceed cache capacity")
    nsplit = max(1, math.ceil(max_len / chunk))
    ws = torch.empty(B * H * nsplit * (D + 2), dtype=torch.float32, device=q.device)
    out = torch.empty_like(q)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    _ok(lib().p2pt_decode_attention(_p(q), _p(k_cache), _p(v_cache), _p(lens), _p(out), _p(ws), B, H, Hkv, D, Smax,
                                    nsplit, chunk, scale, _stream(q)), "decode_attention")
    return out


def argmax(logits: torch.Tensor) -> torch.Tensor:
    """Row-wise argmax (first index on ties) of bf16 logits [B, V] -> int64 [B].

    Every id is in [0, V). NaN never wins: the winner is the first index of the
    largest non-NaN entry (-0.0 and +0.0 compare equal). A row with no winner
    (nothing above -inf: all -inf, all NaN or a mix of the two) returns 0."""
    _check(logits, torch.bfloat16, "logits")
    if logits.dim() != 2:
        raise ValueError("logits must be [B, V]")
    B, V = logits.shape
    out = torch.empty(B, dtype=torch.int64, device=logits.device)
    _ok(lib().p2pt_argmax(_p(logits), _p(out), B, V, _stream(logits)), "argmax")
    return out


def sample_(logits: torch.Tensor, ids: torch.Tensor, params: torch.Tensor) -> torch.Tensor:
    """In-place stochastic sampling (sample.hip): rows of bf16 ``logits`` [B, V]
    whose temperature is > 0 get ``ids[b]`` replaced by a draw from
    softmax(logits / T) after top-k and top-p filtering; greedy rows (T <= 0)
    keep the id already there. ``params``: int64 [5, >= B] (contiguous; column
    b for row b) — float32 bits of T, top_k (<= 0 off), float32 bits of top_p
    (>= 1 off), seed, counter (see ``pack_sampling``)."""
    return _sample(logits, ids, params, 5)


def sample_minp_(logits: torch.Tensor, ids: torch.Tensor, params: torch.Tensor) -> torch.Tensor:
    """``sample_`` with a min_p cut after top-k and top-p (sample.hip's
    ``MINP`` instantiation): ``params`` is int64 [6, >= B], rows 0..4 as
    ``sample_`` takes them and row 5 the float32 bits of ln(min_p) (-inf: off;
    see ``pack_sampling``'s ``min_p``). With z = logits / T and m its row
    maximum, a token stays iff z >= fl32(m + ln(min_p)), i.e. iff its
    probability is at least min_p times the most likely token's."""
    return _sample(logits, ids, params, 6)


def _sample(logits, ids, params, n_params: int):
    """The checks and the launch of ``sample_`` (5 params rows) and ``sample_minp_`` (6)."""
    _check(logits, torch.bfloat16, "logits")
    _check(ids, torch.int64, "ids", logits.device)
    _check(params, torch.int64, "params", logits.device)
    if logits.dim() != 2 or ids.shape != (logits.shape[0],) or params.dim() != 2 or params.shape[0] != n_params:
        raise ValueError(f"need logits [B, V], ids [B], params [{n_params}, >= B]")
    B, V = logits.shape
    if params.shape[1] < B:
        raise ValueError("params need a column per row")
    fn = lib().p2pt_sample if n_params == 5 else lib().p2pt_sample_minp
    _ok(fn(_p(logits), _p(ids), _p(params), B, params.shape[1], V, _stream(logits)), "sample")
    return ids


def logprobs_(logits: torch.Tensor, ids: torch.Tensor, want: torch.Tensor, out_lp: torch.Tensor,
              out_ids: torch.Tensor) -> None:
    """Log-probabilities under softmax(logits) (logprobs.hip), for the rows of
    bf16 ``logits`` [B, V >= 32] that ask: ``want`` (int64 [>= B]) is 0 for a row
    that is off — its outputs are left as they were — and 1 + N for the chosen
    token plus the top N (N in 0..MAX_TOP_LOGPROBS; larger values count as the
    maximum, so callers clamp). ``out_lp`` (float32 [B, 21]): column 0 the
    logprob of ``ids[b]`` (int64 [B], the id chosen after the sampler, wherever
    it ranks), columns 1..N the top N, descending. ``out_ids`` (int32 [B, 20]):
    their ids, ordered by (bf16 value descending, id ascending). The
    distribution is the model's own: temperature, top-k and top-p play no part."""
    _check(logits, torch.bfloat16, "logits")
    _check(ids, torch.int64, "ids", logits.device)
    _check(want, torch.int64, "want", logits.device)
    _check(out_lp, torch.float32, "out_lp", logits.device)
    _check(out_ids, torch.int32, "out_ids", logits.device)
    if logits.dim() != 2 or ids.shape != (logits.shape[0],) or want.dim() != 1:
        raise ValueError("need logits [B, V], ids [B], want [>= B]")
    B, V = logits.shape
    if B < 1 or V < 32:
        raise ValueError("need B >= 1 and V >= 32")
    if want.shape[0] < B:
        raise ValueError("want needs an entry per row")
    if out_lp.shape != (B, MAX_TOP_LOGPROBS + 1) or out_ids.shape != (B, MAX_TOP_LOGPROBS):
        raise ValueError(f"need out_lp [B, {MAX_TOP_LOGPROBS + 1}] and out_ids [B, {MAX_TOP_LOGPROBS}]")
    _ok(lib().p2pt_logprobs(_p(logits), _p(ids), _p(want), _p(out_lp), _p(out_ids), B, V, _stream(logits)),
        "logprobs")


def _penalty_tables(state, bias_n, bias_ids, bias_val):
    """Shape, dtype and device checks of the penalty state shared by ``penalize_`` and ``penalty_reset_``."""
    _check(state, torch.int32, "state")
    dev = state.device
    _check(bias_n, torch.int32, "bias_n", dev)
    _check(bias_ids, torch.int32, "bias_ids", dev)
    _check(bias_val, torch.float32, "bias_val", dev)
    if state.dim() != 2 or state.shape[0] < 1 or state.shape[1] < 32:
        raise ValueError(f"state must be [n_slots >= 1, V >= 32], got {tuple(state.shape)}")
    n_slots, V = state.shape
    if bias_n.shape != (n_slots,) or bias_ids.shape != (n_slots, MAX_LOGIT_BIAS) or bias_val.shape != bias_ids.shape:
        raise ValueError(f"need bias_n [{n_slots}], bias_ids and bias_val [{n_slots}, {MAX_LOGIT_BIAS}]")
    if V % 8 == 0 and state.data_ptr() % 16:
        raise ValueError("state must be 16-byte aligned")
    return n_slots, V


def _check_rows(name: str, in_place: bool, x, work, ids, tok, dec, slot) -> None:
    """The row arguments ``penalize_`` and ``guide_`` share, against their checked first argument ``x`` (bf16
    [B, V], called ``name``): ``work`` bf16 of x's shape, apart from x (``in_place``: or x itself), both 16-byte
    aligned when V % 8 == 0; ``ids`` and ``tok`` int64 [B]; ``dec`` and ``slot`` int64 [>= B]."""
    dev, (B, V) = x.device, x.shape
    _check(work, torch.bfloat16, "work", dev)
    for n, t in (("ids", ids), ("tok", tok), ("dec", dec), ("slot", slot)):
        _check(t, torch.int64, n, dev)
    if work.shape != x.shape:
        raise ValueError(f"work must be {tuple(x.shape)}, got {tuple(work.shape)}")
    lo, hi = x.data_ptr(), x.data_ptr() + x.numel() * 2
    if not (in_place and work.data_ptr() == lo) and work.data_ptr() < hi and lo < work.data_ptr() + work.numel() * 2:
        raise ValueError(f"work must be {name} itself or must not overlap it" if in_place else
                         f"work must not overlap {name} (the raw {name} are never written)")
    if ids.shape != (B,) or tok.shape != (B,):
        raise ValueError("ids and tok must be [B]")
    if dec.dim() != 1 or slot.dim() != 1 or dec.shape[0] < B or slot.shape[0] < B:
        raise ValueError("dec and slot need an entry per row")
    if V % 8 == 0 and (x.data_ptr() % 16 or work.data_ptr() % 16):
        raise ValueError(f"{name} and work must be 16-byte aligned")


PENALTY_ON = 1  # flags word of a ``penalize_`` params column: bit 0 = the row is on


def pack_penalties(repetition: float, frequency: float, presence: float, on: bool = True) -> list[int]:
    """One params column for ``penalize_``."""
    return [f32_bits(repetition), f32_bits(frequency), f32_bits(presence), PENALTY_ON if on else 0]


def penalize_(logits: torch.Tensor, work: torch.Tensor, ids: torch.Tensor, tok: torch.Tensor, dec: torch.Tensor,
              slot: torch.Tensor, params: torch.Tensor, state: torch.Tensor, bias_n: torch.Tensor,
              bias_ids: torch.Tensor, bias_val: torch.Tensor) -> torch.Tensor:
    """Repetition / frequency / presence penalties and logit_bias ahead of the
    sampler (penalty.hip), one workgroup per row of bf16 ``logits`` [B, V >= 32],
    which is never written. ``params``: int64 [4, >= B] (column b for row b; see
    ``pack_penalties``): float32 bits of repetition (1 off), frequency (0 off)
    and presence (0 off), then a flags word, 0 = the row is off. An off row
    gets ``work[b]`` (bf16 [B, V], another buffer than ``logits``) as a
    bit-for-bit copy and nothing else. A row that is on reads the counts of its
    slot ``slot[b]`` (int64 [>= B]; a slot outside ``state`` turns the row off)
    from ``state`` (int32 [n_slots, V]: bits 0..29 times generated, bit 30 "in
    the prompt"); if ``dec[b]`` (int64 [>= B]) is non-zero its input token
    ``tok[b]`` (int64 [B]) counts once more and the incremented word is written
    back. Seen ids (count > 0 or prompt bit) get x > 0 ? x / rep : x * rep, then
    every id x -= freq * count and x -= pres * (count > 0), in fp32, rounded
    to bf16 into ``work``; then the slot's ``bias_n[s]`` (int32 [n_slots])
    entries of ``bias_ids`` / ``bias_val`` (int32 / float32 [n_slots, 300]) are
    added to the stored values; then ``ids[b]`` (int64 [B], in place) becomes the
    argmax of the stored row (lowest id on ties, NaN never wins, 0 without a
    winner). Returns ``work``."""
    _check(logits, torch.bfloat16, "logits")
    dev = logits.device
    _check(params, torch.int64, "params", dev)
    n_slots, V = _penalty_tables(state, bias_n, bias_ids, bias_val)
    if state.device != dev:
        raise ValueError(f"state on {state.device}, expected {dev}")
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] != V:
        raise ValueError(f"logits must be [B >= 1, {V}] (state's vocabulary), got {tuple(logits.shape)}")
    B = logits.shape[0]
    if params.dim() != 2 or params.shape[0] != 4 or params.shape[1] < B:
        raise ValueError("params must be [4, >= B]")
    _check_rows("logits", False, logits, work, ids, tok, dec, slot)
    _ok(lib().p2pt_penalize(_p(logits), _p(work), _p(ids), _p(tok), _p(dec), _p(slot), _p(params), params.shape[1],
                            _p(state), n_slots, _p(bias_n), _p(bias_ids), _p(bias_val), B, V, _stream(logits)),
        "penalize")
    return work


def penalty_reset_(state: torch.Tensor, slot: int, prompt_ids: torch.Tensor, bias_n: torch.Tensor,
                   bias_ids: torch.Tensor, bias_val: torch.Tensor, bias: torch.Tensor | None = None) -> None:
    """Admission of a request into ``slot`` of the penalty state (penalty.hip;
    see ``penalize_`` for the tables): the slot's ``state`` row is zeroed, bit 30
    is set for every id of ``prompt_ids`` (int32 [n >= 1] on the device; ids
    outside [0, V) are ignored) and the slot's bias list becomes ``bias``: None
    for an empty one, or int32 [2, k <= 300] on the device, ids in row 0 and the
    float32 bits of their values in row 1 (the caller keeps the ids distinct).
    A clear and one launch on the current stream: no sync, no allocation, other
    slots untouched. Never captured."""
    n_slots, V = _penalty_tables(state, bias_n, bias_ids, bias_val)
    dev = state.device
    if not _int_in(slot, 0, n_slots):
        raise ValueError(f"slot must be an int in [0, {n_slots}), got {slot!r}")
    _check(prompt_ids, torch.int32, "prompt_ids", dev)
    if prompt_ids.dim() != 1 or prompt_ids.shape[0] < 1:
        raise ValueError("prompt_ids must be [n >= 1]")
    k = 0
    if bias is not None:
        _check(bias, torch.int32, "bias", dev)
        if bias.dim() != 2 or bias.shape[0] != 2 or not 1 <= bias.shape[1] <= MAX_LOGIT_BIAS:
            raise ValueError(f"bias must be int32 [2, 1..{MAX_LOGIT_BIAS}] (ids; float32 bits), got {tuple(bias.shape)}")
        k = bias.shape[1]
    _ok(lib().p2pt_penalty_reset(_p(state), n_slots, V, slot, _p(prompt_ids), prompt_ids.shape[0],
                                 _p(bias_n), _p(bias_ids), _p(bias_val), _p(bias), k, _stream(state)),
        "penalty_reset")


def _guide_tables(base, cur, arena):
    """Shape, dtype and device checks of the guide state shared by ``guide_`` and ``guide_reset_``."""
    _check(arena, torch.int16, "arena")
    dev = arena.device
    _check(base, torch.int32, "base", dev)
    _check(cur, torch.int32, "cur", dev)
    if arena.dim() != 2 or arena.shape[0] < 1 or arena.shape[1] < 32:
        raise ValueError(f"arena must be [arena_states >= 1, V >= 32], got {tuple(arena.shape)}")
    if arena.shape[0] > 32767:
        raise ValueError(f"arena holds at most 32767 states (its entries are int16), got {arena.shape[0]}")
    if base.dim() != 1 or base.shape[0] < 1 or cur.shape != base.shape:
        raise ValueError(f"base and cur must be [n_slots >= 1], got {tuple(base.shape)} and {tuple(cur.shape)}")
    if arena.shape[1] % 8 == 0 and arena.data_ptr() % 16:
        raise ValueError("arena must be 16-byte aligned")
    return base.shape[0], arena.shape[0], arena.shape[1]


def guide_(x: torch.Tensor, work: torch.Tensor, ids: torch.Tensor, tok: torch.Tensor, dec: torch.Tensor,
           slot: torch.Tensor, base: torch.Tensor, cur: torch.Tensor, arena: torch.Tensor) -> torch.Tensor:
    """Guided decoding ahead of the sampler (guide.hip), one workgroup per row
    of bf16 ``x`` [B, V >= 32]. ``arena`` (int16 [arena_states, V]) holds token
    automata one after the other: ``arena[base + c][t]`` is the state after
    token t in state c of the table that starts at arena row ``base``, -1 when t
    is not allowed. Row b belongs to slot ``slot[b]`` (int64 [>= B]); the
    slot's table starts at ``base[s]`` (int32 [n_slots]; negative, like a slot
    outside ``base`` or a state outside the arena, turns the row off) and its
    state is ``cur[s]`` (int32 [n_slots]). An off row gets ``work[b]`` (bf16
    [B, V]: ``x`` itself, or a buffer that does not overlap it) as a bit-for-bit
    copy and nothing else. A row that is on first advances: if ``dec[b]``
    (int64 [>= B]) is non-zero, ``t = arena[base + cur][tok[b]]`` (``tok``:
    int64 [B]) and ``cur[s] = t`` when t >= 0; then ``work[b][v]`` is
    ``x[b][v]`` where ``arena[base + cur][v] >= 0`` and -inf elsewhere; then
    ``ids[b]`` (int64 [B], in place) becomes the argmax of the stored row (lowest
    id on ties, NaN never wins, 0 without a winner). Rows that are on must
    belong to different slots. Returns ``work``."""
    _check(x, torch.bfloat16, "x")
    n_slots, n_states, V = _guide_tables(base, cur, arena)
    if arena.device != x.device:
        raise ValueError(f"arena on {arena.device}, expected {x.device}")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] != V:
        raise ValueError(f"x must be [B >= 1, {V}] (the arena's vocabulary), got {tuple(x.shape)}")
    B = x.shape[0]
    _check_rows("x", True, x, work, ids, tok, dec, slot)
    _ok(lib().p2pt_guide(_p(x), _p(work), _p(ids), _p(tok), _p(dec), _p(slot), _p(base), _p(cur), n_slots, _p(arena),
                         n_states, B, V, _stream(x)), "guide")
    return work


def guide_reset_(base: torch.Tensor, cur: torch.Tensor, arena: torch.Tensor, slot: int, first: int) -> None:
    """Admission of a request into ``slot`` of the guide state (guide.hip; see
    ``guide_`` for the tables): ``base[slot] = first``, the arena row its table
    starts at (-1: the slot is not guided), and ``cur[slot] = 0``. One launch on
    the current stream: no sync, no allocation, other slots untouched. Never
    captured."""
    n_slots, n_states, _ = _guide_tables(base, cur, arena)
    for name, v, lo, hi in (("slot", slot, 0, n_slots), ("first", first, -1, n_states)):
        if not _int_in(v, lo, hi):
            raise ValueError(f"{name} must be an int in [{lo}, {hi}), got {v!r}")
    _ok(lib().p2pt_guide_reset(_p(base), _p(cur), n_slots, slot, first, n_states, _stream(base)), "guide_reset")


def kv_copy_(k_cache: torch.Tensor, v_cache: torch.Tensor, jobs) -> None:
    """In-place slot-to-slot copy of K/V rows (kv_copy.hip). The caches are
    bf16 [n_layers, n_slots, max_seq, Hkv, D]; ``jobs`` is a list of 1..8
    ``(src, dst, n)``: rows [0, n) of slot ``src`` go to slot ``dst`` in every
    layer, for K and V, in ONE launch on the current stream (the triples travel
    in the kernel arguments: no device table, no copy, no sync). Within a call
    no slot may be both a source and a destination and no destination may
    repeat, so the result does not depend on the order of the jobs; n == 0
    moves nothing. Nothing outside the destination rows is written."""
    _check(k_cache, torch.bfloat16, "k_cache")
    _check(v_cache, torch.bfloat16, "v_cache", k_cache.device)
    if k_cache.dim() != 5 or v_cache.dim() != 5:
        raise ValueError("caches must be [n_layers, n_slots, max_seq, Hkv, D]")
    if k_cache.shape != v_cache.shape:
        raise ValueError(f"cache shapes differ: {tuple(k_cache.shape)} and {tuple(v_cache.shape)}")
    L, n_slots, max_seq, Hkv, D = k_cache.shape
    if (Hkv * D * 2) % 16 or Hkv * D == 0 or L == 0 or max_seq == 0:
        raise ValueError("a cache row (Hkv * D bf16) must be a non-empty multiple of 16 bytes")
    jobs = list(jobs)
    if not 1 <= len(jobs) <= MAX_KV_COPY_JOBS:
        raise ValueError(f"need 1..{MAX_KV_COPY_JOBS} jobs, got {len(jobs)}")
    flat, srcs, dsts = [], set(), set()
    for job in jobs:
        if len(job) != 3 or not all(isinstance(x, int) and not isinstance(x, bool) for x in job):
            raise TypeError(f"a job is (src, dst, n) of ints, got {job!r}")
        src, dst, n = job
        if not (0 <= src < n_slots and 0 <= dst < n_slots):
            raise ValueError(f"job {job!r}: slots must be in [0, {n_slots})")
        if not 0 <= n <= max_seq:
            raise ValueError(f"job {job!r}: rows must be in [0, {max_seq}]")
        if src == dst:
            raise ValueError(f"job {job!r}: source and destination are the same slot")
        if dst in dsts:
            raise ValueError(f"slot {dst} is a destination twice")
        srcs.add(src)
        dsts.add(dst)
        flat += [src, dst, n]
    if srcs & dsts:
        raise ValueError(f"slots {sorted(srcs & dsts)} are both a source and a destination in one call")
    arr = (ctypes.c_int * len(flat))(*flat)
    _ok(lib().p2pt_kv_copy(_p(k_cache), _p(v_cache), L, n_slots, max_seq, Hkv * D, len(jobs), arr,
                           _stream(k_cache)), "kv_copy")


EMBED_FIRST, EMBED_LAST = 1, 2  # a job's flags: first / last piece of its sequence


def embed_pool_(resid: torch.Tensor, norm_weight: torch.Tensor, acc: torch.Tensor, out: torch.Tensor, jobs,
                eps: float) -> None:
    """Pool rows of the fused step's final residual into embeddings
    (embed_pool.hip). ``resid`` is bf16 [rows <= 64, dim], ``norm_weight`` bf16
    (dim,), ``acc`` fp32 [n_acc, dim] (running sums of sequences that span
    several steps), ``out`` fp32 [n_out, dim]; ``jobs`` is a list of 1..16
    ``(row0, n, acc, flags, out_row)`` of plain ints, all in ONE launch on the
    current stream (the jobs travel in the kernel arguments: no device table,
    no copy, no sync). A job adds rmsnorm(resid[r]) * norm_weight for r in
    [row0, row0 + n), in fp32 and in row order, to a sum that starts at zero
    (``flags & EMBED_FIRST``) or at ``acc[acc]``; with ``flags & EMBED_LAST``
    the sum, L2-normalised (zeros when its norm is 0 or not finite), goes to
    ``out[out_row]`` and ``acc`` is not written, otherwise the sum goes back to
    ``acc[acc]`` and ``out_row`` must be -1. No ``acc`` index and no
    ``out_row`` may appear twice in a call. Nothing else is written."""
    _check(resid, torch.bfloat16, "resid")
    dev = resid.device
    _check(norm_weight, torch.bfloat16, "norm_weight", dev)
    _check(acc, torch.float32, "acc", dev)
    _check(out, torch.float32, "out", dev)
    if resid.dim() != 2 or not 1 <= resid.shape[0] <= MAX_ROWS:
        raise ValueError(f"resid must be [rows <= {MAX_ROWS}, dim], got {tuple(resid.shape)}")
    rows, dim = resid.shape
    if dim < 8 or dim % 8 or dim > 16384:
        raise ValueError("dim must be a multiple of 8 and <= 16384")
    if norm_weight.shape != (dim,):
        raise ValueError(f"norm_weight shape {tuple(norm_weight.shape)} != ({dim},)")
    if acc.dim() != 2 or acc.shape[1] != dim or acc.shape[0] < 1 or out.dim() != 2 or out.shape[1] != dim or \
            out.shape[0] < 1:
        raise ValueError(f"acc and out must be [n >= 1, {dim}], got {tuple(acc.shape)} and {tuple(out.shape)}")
    if any(t.data_ptr() % 16 for t in (resid, norm_weight, acc, out)):
        raise ValueError("resid, norm_weight, acc and out must be 16-byte aligned")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 <= eps < float("inf"):
        raise ValueError(f"eps must be a finite number >= 0, got {eps!r}")
    jobs = list(jobs)
    if not 1 <= len(jobs) <= MAX_EMBED_JOBS:
        raise ValueError(f"need 1..{MAX_EMBED_JOBS} jobs, got {len(jobs)}")
    flat, accs, outs = [], set(), set()
    for job in jobs:
        if not isinstance(job, (tuple, list)) or len(job) != 5 or \
                not all(isinstance(x, int) and not isinstance(x, bool) for x in job):
            raise TypeError(f"a job is (row0, n, acc, flags, out_row) of ints, got {job!r}")
        row0, n, a, flags, out_row = job
        if n < 1 or row0 < 0 or row0 + n > rows:
            raise ValueError(f"job {job!r}: rows [row0, row0 + n) must be non-empty and inside [0, {rows})")
        if not 0 <= a < acc.shape[0]:
            raise ValueError(f"job {job!r}: acc must be in [0, {acc.shape[0]})")
        if not 0 <= flags <= (EMBED_FIRST | EMBED_LAST):
            raise ValueError(f"job {job!r}: flags must be a combination of EMBED_FIRST and EMBED_LAST")
        if flags & EMBED_LAST:
            if not 0 <= out_row < out.shape[0]:
                raise ValueError(f"job {job!r}: out_row must be in [0, {out.shape[0]})")
            if out_row in outs:
                raise ValueError(f"out row {out_row} appears twice")
            outs.add(out_row)
        elif out_row != -1:
            raise ValueError(f"job {job!r}: a job without EMBED_LAST writes no out row (out_row must be -1)")
        if a in accs:
            raise ValueError(f"acc row {a} appears twice")
        accs.add(a)
        flat += [row0, n, a, flags, out_row]
    arr = (ctypes.c_int * len(flat))(*flat)
    _ok(lib().p2pt_embed_pool(_p(resid), rows, dim, _p(norm_weight), _p(acc), acc.shape[0], _p(out), out.shape[0],
                              float(eps), len(jobs), arr, _stream(resid)), "embed_pool")


def f32_bits(x: float) -> int:
    """The float32 bit pattern of x as a non-negative int (the sampler's params encoding)."""
    import struct
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def ln_min_p(min_p: float) -> float:
    """ln(min_p) as ``sample_minp_`` takes it: computed in float64 (the caller rounds it to float32 once, in
    ``f32_bits``); 0 maps to -inf, which switches the cut off. ``min_p`` outside [0, 1] (NaN and bools included)
    raises."""
    if isinstance(min_p, bool) or not isinstance(min_p, (int, float)) or not 0.0 <= min_p <= 1.0:
        raise ValueError(f"min_p must be a number in [0, 1], got {min_p!r}")
    return math.log(min_p) if min_p > 0.0 else -math.inf


def pack_sampling(temperature: float, top_k: int, top_p: float, seed: int, counter: int,
                  min_p: float | None = None) -> list[int]:
    """One params column for ``sample_``; with ``min_p`` (a number in [0, 1], 0 = off) the six values of a
    ``sample_minp_`` column: the float32 bits of ln(min_p) follow."""
    col = [f32_bits(temperature), int(top_k), f32_bits(top_p), int(seed) & 0x7FFFFFFFFFFFFFFF,
           int(counter) & 0x7FFFFFFFFFFFFFFF]
    return col if min_p is None else col + [f32_bits(ln_min_p(min_p))]


def skinny_gemm(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """bf16(x @ w.T) for a few rows on MFMA (decode-shaped GEMM). x: [M<=64, K]; w: [N, K], each below 2 GiB:
    the kernel addresses both with 32-bit byte offsets, and a larger operand would read as zeros without a fault.
    The shapes are judged first, from the shapes alone, so a refusal needs no device."""
    if not isinstance(x, torch.Tensor) or not isinstance(w, torch.Tensor):
        raise TypeError("x and w must be tensors")
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise ValueError("shapes must be x [M, K], w [N, K]")
    M, K = x.shape
    N = w.shape[0]
    if not 1 <= M <= MAX_ROWS or N % 32 or K % 32:
        raise ValueError(f"need 1 <= M <= {MAX_ROWS}, N % 32 == 0, K % 32 == 0")
    if max(M, N) * K * 2 >= GEMM_OPERAND_LIMIT:
        raise ValueError(f"x [{M}, {K}] and w [{N}, {K}] must each stay below 2 GiB (32-bit byte offsets)")
    _check(x, torch.bfloat16, "x")
    _check(w, torch.bfloat16, "w", x.device)
    out = torch.empty(M, N, dtype=x.dtype, device=x.device)
    _ok(lib().p2pt_skinny_gemm(_p(x), _p(w), _p(out), M, N, K, _stream(x)), "skinny_gemm")
    return out


def quantize_weight_fp8(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """One GEMM weight ``w`` (fp32 [N, K], as it sits in the fused table: folded and interleaved) to the FP8 weight
    format (docs/WEIGHT_FP8.md): ``(q, scale)`` with ``scale[n] = max_k |w[n][k]| / 448`` (fp32; 1.0 for a row
    whose maximum is zero or so small that the division underflows to zero) and ``q[n][k]`` the OCP e4m3fn byte,
    round to nearest even, of ``w[n][k] / scale[n]`` (the division in fp32), as ``torch.float8_e4m3fn``. A row's
    largest magnitude lands on +-448, so nothing saturates and no NaN byte is written. Non-finite weights are
    refused. Plain torch on ``w``'s device: runs without a GPU."""
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 2:
        raise TypeError("quantize_weight_fp8 takes an fp32 [N, K] tensor (fold and quantise in fp32, not through bf16)")
    if not bool(torch.isfinite(w).all()):
        raise ValueError("non-finite weight (NaN or inf): refusing to quantise it to FP8")
    scale = w.abs().amax(1) / E4M3_MAX
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    # |w / scale| <= 448 (1 + 2^-23): below 464, where the cast's rounding to nearest even still gives 448.
    q = (w / scale[:, None]).to(torch.float8_e4m3fn)
    return q.contiguous(), scale.contiguous()


def dequantize_weight_fp8(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``q * scale`` per row in fp32: the weight the FP8 kernels compute with (one fp32 rounding per element, none
    when the scales are powers of two)."""
    if q.dtype == torch.uint8:
        q = q.view(torch.float8_e4m3fn)
    return q.float() * scale.float()[:, None]


def _check_mxfp4_input(w):
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 2 or w.shape[1] % MXFP4_BLOCK:
        raise TypeError(f"quantize_weight_mxfp4 takes an fp32 [N, K] tensor with K a multiple of {MXFP4_BLOCK} (fold and "
                        "quantise in fp32, not through bf16)")
    if not bool(torch.isfinite(w).all()):
        raise ValueError("non-finite weight (NaN or inf): refusing to quantise it to MXFP4")


def pack_weight_mxfp4(codes: torch.Tensor) -> torch.Tensor:
    """Nibble codes ``[N][K]`` (uint8, 0..15: bit 3 the sign, bits 0..2 the index into ``E2M1_VALUES``) to the bytes
    ``[N][K / 2]`` the kernel loads, in the physical order ``WeightTable`` states: byte j of a row holds element 2 j in
    its low nibble and element 2 j + 1 in its high nibble. The one function that makes that order."""
    if not isinstance(codes, torch.Tensor) or codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[1] % 2:
        raise TypeError("pack_weight_mxfp4 takes uint8 nibble codes [N, K] with K even")
    if codes.numel() and int(codes.max()) > 15:
        raise ValueError("a nibble code is 0..15")
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


def unpack_weight_mxfp4(packed: torch.Tensor) -> torch.Tensor:
    """The inverse of ``pack_weight_mxfp4``: bytes ``[N][K / 2]`` to nibble codes ``[N][K]``."""
    if not isinstance(packed, torch.Tensor) or packed.dtype != torch.uint8 or packed.dim() != 2:
        raise TypeError("unpack_weight_mxfp4 takes uint8 bytes [N, K / 2]")
    return torch.stack([packed & 15, packed >> 4], 2).reshape(packed.shape[0], -1).contiguous()


def quantize_weight_mxfp4(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """One GEMM weight ``w`` (fp32 [N, K], K a multiple of 32, as it sits in the fused table: folded and interleaved)
    to OCP Microscaling MXFP4 (docs/WEIGHT_MXFP4.md): ``(bytes, scales)``, uint8 ``[N][K / 2]`` in
    ``pack_weight_mxfp4``'s order and uint8 ``[N][K / 32]``. Plain torch on ``w``'s device: runs without a GPU.

    Blocks are 32 consecutive elements of a row. A block's scale byte E (e8m0: the scale is 2^(E - 127)) is
    ``E - 127 = floor(log2(amax)) - 2`` of the block's largest magnitude, so amax / 2^(E - 127) lies in [4, 8) and
    the largest e2m1 magnitude, 6 = 1.5 * 2^2, shares amax's binade. E is clamped to [2, 252], the range in which
    every decoded value is a normal bf16 number: the smallest non-zero one is 0.5 * 2^(E - 127) >= 2^-126 (bf16's
    smallest normal) iff E >= 2, and the largest, 6 * 2^(E - 127) < 2^(E - 124), is below 2^128 iff E <= 252. The
    upper end binds for no fp32 input (amax < 2^128 gives E <= 252 by the rule itself); the lower one holds blocks
    with amax < 2^-123 at E = 2, where their elements round towards zero like any small element. 255 (e8m0's NaN) is
    never emitted. An all-zero block (-0.0 included) gets E = 127 and zero nibbles.

    An element is x / 2^(E - 127) (exact in fp32: a power-of-two factor, and the quotient of anything that does not
    round to zero is normal) rounded to the nearest e2m1 magnitude {0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the even
    mantissa (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), saturating at 6, with the sign
    in bit 3; what rounds to zero is the nibble 0, never 8.

    Error, per element, with s = 2^(E - 127) and y = |x| / s < 8: |dequant - x| <= s / 4 for y <= 2 (steps of 0.5),
    s / 2 for y <= 4 (steps of 1), s for y <= 6 (steps of 2), and y - 6 < 2 in units of s above 6, where the value
    saturates: the top binade is the worst case, and |dequant - x| < 2 s <= amax / 2 in every block whose E the lower
    clamp did not raise (s <= amax / 4 there; a block held at E = 2 has y <= 2 and so the s / 4 bound, 2^-127).
    Non-finite weights are refused."""
    _check_mxfp4_input(w)
    N, K = w.shape
    blocks = w.reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = blocks.abs().amax(2)
    _, e = torch.frexp(amax)  # amax = m 2^e with m in [0.5, 1): floor(log2(amax)) = e - 1, subnormals included
    E = torch.where(amax > 0, (e - 3 + 127).clamp(MXFP4_EXP_MIN, MXFP4_EXP_MAX), torch.full_like(e, 127))
    y = torch.ldexp(blocks, (127 - E)[:, :, None].to(torch.int32)).abs()
    code = ((y > 0.25).to(torch.uint8) + (y >= 0.75) + (y > 1.25) + (y >= 1.75) + (y > 2.5) + (y >= 3.5) + (y > 5.0))
    code = code.to(torch.uint8)
    code = code | (((blocks < 0) & (code > 0)).to(torch.uint8) << 3)
    return pack_weight_mxfp4(code.reshape(N, K)), E.to(torch.uint8).contiguous()


def dequantize_weight_mxfp4(packed: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """``e2m1(nibble) * 2^(E - 127)`` in fp32 ``[N][K]``: the weight the MXFP4 kernels compute with. Exact, and for
    the scales ``quantize_weight_mxfp4`` emits every value is a bf16 number, so ``.to(torch.bfloat16)`` is exact too."""
    codes = unpack_weight_mxfp4(packed)
    N, K = codes.shape
    if not isinstance(scales, torch.Tensor) or scales.dtype != torch.uint8 or \
            tuple(scales.shape) != (N, K // MXFP4_BLOCK) or K % MXFP4_BLOCK:
        raise TypeError(f"scales must be uint8 [N, K / {MXFP4_BLOCK}] e8m0 bytes of the weight's blocks")
    mag = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=codes.device)[(codes & 7).long()]
    val = torch.where((codes & 8) != 0, -mag, mag).reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    return torch.ldexp(val, (scales.to(torch.int32) - 127)[:, :, None]).reshape(N, K)


class FusedLlamaDecoder:
    """Host handle for the fused decode step (decode_fused.hip): 5 kernels per layer + 3
    (6 per layer with ``dims.qk_norm``: the per-head q/k RMSNorm of Qwen3 runs in a kernel of its own;
    with ``dims.qkv_bias`` the q/k/v bias of Qwen2 is added in the QKV GEMM's epilogue, still 5; with
    ``dims.rope_table`` the kernel that rotates reads its frequencies from the table's ``inv_freq`` entry, and the
    kernel count does not change; with ``dims.kv_fp8`` the caches are ``torch.float8_e4m3fn`` (or uint8), one OCP
    e4m3 byte per element at scale 1 (or with ``kv_scales``, below), written by the _KV8 epilogues / ``k_qknorm_rope`` variant and read by
    ``k_attn<D, G, true>``: the same kernel count again).

    ``weights`` is laid out as ``WeightTable(dims, weight_fp8, weight_format)`` says, and every entry is checked
    against it. ``weight_format`` (``as_weight_format``: a ``WeightFormat`` or "bf16", "fp8", "mxfp4") in place of
    ``weight_fp8``; "mxfp4" (docs/WEIGHT_MXFP4.md, ``quantize_weight_mxfp4``) has each layer's four GEMM weights as
    MXFP4 bytes with e8m0 block scales, run by the ``k_skinny<.., W8 = 2>`` instantiations, and an FP8 LM head.
    ``weight_fp8``: the five GEMM weights as OCP e4m3 bytes with one fp32 scale per output row, each (N,) in the
    row order of its weight (docs/WEIGHT_FP8.md, ``quantize_weight_fp8``). Every ``k_skinny`` is then its FP8-weight
    instantiation; the kernel count, ``step_plan`` and the workspace are the same.

    ``kv_scales`` (with ``dims.kv_fp8`` only): fp32 ``[4, n_layers, Hkv]`` on the caches' device, the reciprocals
    1 / k_scale and 1 / v_scale, then k_scale and v_scale (``models.kv_scales.KvScales.table``), every entry finite
    and > 0. A stored byte is then ``e4m3(clamp(x * (1 / s)))`` of its layer's and KV head's scale, and ``k_attn``
    undoes the scale (K's in the score scale, V's in the final normalisation). It is no part of ``dims`` or of the
    weight table: the plans, the table and the workspace are those of the model without scales, and None runs the
    step exactly as before.

    ``windows``: None, or one int per layer: 0 for full attention, W >= 1 for a sliding window (the layer's rows
    attend to their last W positions, their own included: docs/SLIDING_WINDOW.md). Such a layer runs
    ``k_attn<D, G, KV8, true>`` on ``window_plan``'s slots. Like the scales it is no part of ``dims``, of a plan or of
    the weight table, and None or all zeros runs the step exactly as before.

    Holds the weight pointer table and a zero-initialised workspace; ``step``
    validates the per-call tensors and launches on the current stream (capturable
    into a hipGraph: no host sync, no allocation, grids sized by the row count).
    """

    def __init__(self, dims: LlamaDims, weights: list, k_cache: torch.Tensor, v_cache: torch.Tensor,
                 weight_fp8: bool = False, kv_scales: torch.Tensor | None = None, windows=None, weight_format=None):
        self.dims = dims
        self.windows = check_windows(windows, dims.n_layers)
        self._windows = (ctypes.c_int * dims.n_layers)(*self.windows) if self.windows is not None else None
        self.weight_format = fmt = as_weight_format(weight_fp8, weight_format)
        self.weight_fp8 = fmt.layers == 1  # FP8 throughout
        self._wplan = WeightPlan(w8=int(self.weight_fp8))
        dev = k_cache.device
        # The cache dtype against dims.kv_fp8 first (a host-only check): a mismatch would have every kernel read
        # and write rows of the wrong width.
        if dims.kv_fp8 not in (0, 1):
            raise ValueError("dims.kv_fp8 must be 0 or 1")
        for name, c in (("k_cache", k_cache), ("v_cache", v_cache)):
            if dims.kv_fp8 and c.dtype not in KV_FP8_DTYPES:
                raise TypeError(f"{name}: dims.kv_fp8 is set, so the cache must be torch.float8_e4m3fn (or uint8), "
                                f"got {c.dtype}")
            if not dims.kv_fp8 and c.dtype in KV_FP8_DTYPES:
                raise TypeError(f"{name}: a {c.dtype} cache needs dims.kv_fp8 = 1")
        if dims.rope_table not in (0, 1):
            raise ValueError("dims.rope_table must be 0 or 1")
        if kv_scales is not None:
            if not dims.kv_fp8:
                raise ValueError("kv_scales need an FP8 cache (dims.kv_fp8 = 1): a bf16 KV cache has no scales")
            if not isinstance(kv_scales, torch.Tensor) or kv_scales.dtype != torch.float32 or \
                    tuple(kv_scales.shape) != (4, dims.n_layers, dims.Hkv):
                raise ValueError(f"kv_scales must be fp32 [4, {dims.n_layers}, {dims.Hkv}] (1 / k, 1 / v, k, v per layer "
                                 f"and KV head), got {getattr(kv_scales, 'dtype', type(kv_scales))} "
                                 f"{tuple(getattr(kv_scales, 'shape', ()))}")
        self.table = table = WeightTable(dims, weight_format=fmt)
        if len(weights) != len(table):
            raise ValueError(f"weight table: embed, final_norm, lm_head, "
                             + ("inv_freq, " if dims.rope_table else "") + f"then {table.per_layer} per layer "
                             "(wqkv, w_gate_up and lm_head with the preceding norm weight folded in"
                             + ("; q_norm and k_norm last)" if dims.qk_norm else
                                "; bqkv last)" if dims.qkv_bias else ")")
                             + ("; weight_fp8: then the fp32 row scales, lm_head's and four per layer"
                                if self.weight_fp8 else "")
                             + ("; mxfp4: then lm_head's fp32 row scales and four e8m0 block-scale tensors per layer"
                                if fmt.layers == 2 else ""))
        # Every entry's dtype and shape, from the description alone: a refusal here needs no device. A weight shorter
        # than dims says would be read past its end (k_skinny sizes its descriptors from dims, k_embed indexes vocab
        # rows). The norm slots the kernels do not read are held to (dim,) too.
        for e, t in zip(table, weights):
            name = label(e.name, e.layer)
            if not isinstance(t, torch.Tensor) or t.dtype not in e.dtypes:
                got = getattr(t, "dtype", type(t))
                if fmt.layers == 2 and e.dtypes == (torch.uint8,):
                    raise TypeError(f"{name}: the weight format is mxfp4, so "
                                    + ("the block scales must be e8m0 bytes (torch.uint8)" if e.name.endswith(" scale")
                                       else "the weight must be nibble bytes (torch.uint8)") + f", got {got}")
                if len(e.dtypes) > 1:
                    raise TypeError(f"{name}: weight_fp8 is set, so the weight must be torch.float8_e4m3fn (or uint8), "
                                    f"got {got}")
                if got == torch.float8_e4m3fn:
                    raise TypeError(f"{name} is {got}: an FP8 weight table needs weight_fp8=True")
                raise TypeError(f"{name}: expected {e.dtypes[0]}, got {got}")
            if tuple(t.shape) != e.shape:
                raise ValueError(f"{name} has shape {tuple(t.shape)}, not {e.shape}"
                                 + ("" if not e.name.endswith(" scale") else
                                    f": one e8m0 byte per {MXFP4_BLOCK}-element block" if e.dtypes == (torch.uint8,)
                                    else ": one fp32 scale per output row")
                                 + (": two nibbles per byte" if fmt.layers == 2 and e.name in LAYER_GEMMS else ""))
        L, Bmax, S, Hkv, D = k_cache.shape
        if (L, Bmax, S, Hkv, D) != (dims.n_layers, dims.max_batch, dims.max_seq, dims.Hkv, dims.D):
            raise ValueError("cache shape does not match dims")
        if v_cache.shape != k_cache.shape or v_cache.dtype != k_cache.dtype:
            raise ValueError("k_cache and v_cache must have the same shape and dtype")
        # From here on the device: where every tensor lives, contiguity, alignment, the RoPE table's values.
        # Alignment first (an address needs no device to be judged), then the device: where every tensor lives,
        # contiguity, the RoPE table's values.
        for e, t in zip(table, weights):
            if t.data_ptr() % e.align:
                raise ValueError(f"{label(e.name, e.layer)} must be {e.align}-byte aligned")
        for e, t in zip(table, weights):
            _check(t, t.dtype, label(e.name, e.layer), dev)
        if dims.rope_table:
            _check_inv_freq(weights[table.index("inv_freq")], dims.D, dev)
        for name, c in (("k_cache", k_cache), ("v_cache", v_cache)):
            _check(c, c.dtype if dims.kv_fp8 else torch.bfloat16, name, dev)
        if kv_scales is not None:
            _check(kv_scales, torch.float32, "kv_scales", dev)
            if not bool((torch.isfinite(kv_scales) & (kv_scales > 0)).all().item()):
                raise ValueError("kv_scales entries (and their reciprocals) must be finite and > 0")
        self.kv_scales = kv_scales  # keep alive
        nbytes = lib().p2pt_llama_ws_bytes(ctypes.byref(dims))
        if nbytes == 0:
            raise ValueError("model dims not supported by the fused decode kernels")
        self.weights = weights  # keep alive
        self._wptr = (ctypes.c_void_p * len(weights))(*[t.data_ptr() for t in weights])
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.k_cache, self.v_cache = k_cache, v_cache
        self.device = dev
        self._resid = None  # embed_pool's view of the workspace's resid buffer

    # Workspace buffers in the order p2pt_llama_ws_layout reports them.
    _WS_BUFFERS = (("resid", torch.bfloat16), ("q", torch.bfloat16), ("attn", torch.bfloat16), ("h", torch.bfloat16),
                   ("ss", torch.float32), ("part_o", torch.float32), ("part_ml", torch.float32),
                   ("am_val", torch.float32), ("am_idx", torch.int32), ("counters", torch.int32),
                   ("qkv", torch.bfloat16))

    def workspace_views(self) -> dict:
        """Typed, shaped views into the workspace (no copies; the layout comes from
        ``p2pt_llama_ws_layout``): what the last ``step`` left in each buffer.

        resid [64, dim], q [64, H, D], attn [64, H*D], h [64, ffn] (bf16);
        ss [parts, 64], part_o [64, H, nsplit, D], part_ml [64, H, nsplit, 2],
        am_val [blocks, 64] (fp32); am_idx [blocks, 64], counters [64*H] (int32);
        qkv [64, (H+2*Hkv)*D] (bf16): the raw QKV projection of a QK-norm model's
        last layer, as ``k_qknorm_rope`` read it ([0, ...] for other models).
        Read them after a stream sync; only the first B rows of a step are defined."""
        d = self.dims
        n = len(self._WS_BUFFERS)
        off, cnt = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
        if lib().p2pt_llama_ws_layout(ctypes.byref(d), off, cnt, n) != n:
            raise RuntimeError("workspace layout: buffer list out of step with decode_fused.hip")
        views = {}
        for (name, dtype), o, c in zip(self._WS_BUFFERS, off, cnt):
            size = torch.empty(0, dtype=dtype).element_size()
            if o % size or o + c * size > self.ws.numel():
                raise RuntimeError(f"workspace layout: {name} lies outside the workspace")
            views[name] = self.ws[o:o + c * size].view(dtype)
        M = MAX_ROWS
        shapes = {"resid": (M, d.dim), "q": (M, d.H, d.D), "attn": (M, d.H * d.D), "h": (M, d.ffn), "ss": (-1, M),
                  "part_o": (M, d.H, -1, d.D), "part_ml": (M, d.H, -1, 2), "am_val": (-1, M), "am_idx": (-1, M),
                  "counters": (M * d.H,), "qkv": (M if d.qk_norm else 0, (d.H + 2 * d.Hkv) * d.D)}
        return {name: v.view(*shapes[name]) for name, v in views.items()}

    def embed_pool(self, acc: torch.Tensor, out: torch.Tensor, jobs) -> None:
        """``embed_pool_`` over the rows the last ``step`` left in ``resid`` (the
        final residual of every row, prefill rows included), with the final-norm
        weight and this model's eps."""
        if self._resid is None:
            self._resid = self.workspace_views()["resid"]
        embed_pool_(self._resid, self.weights[self.table.index("final_norm")], acc, out, jobs, self.dims.eps)

    def step(self, tokens: torch.Tensor, pos: torch.Tensor, logits: torch.Tensor, ids: torch.Tensor,
             slots: torch.Tensor | None = None, emit_rows: int = 0) -> None:
        """One step over B <= 64 token rows (16-row MFMA tiles). Row b is token
        ``tokens[b]`` at cache position ``pos[b]`` of cache slot ``slots[b]``
        (default: slot b). Rows of one slot at consecutive positions are a prefill
        chunk (causal within the step). Only rows [0, emit_rows) get logits and
        ids (0: all): the LM head skips prefill rows that sample nothing."""
        d = self.dims
        _check(tokens, torch.int64, "tokens", self.device)
        _check(pos, torch.int32, "pos", self.device)
        _check(logits, torch.bfloat16, "logits", self.device)
        _check(ids, torch.int64, "ids", self.device)
        B = tokens.shape[0]
        if slots is not None:
            _check(slots, torch.int32, "slots", self.device)
            if slots.shape != (B,):
                raise ValueError("slots must be [B]")
        limit = MAX_ROWS if slots is not None else min(MAX_ROWS, d.max_batch)
        if not 0 <= emit_rows <= B:
            raise ValueError("emit_rows must be in 0..B")
        if not 1 <= B <= limit or pos.shape != (B,) or ids.shape != (B,):
            raise ValueError(f"rows must be 1..{limit} with matching pos/ids")
        if logits.shape != (B, d.vocab):
            raise ValueError("logits must be [B, vocab]")
        if self.weight_format.layers != self.weight_format.lm_head:  # MXFP4: only the _fmt entry point says so
            _ok(lib().p2pt_llama_decode_fmt(ctypes.byref(d), ctypes.byref(self.weight_format), _p(self.kv_scales),
                                            self._windows, self._wptr, _p(self.k_cache), _p(self.v_cache), _p(tokens),
                                            _p(pos), _p(slots), B, emit_rows, _p(self.ws), self.ws.numel(),
                                            _p(logits), _p(ids), _stream(tokens)), "llama_decode")
            return
        if self._windows is not None:
            _ok(lib().p2pt_llama_decode_win(ctypes.byref(d), ctypes.byref(self._wplan), _p(self.kv_scales),
                                            self._windows, self._wptr, _p(self.k_cache), _p(self.v_cache), _p(tokens),
                                            _p(pos), _p(slots), B, emit_rows, _p(self.ws), self.ws.numel(),
                                            _p(logits), _p(ids), _stream(tokens)), "llama_decode")
            return
        if self.kv_scales is not None:
            _ok(lib().p2pt_llama_decode_kv(ctypes.byref(d), ctypes.byref(self._wplan), _p(self.kv_scales), self._wptr,
                                           _p(self.k_cache), _p(self.v_cache), _p(tokens), _p(pos), _p(slots), B,
                                           emit_rows, _p(self.ws), self.ws.numel(), _p(logits), _p(ids),
                                           _stream(tokens)), "llama_decode")
            return
        if self.weight_fp8:
            _ok(lib().p2pt_llama_decode_w(ctypes.byref(d), ctypes.byref(self._wplan), self._wptr, _p(self.k_cache),
                                          _p(self.v_cache), _p(tokens), _p(pos), _p(slots), B, emit_rows,
                                          _p(self.ws), self.ws.numel(), _p(logits), _p(ids), _stream(tokens)),
                "llama_decode")
            return
        _ok(lib().p2pt_llama_decode(ctypes.byref(d), self._wptr, _p(self.k_cache), _p(self.v_cache), _p(tokens),
                                    _p(pos), _p(slots), B, emit_rows, _p(self.ws), self.ws.numel(), _p(logits),
                                    _p(ids), _stream(tokens)), "llama_decode")
