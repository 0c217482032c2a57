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
    only, with an FP8 LM head), 3 grouped int4 (docs/WEIGHT_INT4.md: the layers only, with a bf16 LM head), 4 block-scaled FP8
    (docs/WEIGHT_FP8G128.md: the layers only, with a bf16 LM head). The supported pairs are ``WEIGHT_FORMATS``' values."""
    _fields_ = [("layers", _INT), ("lm_head", _INT)]

    def __repr__(self):
        return f"WeightFormat(layers={self.layers}, lm_head={self.lm_head})"


# weight dtype -> (layers, lm_head) of WeightFormat. "int4g128" (docs/WEIGHT_INT4.md): grouped uint4 layers, GPTQ / AWQ
# style, groups of 128, with a bf16 LM head. The name says the group size: plain "int4" stays an unknown dtype.
# "fp8g128" (docs/WEIGHT_FP8G128.md): e4m3 layers with one fp32 scale per output row and 128 input features, what
# block-FP8 checkpoints (weight_block_size [128, 128]) expand to, with a bf16 LM head.
WEIGHT_FORMATS = {"bf16": (0, 0), "fp8": (1, 1), "mxfp4": (2, 1), "int4g128": (3, 0), "fp8g128": (4, 0)}


def as_weight_format(weight_fp8: bool = False, weight_format=None) -> WeightFormat:
    """The ``WeightFormat`` a caller means: ``weight_format`` (a ``WeightFormat``, or one of "bf16", "fp8", "mxfp4", "int4g128",
    "fp8g128") where given, else FP8 throughout for ``weight_fp8`` and bf16 without. Both at once, an unknown name or a pair of
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


class ChunkPlan(ctypes.Structure):
    """Mirror of ``ChunkPlan``: what ``k_attn_chunk<D, G, KV8>`` launches for B rows (docs/CHUNK_ATTN.md), beside the
    step's ``StepPlan`` as ``WindowPlan`` is: ``slots`` x ``grid_y`` workgroups of ``waves`` waves, ``grid_y`` =
    ``tiles`` (16-row tiles) x Hkv; ``stride`` partial slots per head in part_o / part_ml, ``StepPlan.attn.stride``."""
    _fields_ = [(n, _INT) for n in ("D", "G", "tiles", "slots", "stride", "grid_y", "waves")]


class MoeDims(ctypes.Structure):
    """Mirror of ``MoeDims`` (decode_moe.h): the routed-expert FFN of a model, beside ``LlamaDims`` and the plans as
    ``WeightFormat`` is (docs/MOE.md). ``n_experts`` E <= 128, ``top_k`` experts per token (<= min(8, E)),
    ``norm_topk``: 1 when the top-k probabilities are renormalised to sum to one. With it ``dims.ffn`` is the
    per-expert intermediate size."""
    _fields_ = [("n_experts", _INT), ("top_k", _INT), ("norm_topk", _INT)]

    def __repr__(self):
        return f"MoeDims(n_experts={self.n_experts}, top_k={self.top_k}, norm_topk={self.norm_topk})"


class MoePlan(ctypes.Structure):
    """Mirror of ``MoePlan``: what the four kernels of an MoE layer launch for B rows. ``k_moe_route`` on
    ``route_grid`` workgroups; ``k_moe_gate_up<gu_nw, gu_rt, gu_um>`` on ``gu_grid_x`` x ``gu_grid_y`` (column tiles x
    experts), ``k_moe_down`` likewise; ``k_moe_combine`` on ``cb_grid`` workgroups of ``cb_cols`` columns, ``cb_grid``
    being the ``ss_in`` of the next QKV GEMM and of the LM head."""
    _fields_ = [(n, _INT) for n in ("route_grid", "route_waves", "gu_grid_x", "gu_grid_y", "gu_nw", "gu_rt", "gu_um",
                                    "dn_grid_x", "dn_grid_y", "dn_nw", "dn_rt", "dn_um", "cb_grid", "cb_cols",
                                    "cb_waves")]


MAX_EXPERTS, MAX_TOP_K = 128, 8  # decode_moe.h's kMaxExperts and kMaxTopK


class ExpertFormat(ctypes.Structure):
    """Mirror of ``ExpertFormat`` (decode_moe.h): the format of an MoE model's stacked expert matrices, beside
    ``MoeDims`` as ``WeightFormat`` is beside the plans (docs/MOE_FP8.md). ``w8``: 0 bf16; 1 OCP e4m3fn bytes in
    k-step-pair order (``block_expert_fp8``) with one fp32 scale per (expert, output row); 2 OCP MXFP4 nibble bytes in
    k-step-quad order (``block_expert_mxfp4``) with one e8m0 byte per 32-element block (docs/MOE_MXFP4.md)."""
    _fields_ = [("w8", _INT)]

    def __repr__(self):
        return f"ExpertFormat(w8={self.w8})"


class LoraPlan(ctypes.Structure):
    """decode_lora.h's LoraPlan: what ``k_lora_delta`` launches for one projection (docs/LORA.md)."""
    _fields_ = [(n, _INT) for n in ("grid_x", "grid_y", "waves", "cols", "passes")]


class LoraTable(ctypes.Structure):
    """decode_fused.hip's LoraTable: the adapters of a decoder. ``rank``: the padded R of wqkv, wo, w_gate_up, w_down;
    ``tables``: per layer eight device pointers, A' then B' of each of the four."""
    _fields_ = [("n_adapters", _INT), ("rank", _INT * 4), ("tables", ctypes.POINTER(ctypes.c_void_p))]


class LmScorePlan(ctypes.Structure):
    """What ``lm_score_`` launches (lm_score.hip): ``k_lm_score`` on ``slabs * tiles`` workgroups of ``threads``, each
    a slab of ``slab`` vocabulary columns of one 16-row tile, then the merge on one wave per row; ``work_words``
    4-byte words of scratch."""
    _fields_ = [(n, _INT) for n in ("slab", "slabs", "tiles", "threads", "work_words")]


class StepOptions(ctypes.Structure):
    """Mirror of ``StepOptions``: every option of a fused step, as ``p2pt_llama_step``, ``p2pt_llama_step_kernels``,
    ``p2pt_llama_step_ws`` and ``p2pt_llama_step_weights`` take them. All zero: the bf16 dense step. ``kv_scales``: a
    device address; ``windows``: a host array of ``n_layers`` ints. Build one with ``step_options``."""
    _fields_ = [("fmt", WeightFormat), ("kv_scales", ctypes.c_void_p), ("windows", ctypes.POINTER(_INT)),
                ("chunk_attn", _INT), ("moe", ctypes.POINTER(MoeDims)), ("experts", ctypes.POINTER(ExpertFormat)),
                ("lora", ctypes.POINTER(LoraTable))]


def step_options(fmt: WeightFormat, kv_scales: torch.Tensor | None = None, windows=None, chunk_attn: bool = False,
                 moe: MoeDims | None = None, experts: ExpertFormat | None = None,
                 lora: LoraTable | None = None) -> StepOptions:
    """A ``StepOptions`` of checked values (``as_weight_format``, ``check_windows``, ``check_moe``,
    ``as_expert_format``); None leaves a pointer null. The struct keeps the ctypes objects it points to alive; the
    ``kv_scales`` tensor is the caller's to keep."""
    o = StepOptions(fmt=fmt, kv_scales=kv_scales.data_ptr() if kv_scales is not None else None,
                    chunk_attn=int(chunk_attn))
    if windows is not None:
        o.windows = (_INT * len(windows))(*windows)
    for name, value in (("moe", moe), ("experts", experts), ("lora", lora)):
        if value is not None:
            setattr(o, name, ctypes.pointer(value))
    return o


EXPERT_FORMATS = {"bf16": 0, "fp8": 1, "mxfp4": 2}  # expert dtype -> ExpertFormat.w8
EXPERT_BLOCK = 64  # K elements per block of the FP8 experts' byte order: a pair of k-steps
EXPERT_QUAD = 128  # K elements per block of the MXFP4 experts' byte order: a quad of k-steps, 64 nibble bytes


def as_expert_format(expert_format=None, moe=None, dim: int = 0, ffn: int = 0) -> ExpertFormat:
    """The ``ExpertFormat`` a caller means: None or "bf16", "fp8", "mxfp4", or an ``ExpertFormat`` of w8 0, 1 or 2.
    FP8 experts need a routed-expert FFN (``moe``) whose ``dim`` and per-expert ``ffn`` are multiples of 64, MXFP4
    experts one whose two are multiples of 128: every refusal says why (host only: no library)."""
    f = expert_format
    if f is None:
        return ExpertFormat(0)
    if isinstance(f, str):
        if f not in EXPERT_FORMATS:
            raise ValueError(f"expert_dtype must be one of {sorted(EXPERT_FORMATS)}, got {f!r}")
        f = ExpertFormat(EXPERT_FORMATS[f])
    if not isinstance(f, ExpertFormat) or f.w8 not in EXPERT_FORMATS.values():
        raise ValueError(f"expert_format must be an ExpertFormat of w8 0, 1 or 2 or one of {sorted(EXPERT_FORMATS)}, "
                         f"got {expert_format!r}")
    if f.w8 == 2:
        if moe is None:
            raise ValueError("expert_dtype mxfp4 needs a routed-expert FFN: a dense model has no experts "
                             "(its GEMM weights follow weight_dtype)")
        if dim % EXPERT_QUAD or ffn % EXPERT_QUAD:
            raise ValueError(f"MXFP4 experts are stored in blocks of {EXPERT_QUAD} (quads of k-steps): dim and the "
                             f"per-expert ffn must be multiples of {EXPERT_QUAD}, got dim {dim}, ffn {ffn}")
    elif f.w8:
        if moe is None:
            raise ValueError("expert_dtype fp8 needs a routed-expert FFN: a dense model has no experts "
                             "(its GEMM weights follow weight_dtype)")
        if dim % EXPERT_BLOCK or ffn % EXPERT_BLOCK:
            raise ValueError(f"FP8 experts are stored in blocks of {EXPERT_BLOCK} (pairs of k-steps): dim and the "
                             f"per-expert ffn must be multiples of {EXPERT_BLOCK}, got dim {dim}, ffn {ffn}")
    return ExpertFormat(f.w8)


def _expert_perm(K: int, device=None) -> torch.Tensor:
    """``perm[i]``: the natural k of byte i of a row in k-step-pair order."""
    i = torch.arange(K, device=device)
    j, g, half = i % EXPERT_BLOCK, (i % EXPERT_BLOCK) // 16, (i % 16) // 8
    return i - j + 32 * half + 8 * g + i % 8


def _check_expert_bytes(q, what: str):
    if not isinstance(q, torch.Tensor) or q.dtype not in KV_FP8_DTYPES or q.dim() != 3:
        raise TypeError(f"{what} takes e4m3 (or uint8) bytes [E, N, K]")
    if q.shape[2] % EXPERT_BLOCK:
        raise ValueError(f"K must be a multiple of {EXPERT_BLOCK} (a pair of k-steps), got {q.shape[2]}")


def block_expert_fp8(q: torch.Tensor) -> torch.Tensor:
    """FP8 expert bytes ``[E, N, K]`` from natural K order to the device order ``k_moe_gate_up`` / ``k_moe_down``
    stream (docs/MOE_FP8.md): inside every 64-element block of a row, lane group g = 0..3 owns 16 contiguous bytes,
    bytes ``16 g .. 16 g + 7`` the natural bytes ``8 g .. 8 g + 7`` (the even k-step of the pair) and bytes
    ``16 g + 8 .. 16 g + 15`` the natural bytes ``32 + 8 g .. 32 + 8 g + 7`` (the odd one), so one 16-byte load feeds
    two k-steps. A new contiguous tensor of ``q``'s dtype; plain torch on ``q``'s device."""
    _check_expert_bytes(q, "block_expert_fp8")
    return q.view(torch.uint8)[..., _expert_perm(q.shape[2], q.device)].contiguous().view(q.dtype)


def unblock_expert_fp8(q: torch.Tensor) -> torch.Tensor:
    """The inverse of ``block_expert_fp8``: device order back to natural K order."""
    _check_expert_bytes(q, "unblock_expert_fp8")
    out = torch.empty_like(q.view(torch.uint8))
    out[..., _expert_perm(q.shape[2], q.device)] = q.view(torch.uint8)
    return out.view(q.dtype)


def _expert_perm_mxfp4(Kb: int, device=None) -> torch.Tensor:
    """``perm[i]``: the natural byte of byte i of a row of ``Kb`` nibble bytes in k-step-quad order."""
    i = torch.arange(Kb, device=device)
    j = i % (EXPERT_QUAD // 2)
    g, h, b = j // 16, (j % 16) // 4, j % 4
    return i - j + 16 * h + 4 * g + b


def _check_expert_nibbles(packed, what: str):
    if not isinstance(packed, torch.Tensor) or packed.dtype != torch.uint8 or packed.dim() != 3:
        raise TypeError(f"{what} takes uint8 nibble bytes [E, N, K / 2]")
    if packed.shape[2] % (EXPERT_QUAD // 2):
        raise ValueError(f"K must be a multiple of {EXPERT_QUAD} (a quad of k-steps, {EXPERT_QUAD // 2} nibble bytes), "
                         f"got {2 * packed.shape[2]}")


def block_expert_mxfp4(packed: torch.Tensor) -> torch.Tensor:
    """MXFP4 expert nibble bytes ``[E, N, K / 2]`` from ``pack_weight_mxfp4``'s natural order to the device order
    ``k_moe_gate_up`` / ``k_moe_down`` stream (docs/MOE_MXFP4.md): inside every 64-byte block of a row (128 K elements)
    device byte ``16 g + 4 h + b`` is natural byte ``16 h + 4 g + b``, for lane group g, k-step h of the quad and byte
    b, each 0..3. The 16 contiguous bytes of lane group g are then its 8 k-values of the quad's four k-steps in
    order, so one 16-byte load feeds four k-steps. Nibble order inside a byte and the e8m0 scale bytes do not move. A
    new contiguous tensor; plain torch on ``packed``'s device."""
    _check_expert_nibbles(packed, "block_expert_mxfp4")
    return packed[..., _expert_perm_mxfp4(packed.shape[2], packed.device)].contiguous()


def unblock_expert_mxfp4(packed: torch.Tensor) -> torch.Tensor:
    """The inverse of ``block_expert_mxfp4``: device order back to natural order."""
    _check_expert_nibbles(packed, "unblock_expert_mxfp4")
    out = torch.empty_like(packed)
    out[..., _expert_perm_mxfp4(packed.shape[2], packed.device)] = packed
    return out


def check_moe(moe, dim: int, ffn: int) -> "MoeDims | None":
    """``moe`` as the fused step takes it: None (a dense model), or a ``MoeDims`` the kernels run for per-expert
    shapes ``[2 * ffn, dim]`` and ``[dim, ffn]``. Every refusal says why (host only: no library)."""
    if moe is None:
        return None
    if not isinstance(moe, MoeDims):
        raise TypeError(f"moe must be an ops.MoeDims or None, got {type(moe).__name__}")
    E, k = moe.n_experts, moe.top_k
    if not 1 <= E <= MAX_EXPERTS:
        raise ValueError(f"n_experts must be 1..{MAX_EXPERTS}, got {E}")
    if not 1 <= k <= min(MAX_TOP_K, E):
        raise ValueError(f"top_k must be 1..min({MAX_TOP_K}, n_experts), got {k} with {E} experts")
    if moe.norm_topk not in (0, 1):
        raise ValueError(f"norm_topk must be 0 or 1, got {moe.norm_topk}")
    if dim % 32 or ffn % 32 or dim <= 0 or ffn <= 0:
        raise ValueError(f"an expert's shapes must be multiples of 32 (whole k-steps), got dim {dim}, ffn {ffn}")
    if 2 * ffn * dim * 2 >= GEMM_OPERAND_LIMIT:
        raise ValueError(f"one expert's gate/up slice ({2 * ffn} x {dim} bf16) must stay below 2 GiB")
    return MoeDims(E, k, moe.norm_topk)


def _signatures() -> dict:
    """Every symbol ``lib()`` binds -> its argtypes. The restype is ``c_int`` unless ``_RESTYPES`` names another."""
    vp, i, f, sz, ptr = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.POINTER
    dims, wp, ip, szp, wf = ptr(LlamaDims), ptr(WeightPlan), ptr(i), ptr(sz), ptr(WeightFormat)
    moe, ef, opts = ptr(MoeDims), ptr(ExpertFormat), ptr(StepOptions)
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
        "p2pt_lm_score": [vp, i, i, vp, vp, i, i, f, vp, vp, sz, vp, vp, vp, vp, vp],
        "p2pt_lm_score_plan": [i, i, i, ptr(LmScorePlan)],
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
        "p2pt_llama_weight_layout": [dims, wp, ip, ip, i],
        "p2pt_llama_window_plan": [dims, i, i, ptr(WindowPlan)],
        "p2pt_llama_plan_kernels_win": [dims, i, i, wp, ip],
        "p2pt_llama_decode_win": [dims, wp, vp, ip, ptr(vp), vp, vp, vp, vp, vp, i, i, vp, sz, vp, vp, vp],
        "p2pt_llama_weight_format": [dims, i, i, wf],
        "p2pt_llama_plan_fmt": [dims, wf, i, i, ptr(StepPlan)],
        "p2pt_llama_ws_bytes_fmt": [dims, wf],
        "p2pt_llama_ws_layout_fmt": [dims, wf, szp, szp, i],
        "p2pt_llama_plan_kernels_fmt": [dims, i, i, wf, ip],
        "p2pt_llama_weight_layout_fmt": [dims, wf, ip, ip, i],
        "p2pt_llama_decode_fmt": [dims, wf, vp, ip, ptr(vp), vp, vp, vp, vp, vp, i, i, vp, sz, vp, vp, vp],
        "p2pt_llama_chunk_plan": [dims, i, ptr(ChunkPlan)],
        "p2pt_llama_decode_chunk": [dims, wf, vp, ip, ptr(vp), vp, vp, vp, vp, vp, i, i, vp, sz, vp, vp, vp, i],
        "p2pt_chunk_attention": [vp, vp, vp, vp, vp, i, i, i, i, i, i, i, vp, vp, vp, vp, vp, vp, vp],
        "p2pt_llama_ws_bytes_moe": [dims, moe],
        "p2pt_llama_ws_layout_moe": [dims, moe, szp, szp, i],
        "p2pt_llama_moe_plan": [dims, moe, i, ptr(MoePlan)],
        "p2pt_llama_weight_layout_moe": [dims, moe, ip, i],
        "p2pt_llama_decode_moe": [dims, wf, vp, ip, ptr(vp), vp, vp, vp, vp, vp, i, i, vp, sz, vp, vp, vp, i, moe],
        "p2pt_moe_ffn": [vp, vp, i, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, f, vp],
        "p2pt_moe_ffn_plan": [i, i, i, i, i, i, ptr(MoePlan)],
        "p2pt_llama_plan_kernels_experts": [dims, i, i, wf, ip, i, moe, ef],
        "p2pt_llama_weight_layout_experts": [dims, moe, ef, ip, ip, i],
        "p2pt_moe_ffn_experts": [vp, vp, i, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, f, vp, ef, vp, vp],
        "p2pt_moe_ffn_mxfp4": [vp, vp, i, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, f, vp, vp, vp],
        "p2pt_lora_delta": [vp, vp, vp, vp, vp, i, i, i, i, i, vp],
        "p2pt_lora_plan": [i, i, i, i, i, ptr(LoraPlan)],
        "p2pt_lora_max_adapters": [],
        "p2pt_lora_max_rank": [],
        "p2pt_llama_step": [dims, opts, ptr(vp), vp, vp, vp, vp, vp, i, i, vp, sz, vp, vp, vp, vp],
        "p2pt_llama_step_kernels": [dims, opts, i, i],
        "p2pt_llama_step_ws": [dims, opts, szp, szp, i],
        "p2pt_llama_step_weights": [dims, opts, ip, ip, i],
        "p2pt_attn_span": [i, i],
        "p2pt_max_rows": [],
        "p2pt_skinny_bench": [vp, vp, vp, i, i, i, i, i, i, vp],  # microbenchmark hooks (scripts/bench_skinny.py)
        "p2pt_attn_bench": [vp, vp, vp, vp, i, i, i, i, i, vp, vp, vp, vp, i, vp],
    }


_RESTYPES = {"p2pt_llama_ws_bytes": ctypes.c_size_t, "p2pt_llama_ws_bytes_moe": ctypes.c_size_t,
             "p2pt_llama_ws_bytes_fmt": ctypes.c_size_t, "p2pt_llama_step_ws": ctypes.c_size_t}


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
        if (_LIB.p2pt_lora_max_adapters(), _LIB.p2pt_lora_max_rank()) != (LORA_MAX_ADAPTERS, LORA_MAX_RANK):
            raise RuntimeError(f"LORA_MAX_ADAPTERS, LORA_MAX_RANK = {LORA_MAX_ADAPTERS}, {LORA_MAX_RANK}, but {path} "
                               f"was built for {_LIB.p2pt_lora_max_adapters()}, {_LIB.p2pt_lora_max_rank()}")
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
W4G_GROUP = 128  # K elements per group of an int4 weight: one scale and zero point each (a quad of k_skinny's k-steps)
F8G_GROUP = 128  # K elements per scale of a block-scaled FP8 weight row (a quad of k-steps, two 64-byte k-step pairs)
W4G_ZERO_MAX = 16  # the largest zero point a group word may carry (GPTQ v1 stores z - 1 in a nibble)
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # the magnitudes of an e2m1 nibble's low three bits; bit 3: sign
MAX_TOP_LOGPROBS = 20  # top (id, logprob) pairs per row of logprobs_ (logprobs.hip's kMaxTop; the OpenAI API's limit)
LORA_MAX_ADAPTERS = 8  # adapters beside one base model (decode_lora.h's kMaxAdapters)
LORA_MAX_RANK = 192  # padded rank R of one projection: three stacked parts of PEFT rank <= 64 (kMaxRank)
LORA_MODULE_MAX_RANK = 64  # PEFT r of one target module
# A fused projection's PEFT target modules, in the order their parts are stacked in A' and B' (docs/LORA.md).
LORA_PARTS = {"wqkv": ("q_proj", "k_proj", "v_proj"), "wo": ("o_proj",), "w_gate_up": ("gate_proj", "up_proj"),
              "w_down": ("down_proj",)}


def step_plan(dims: LlamaDims, B: int, emit_rows: int = 0, weight_format=None) -> StepPlan:
    """What ``p2pt_llama_decode`` launches for B rows: the kernel variant, grid and partial counts of every
    stage, from the library's own planning function (host only: needs the library, not a GPU).
    ``weight_format`` (``as_weight_format``): the plan of a step in those formats. Only "int4g128" and "fp8g128" differ from
    the plan without it: their K parts carry whole groups of 128 (docs/WEIGHT_INT4.md, docs/WEIGHT_FP8G128.md)."""
    plan = StepPlan()
    if weight_format is not None:
        f = as_weight_format(False, weight_format)
        if lib().p2pt_llama_plan_fmt(ctypes.byref(dims), ctypes.byref(f), B, emit_rows, ctypes.byref(plan)) != 0:
            raise ValueError("dims, row count or weight format not supported by the fused decode kernels")
        return plan
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


def chunk_plan(dims: LlamaDims, B: int) -> ChunkPlan:
    """What a layer that runs chunk attention launches for attention at B rows (host only): ``k_attn_chunk``'s grid
    and span slots. A decoder built with ``chunk_attn=True`` follows it on every layer without a window in steps of
    more than 16 rows; everything else of the step is ``step_plan(dims, B)``."""
    plan = ChunkPlan()
    if lib().p2pt_llama_chunk_plan(ctypes.byref(dims), B, ctypes.byref(plan)) != 0:
        raise ValueError("dims or row count not supported by the fused decode kernels")
    return plan


def moe_plan(dims: LlamaDims, moe: MoeDims, B: int) -> MoePlan:
    """What the routed-expert FFN's four kernels launch for B rows, beside ``step_plan(dims, B)`` (host only: the
    library, no GPU). A function of (B, dims, moe) alone."""
    plan = MoePlan()
    moe = check_moe(moe, dims.dim, dims.ffn)
    if moe is None or lib().p2pt_llama_moe_plan(ctypes.byref(dims), ctypes.byref(moe), B, ctypes.byref(plan)) != 0:
        raise ValueError("dims, MoE dims or row count not supported by the fused decode kernels")
    return plan


def plan_kernels_ok(dims: LlamaDims, B: int, emit_rows: int = 0, weight_fp8: bool = False, windows=None,
                    weight_format=None, chunk_attn: bool = False, moe: MoeDims | None = None,
                    expert_format=None, lora=None) -> bool:
    """Whether every stage of ``step_plan(dims, B, emit_rows)``, ``kv_plan(dims)`` and
    ``weight_plan(dims, weight_fp8)`` names a kernel the library instantiates, by the lookups its launchers use
    (host only). ``windows``: the per-layer sliding windows (``check_windows``); every layer's ``window_plan`` is
    then looked up too. ``weight_format`` (see ``as_weight_format``): the formats instead of ``weight_fp8``.
    ``chunk_attn``: the layers that then run ``k_attn_chunk`` (``chunk_plan``) are looked up as that.
    ``expert_format`` (``as_expert_format``; with ``moe`` only): the experts' format, whose ``k_moe_gate_up`` /
    ``k_moe_down`` instantiations are then the ones looked up.
    ``lora`` (docs/LORA.md): the padded ranks of wqkv, wo, w_gate_up and w_down (``lora_rank``); the four layer stages
    are then looked up as their LoRA-delta variants, which exist for bf16 dense models without QK-norm."""
    windows = check_windows(windows, dims.n_layers)
    moe = check_moe(moe, dims.dim, dims.ffn)
    experts = as_expert_format(expert_format, moe, dims.dim, dims.ffn)
    f = as_weight_format(weight_fp8, weight_format)
    table = None
    if lora is not None:
        if moe is not None or (f.layers, f.lm_head) != (0, 0) or dims.qk_norm:
            raise ValueError("LoRA adapters need a dense bf16 model without QK-norm")
        table = LoraTable(n_adapters=1, rank=(_INT * 4)(*lora))
    opts = step_options(f, None, windows, chunk_attn, moe, experts, table)
    rc = lib().p2pt_llama_step_kernels(ctypes.byref(dims), ctypes.byref(opts), B, emit_rows)
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
    ``unpack_weight_mxfp4`` undoes it, and decode_fused.hip's accessor and the kernel's offsets mirror it.

    "int4g128" (docs/WEIGHT_INT4.md): embed, the norms and lm_head (final_norm folded in) are the bf16 table's; each
    layer's four GEMM weights are uint8 ``(N, K / 2)`` in ``pack_weight_w4g``'s order, 16-byte aligned, with no norm
    weight folded in, and after the table come, per layer, their group words, int32 ``(N, K / 128)``, named
    ``"<weight> scale"`` too. attn_norm and ffn_norm are read by this format: the residual's producers multiply by them.

    "fp8g128" (docs/WEIGHT_FP8G128.md): embed, the norms and lm_head (final_norm folded in) are the bf16 table's; each
    layer's four GEMM weights are e4m3 (or uint8) bytes ``(N, K)``, 16-byte aligned, with no norm weight folded in, and
    after the table come, per layer, their scales, fp32 ``(N, K / 128)``, 4-byte aligned, named ``"<weight> scale"``:
    ``W[n][k] = e4m3(byte) * scale[n][k // 128]``. The physical byte order of a row is k-step-pair order, stated here
    once: inside every 64 bytes, byte ``16 g + 8 h + j`` holds ``k = 32 h + 8 g + j`` of that block, for lane group
    g = 0..3, k-step h = 0..1 of the pair and j = 0..7 (``block_expert_fp8``'s order), so the 16 bytes at
    ``n K + 64 P + 16 (lane >> 4)`` are a lane's 8 k-values of k-steps 2 P and 2 P + 1. ``pack_weight_fp8g128`` makes
    this order from natural bytes, ``unpack_weight_fp8g128`` undoes it. attn_norm and ffn_norm (16-byte aligned) are
    read by this format: the QKV and gate/up kernels multiply their A fragments by them.

    ``moe`` (a ``MoeDims``; docs/MOE.md): ``dims.ffn`` is the per-expert size, w_gate_up is
    ``(E, 2 * ffn, dim)``, folded and pair-interleaved per expert, w_down ``(E, dim, ffn)``, and every layer ends with
    router, bf16 ``(E, dim)`` with the FFN norm folded in, 16-byte aligned. None: the dense table, unchanged.
    ``weight_format`` stays bf16 with it; ``expert_format`` (``as_expert_format``; docs/MOE_FP8.md) "fp8" makes
    w_gate_up and w_down e4m3 (or uint8) bytes of the same shapes, 16-byte aligned, rows in ``block_expert_fp8``'s
    order, and appends after every other entry, per layer, their fp32 row scales ``(E, 2 * ffn)`` and ``(E, dim)``,
    named ``"w_gate_up scale"`` and ``"w_down scale"``. "mxfp4" (docs/MOE_MXFP4.md) makes them uint8 nibble bytes
    ``(E, 2 * ffn, dim / 2)`` and ``(E, dim, ffn / 2)``, 16-byte aligned, rows in ``block_expert_mxfp4``'s order, and the
    two appended entries their e8m0 bytes ``(E, 2 * ffn, dim / 32)`` and ``(E, dim, ffn / 32)``, uint8, natural order,
    4-byte aligned. None or "bf16": the bf16 MoE table, unchanged."""

    def __init__(self, dims: LlamaDims, weight_fp8: bool = False, weight_format=None, moe: MoeDims | None = None,
                 expert_format=None):
        self.format = fmt = as_weight_format(weight_fp8, weight_format)
        self.moe = moe = check_moe(moe, dims.dim, dims.ffn)
        self.expert_format = experts = as_expert_format(expert_format, moe, dims.dim, dims.ffn)
        if moe is not None and fmt.layers != 0:
            raise ValueError("an MoE model's expert weights are bf16 only: weight_dtype fp8 and mxfp4 are not "
                             "supported with a routed-expert FFN (expert_format='fp8' quantises the experts alone)")
        d, bf, f32, u8 = dims, (torch.bfloat16,), (torch.float32,), (torch.uint8,)
        gemm, ga = (WEIGHT_FP8_DTYPES, 8) if fmt.lm_head else (bf, 2)
        # int4: the embedding kernel reads layer 0's attn_norm with 16-byte loads; fp8g128: the normed GEMMs do
        n_qkv, norm = (d.H + 2 * d.Hkv) * d.D, (bf, (d.dim,), 16 if fmt.layers in (3, 4) else 2)
        top = {"embed": (bf, (d.vocab, d.dim), 2), "final_norm": norm, "lm_head": (gemm, (d.vocab, d.dim), ga)}
        if d.rope_table:
            top["inv_freq"] = (f32, (d.D // 2,), 8)
        shapes = {"wqkv": (n_qkv, d.dim), "wo": (d.dim, d.H * d.D), "w_gate_up": (2 * d.ffn, d.dim),
                  "w_down": (d.dim, d.ffn)}
        if fmt.layers in (3, 4):
            check_w4g_dims(d, "int4" if fmt.layers == 3 else "fp8g128")
        if fmt.layers == 2:  # nibbles, two to a byte
            lg = {n: (u8, (N, K // 2), 4) for n, (N, K) in shapes.items()}
        elif fmt.layers == 3:  # nibbles in k-step-quad order: one 16-byte load per lane and quad
            lg = {n: (u8, (N, K // 2), 16) for n, (N, K) in shapes.items()}
        elif fmt.layers == 4:  # e4m3 bytes in k-step-pair order: one 16-byte load per lane and pair
            lg = {n: (WEIGHT_FP8_DTYPES, shape, 16) for n, shape in shapes.items()}
        else:
            lg = {n: (gemm, shape, ga) for n, shape in shapes.items()}
        layer = {"attn_norm": norm, "wqkv": lg["wqkv"], "wo": lg["wo"], "ffn_norm": norm, "w_gate_up": lg["w_gate_up"],
                 "w_down": lg["w_down"]}
        if d.qk_norm:
            layer.update(q_norm=(bf, (d.D,), 2), k_norm=(bf, (d.D,), 2))
        elif d.qkv_bias:
            layer["bqkv"] = (bf, (n_qkv,), 2)
        if moe is not None:  # stacked experts (16-byte loads of a router row) and the router, after every other entry
            layer["w_gate_up"] = (bf, (moe.n_experts, 2 * d.ffn, d.dim), 2)
            layer["w_down"] = (bf, (moe.n_experts, d.dim, d.ffn), 2)
            layer["router"] = (bf, (moe.n_experts, d.dim), 16)
            if experts.w8 == 1:  # one 16-byte load per lane and k-step pair
                layer["w_gate_up"] = (WEIGHT_FP8_DTYPES, (moe.n_experts, 2 * d.ffn, d.dim), 16)
                layer["w_down"] = (WEIGHT_FP8_DTYPES, (moe.n_experts, d.dim, d.ffn), 16)
            if experts.w8 == 2:  # one 16-byte load per lane and k-step quad
                layer["w_gate_up"] = (u8, (moe.n_experts, 2 * d.ffn, d.dim // 2), 16)
                layer["w_down"] = (u8, (moe.n_experts, d.dim, d.ffn // 2), 16)
        groups = [(None, top)] + [(L, layer) for L in range(d.n_layers)]
        super().__init__(WeightEntry(n, L, *v) for L, group in groups for n, v in group.items())
        if fmt.lm_head:  # the scales, in the order of their weights: fp32 per row, or MXFP4's e8m0 byte per block
            self += [WeightEntry(n + " scale", L, u8, (shapes[n][0], shapes[n][1] // MXFP4_BLOCK), 1)
                     if L is not None and fmt.layers == 2 else WeightEntry(n + " scale", L, f32, v[1][:1], 4)
                     for L, group in groups for n, v in group.items() if n == "lm_head" or n in LAYER_GEMMS]
        if fmt.layers == 3:  # the group words of each layer's four; the LM head is bf16 and has none
            self += [WeightEntry(n + " scale", L, (torch.int32,), (shapes[n][0], shapes[n][1] // W4G_GROUP), 4)
                     for L in range(d.n_layers) for n in LAYER_GEMMS]
        if fmt.layers == 4:  # one fp32 scale per row and 128 k of each layer's four; the LM head is bf16 and has none
            self += [WeightEntry(n + " scale", L, f32, (shapes[n][0], shapes[n][1] // F8G_GROUP), 4)
                     for L in range(d.n_layers) for n in LAYER_GEMMS]
        if experts.w8 == 1:  # the experts' row scales, after every other entry
            self += [WeightEntry(n + " scale", L, f32, layer[n][1][:2], 4)
                     for L in range(d.n_layers) for n in ("w_gate_up", "w_down")]
        if experts.w8 == 2:  # in their place the e8m0 byte of every 32-element block: a 4-byte load per k-step quad
            self += [WeightEntry(n + " scale", L, u8, layer[n][1][:2] + (layer[n][1][2] // (MXFP4_BLOCK // 2),), 4)
                     for L in range(d.n_layers) for n in ("w_gate_up", "w_down")]
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


def check_w4g_dims(dims: LlamaDims, what: str = "int4") -> None:
    """Grouped int4 weights, and ``what`` "fp8g128" block-scaled FP8 ones, need every K of a layer GEMM in whole groups
    of 128 (host only)."""
    if dims.dim % W4G_GROUP or dims.ffn % W4G_GROUP or (dims.H * dims.D) % W4G_GROUP:
        raise ValueError(f"{what} weights are stored in groups of {W4G_GROUP} (quads of k-steps): dim, ffn and "
                         f"n_heads * head_dim must be multiples of {W4G_GROUP}, got dim {dims.dim}, ffn {dims.ffn}, "
                         f"n_heads * head_dim {dims.H * dims.D}")


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


def chunk_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: torch.Tensor,
                    slots: torch.Tensor | None = None, k_scale: torch.Tensor | None = None,
                    v_scale: torch.Tensor | None = None) -> torch.Tensor:
    """GQA attention of B <= 64 token rows over the KV cache with ``k_attn_chunk`` (docs/CHUNK_ATTN.md): one K/V pass
    per 16-row tile and distinct slot in it. q: bf16 [B, H, D]; caches [nslots, Smax, Hkv, D], bf16 or FP8
    (``KV_FP8_DTYPES``); row b reads slot ``slots[b]`` (int32 [B]; None: slot b) and attends to positions
    0..``pos[b]`` (int32 [B]), both clamped into range by the kernel as ``k_attn`` clamps them. ``k_scale`` /
    ``v_scale``: fp32 [Hkv] scales of an FP8 cache, both or neither. Returns bf16 [B, H, D]."""
    _check(q, torch.bfloat16, "q")
    kv8 = isinstance(k_cache, torch.Tensor) and k_cache.dtype in KV_FP8_DTYPES
    _check(k_cache, k_cache.dtype if kv8 else torch.bfloat16, "k_cache", q.device)
    _check(v_cache, k_cache.dtype, "v_cache", q.device)
    _check(pos, torch.int32, "pos", q.device)
    if q.dim() != 3 or k_cache.dim() != 4:
        raise ValueError("q must be [B, H, D] and the caches [nslots, Smax, Hkv, D]")
    B, H, D = q.shape
    nslots, Smax, Hkv = k_cache.shape[:3]
    if k_cache.shape != (nslots, Smax, Hkv, D) or v_cache.shape != k_cache.shape:
        raise ValueError("cache shape mismatch")
    if D not in (64, 128):
        raise ValueError("head_dim must be 64 or 128")
    if not 1 <= B <= MAX_ROWS:
        raise ValueError(f"rows must be 1..{MAX_ROWS}")
    if Hkv < 1 or H % Hkv or H // Hkv not in (1, 2, 4, 5, 6, 7, 8):
        raise ValueError("n_heads / n_kv_heads must be one of 1, 2, 4, 5, 6, 7, 8")
    if nslots < 1 or Smax < 1:
        raise ValueError("the caches must hold at least one row")
    if pos.shape != (B,):
        raise ValueError("pos must be [B]")
    if slots is not None:
        _check(slots, torch.int32, "slots", q.device)
        if slots.shape != (B,):
            raise ValueError("slots must be [B]")
    elif B > nslots:
        raise ValueError("without slots, row b reads slot b: B must be <= nslots")
    if (k_scale is None) != (v_scale is None) or (k_scale is not None and not kv8):
        raise ValueError("k_scale and v_scale come together, and with an FP8 cache only")
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if t is not None:
            _check(t, torch.float32, name, q.device)
            if t.shape != (Hkv,):
                raise ValueError(f"{name} must be [Hkv]")
    stride = min(16, (Smax + 63) // 64)  # attn_part_stride: the most span slots a launch can have
    part_o = torch.empty(B * H * stride * D, dtype=torch.float32, device=q.device)
    part_ml = torch.empty(B * H * stride * 2, dtype=torch.float32, device=q.device)
    counters = torch.zeros(((B + 15) // 16) * Hkv, dtype=torch.int32, device=q.device)
    out = torch.empty_like(q)
    _ok(lib().p2pt_chunk_attention(_p(q), _p(k_cache), _p(v_cache), _p(pos), _p(slots), B, H, Hkv, D, nslots, Smax,
                                   int(kv8), _p(k_scale), _p(v_scale), _p(part_o), _p(part_ml), _p(counters), _p(out),
                                   _stream(q)), "chunk_attention")
    return out


def moe_ffn_plan(B: int, dim: int, ffn: int, moe: MoeDims) -> MoePlan:
    """``moe_plan`` for the standalone op's shapes (host only)."""
    plan, moe = MoePlan(), check_moe(moe, dim, ffn)
    if moe is None or lib().p2pt_moe_ffn_plan(B, dim, ffn, moe.n_experts, moe.top_k, moe.norm_topk,
                                              ctypes.byref(plan)) != 0:
        raise ValueError("shapes, MoE dims or row count not supported by the MoE kernels")
    return plan


def moe_ffn(resid: torch.Tensor, ss: torch.Tensor, router: torch.Tensor, w_gate_up: torch.Tensor,
            w_down: torch.Tensor, top_k: int, norm_topk: bool = True, eps: float = 1e-5, out: dict | None = None,
            ss_in: int | None = None, gate_up_scale: torch.Tensor | None = None,
            down_scale: torch.Tensor | None = None, gate_up_exp: torch.Tensor | None = None,
            down_exp: torch.Tensor | None = None) -> dict:
    """One routed-expert FFN layer on caller tensors, with the fused step's four kernels (docs/MOE.md):
    ``resid += sum_j route_w[j] * down_e(SwiGLU(gate_up_e(rmsnorm(resid))))`` over each row's ``top_k`` experts.

    resid: bf16 [B <= 64, dim], updated in place. ss: fp32 [parts, 64], partial sums of squares of resid's rows
    (row b's sum is ``ss[:ss_in, b].sum()``; ``ss_in`` None: every row of ss), as the producer of the residual leaves
    them; replaced by those of the new rows, ``ss[:cb_grid]`` of ``moe_ffn_plan``, so it needs at least ``cb_grid`` rows. router: bf16 [E, dim];
    w_gate_up: bf16 [E, 2 * ffn, dim], rows interleaved (gate_j, up_j); w_down: bf16 [E, dim, ffn]; the router and
    w_gate_up carry the norm weight folded into their columns. Returns the intermediates, each written in every slot
    a (row, choice) pair owns: route_id int32 [B, top_k] (descending probability, ties to the lower id), route_w fp32
    [B, top_k], route_rs fp32 [B], moe_h bf16 [B * top_k, ffn], moe_part fp32 [B, top_k, dim]. ``out``: tensors to
    use for them instead of fresh ones (tests poison them).

    FP8 experts (docs/MOE_FP8.md): with ``gate_up_scale`` (fp32 [E, 2 * ffn]) and ``down_scale`` (fp32 [E, dim]) both
    given, w_gate_up and w_down are e4m3 (or uint8) bytes of the same shapes in ``block_expert_fp8``'s order, and the
    two GEMMs run their FP8 instantiations; dim and ffn must be multiples of 64. One scale without the other is
    refused. The router stays bf16.

    MXFP4 experts (docs/MOE_MXFP4.md): with ``gate_up_exp`` (uint8 e8m0 [E, 2 * ffn, dim / 32]) and ``down_exp`` (uint8
    [E, dim, ffn / 32]) both given, w_gate_up and w_down are uint8 nibble bytes [E, 2 * ffn, dim / 2] and
    [E, dim, ffn / 2] in ``block_expert_mxfp4``'s order (the scale bytes in natural order), and the two GEMMs run their
    MXFP4 instantiations; dim and ffn must be multiples of 128. One without the other, or either together with the
    fp32 scales, is refused."""
    if (gate_up_scale is None) != (down_scale is None):
        raise ValueError("FP8 experts need both gate_up_scale and down_scale; bf16 experts take neither")
    if (gate_up_exp is None) != (down_exp is None):
        raise ValueError("MXFP4 experts need both gate_up_exp and down_exp; bf16 and FP8 experts take neither")
    w4 = gate_up_exp is not None
    if w4 and gate_up_scale is not None:
        raise ValueError("MXFP4 experts take no fp32 row scales: pass gate_up_exp and down_exp (e8m0 block scales) or "
                         "gate_up_scale and down_scale (FP8 experts), not both")
    for name, t, w in (("gate_up_exp", gate_up_exp, w_gate_up), ("down_exp", down_exp, w_down)):
        shape = tuple(getattr(w, "shape", ()))  # one e8m0 byte per 32 elements, i.e. 16 nibble bytes (host only)
        shape = shape[:2] + (shape[2] // 16,) if len(shape) == 3 else shape
        if w4 and (not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or tuple(t.shape) != shape):
            raise ValueError(f"{name} must be uint8 {shape}: one e8m0 byte per expert, output row and 32-element block, "
                             f"got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    w8 = gate_up_scale is not None
    for name, t, w in (("gate_up_scale", gate_up_scale, w_gate_up), ("down_scale", down_scale, w_down)):
        shape = tuple(getattr(w, "shape", ()))[:2]  # one scale per expert and output row (host only: no device yet)
        if w8 and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape):
            raise ValueError(f"{name} must be fp32 {shape}: one scale per expert and output row, got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    _check(resid, torch.bfloat16, "resid")
    dev = resid.device
    _check(router, torch.bfloat16, "router", dev)
    for name, t in (("w_gate_up", w_gate_up), ("w_down", w_down)):
        if w8 and (not isinstance(t, torch.Tensor) or t.dtype not in WEIGHT_FP8_DTYPES):
            raise TypeError(f"{name}: with scales the experts are FP8, so it must be torch.float8_e4m3fn (or uint8), "
                            f"got {getattr(t, 'dtype', type(t))}")
        if w4 and (not isinstance(t, torch.Tensor) or t.dtype != torch.uint8):
            raise TypeError(f"{name}: with e8m0 scales the experts are MXFP4, so it must be nibble bytes (torch.uint8), "
                            f"got {getattr(t, 'dtype', type(t))}")
        _check(t, t.dtype if w8 or w4 else torch.bfloat16, name, dev)
    _check(ss, torch.float32, "ss", dev)
    if resid.dim() != 2 or router.dim() != 2:
        raise ValueError("resid must be [B, dim] and router [E, dim]")
    (B, dim), E = resid.shape, router.shape[0]
    if w_down.dim() != 3:
        raise ValueError("w_down must be [E, dim, ffn]")
    ffn = w_down.shape[2] * (2 if w4 else 1)
    if not 1 <= B <= MAX_ROWS:
        raise ValueError(f"rows must be 1..{MAX_ROWS}")
    if not _int_in(top_k, 1, MAX_TOP_K + 1):
        raise ValueError(f"top_k must be an int in 1..{MAX_TOP_K}, got {top_k!r}")
    moe = check_moe(MoeDims(E, top_k, int(bool(norm_topk))), dim, ffn)
    experts = as_expert_format("fp8" if w8 else "mxfp4" if w4 else None, moe, dim, ffn)
    for name, t in (("gate_up_scale", gate_up_scale), ("down_scale", down_scale)):
        if w8:
            _check(t, torch.float32, name, dev)
    for name, t in (("gate_up_exp", gate_up_exp), ("down_exp", down_exp)):
        if w4:
            _check(t, torch.uint8, name, dev)
            if t.data_ptr() % 4:
                raise ValueError(f"{name} must be 4-byte aligned")
    kd = 2 if w4 else 1  # K elements per weight byte or element
    if router.shape != (E, dim) or w_gate_up.shape != (E, 2 * ffn, dim // kd) or w_down.shape != (E, dim, ffn // kd):
        raise ValueError(f"expected router [{E}, {dim}], w_gate_up [{E}, {2 * ffn}, {dim // kd}], "
                         f"w_down [{E}, {dim}, {ffn // kd}]")
    for name, t in (("resid", resid), ("router", router), ("w_gate_up", w_gate_up), ("w_down", w_down)):
        if t.data_ptr() % 16:
            raise ValueError(f"{name} must be 16-byte aligned")
    plan = moe_ffn_plan(B, dim, ffn, moe)
    if ss.dim() != 2 or ss.shape[1] != MAX_ROWS or ss.shape[0] < plan.cb_grid or ss.shape[0] < 1:
        raise ValueError(f"ss must be fp32 [parts >= {plan.cb_grid}, {MAX_ROWS}]")
    ss_in = ss.shape[0] if ss_in is None else ss_in
    if not _int_in(ss_in, 1, ss.shape[0] + 1):
        raise ValueError(f"ss_in must be an int in 1..{ss.shape[0]}, got {ss_in!r}")
    want = {"route_id": (torch.int32, (B, top_k)), "route_w": (torch.float32, (B, top_k)),
            "route_rs": (torch.float32, (B,)), "moe_h": (torch.bfloat16, (B * top_k, ffn)),
            "moe_part": (torch.float32, (B, top_k, dim))}
    res = {}
    for name, (dtype, shape) in want.items():
        t = out[name] if out is not None else torch.empty(shape, dtype=dtype, device=dev)
        _check(t, dtype, name, dev)
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
        res[name] = t
    if w4:
        _ok(lib().p2pt_moe_ffn_mxfp4(_p(resid), _p(ss), ss_in, _p(router), _p(w_gate_up), _p(w_down),
                                     _p(res["route_id"]), _p(res["route_w"]), _p(res["route_rs"]), _p(res["moe_h"]),
                                     _p(res["moe_part"]), B, dim, ffn, E, top_k, moe.norm_topk, eps, _stream(resid),
                                     _p(gate_up_exp), _p(down_exp)), "moe_ffn")
        return res
    if w8:
        _ok(lib().p2pt_moe_ffn_experts(_p(resid), _p(ss), ss_in, _p(router), _p(w_gate_up), _p(w_down),
                                       _p(res["route_id"]), _p(res["route_w"]), _p(res["route_rs"]), _p(res["moe_h"]),
                                       _p(res["moe_part"]), B, dim, ffn, E, top_k, moe.norm_topk, eps, _stream(resid),
                                       ctypes.byref(experts), _p(gate_up_scale), _p(down_scale)), "moe_ffn")
        return res
    _ok(lib().p2pt_moe_ffn(_p(resid), _p(ss), ss_in, _p(router), _p(w_gate_up), _p(w_down), _p(res["route_id"]),
                           _p(res["route_w"]), _p(res["route_rs"]), _p(res["moe_h"]), _p(res["moe_part"]), B, dim, ffn,
                           E, top_k, moe.norm_topk, eps, _stream(resid)), "moe_ffn")
    return res


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


def lm_score_plan(V: int, dim: int, rows: int) -> LmScorePlan:
    """The grids of ``lm_score_`` for a ``[V, dim]`` LM head and ``rows`` rows of resid (host only: the library, no
    GPU). A function of the shapes alone."""
    plan = LmScorePlan()
    if not all(_int_in(v, 1, 1 << 31) for v in (V, dim, rows)) or \
            lib().p2pt_lm_score_plan(V, dim, rows, ctypes.byref(plan)) != 0:
        raise ValueError(f"lm_score needs V >= 1, dim a multiple of 32 up to 16384 and 1..{MAX_ROWS} rows, got V {V!r}, "
                         f"dim {dim!r}, rows {rows!r}")
    return plan


def lm_score_(resid: torch.Tensor, lm_head: torch.Tensor, scale: torch.Tensor | None, eps: float,
              target: torch.Tensor, lse: torch.Tensor, z_target: torch.Tensor, z_top: torch.Tensor,
              id_top: torch.Tensor, work: torch.Tensor | None = None, check_targets: bool = True) -> None:
    """Score rows of the fused step's final residual against the LM head without writing a logit (lm_score.hip;
    docs/PROMPT_LOGPROBS.md). ``resid`` is bf16 [rows <= 64, dim]; ``lm_head`` the fused table's entry, [V, dim] with
    the final-norm weight folded in, bf16 with ``scale`` None or e4m3 (or uint8) bytes with ``scale`` fp32 (V,);
    ``target`` int32 (rows,), a negative entry turns its row off. For every other row, with
    ``z[v] = ((x . W'[v]) * scale[v]) / rms(x)`` held in fp32 from the MFMA accumulator on, ``lse`` = log sum exp z,
    ``z_target`` = z[target], ``z_top`` = max z and ``id_top`` its lowest id (fp32, fp32, fp32, int32, each (rows,));
    the token's log-probability is ``z_target - lse``. A row that is off touches no output. ``work``: int32 scratch
    of ``lm_score_plan(..).work_words`` words (allocated when None). ``check_targets=False`` skips the one check
    that reads the device (``target < V``; a target past V matches no column and leaves ``z_target`` at -inf): a
    caller that built the targets on the host, as the engine does, has checked them there."""
    _check(resid, torch.bfloat16, "resid")
    dev = resid.device
    if resid.dim() != 2 or not 1 <= resid.shape[0] <= MAX_ROWS:
        raise ValueError(f"resid must be [rows <= {MAX_ROWS}, dim], got {tuple(resid.shape)}")
    rows, dim = resid.shape
    if not isinstance(lm_head, torch.Tensor) or lm_head.dim() != 2 or lm_head.shape[1] != dim or lm_head.shape[0] < 1:
        raise ValueError(f"lm_head must be [V >= 1, {dim}], got {tuple(getattr(lm_head, 'shape', ()))}")
    V = lm_head.shape[0]
    plan = lm_score_plan(V, dim, rows)
    w8 = lm_head.dtype in WEIGHT_FP8_DTYPES
    _check(lm_head, lm_head.dtype if w8 else torch.bfloat16, "lm_head", dev)
    if w8:
        if scale is None:
            raise ValueError("an FP8 lm_head needs its fp32 row scales")
        _check(scale, torch.float32, "scale", dev)
        if scale.shape != (V,):
            raise ValueError(f"scale shape {tuple(scale.shape)} != ({V},)")
    elif scale is not None:
        raise ValueError("a bf16 lm_head has no scales")
    _check(target, torch.int32, "target", dev)
    for name, t, dt in (("lse", lse, torch.float32), ("z_target", z_target, torch.float32),
                        ("z_top", z_top, torch.float32), ("id_top", id_top, torch.int32)):
        _check(t, dt, name, dev)
    if any(t.shape != (rows,) for t in (target, lse, z_target, z_top, id_top)):
        raise ValueError(f"target, lse, z_target, z_top and id_top must be ({rows},)")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 <= eps < float("inf"):
        raise ValueError(f"eps must be a finite number >= 0, got {eps!r}")
    if work is None:
        work = torch.empty(plan.work_words, dtype=torch.int32, device=dev)
    _check(work, torch.int32, "work", dev)
    if work.numel() < plan.work_words:
        raise ValueError(f"work holds {work.numel()} words, lm_score_plan asks for {plan.work_words}")
    if resid.data_ptr() % 16 or work.data_ptr() % 16 or lm_head.data_ptr() % (8 if w8 else 16):
        raise ValueError("resid, work and a bf16 lm_head must be 16-byte aligned, an FP8 lm_head 8-byte aligned")
    if check_targets and int(target.max().item()) >= V:
        raise ValueError(f"target ids must be below V = {V}")
    _ok(lib().p2pt_lm_score(_p(resid), rows, dim, _p(lm_head), _p(scale), int(w8), V, float(eps), _p(target), _p(work),
                            work.numel(), _p(lse), _p(z_target), _p(z_top), _p(id_top), _stream(resid)), "lm_score")


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


def _check_w4g(q, z, s, what: str):
    if not isinstance(q, torch.Tensor) or q.dtype != torch.uint8 or q.dim() != 2 or q.shape[1] % W4G_GROUP or \
            not q.shape[1]:
        raise TypeError(f"{what}: q must be uint8 [N, K] with K a multiple of {W4G_GROUP} (the group size)")
    groups = (q.shape[0], q.shape[1] // W4G_GROUP)
    if not isinstance(z, torch.Tensor) or z.dtype != torch.uint8 or tuple(z.shape) != groups:
        raise TypeError(f"{what}: z must be uint8 [N, K / {W4G_GROUP}], one zero point per group")
    if not isinstance(s, torch.Tensor) or s.dtype != torch.float16 or tuple(s.shape) != groups:
        raise TypeError(f"{what}: s must be fp16 [N, K / {W4G_GROUP}], one scale per group")
    if q.numel() and (int(q.max()) > 15 or int(z.max()) > W4G_ZERO_MAX):
        raise ValueError(f"{what}: q must be 0..15 and z 0..{W4G_ZERO_MAX}")
    if not bool(torch.isfinite(s).all()):
        raise ValueError(f"{what}: non-finite group scale")


def pack_weight_w4g(q: torch.Tensor, z: torch.Tensor, s: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """A grouped int4 weight ``W[n][k] = (q[n][k] - z[n][k // 128]) * s[n][k // 128]`` (``q`` uint8 [N, K] in 0..15,
    ``z`` uint8 [N, K / 128] in 0..16, ``s`` fp16 [N, K / 128]) to what ``k_skinny<.., W8 = 3>`` loads
    (docs/WEIGHT_INT4.md): ``(nibbles, groups)``.

    ``nibbles`` uint8 [N, K / 2], every row in k-step-quad order: byte ``64 Q + 16 kq + 4 u + b`` holds
    ``k = 128 Q + 32 u + 8 kq + 2 b`` in its low nibble and ``k + 1`` in its high one, for quad Q, lane group kq,
    k-step u of the quad and byte b, each of the last three 0..3 (``block_expert_mxfp4``'s order). The 16 bytes of a
    lane group are then its 8 k-values of the quad's four k-steps: one load. ``groups`` int32 [N, K / 128]: the fp16
    bits of ``s`` in bits 0..15 and ``z`` in bits 16..23. The one function that makes this order."""
    _check_w4g(q, z, s, "pack_weight_w4g")
    natural = q[:, 0::2] | (q[:, 1::2] << 4)
    nibbles = natural[:, _expert_perm_mxfp4(natural.shape[1], q.device)].contiguous()
    groups = (s.view(torch.int16).to(torch.int32) & 0xffff) | (z.to(torch.int32) << 16)
    return nibbles, groups.contiguous()


def unpack_weight_w4g(nibbles: torch.Tensor, groups: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The inverse of ``pack_weight_w4g``: ``(q, z, s)``."""
    if not isinstance(nibbles, torch.Tensor) or nibbles.dtype != torch.uint8 or nibbles.dim() != 2 or \
            nibbles.shape[1] % (W4G_GROUP // 2) or not isinstance(groups, torch.Tensor) or \
            groups.dtype != torch.int32 or tuple(groups.shape) != (nibbles.shape[0], nibbles.shape[1] * 2 // W4G_GROUP):
        raise TypeError(f"unpack_weight_w4g takes uint8 nibble bytes [N, K / 2] and int32 group words "
                        f"[N, K / {W4G_GROUP}]")
    natural = torch.empty_like(nibbles)
    natural[:, _expert_perm_mxfp4(nibbles.shape[1], nibbles.device)] = nibbles
    q = torch.stack([natural & 15, natural >> 4], 2).reshape(nibbles.shape[0], -1).contiguous()
    s = (groups & 0xffff).to(torch.int16).view(torch.float16)
    return q, ((groups >> 16) & 0xff).to(torch.uint8), s


def quantize_weight_w4g(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One GEMM weight ``w`` (fp32 [N, K], K a multiple of 128, in the fused table's row order, no norm weight folded
    in) to grouped int4 by asymmetric round-to-nearest, nothing calibrated: ``(q, z, s)`` as ``pack_weight_w4g`` takes
    them. Plain torch on ``w``'s device: runs without a GPU.

    Per group of 128 consecutive k of a row, with lo = min(group, 0) and hi = max(group, 0) (zero lies in the range, as
    in GPTQ's and AWQ's own quantisers, so a zero point in 0..15 always reaches lo): ``s = fp16((hi - lo) / 15)``,
    ``z = clamp(round(-lo / s), 0, 15)`` and ``q = clamp(round(w / s) + z, 0, 15)``. z is 0 for a group without negative
    values and 15 for one without positive ones. A group whose s would round below fp16's smallest normal, 2^-14 (an
    all-zero group among them), gets s = 2^-14: every element then still lies within 15 steps. A scale beyond fp16's range is
    refused, as are non-finite weights. Error: |w - (q - z) s| <= s / 2 + 16 * 2^-11 * s per element (the second term
    is the fp16 rounding of s, which can push the largest element just past step 15), before bf16's own rounding of
    the dequantised value."""
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 2 or w.shape[1] % W4G_GROUP or \
            not w.shape[1]:
        raise TypeError(f"quantize_weight_w4g takes an fp32 [N, K] tensor with K a multiple of {W4G_GROUP}")
    if not bool(torch.isfinite(w).all()):
        raise ValueError("non-finite weight (NaN or inf): refusing to quantise it to int4")
    N, K = w.shape
    g = w.reshape(N, K // W4G_GROUP, W4G_GROUP)
    lo, hi = g.amin(2).clamp(max=0.0), g.amax(2).clamp(min=0.0)
    s32 = (hi - lo) / 15.0
    if bool((s32 > 65504.0).any()):
        raise ValueError("a group's scale exceeds fp16's range: refusing to quantise it to int4")
    s = s32.to(torch.float16).clamp(min=2.0 ** -14)
    sf = s.float()
    z = torch.round(-lo / sf).clamp(0, 15)
    q = (torch.round(g / sf[:, :, None]) + z[:, :, None]).clamp(0, 15)
    return q.to(torch.uint8).reshape(N, K), z.to(torch.uint8), s


def dequantize_weight_w4g(q: torch.Tensor, z: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """``W_deq = bf16_rne(fp32(q - z) * fp32(s))``, bf16 [N, K]: the weight the int4 kernels compute with, by
    definition. The fp32 product is exact (at most 5 + 11 significand bits), so there is one rounding."""
    _check_w4g(q, z, s, "dequantize_weight_w4g")
    d = q.float() - z.float().repeat_interleave(W4G_GROUP, 1)
    return (d * s.float().repeat_interleave(W4G_GROUP, 1)).to(torch.bfloat16)


# ------------------------------------------------------------ LoRA adapters (docs/LORA.md)
def lora_rank(*ranks: int) -> int:
    """The padded rank R of a projection whose stacked parts have PEFT ranks ``ranks`` (0: the adapter leaves the
    module out): their sum rounded up to a whole 16-rank MFMA tile, 16 at least."""
    for r in ranks:
        if not _int_in(r, 0, LORA_MODULE_MAX_RANK + 1):
            raise ValueError(f"a LoRA module's rank must be an int in 0..{LORA_MODULE_MAX_RANK}, got {r!r}")
    return max(16, (sum(ranks) + 15) // 16 * 16)


def lora_shapes(cfg) -> dict:
    """name -> (part output sizes, K) of the four projections of a model of ``cfg`` (a ``LlamaConfig``), parts in
    ``LORA_PARTS``' order."""
    q, kv = cfg.n_heads * cfg.head_dim, cfg.n_kv_heads * cfg.head_dim
    return {"wqkv": ((q, kv, kv), cfg.dim), "wo": ((cfg.dim,), q), "w_gate_up": ((cfg.ffn, cfg.ffn), cfg.dim),
            "w_down": ((cfg.dim,), cfg.ffn)}


def pack_lora(cfg, name: str, lora_A, lora_B, scaling, norm_weight: torch.Tensor | None = None,
              rank: int | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """One adapter's tables for projection ``name`` ("wqkv", "wo", "w_gate_up", "w_down") as ``k_lora_delta`` reads
    them: ``(A' [R, K], B' [N, R])``, bf16, on the parts' device. Plain torch: runs without a GPU.

    ``lora_A`` / ``lora_B``: per part of ``LORA_PARTS[name]`` PEFT's ``lora_A.weight [r, K]`` and ``lora_B.weight
    [n_part, r]``, or None for a module the adapter leaves out (a bare tensor for a one-part projection).
    ``scaling``: PEFT's ``lora_alpha / r`` (``lora_alpha / sqrt(r)`` with ``use_rslora``), one float or one per part;
    it is folded into B'. The parts are stacked: A' = [A_0; A_1; ..] and B' block-structured (part i's rows times part
    i's ranks, zeros elsewhere), so B' A' x is each part's own B_i A_i x. ``norm_weight``: the RMSNorm weight [K] that
    the base weight has folded into its columns (wqkv: attn_norm, w_gate_up: ffn_norm; required there, refused
    elsewhere): folded into A's columns likewise, since the kernel reads the raw residual. B' rows go through
    ``fused_row_perm``, the base weight's row order. ``rank``: the R to pad to with zero rows of A' and zero columns
    of B' (default ``lora_rank`` of the parts' ranks); every adapter of a decoder shares it. The products are formed
    in fp32 and rounded to bf16 once."""
    from p2p_llm_tunnel_amd.models.tiny_llm import FOLDED_NORM, fused_row_perm
    if name not in LORA_PARTS:
        raise ValueError(f"pack_lora: {name!r} is no projection of a layer ({', '.join(LORA_PARTS)})")
    parts = LORA_PARTS[name]
    sizes, K = lora_shapes(cfg)[name]
    if isinstance(lora_A, torch.Tensor) or lora_A is None:
        lora_A, lora_B = [lora_A], [lora_B]
    if len(lora_A) != len(parts) or len(lora_B) != len(parts):
        raise ValueError(f"{name}: one lora_A and one lora_B per part {parts} (None for a module left out)")
    scal = [float(scaling)] * len(parts) if isinstance(scaling, (int, float)) else [float(s) for s in scaling]
    if (norm_weight is not None) != (name in FOLDED_NORM):
        raise ValueError(f"{name}: " + ("the preceding norm's weight is folded into A' (norm_weight is required)"
                                       if name in FOLDED_NORM else "no norm precedes this projection"))
    ranks = []
    for mod, A, B, n in zip(parts, lora_A, lora_B, sizes):
        if (A is None) != (B is None):
            raise ValueError(f"{mod}: lora_A and lora_B come together")
        if A is not None and (A.dim() != 2 or B.dim() != 2 or A.shape[1] != K or tuple(B.shape) != (n, A.shape[0])):
            raise ValueError(f"{mod}: lora_A {tuple(A.shape)} and lora_B {tuple(B.shape)} do not match the base model "
                             f"(lora_A [r, {K}], lora_B [{n}, r])")
        ranks.append(0 if A is None else A.shape[0])
    R = lora_rank(*ranks) if rank is None else rank
    if R % 16 or not sum(ranks) <= R <= LORA_MAX_RANK:
        raise ValueError(f"{name}: rank must be a multiple of 16 in {max(16, sum(ranks))}..{LORA_MAX_RANK}, got {R}")
    dev = next((A.device for A in lora_A if A is not None), "cpu")
    Ap = torch.zeros(R, K, dtype=torch.float32, device=dev)
    Bp = torch.zeros(sum(sizes), R, dtype=torch.float32, device=dev)
    r0 = n0 = 0
    for A, B, n, s in zip(lora_A, lora_B, sizes, scal):
        if A is not None:
            r = A.shape[0]
            Ap[r0:r0 + r] = A.float() if norm_weight is None else A.float() * norm_weight.float().to(dev)[None, :]
            Bp[n0:n0 + n, r0:r0 + r] = B.float() * s
            r0 += r
        n0 += n
    if not bool(torch.isfinite(Ap).all()) or not bool(torch.isfinite(Bp).all()):
        raise ValueError(f"{name}: non-finite adapter weight (NaN or inf)")
    perm = fused_row_perm(cfg, name, dev)
    if perm is not None:
        Bp = Bp[perm]
    return Ap.to(torch.bfloat16).contiguous(), Bp.to(torch.bfloat16).contiguous()


def unpack_lora(cfg, name: str, A: torch.Tensor, B: torch.Tensor,
                norm_weight: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """``pack_lora``'s inverse, in fp64: ``(A [R, K], B [N, R])`` with the norm weight divided out of A's columns and
    B's rows back in the plain order of the stacked parts, so that ``B @ A`` is the delta of the plain weight."""
    from p2p_llm_tunnel_amd.models.tiny_llm import fused_row_perm
    A64, B64 = A.double(), B.double()
    if norm_weight is not None:
        A64 = A64 / norm_weight.double().to(A.device)[None, :]
    perm = fused_row_perm(cfg, name, B.device)
    if perm is not None:
        plain = torch.empty_like(B64)
        plain[perm] = B64
        B64 = plain
    return A64, B64


def _check_lora_shapes(M: int, N: int, K: int, R: int, n: int) -> None:
    if not 1 <= M <= MAX_ROWS or N < 16 or N % 16 or K < 32 or K % 32:
        raise ValueError(f"lora: need 1 <= M <= {MAX_ROWS}, N % 16 == 0, K % 32 == 0, got M {M}, N {N}, K {K}")
    if R < 16 or R % 16 or R > LORA_MAX_RANK:
        raise ValueError(f"lora: the padded rank must be a multiple of 16 up to {LORA_MAX_RANK}, got {R}")
    if not 1 <= n <= LORA_MAX_ADAPTERS:
        raise ValueError(f"lora: 1..{LORA_MAX_ADAPTERS} adapters, got {n}")
    if max(M * K, R * K, N * R) * 2 >= GEMM_OPERAND_LIMIT:
        raise ValueError("lora: x, one adapter's A' and one adapter's B' must each stay below 2 GiB")


def lora_plan(M: int, N: int, K: int, R: int, n_adapters: int = 1) -> LoraPlan:
    """What ``k_lora_delta`` launches for M rows of a projection [N, K] at padded rank R (host only: the library, no
    GPU): (column tiles of delta, 16-row tiles) workgroups of ``waves`` waves, ``cols`` delta columns each, and
    ``passes`` shrink passes per distinct adapter of a row tile."""
    _check_lora_shapes(M, N, K, R, n_adapters)
    plan = LoraPlan()
    _ok(lib().p2pt_lora_plan(M, N, K, R, n_adapters, ctypes.byref(plan)), "lora_plan")
    return plan


def lora_delta(x: torch.Tensor, A: torch.Tensor, B: torch.Tensor, aid: torch.Tensor) -> torch.Tensor:
    """``k_lora_delta`` alone: fp32 ``delta[m] = B[aid[m]] @ bf16(A[aid[m]] @ x[m])`` for every row, exactly 0 where
    ``aid[m]`` is -1. x bf16 [M <= 64, K]; A bf16 [n, R, K]; B bf16 [n, N, R]; aid int32 [M]. The shapes are judged
    first, from the shapes alone, so a refusal needs no device."""
    for name, t in (("x", x), ("A", A), ("B", B), ("aid", aid)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor")
    if x.dim() != 2 or A.dim() != 3 or B.dim() != 3 or A.shape[2] != x.shape[1] or B.shape[0] != A.shape[0] or \
            B.shape[2] != A.shape[1] or tuple(aid.shape) != (x.shape[0],):
        raise ValueError("shapes must be x [M, K], A [n, R, K], B [n, N, R], aid [M]")
    (M, K), (n, R, _), N = x.shape, A.shape, B.shape[1]
    _check_lora_shapes(M, N, K, R, n)
    _check(x, torch.bfloat16, "x")
    _check(A, torch.bfloat16, "A", x.device)
    _check(B, torch.bfloat16, "B", x.device)
    _check(aid, torch.int32, "aid", x.device)
    delta = torch.empty(M, N, dtype=torch.float32, device=x.device)
    _ok(lib().p2pt_lora_delta(_p(x), _p(aid), _p(A), _p(B), _p(delta), M, N, K, R, n, _stream(x)), "lora_delta")
    return delta


def check_lora(cfg_dims: LlamaDims, lora, device=None) -> tuple[int, tuple]:
    """``lora`` as ``FusedLlamaDecoder`` takes it: one dict per layer, name -> ``(A [n, R, K], B [n, N, R])`` (bf16,
    the adapters stacked on dim 0) for each of ``LAYER_GEMMS``, the same n and the same R per projection in every
    layer. Returns (n, the four ranks). Shapes and dtypes only unless ``device`` is given."""
    d = cfg_dims
    shapes = {"wqkv": ((d.H + 2 * d.Hkv) * d.D, d.dim), "wo": (d.dim, d.H * d.D), "w_gate_up": (2 * d.ffn, d.dim),
              "w_down": (d.dim, d.ffn)}
    if not isinstance(lora, (list, tuple)) or len(lora) != d.n_layers:
        raise ValueError(f"lora must hold one dict per layer ({d.n_layers})")
    n, ranks = None, {}
    for L, layer in enumerate(lora):
        if set(layer) != set(LAYER_GEMMS):
            raise ValueError(f"layer {L}: lora needs exactly {', '.join(LAYER_GEMMS)}")
        for name in LAYER_GEMMS:
            A, B = layer[name]
            N, K = shapes[name]
            for what, t in (("A'", A), ("B'", B)):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16 or t.dim() != 3:
                    raise TypeError(f"{label(name, L)} lora {what}: expected a bf16 tensor with the adapters on dim 0")
            n = A.shape[0] if n is None else n
            R = ranks.setdefault(name, A.shape[1])
            if tuple(A.shape) != (n, R, K) or tuple(B.shape) != (n, N, R):
                raise ValueError(f"{label(name, L)} lora: A' {tuple(A.shape)} and B' {tuple(B.shape)}, not "
                                 f"({n}, {R}, {K}) and ({n}, {N}, {R})")
            _check_lora_shapes(MAX_ROWS, N, K, R, n)
            if device is not None:
                _check(A, torch.bfloat16, f"{label(name, L)} lora A'", device)
                _check(B, torch.bfloat16, f"{label(name, L)} lora B'", device)
                if A.data_ptr() % 16 or B.data_ptr() % 16:
                    raise ValueError(f"{label(name, L)} lora: A' and B' must be 16-byte aligned")
    return n, tuple(ranks[name] for name in LAYER_GEMMS)


# Every workspace buffer in the order of decode_fused.hip's WsBuf, which p2pt_llama_step_ws reports them in. The first
# WS_DENSE every step has (qkv empty without QK-norm); then an MoE model's five, an int4 model's xg, the adapters' delta.
WS_BUFFERS = (("resid", torch.bfloat16), ("q", torch.bfloat16), ("attn", torch.bfloat16), ("h", torch.bfloat16),
              ("ss", torch.float32), ("part_o", torch.float32), ("part_ml", torch.float32), ("am_val", torch.float32),
              ("am_idx", torch.int32), ("counters", torch.int32), ("qkv", torch.bfloat16), ("route_id", torch.int32),
              ("route_w", torch.float32), ("route_rs", torch.float32), ("moe_h", torch.bfloat16),
              ("moe_part", torch.float32), ("xg", torch.bfloat16), ("delta", torch.float32))
WS_DENSE = 11


def workspace_layout(dims: LlamaDims, opts: StepOptions) -> tuple:
    """The workspace of a step with ``opts`` (host only): its bytes, and ``{name: (dtype, byte offset, elements)}`` of
    the buffers it has, in ``WS_BUFFERS``' order: the dense ones always, a later one when it is not empty."""
    n = len(WS_BUFFERS)
    off, cnt = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
    nbytes = lib().p2pt_llama_step_ws(ctypes.byref(dims), ctypes.byref(opts), off, cnt, n)
    if nbytes == 0:
        raise ValueError("model dims not supported by the fused decode kernels")
    # Each buffer starts where the 256-byte-aligned one before it ends: a list that differs from WsBuf fails here.
    end = 0
    for (name, dtype), o, c in zip(WS_BUFFERS, off, cnt):
        if o != end:
            raise RuntimeError(f"workspace layout: buffer list out of step with decode_fused.hip at {name}")
        end = o + (c * dtype.itemsize + 255) // 256 * 256
    if end != nbytes:
        raise RuntimeError("workspace layout: buffer list out of step with decode_fused.hip")
    return nbytes, {name: (dtype, o, c) for i, ((name, dtype), o, c) in enumerate(zip(WS_BUFFERS, off, cnt))
                    if i < WS_DENSE or c}


def _check_fp8g128(q, scale, what: str):
    if not isinstance(q, torch.Tensor) or q.dtype not in WEIGHT_FP8_DTYPES or q.dim() != 2 or \
            q.shape[1] % F8G_GROUP or not q.shape[1]:
        raise TypeError(f"{what}: q must be e4m3 (or uint8) bytes [N, K] with K a multiple of {F8G_GROUP}")
    if scale is not None and (not isinstance(scale, torch.Tensor) or scale.dtype != torch.float32 or
                              tuple(scale.shape) != (q.shape[0], q.shape[1] // F8G_GROUP)):
        raise TypeError(f"{what}: scale must be fp32 [N, K / {F8G_GROUP}], one per output row and {F8G_GROUP} k")


def pack_weight_fp8g128(q: torch.Tensor) -> torch.Tensor:
    """The e4m3 bytes ``[N, K]`` of a block-scaled FP8 weight from natural K order to what ``k_skinny<.., W8 = 4>`` loads
    (docs/WEIGHT_FP8G128.md): every row in the k-step-pair order ``WeightTable`` states. The scales do not move. The one
    function that makes this order; a new contiguous tensor of ``q``'s dtype."""
    _check_fp8g128(q, None, "pack_weight_fp8g128")
    return q.view(torch.uint8)[:, _expert_perm(q.shape[1], q.device)].contiguous().view(q.dtype)


def unpack_weight_fp8g128(q: torch.Tensor) -> torch.Tensor:
    """The inverse of ``pack_weight_fp8g128``: device order back to natural K order."""
    _check_fp8g128(q, None, "unpack_weight_fp8g128")
    out = torch.empty_like(q.view(torch.uint8))
    out[:, _expert_perm(q.shape[1], q.device)] = q.view(torch.uint8)
    return out.view(q.dtype)


def quantize_weight_fp8g128(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """One GEMM weight ``w`` (fp32 [N, K], K a multiple of 128, in the fused table's row order, no norm weight folded
    in) to block-scaled FP8 per 1 x 128 group, nothing calibrated: ``(q, scale)``, e4m3 ``[N, K]`` in natural K order and
    fp32 ``[N, K / 128]`` with ``scale = max |group| / 448`` (1.0 for a group whose maximum is zero or so small that the
    division underflows to zero) and ``q`` the e4m3fn byte, round to nearest even, of ``w / scale`` (the division in
    fp32): ``quantize_weight_fp8``'s rule on every group. Plain torch on ``w``'s device: runs without a GPU."""
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 2 or w.shape[1] % F8G_GROUP or \
            not w.shape[1]:
        raise TypeError(f"quantize_weight_fp8g128 takes an fp32 [N, K] tensor with K a multiple of {F8G_GROUP}")
    N, K = w.shape
    q, scale = quantize_weight_fp8(w.reshape(N * (K // F8G_GROUP), F8G_GROUP))
    return q.reshape(N, K), scale.reshape(N, K // F8G_GROUP)


def dequantize_weight_fp8g128(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``e4m3(q) * scale[n][k // 128]`` in fp32 ``[N, K]`` (``q`` in natural K order): the weight the block-scaled FP8
    kernels compute with. One fp32 rounding per element, none when the scales are powers of two."""
    _check_fp8g128(q, scale, "dequantize_weight_fp8g128")
    return q.view(torch.float8_e4m3fn).float() * scale.repeat_interleave(F8G_GROUP, 1)


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
    MXFP4 bytes with e8m0 block scales, run by the ``k_skinny<.., W8 = 2>`` instantiations, and an FP8 LM head;
    "int4g128" (docs/WEIGHT_INT4.md, ``pack_weight_w4g``) has them as grouped uint4 with an fp16 scale and a zero point per
    128 k, run by the ``W8 = 3`` instantiations on ``step_plan(.., weight_format="int4g128")``, with a bf16 LM head; its
    workspace has one more buffer, xg;
    "fp8g128" (docs/WEIGHT_FP8G128.md, ``pack_weight_fp8g128``) has them as e4m3 bytes with one fp32 scale per row and
    128 k, run by the ``W8 = 4`` instantiations on ``step_plan(.., weight_format="fp8g128")``, with a bf16 LM head and
    the dense bf16 workspace.
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

    ``chunk_attn`` (docs/CHUNK_ATTN.md; off by default, and then nothing above changes): in a step of more than 16
    rows, every layer without a window attends with ``k_attn_chunk`` on ``chunk_plan``'s grid, one K/V pass per 16-row
    tile and distinct slot in it, instead of ``k_attn``'s one per row. Steps of up to 16 rows and windowed layers
    launch what they did; ``step_plan`` and the workspace are the same.

    ``moe`` (a ``MoeDims``; docs/MOE.md; None, and then nothing above changes): a routed-expert FFN. ``dims.ffn`` is
    the per-expert size, the table is ``WeightTable(.., moe=moe)`` (stacked experts and a router per layer, bf16
    only), and each layer's gate/up and down kernels give way to ``k_moe_route``, ``k_moe_gate_up``, ``k_moe_down`` and
    ``k_moe_combine`` on ``moe_plan``'s grids: 7 kernels per layer, still one capturable call.
    ``expert_format`` (``as_expert_format``; with ``moe`` only; docs/MOE_FP8.md): "fp8" has the stacked experts as
    e4m3 bytes in ``block_expert_fp8``'s order with fp32 row scales after the table
    (``WeightTable(.., expert_format=)``), run by the FP8 instantiations of ``k_moe_gate_up`` and ``k_moe_down`` on the
    same plan; "mxfp4" (docs/MOE_MXFP4.md) has them as nibble bytes in ``block_expert_mxfp4``'s order with their e8m0
    block scales after the table, run by the MXFP4 instantiations; everything else of the model stays bf16. None or
    "bf16": nothing above changes.

    ``lora`` (docs/LORA.md; None, and then nothing above changes): up to 8 LoRA adapters beside the base weights, as
    ``check_lora`` describes them (``pack_lora`` builds one adapter's tables). Dense bf16 models without QK-norm only.
    The workspace grows by one buffer, delta, and ``step(.., adapters=)`` names each row's adapter: ahead of each of a
    layer's four projections ``k_lora_delta`` writes the rows' fp32 low-rank term there and the projection runs as
    its ``k_skinny<.., LORA = 1>`` variant on the same ``step_plan``, which adds it to the accumulator ahead of its
    epilogue. ``adapters=None`` launches the base step, kernel for kernel.

    Holds the weight pointer table and a zero-initialised workspace; ``step``
    validates the per-call tensors and launches on the current stream (capturable
    into a hipGraph: no host sync, no allocation, grids sized by the row count).
    """

    def __init__(self, dims: LlamaDims, weights: list, k_cache: torch.Tensor, v_cache: torch.Tensor,
                 weight_fp8: bool = False, kv_scales: torch.Tensor | None = None, windows=None, weight_format=None,
                 chunk_attn: bool = False, moe: MoeDims | None = None, expert_format=None, lora=None):
        self.dims = dims
        self.moe = check_moe(moe, dims.dim, dims.ffn)
        self.expert_format = as_expert_format(expert_format, self.moe, dims.dim, dims.ffn)
        if not isinstance(chunk_attn, bool):
            raise TypeError(f"chunk_attn must be a bool, got {chunk_attn!r}")
        self.chunk_attn = chunk_attn
        self.windows = check_windows(windows, dims.n_layers)
        self.weight_format = fmt = as_weight_format(weight_fp8, weight_format)
        self.weight_fp8 = fmt.layers == 1  # FP8 throughout
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
        self.table = table = WeightTable(dims, weight_format=fmt, moe=self.moe, expert_format=self.expert_format)
        if len(weights) != len(table):
            raise ValueError(f"weight table: embed, final_norm, lm_head, "
                             + ("inv_freq, " if dims.rope_table else "") + f"then {table.per_layer} per layer "
                             "(wqkv, w_gate_up and lm_head with the preceding norm weight folded in"
                             + ("; q_norm and k_norm last)" if dims.qk_norm else
                                "; bqkv last)" if dims.qkv_bias else ")")
                             + ("; weight_fp8: then the fp32 row scales, lm_head's and four per layer"
                                if self.weight_fp8 else "")
                             + ("; mxfp4: then lm_head's fp32 row scales and four e8m0 block-scale tensors per layer"
                                if fmt.layers == 2 else "")
                             + ("; int4: no norm weight folded into a layer's four, and then four group-word tensors "
                                "per layer" if fmt.layers == 3 else "")
                             + ("; fp8g128: no norm weight folded into a layer's four, and then four fp32 group-scale "
                                "tensors per layer" if fmt.layers == 4 else "")
                             + ("; MoE: w_gate_up and w_down stacked per expert, and router last in every layer"
                                if self.moe is not None else "")
                             + ("; FP8 experts: then their fp32 row scales, w_gate_up's and w_down's per layer"
                                if self.expert_format.w8 == 1 else "")
                             + ("; MXFP4 experts: then their e8m0 block scales, w_gate_up's and w_down's per layer"
                                if self.expert_format.w8 == 2 else ""))
        # Every entry's dtype and shape, from the description alone: a refusal here needs no device. A weight shorter
        # than dims says would be read past its end (k_skinny sizes its descriptors from dims, k_embed indexes vocab
        # rows). The norm slots the kernels do not read are held to (dim,) too.
        for e, t in zip(table, weights):
            name = label(e.name, e.layer)
            if not isinstance(t, torch.Tensor) or t.dtype not in e.dtypes:
                got = getattr(t, "dtype", type(t))
                if fmt.layers == 3 and e.dtypes in ((torch.uint8,), (torch.int32,)):
                    raise TypeError(f"{name}: the weight format is int4, so "
                                    + ("the group words must be torch.int32" if e.name.endswith(" scale")
                                       else "the weight must be nibble bytes (torch.uint8)") + f", got {got}")
                if fmt.layers == 4 and (len(e.dtypes) > 1 or e.name.endswith(" scale")):
                    raise TypeError(f"{name}: the weight format is fp8g128, so "
                                    + ("the group scales must be torch.float32" if e.name.endswith(" scale")
                                       else "the weight must be torch.float8_e4m3fn (or uint8)") + f", got {got}")
                if fmt.layers == 2 and e.dtypes == (torch.uint8,):
                    raise TypeError(f"{name}: the weight format is mxfp4, so "
                                    + ("the block scales must be e8m0 bytes (torch.uint8)" if e.name.endswith(" scale")
                                       else "the weight must be nibble bytes (torch.uint8)") + f", got {got}")
                if self.expert_format.w8 == 2 and e.dtypes == (torch.uint8,):
                    raise TypeError(f"{name}: the experts are MXFP4, so "
                                    + ("the block scales must be e8m0 bytes (torch.uint8)" if e.name.endswith(" scale")
                                       else "the weight must be nibble bytes (torch.uint8)") + f", got {got}")
                if len(e.dtypes) > 1 and self.expert_format.w8:
                    raise TypeError(f"{name}: the experts are FP8, so the weight must be torch.float8_e4m3fn (or "
                                    f"uint8), got {got}")
                if len(e.dtypes) > 1:
                    raise TypeError(f"{name}: weight_fp8 is set, so the weight must be torch.float8_e4m3fn (or uint8), "
                                    f"got {got}")
                if got == torch.float8_e4m3fn:
                    raise TypeError(f"{name} is {got}: an FP8 weight table needs weight_fp8=True")
                raise TypeError(f"{name}: expected {e.dtypes[0]}, got {got}")
            if tuple(t.shape) != e.shape:
                raise ValueError(f"{name} has shape {tuple(t.shape)}, not {e.shape}"
                                 + ("" if not e.name.endswith(" scale") else
                                    f": one group word per {W4G_GROUP} k" if e.dtypes == (torch.int32,) else
                                    f": one e8m0 byte per {MXFP4_BLOCK}-element block" if e.dtypes == (torch.uint8,)
                                    else f": one fp32 scale per output row and {F8G_GROUP} k" if fmt.layers == 4
                                    else ": one fp32 scale per expert and output row" if self.expert_format.w8
                                    else ": one fp32 scale per output row")
                                 + (": two nibbles per byte" if e.name in LAYER_GEMMS and e.dtypes == (torch.uint8,) and
                                    (fmt.layers in (2, 3) or self.expert_format.w8 == 2) else ""))
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
        self.lora = self._lora = None
        if lora is not None:
            if self.moe is not None or (fmt.layers, fmt.lm_head) != (0, 0):
                raise ValueError("lora: adapters need a dense model with bf16 weights (no MoE, no --weight-dtype)")
            if dims.qk_norm:
                raise ValueError("lora: adapters on a QK-norm model (Qwen3) are not supported: its QKV projection "
                                 "has no LoRA-delta kernel variant")
            n, ranks = check_lora(dims, lora, dev)
            ptrs = [layer[name][j].data_ptr() for layer in lora for name in LAYER_GEMMS for j in (0, 1)]
            self._lora_ptrs = (ctypes.c_void_p * len(ptrs))(*ptrs)
            self._lora = LoraTable(n_adapters=n, rank=(_INT * 4)(*ranks), tables=self._lora_ptrs)
            self.lora = lora  # keep alive
            # Every row count: K parts, and with them waves and load batch, change with it (host-only lookups).
            for B in range(1, MAX_ROWS + 1):
                if not plan_kernels_ok(dims, B, windows=self.windows, chunk_attn=chunk_attn, lora=ranks):
                    raise ValueError(f"the fused decode kernels have no LoRA variant for a step of {B} rows of this "
                                     "model")
        # What every call into the library takes beside dims. It points into kv_scales and the adapters, kept alive above.
        self._opts = step_options(fmt, kv_scales, self.windows, chunk_attn, self.moe, self.expert_format, self._lora)
        nbytes, _ = workspace_layout(dims, self._opts)
        # The MoE kernels a step can name (RT follows the row count; waves and load batch the per-expert shapes): a
        # plan without its instantiation is refused here with a message, not at the first launch with an error code.
        for B in (1, 17, 33):
            if self.moe is not None and not plan_kernels_ok(dims, B, windows=self.windows, weight_format=fmt,
                                                            chunk_attn=chunk_attn, moe=self.moe,
                                                            expert_format=self.expert_format):
                raise ValueError(f"the fused decode kernels have no instantiation for a step of {B} rows of this "
                                 f"MoE model ({self.moe!r}, dim {dims.dim}, ffn {dims.ffn})")
        self.weights = weights  # keep alive
        self._wptr = (ctypes.c_void_p * len(weights))(*[t.data_ptr() for t in weights])
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.k_cache, self.v_cache = k_cache, v_cache
        self.device = dev
        self._resid = None  # embed_pool's and lm_score's view of the workspace's resid buffer
        self._score_work = None  # lm_score's partials, allocated on first use

    _WS_BUFFERS = WS_BUFFERS[:WS_DENSE]  # the buffers p2pt_llama_ws_layout reports

    def workspace_views(self) -> dict:
        """Typed, shaped views into the workspace (no copies; the layout comes from
        ``p2pt_llama_step_ws``): what the last ``step`` left in each buffer.

        resid [64, dim], q [64, H, D], attn [64, H*D], h [64, ffn] (bf16);
        ss [parts, 64], part_o [64, H, nsplit, D], part_ml [64, H, nsplit, 2],
        am_val [blocks, 64] (fp32); am_idx [blocks, 64], counters [64*H] (int32);
        qkv [64, (H+2*Hkv)*D] (bf16): the raw QKV projection of a QK-norm model's
        last layer, as ``k_qknorm_rope`` read it ([0, ...] for other models).
        An int4 model adds xg [64, dim] (bf16): the last residual times the norm weight its producer was given.
        A decoder with ``lora`` adds delta [64, widest projection] (fp32): row m of the last ``k_lora_delta`` launch,
        the last layer's down projection, lies in ``delta.view(-1)[m * dim:(m + 1) * dim]``.
        An MoE model adds its last layer's route_id, route_w [64, top_k], route_rs [64], moe_h [64 * top_k, ffn]
        and moe_part [64, top_k, dim] (``moe_ffn``), and its h stays unwritten.
        Read them after a stream sync; only the first B rows of a step are defined."""
        d = self.dims
        nbytes, layout = workspace_layout(d, self._opts)
        if nbytes != self.ws.numel():
            raise RuntimeError("workspace layout: the buffers would lie outside the workspace")
        M, k = MAX_ROWS, self.moe.top_k if self.moe is not None else 0
        shapes = {"resid": (M, d.dim), "q": (M, d.H, d.D), "attn": (M, d.H * d.D), "h": (M, d.ffn), "ss": (-1, M),
                  "part_o": (M, d.H, -1, d.D), "part_ml": (M, d.H, -1, 2), "am_val": (-1, M), "am_idx": (-1, M),
                  "counters": (M * d.H,), "qkv": (M if d.qk_norm else 0, (d.H + 2 * d.Hkv) * d.D),
                  "route_id": (M, k), "route_w": (M, k), "route_rs": (M,), "moe_h": (M * k, d.ffn),
                  "moe_part": (M, k, d.dim), "xg": (M, d.dim), "delta": (M, -1)}
        return {name: self.ws[o:o + c * dtype.itemsize].view(dtype).view(*shapes[name])
                for name, (dtype, o, c) in layout.items()}

    def embed_pool(self, acc: torch.Tensor, out: torch.Tensor, jobs) -> None:
        """``embed_pool_`` over the rows the last ``step`` left in ``resid`` (the
        final residual of every row, prefill rows included), with the final-norm
        weight and this model's eps."""
        if self._resid is None:
            self._resid = self.workspace_views()["resid"]
        embed_pool_(self._resid, self.weights[self.table.index("final_norm")], acc, out, jobs, self.dims.eps)

    def lm_score(self, target: torch.Tensor, lse: torch.Tensor, z_target: torch.Tensor, z_top: torch.Tensor,
                 id_top: torch.Tensor) -> None:
        """``lm_score_`` over the first ``len(target)`` rows the last ``step`` left in ``resid``, with this model's
        LM head (and its row scales when it is FP8) and eps. The targets are the caller's, built on the host and
        below ``dims.vocab``: nothing here reads the device, so the call can follow a graph replay on the stream."""
        if self._resid is None:
            self._resid = self.workspace_views()["resid"]
        if self._score_work is None:
            words = lm_score_plan(self.dims.vocab, self.dims.dim, MAX_ROWS).work_words
            self._score_work = torch.empty(words, dtype=torch.int32, device=self.device)
        scale = self.weights[self.table.scale_index("lm_head")] if self.weight_format.lm_head else None
        lm_score_(self._resid[:target.shape[0]], self.weights[self.table.index("lm_head")], scale, self.dims.eps,
                  target, lse, z_target, z_top, id_top, self._score_work, check_targets=False)

    def step(self, tokens: torch.Tensor, pos: torch.Tensor, logits: torch.Tensor, ids: torch.Tensor,
             slots: torch.Tensor | None = None, emit_rows: int = 0, adapters: torch.Tensor | None = None) -> None:
        """One step over B <= 64 token rows (16-row MFMA tiles). Row b is token
        ``tokens[b]`` at cache position ``pos[b]`` of cache slot ``slots[b]``
        (default: slot b). Rows of one slot at consecutive positions are a prefill
        chunk (causal within the step). Only rows [0, emit_rows) get logits and
        ids (0: all): the LM head skips prefill rows that sample nothing.
        ``adapters`` (a decoder with ``lora`` only): int32 [B], the adapter of each row, -1 for none. None runs the
        base step."""
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
        if adapters is not None:
            if self._lora is None:
                raise ValueError("adapters: this decoder was built without lora")
            _check(adapters, torch.int32, "adapters", self.device)
            if adapters.shape != (B,):
                raise ValueError("adapters must be [B]")
        _ok(lib().p2pt_llama_step(ctypes.byref(d), ctypes.byref(self._opts), self._wptr, _p(self.k_cache),
                                  _p(self.v_cache), _p(tokens), _p(pos), _p(slots), B, emit_rows, _p(self.ws),
                                  self.ws.numel(), _p(logits), _p(ids), _stream(tokens), _p(adapters)), "llama_decode")
