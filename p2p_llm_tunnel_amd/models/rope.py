"""RoPE frequency scaling (``rope_scaling`` / ``rope_parameters`` of a Hugging Face config): the ``llama3`` rule
of Llama 3.1 / 3.2 / 3.3 and their distillations, and ``linear`` (position interpolation).

A model with default RoPE has none of this: its kernels compute ``inv_freq_i = theta^(-2i/D)`` inline. A scaled
model's frequencies do not follow one formula in i, so the host computes them once per model into an fp32 table
``inv_freq[D/2]`` (``inv_freq`` below), and every kernel that rotates q and k reads its frequency from that table
(``ops``: the ``EPI_ROPE_TAB`` epilogues, ``k_qknorm_rope<D, true>``, ``rope_qkv_cache(..., inv_freq=)``). The fp32
reference (``TinyLlama.reference_hidden``) takes the same table.

``llama3`` rescales by wavelength ``2 pi / inv_freq``: wavelengths above ``original_max_seq / low_freq_factor``
are divided by ``factor``, those below ``original_max_seq / high_freq_factor`` are kept, and the band between is
interpolated. ``linear`` divides every frequency by ``factor``. Both leave cos and sin unscaled (the attention
factor transformers returns with them is 1.0), so the kernels take no scale.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

KINDS = ("llama3", "linear")


@dataclass(frozen=True)
class RopeScaling:
    """Hashable, so that it can sit in the frozen ``LlamaConfig``. ``linear`` reads ``factor`` alone."""
    kind: str
    factor: float
    low_freq_factor: float = 0.0
    high_freq_factor: float = 0.0
    original_max_seq: int = 0

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"rope scaling kind {self.kind!r} is not supported (one of {list(KINDS)})")
        if not (math.isfinite(self.factor) and self.factor >= 1.0):
            raise ValueError(f"rope scaling: factor must be finite and >= 1, got {self.factor!r}")
        if self.kind == "llama3":
            lo, hi = self.low_freq_factor, self.high_freq_factor
            if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo < hi):
                raise ValueError("rope scaling: need 0 < low_freq_factor < high_freq_factor, got "
                                 f"{lo!r} and {hi!r}")
            if isinstance(self.original_max_seq, bool) or not isinstance(self.original_max_seq, int) \
                    or self.original_max_seq <= 0:
                raise ValueError("rope scaling: original_max_position_embeddings must be a positive int, got "
                                 f"{self.original_max_seq!r}")


def inv_freq(theta: float, head_dim: int, scaling: RopeScaling, device=None) -> torch.Tensor:
    """The fp32 table ``inv_freq[head_dim / 2]`` of a scaled model, computed on the CPU and moved to ``device``.

    The same torch fp32 expressions in the same order as transformers' ``ROPE_INIT_FUNCTIONS["llama3"]`` and
    ``["linear"]`` (``base ** (arange / dim)``, its reciprocal, then the rule), so the table is bit for bit
    theirs: tests/test_llama3_rope.py compares with ``torch.equal``."""
    base = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).to(dtype=torch.float) / head_dim))
    factor = scaling.factor
    if scaling.kind == "linear":
        out = base / factor
    else:
        old_len = scaling.original_max_seq
        low_wavelen = old_len / scaling.low_freq_factor
        high_wavelen = old_len / scaling.high_freq_factor
        wavelen = 2 * math.pi / base
        out = torch.where(wavelen > low_wavelen, base / factor, base)
        smooth = (old_len / wavelen - scaling.low_freq_factor) / (scaling.high_freq_factor - scaling.low_freq_factor)
        smoothed = (1 - smooth) * out / factor + smooth * out
        medium = ~(wavelen < high_wavelen) * ~(wavelen > low_wavelen)
        out = torch.where(medium, smoothed, out)
    out = out.contiguous()
    # Checked here, once and on the host, so that the per-step callers of the kernels need not read it back.
    if not bool((torch.isfinite(out) & (out > 0)).all()):
        raise ValueError(f"rope scaling: theta {theta!r} and {scaling!r} give frequencies that are not finite and > 0")
    return out.to(device) if device is not None else out


def from_hf(rope: dict) -> RopeScaling | None:
    """``RopeScaling`` from a config's ``rope_scaling`` (transformers 4) or ``rope_parameters`` (5) dict; None for
    default RoPE. Every key the type needs must be there: nothing is defaulted. Other types are refused."""
    kind = rope.get("rope_type", rope.get("type", "default"))
    if kind == "default":
        return None
    if kind not in KINDS:
        raise ValueError(f"rope type {kind!r} is not supported by the decode kernels")
    need = ("factor", "low_freq_factor", "high_freq_factor", "original_max_position_embeddings") \
        if kind == "llama3" else ("factor",)
    for k in need:
        v = rope.get(k)
        if v is None:
            raise ValueError(f"rope type {kind!r} needs {k!r} in the config's rope parameters")
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"rope type {kind!r}: {k!r} must be a number, got {v!r}")
    if kind == "linear":
        return RopeScaling("linear", float(rope["factor"]))
    orig = rope["original_max_position_embeddings"]
    if not math.isfinite(orig) or orig != int(orig):
        raise ValueError(f"rope type 'llama3': 'original_max_position_embeddings' must be an integer, got {orig!r}")
    return RopeScaling("llama3", float(rope["factor"]), float(rope["low_freq_factor"]),
                       float(rope["high_freq_factor"]), int(orig))
