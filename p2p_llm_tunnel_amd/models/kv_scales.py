"""Per-layer, per-KV-head scales of an FP8 (e4m3) KV cache (docs/KV_FP8.md).

A model with ``kv_dtype="fp8"`` may carry positive, finite fp32 scales ``k_scale[L][Hkv]`` and ``v_scale[L][Hkv]``.
The stored byte is ``e4m3(clamp(x * r))`` with ``r = fp32(1 / s)`` computed once on the host (``KvScales.table``),
and attention undoes the scale: K's joins the score scale, V's the final normalisation. Scale 1 is the unscaled
cache bit for bit; a power-of-two scale makes both multiplies exact.

``KvScales``            the value type: two fp32 ``[L][Hkv]`` tensors on the host, validated before any launch.
``parse_kv_scales``     ``--kv-scales checkpoint|FILE`` / ``start_server(kv_scales=)``.
``read_checkpoint``     the ``k_scale`` / ``v_scale`` (or ``kv_scale``) tensors of a checkpoint.
``absmax`` / ``scales_from_absmax``   the calibrator's reduction over cache tensors (scripts/calibrate_kv.py).
"""
from __future__ import annotations

import json
from dataclasses import dataclass

import torch

E4M3_MAX = 448.0
CHECKPOINT = "checkpoint"  # the --kv-scales value that reads the checkpoint's own tensors


def _as_table(x, name: str) -> torch.Tensor:
    try:
        t = torch.as_tensor(x, dtype=torch.float32).detach().cpu().contiguous()
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"kv_scales.{name} must be numbers [n_layers][n_kv_heads]: {e}") from None
    if t.dim() != 2 or t.numel() == 0:
        raise ValueError(f"kv_scales.{name} must be [n_layers][n_kv_heads], got shape {tuple(t.shape)}")
    return t


@dataclass(frozen=True, eq=False)
class KvScales:
    """``k`` and ``v``: fp32 ``[n_layers][n_kv_heads]`` (anything ``torch.as_tensor`` takes), kept on the host.
    Every entry is finite and > 0, and so is its fp32 reciprocal (checked here); ``check`` holds them to a model."""
    k: torch.Tensor
    v: torch.Tensor

    def __post_init__(self):
        object.__setattr__(self, "k", _as_table(self.k, "k"))
        object.__setattr__(self, "v", _as_table(self.v, "v"))
        if self.k.shape != self.v.shape:
            raise ValueError(f"kv_scales: k has shape {tuple(self.k.shape)} but v has {tuple(self.v.shape)}")
        for name, t in (("k", self.k), ("v", self.v)):
            if not bool((torch.isfinite(t) & (t > 0)).all()):
                raise ValueError(f"kv_scales.{name} entries must be finite and > 0")
            if not bool(torch.isfinite(1.0 / t).all()):
                raise ValueError(f"kv_scales.{name} entries must have a finite fp32 reciprocal (too close to zero)")

    def __eq__(self, other):
        return isinstance(other, KvScales) and torch.equal(self.k, other.k) and torch.equal(self.v, other.v)

    def check(self, n_layers: int, n_kv_heads: int, kv_dtype: str = "fp8") -> "KvScales":
        """Refuse scales that do not belong to a model of these sizes, or to a bf16 cache."""
        if kv_dtype != "fp8":
            raise ValueError(f"kv_scales need kv_dtype='fp8' (--kv-dtype fp8): a {kv_dtype} KV cache has no scales")
        if tuple(self.k.shape) != (n_layers, n_kv_heads):
            raise ValueError(f"kv_scales have shape {tuple(self.k.shape)}, but the model has (n_layers, n_kv_heads) = "
                             f"({n_layers}, {n_kv_heads})")
        return self

    def recip(self) -> tuple[torch.Tensor, torch.Tensor]:
        """``fp32(1 / s)`` of k and v: what the writers multiply by."""
        return 1.0 / self.k, 1.0 / self.v

    def table(self, device) -> torch.Tensor:
        """The device buffer the fused step takes: fp32 ``[4][L][Hkv]``: 1 / k, 1 / v, k, v."""
        rk, rv = self.recip()
        return torch.stack([rk, rv, self.k, self.v]).contiguous().to(device)

    def range(self) -> tuple[float, float, float, float]:
        return float(self.k.min()), float(self.k.max()), float(self.v.min()), float(self.v.max())

    def describe(self) -> str:
        """For the start-up log."""
        a, b, c, d = self.range()
        return f"k_scale {a:g} .. {b:g}, v_scale {c:g} .. {d:g} per layer and KV head"

    def to_json(self) -> str:
        return json.dumps({"k": self.k.tolist(), "v": self.v.tolist()})

    @classmethod
    def from_json(cls, text: str) -> "KvScales":
        try:
            raw = json.loads(text)
        except ValueError as e:
            raise ValueError(f"kv_scales: not JSON ({e})") from None
        if not isinstance(raw, dict) or set(raw) != {"k", "v"}:
            raise ValueError('kv_scales: the JSON must be {"k": [[...]], "v": [[...]]}, one row per layer and one '
                             "number per KV head")
        return cls(raw["k"], raw["v"])

    def save(self, path: str) -> None:
        with open(path, "w") as fh:
            fh.write(self.to_json() + "\n")

    @classmethod
    def load(cls, path: str) -> "KvScales":
        try:
            with open(path) as fh:
                text = fh.read()
        except OSError as e:
            raise ValueError(f"kv_scales: cannot read {path!r} ({e.strerror or e}); pass 'checkpoint' or a JSON file") \
                from None
        return cls.from_json(text)


def parse_kv_scales(spec, kv_dtype: str = "fp8"):
    """``--kv-scales`` / ``start_server(kv_scales=)``: None (no scales), a ``KvScales``, ``"checkpoint"`` (returned
    as is: ``load_llama`` reads the checkpoint's tensors) or the path of a JSON file, which is read here. Anything
    but None is refused with a bf16 cache."""
    if spec is None:
        return None
    if kv_dtype != "fp8":
        raise ValueError(f"kv_scales need kv_dtype='fp8' (--kv-dtype fp8): a {kv_dtype} KV cache has no scales")
    if isinstance(spec, KvScales) or spec == CHECKPOINT:
        return spec
    if isinstance(spec, str):
        return KvScales.load(spec)
    raise ValueError(f"kv_scales must be a KvScales, 'checkpoint' or the path of a JSON file, got {spec!r}")


def read_checkpoint(has, get, n_layers: int, n_kv_heads: int, prefix: str = "model.") -> KvScales:
    """The scales an FP8-KV checkpoint carries: per layer ``{prefix}layers.N.self_attn.k_scale`` and ``.v_scale``
    (a scalar or shape [1], broadcast over the layer's KV heads; [n_kv_heads] is taken as is), or one ``kv_scale``
    for both. ``has(name)`` / ``get(name)``: the checkpoint's tensors. A layer without them is refused."""
    k, v = [], []
    for i in range(n_layers):
        p = f"{prefix}layers.{i}.self_attn."
        row = {}
        for which in ("k", "v"):
            name = p + which + "_scale" if has(p + which + "_scale") else p + "kv_scale"
            if not has(name):
                raise ValueError(f"--kv-scales checkpoint: the checkpoint has no {p}{which}_scale (nor {p}kv_scale); "
                                 "every layer needs its scales. Calibrate them (scripts/calibrate_kv.py) and pass the "
                                 "file, or serve without --kv-scales")
            t = get(name).float().flatten()
            if t.numel() not in (1, n_kv_heads):
                raise ValueError(f"{name}: expected a scalar, shape [1] or [{n_kv_heads}], got {t.numel()} values")
            row[which] = t.expand(n_kv_heads).tolist()
        k.append(row["k"])
        v.append(row["v"])
    return KvScales(k, v)


# ------------------------------------------------------------------ calibration
def absmax(k_cache: torch.Tensor, v_cache: torch.Tensor, lengths) -> tuple[torch.Tensor, torch.Tensor]:
    """Per (layer, KV head) largest magnitude of the rows written: caches ``[L][slots][S][Hkv][D]`` (any float
    dtype), ``lengths[s]`` the rows slot s holds (rows past it, and slots past ``len(lengths)``, are not read).
    Returns fp32 ``[L][Hkv]`` for K and for V; zeros where nothing was written."""
    if k_cache.dim() != 5 or v_cache.shape != k_cache.shape:
        raise ValueError("caches must be [n_layers, n_slots, max_seq, Hkv, D], K and V alike")
    L, n_slots, S, Hkv, _ = k_cache.shape
    lengths = [int(n) for n in lengths]
    if len(lengths) > n_slots or any(not 0 <= n <= S for n in lengths):
        raise ValueError(f"lengths must name at most {n_slots} slots, each in [0, {S}]")
    out = []
    for cache in (k_cache, v_cache):
        m = torch.zeros(L, Hkv, dtype=torch.float32)
        for s, n in enumerate(lengths):
            if n:
                m = torch.maximum(m, cache[:, s, :n].float().abs().amax(dim=(1, 3)).cpu())
        out.append(m)
    return out[0], out[1]


def scales_from_absmax(k_absmax: torch.Tensor, v_absmax: torch.Tensor) -> KvScales:
    """``s = absmax / 448`` rounded up to a power of two: the largest value seen lands in (224, 448] (headroom of
    1 to 2), and the multiply by 1 / s is exact. A head that saw only zeros gets scale 1."""
    def one(a):
        a = a.double()
        e = torch.ceil(torch.log2(torch.where(a > 0, a / E4M3_MAX, torch.ones_like(a))))
        s = torch.exp2(e)
        s = torch.where(s * E4M3_MAX < a, s * 2, s)  # log2 off by a rounding: never below absmax / 448
        return s.clamp(2.0 ** -100, 2.0 ** 100).float()
    if not bool(torch.isfinite(k_absmax).all() and torch.isfinite(v_absmax).all()):
        raise ValueError("non-finite K or V values in the calibration rows")
    return KvScales(one(k_absmax), one(v_absmax))


def is_power_of_two(t: torch.Tensor) -> bool:
    m, _ = torch.frexp(t.float())
    return bool((m == 0.5).all())


__all__ = ["KvScales", "parse_kv_scales", "read_checkpoint", "absmax", "scales_from_absmax", "is_power_of_two",
           "CHECKPOINT"]
