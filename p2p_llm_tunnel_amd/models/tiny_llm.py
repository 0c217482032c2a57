"""Llama-style decoder for the on-node inference upstream.

The tunnel's serve side fronts an OpenAI/Ollama-compatible endpoint running
on the MI355X node (BASELINE.json north star). This module is that
endpoint's model: random-init weights (no checkpoints offline), bf16.

Two decode paths over the same weights and caches:

* fused (default, up to 64 token rows per step): ``ops.FusedLlamaDecoder`` — one
  C++ call launching 5 kernels per layer + 3 (decode_fused.hip: MFMA skinny
  GEMMs with RMSNorm prologues and RoPE/KV-append, SwiGLU, residual and
  argmax epilogues; split-K attention with in-kernel merge);
* unfused: the standalone kernels of kernels.hip (residual+RMSNorm,
  RoPE+KV-append, flash-decoding, SwiGLU, argmax) around hipBLASLt GEMMs
  (``torch.nn.functional.linear``) — kept as the cross-check and for batches
  above 64.

``reference_logits`` recomputes the same network in fp32 PyTorch (full
causal attention over the whole sequence) for numerics tests.
"""
from __future__ import annotations

import math
from dataclasses import InitVar, dataclass

import torch
import torch.nn.functional as F

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models import rope as rope_mod
from p2p_llm_tunnel_amd.models.kv_scales import KvScales
from p2p_llm_tunnel_amd.models.rope import RopeScaling


@dataclass(frozen=True)
class LlamaConfig:
    vocab: int = 32000
    dim: int = 1024
    n_layers: int = 4
    n_heads: int = 16
    n_kv_heads: int = 4
    head_dim: int = 64
    ffn: int = 2816
    max_seq: int = 2048
    eps: float = 1e-5
    rope_theta: float = 10000.0
    qk_norm: bool = False  # per-head RMSNorm on q and k before RoPE (Qwen3): layers carry q_norm, k_norm [head_dim]
    qkv_bias: bool = False  # bias on the q, k and v projections (Qwen2): layers carry bqkv [(H + 2 Hkv) * head_dim]
    # llama3 / linear RoPE scaling (Llama 3.1+): the kernels read inv_freq from a table instead of computing it
    rope_scaling: RopeScaling | None = None
    # Sliding-window attention (docs/SLIDING_WINDOW.md): None, or one int per layer, 0 for full attention and W >= 1
    # for a layer whose token at position p attends to positions (p - W, p]: W tokens, its own included. None and all
    # zeros are the decoder without windows.
    windows: tuple | None = None
    sliding_window: InitVar[int | None] = None  # shorthand: the same window on every layer (it sets ``windows``)

    def __post_init__(self, sliding_window):
        if sliding_window is not None:
            if isinstance(sliding_window, bool) or not isinstance(sliding_window, int) or sliding_window < 1:
                raise ValueError(f"sliding_window must be an int >= 1, got {sliding_window!r}")
            if self.windows is not None:
                raise ValueError("give sliding_window (every layer) or windows (per layer), not both")
            object.__setattr__(self, "windows", (sliding_window,) * self.n_layers)
        elif self.windows is not None:
            w = tuple(self.windows)
            if len(w) != self.n_layers:
                raise ValueError(f"windows must hold one entry per layer ({self.n_layers}), got {len(w)}")
            if any(isinstance(x, bool) or not isinstance(x, int) or x < 0 for x in w):
                raise ValueError(f"windows must be ints >= 0 (0: full attention), got {w!r}")
            object.__setattr__(self, "windows", w)

    @property
    def windowed(self) -> bool:
        """Whether any layer has a sliding window."""
        return bool(self.windows) and any(self.windows)


CONFIGS = {
    "tiny": LlamaConfig(),
    "micro": LlamaConfig(vocab=4096, dim=256, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512, max_seq=512),
    "small": LlamaConfig(vocab=32000, dim=2048, n_layers=8, n_heads=16, n_kv_heads=4, head_dim=128, ffn=5632,
                         max_seq=4096),
}


KV_DTYPES = {"bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn}  # TinyLlama(kv_dtype=): the caches' dtype
# TinyLlama(weight_dtype=): the format of the GEMM weights. "mxfp4": a layer's four as MXFP4, the LM head as FP8.
WEIGHT_DTYPES = ("bf16", "fp8", "mxfp4")
GEMM_WEIGHTS = ops.LAYER_GEMMS  # a layer's GEMM weights, in the order of their scales
FOLDED_NORM = {"wqkv": "attn_norm", "w_gate_up": "ffn_norm", "lm_head": "final_norm"}  # GEMM: the norm in its columns


def _pairs(n, device):  # [0, n, 1, n + 1, ...]
    return torch.stack([torch.arange(n), torch.arange(n) + n], 1).flatten().to(device)


def fused_row_perm(cfg: "LlamaConfig", name: str, device) -> torch.Tensor | None:
    """The row order of entry ``name`` in the fused table: row i of the table is row perm[i] of the plain weight
    (RoPE partners of a head, for wqkv and its bias; gate_j / up_j, in pairs); None where the table keeps the plain
    order."""
    if name in ("wqkv", "bqkv") and not cfg.qk_norm:
        heads = cfg.n_heads + 2 * cfg.n_kv_heads
        return (torch.arange(heads, device=device)[:, None] * cfg.head_dim
                + _pairs(cfg.head_dim // 2, device)[None, :]).flatten()
    if name == "w_gate_up":
        return _pairs(cfg.ffn, device)
    return None


def quantize_gemm_weight(w: torch.Tensor, g: torch.Tensor | None, perm: torch.Tensor | None,
                         weight_dtype: str = "fp8"):
    """A GEMM weight as the fused table holds it, W'[n][k] = w[perm[n]][k] * g[k] with the fold in fp32, quantised
    from that fp32 value (``ops.quantize_weight_fp8``, or ``ops.quantize_weight_mxfp4`` for ``weight_dtype`` "mxfp4"),
    not through bf16: ``(q, scale)`` in the table's row order."""
    wf = w.float()
    if g is not None:
        wf = wf * g.float()[None, :]
    if perm is not None:
        wf = wf[perm]
    quantize = ops.quantize_weight_mxfp4 if weight_dtype == "mxfp4" else ops.quantize_weight_fp8
    return quantize(wf.contiguous())


def layer_weight_dtype(L: dict) -> str:
    """The format of a layer's GEMM weights, read off its tensors: "bf16", or what ``quantize_layer_`` made of them
    ("fp8": fp32 row scales; "mxfp4": e8m0 block-scale bytes)."""
    s = next((L[n + "_s"] for n in GEMM_WEIGHTS if n + "_s" in L), None)
    return "bf16" if s is None else "mxfp4" if s.dtype == torch.uint8 else "fp8"


def quantize_layer_(cfg: "LlamaConfig", L: dict, weight_dtype: str = "fp8") -> dict:
    """One layer's four GEMM weights to FP8 (or, ``weight_dtype`` "mxfp4", to MXFP4) in place: ``L[name]`` (bf16)
    gives way to ``L[name + "_q"]`` (e4m3, or MXFP4 nibble bytes; folded and interleaved as the fused table wants
    it) and ``L[name + "_s"]`` (fp32 row scales, or e8m0 block-scale bytes). The loader calls it layer by layer, so
    the bf16 and quantised copies of all layers are never resident together."""
    for name in GEMM_WEIGHTS:
        if name + "_q" in L:
            continue
        w = L.pop(name)
        L[name + "_q"], L[name + "_s"] = quantize_gemm_weight(w, L.get(FOLDED_NORM.get(name)),
                                                              fused_row_perm(cfg, name, w.device), weight_dtype)
        del w
    return L


def dequantize_gemm_weight(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """``(q, s)`` of ``quantize_gemm_weight`` back in fp32, whichever format made them."""
    return ops.dequantize_weight_mxfp4(q, s) if s.dtype == torch.uint8 else ops.dequantize_weight_fp8(q, s)


def llama_dims(cfg: "LlamaConfig", max_batch: int, kv_fp8: bool = False) -> ops.LlamaDims:
    """The fused step's ``LlamaDims`` of a model of ``cfg`` with ``max_batch`` cache slots."""
    c = cfg
    return ops.LlamaDims(vocab=c.vocab, dim=c.dim, n_layers=c.n_layers, H=c.n_heads, Hkv=c.n_kv_heads, D=c.head_dim,
                         ffn=c.ffn, max_seq=c.max_seq, max_batch=max_batch, eps=c.eps, theta=c.rope_theta,
                         qk_norm=int(c.qk_norm), qkv_bias=int(c.qkv_bias), rope_table=int(c.rope_scaling is not None),
                         kv_fp8=int(kv_fp8))


def e4m3_round(x: torch.Tensor) -> torch.Tensor:
    """x (fp32) as the FP8 KV cache holds it (OCP e4m3fn, scale 1), back in fp32: finite values clamped to +-448,
    then one rounding to nearest-even (torch's own cast, which does that for |x| <= 448 and would give NaN above
    464: hence the clamp first). NaN stays NaN. ``utils/kv_fp8_ref.py`` is the same rule in NumPy integers."""
    return x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()


def capture(fn, device, warmup: int = 2):
    """``fn()`` as a hipGraph (torch.cuda.CUDAGraph): ``warmup`` calls on a side
    stream keep allocator and GEMM-heuristics warm-up outside the capture.
    Returns (graph, what ``fn`` returned under capture: the static outputs)."""
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.no_grad(), torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = fn()
    return graph, out


class TinyLlama:
    def __init__(self, cfg: LlamaConfig | str = "tiny", device="cuda", max_batch: int = 8, seed: int = 0,
                 fused: bool = True, weights: dict | None = None, kv_dtype: str = "bf16",
                 weight_dtype: str = "bf16", kv_scales: KvScales | None = None):
        """``kv_dtype``: "bf16" (default) or "fp8": the K/V caches as ``torch.float8_e4m3fn`` (OCP e4m3, half the
        bytes; docs/KV_FP8.md), which only the fused step reads and writes. ``kv_scales`` (a ``KvScales``; "fp8"
        only): fp32 scales per layer and KV head, so the stored byte is e4m3(x / s) and attention undoes the scale;
        None is scale 1.

        ``weight_dtype``: "bf16" (default) or "fp8": wqkv, wo, w_gate_up, w_down and lm_head as e4m3 bytes with
        one fp32 scale per output row (docs/WEIGHT_FP8.md), quantised here layer by layer (the bf16 tensor of each
        is dropped as it goes; ``weights`` may bring layers ``quantize_layer_`` has already seen). Only the fused
        step reads them. The embedding stays bf16, so a tied model keeps it and gets an FP8 copy for the LM head.
        "mxfp4": a layer's four GEMM weights as OCP Microscaling FP4 (e2m1 nibbles, one e8m0 scale byte per block of
        32; docs/WEIGHT_MXFP4.md) and the LM head in the FP8 format above.

        Random-init weights from ``seed``, or ``weights`` (embed, final_norm,
        lm_head, layers[{attn_norm, wqkv, wo, ffn_norm, w_gate_up, w_down}, plus
        q_norm, k_norm when ``cfg.qk_norm``, or bqkv in plain q | k | v order when
        ``cfg.qkv_bias``], bf16 on ``device``) — see ``checkpoint.load_llama``."""
        self.cfg = CONFIGS[cfg] if isinstance(cfg, str) else cfg
        if self.cfg.qkv_bias and self.cfg.qk_norm:
            raise ValueError("qkv_bias with qk_norm: no supported family has both, and the fused step refuses it")
        if kv_dtype not in KV_DTYPES:
            raise ValueError(f"kv_dtype must be one of {sorted(KV_DTYPES)}, got {kv_dtype!r}")
        if weight_dtype not in WEIGHT_DTYPES:
            raise ValueError(f"weight_dtype must be one of {list(WEIGHT_DTYPES)}, got {weight_dtype!r}")
        self.kv_dtype = kv_dtype
        if kv_scales is not None:
            if not isinstance(kv_scales, KvScales):
                raise TypeError(f"kv_scales must be a KvScales, got {type(kv_scales).__name__}")
            kv_scales.check(self.cfg.n_layers, self.cfg.n_kv_heads, kv_dtype)
        self.kv_scales = kv_scales
        self.weight_dtype = weight_dtype
        self.lm_head_q = self.lm_head_s = None  # weight_dtype "fp8": the LM head's bytes and row scales
        self.fused = fused
        self._fused = None
        self._graphs = {}  # rows -> (graph, tokens, pos, slots, ids, logits)
        self._embed_acc = None  # embed_pool's running sums, allocated on first use
        self._inv_freq = None  # the scaled model's RoPE frequency table on the device, made on first use
        c = self.cfg
        self.device = torch.device(device)
        self.max_batch = max_batch
        if weights is not None:
            self.embed, self.final_norm, self.lm_head = weights["embed"], weights["final_norm"], weights["lm_head"]
            self.layers = weights["layers"]
            if c.qk_norm:
                for i, L in enumerate(self.layers):
                    for n in ("q_norm", "k_norm"):
                        if n not in L or tuple(L[n].shape) != (c.head_dim,):
                            raise ValueError(f"layer {i}: a QK-norm model needs {n} of shape ({c.head_dim},)")
            if c.qkv_bias:
                n_qkv = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim
                for i, L in enumerate(self.layers):
                    if "bqkv" not in L or tuple(L["bqkv"].shape) != (n_qkv,):
                        raise ValueError(f"layer {i}: a QKV-bias model needs bqkv of shape ({n_qkv},)")
            self._quantize_weights()
            self._alloc_caches()
            return
        g = torch.Generator(device="cpu").manual_seed(seed)

        def w(*shape, scale):
            return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(self.device)

        def norm_w(n):
            return (1.0 + 0.1 * torch.randn(n, generator=g)).to(torch.bfloat16).to(self.device)

        qkv_out = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim
        self.embed = w(c.vocab, c.dim, scale=1.0)
        self.layers = []
        for _ in range(c.n_layers):
            self.layers.append({
                "attn_norm": norm_w(c.dim),
                "wqkv": w(qkv_out, c.dim, scale=1 / math.sqrt(c.dim)),
                "wo": w(c.dim, c.n_heads * c.head_dim, scale=1 / math.sqrt(c.n_heads * c.head_dim)),
                "ffn_norm": norm_w(c.dim),
                "w_gate_up": w(2 * c.ffn, c.dim, scale=1 / math.sqrt(c.dim)),
                "w_down": w(c.dim, c.ffn, scale=1 / math.sqrt(c.ffn)),
            })
            if c.qk_norm:  # drawn well away from 1 and from each other: a missing or swapped weight shows
                for n in ("q_norm", "k_norm"):
                    self.layers[-1][n] = (0.5 + torch.rand(c.head_dim, generator=g)).to(torch.bfloat16).to(self.device)
            if c.qkv_bias:  # up to a few units, as real k-biases are: one that is dropped or scaled by 1/rms shows
                self.layers[-1]["bqkv"] = w(qkv_out, scale=1.0)
        self.final_norm = norm_w(c.dim)
        self.lm_head = w(c.vocab, c.dim, scale=1 / math.sqrt(c.dim))
        self._quantize_weights()
        self._alloc_caches()

    @classmethod
    def from_weights(cls, cfg: LlamaConfig, weights: dict, device="cuda", max_batch: int = 8, fused: bool = True,
                     kv_dtype: str = "bf16", weight_dtype: str = "bf16", kv_scales: KvScales | None = None):
        return cls(cfg, device=device, max_batch=max_batch, fused=fused, weights=weights, kv_dtype=kv_dtype,
                   weight_dtype=weight_dtype, kv_scales=kv_scales)

    def _quantize_weights(self):
        """``weight_dtype`` "fp8": every layer's GEMM weights and the LM head to e4m3 + row scales, one tensor at
        a time. The bf16 LM head is dropped unless it is the embedding itself (a tied model)."""
        for L in self.layers:
            have = layer_weight_dtype(L)
            if have != "bf16" and have != self.weight_dtype:
                raise ValueError(f"the weights hold {'FP8' if have == 'fp8' else 'MXFP4'} layers: "
                                 f"pass weight_dtype='{have}'")
        if self.weight_dtype == "bf16":
            return
        self.layers = [quantize_layer_(self.cfg, dict(L), self.weight_dtype) for L in self.layers]
        self.lm_head_q, self.lm_head_s = quantize_gemm_weight(self.lm_head, self.final_norm, None)
        self.lm_head = None

    def weight_bytes(self) -> dict:
        """Bytes of the weights on the device: ``gemm`` (the five GEMM weights, with their scales when FP8),
        ``embed`` (the bf16 embedding table, which FP8 weights leave alone) and ``total`` (those and the norms,
        biases and QK-norm weights). A tied bf16 model counts its one shared table under ``embed`` only."""
        nb = lambda t: t.numel() * t.element_size()
        gemm = other = 0
        for L in self.layers:
            for k, t in L.items():
                if k in GEMM_WEIGHTS or k[:-2] in GEMM_WEIGHTS:  # name, name_q, name_s
                    gemm += nb(t)
                else:
                    other += nb(t)
        if self.weight_dtype != "bf16":
            gemm += nb(self.lm_head_q) + nb(self.lm_head_s)
        elif self.lm_head is not self.embed and self.lm_head.data_ptr() != self.embed.data_ptr():
            gemm += nb(self.lm_head)
        embed = nb(self.embed)
        return {"gemm": gemm, "embed": embed, "total": gemm + embed + other + nb(self.final_norm)}

    def _alloc_caches(self):
        c = self.cfg
        # One spare slot (index max_batch) absorbs the K/V writes of padding rows.
        self.scratch_slot = self.max_batch
        cache_shape = (c.n_layers, self.max_batch + 1, c.max_seq, c.n_kv_heads, c.head_dim)
        self.k_cache = torch.zeros(cache_shape, dtype=KV_DTYPES[self.kv_dtype], device=self.device)
        self.v_cache = torch.zeros(cache_shape, dtype=KV_DTYPES[self.kv_dtype], device=self.device)

    def kv_cache_bytes(self) -> int:
        """Bytes of the K and V caches together."""
        return self.k_cache.nbytes + self.v_cache.nbytes

    def kv_copy(self, jobs) -> None:
        """Copy K/V rows between cache slots on the current stream: ``jobs`` is a
        list of ``(src, dst, n)``, rows [0, n) of slot src -> slot dst in every
        layer (``ops.kv_copy_``, at most ``ops.MAX_KV_COPY_JOBS`` per call). An FP8 cache goes through the same
        kernel as bf16 [L, slots, S, Hkv, D / 2]: the rows are moved bit for bit, two e4m3 bytes per element."""
        if self.kv_dtype == "fp8":
            shape = tuple(self.k_cache.shape[:-1]) + (self.cfg.head_dim // 2,)
            ops.kv_copy_(self.k_cache.view(torch.bfloat16).view(shape), self.v_cache.view(torch.bfloat16).view(shape),
                         jobs)
            return
        ops.kv_copy_(self.k_cache, self.v_cache, jobs)

    def embed_pool(self, jobs, out: torch.Tensor) -> None:
        """Pool rows of the last fused step's final hidden state into embeddings
        on the current stream: ``jobs`` is a list of ``(row0, n, acc, flags,
        out_row)`` (``ops.embed_pool_``, at most ``ops.MAX_EMBED_JOBS`` per call);
        ``acc`` indexes this model's own running sums (fp32 [max_batch + 1, dim],
        one per cache slot), ``out`` is fp32 [n, dim] on the model's device."""
        if not self.fused:
            raise ValueError("embed_pool needs the fused path (it reads the fused step's workspace)")
        if self._embed_acc is None:
            self._embed_acc = torch.zeros(self.max_batch + 1, self.cfg.dim, dtype=torch.float32, device=self.device)
        self.fused_decoder().embed_pool(self._embed_acc, out, jobs)

    # ------------------------------------------------------------------ HIP path
    @torch.no_grad()
    def decode_step(self, tokens: torch.Tensor, pos: torch.Tensor, pos_range: tuple[int, int],
                    return_logits: bool = False, slots: torch.Tensor | None = None, emit_rows: int = 0):
        """One step of token rows. tokens: int64 [B]; pos: int32 [B] (cache position of
        each token); slots: int32 [B] cache slot of each row (default: row b -> slot b).
        With ``slots`` (fused path, B <= 64) several rows may feed one sequence at
        consecutive positions: a causal prefill chunk. ``emit_rows`` > 0: only the
        first rows get ids/logits (fused path; the LM head skips the rest).

        Returns next-token ids (int64 [B]) and optionally the bf16 logits.
        """
        c = self.cfg
        B = tokens.shape[0]
        if slots is None and B > self.max_batch:
            raise ValueError("batch exceeds max_batch")
        if slots is not None and not (self.fused and B <= ops.MAX_ROWS):
            raise ValueError(f"row->slot mapping needs the fused path and at most {ops.MAX_ROWS} rows")
        if pos_range[0] < 0 or pos_range[1] >= c.max_seq:
            raise ValueError("positions out of [0, max_seq)")
        ids, logits = self.step_rows(tokens, pos, slots, emit_rows, pos_range)
        return (ids, logits) if return_logits else ids

    def rope_inv_freq(self) -> torch.Tensor | None:
        """fp32 [head_dim / 2] RoPE frequencies of a model with ``cfg.rope_scaling`` (``rope.inv_freq``), on the
        model's device; None for default RoPE, whose kernels compute theirs inline. Made once, and its entries
        checked then (``rope.inv_freq``): the unfused step passes it on with ``inv_freq_checked``."""
        c = self.cfg
        if c.rope_scaling is None:
            return None
        if self._inv_freq is None:
            self._inv_freq = rope_mod.inv_freq(c.rope_theta, c.head_dim, c.rope_scaling, self.device)
        return self._inv_freq

    def fused_weights(self) -> list:
        """The fused step's weight table (device-independent: plain torch)."""
        c = self.cfg
        # The fused GEMMs take the RMSNorm weight folded into the following
        # projection's columns (W[n][k] * g[k]), and QKV / gate-up rows
        # interleaved in pairs so a 16-column tile holds both members of a
        # RoPE pair or a SwiGLU pair; see decode_fused.hip. A QK-norm model keeps
        # wqkv's rows in plain order (its RoPE runs in k_qknorm_rope, which pairs
        # the partners itself) and appends q_norm, k_norm to each layer's six. A
        # QKV-bias model appends bqkv, interleaved like wqkv's rows (the fold
        # touches only wqkv). A model with scaled RoPE carries its frequency table (fp32)
        # as a fourth global entry, between lm_head and the layers.
        # With FP8 weights the five GEMM weights are e4m3 bytes, quantised after the fold and the
        # interleave (_quantize_weights), and their row scales follow the table. With MXFP4 weights a layer's four
        # are nibble bytes and their scales the blocks' e8m0 bytes; the LM head is the FP8 one.
        fp8 = self.weight_dtype != "bf16"
        top = {"embed": self.embed, "final_norm": self.final_norm, "lm_head": self.lm_head,
               "lm_head_q": self.lm_head_q, "lm_head_s": self.lm_head_s, "inv_freq": self.rope_inv_freq()}

        def entry(name, layer):
            src = top if layer is None else self.layers[layer]
            if name.endswith(" scale"):
                return src[name[:-len(" scale")] + "_s"]
            if fp8 and (name in GEMM_WEIGHTS or name == "lm_head"):
                return src[name + "_q"]
            w = src[name]
            if name in FOLDED_NORM:
                w = (w.float() * src[FOLDED_NORM[name]].float()[None, :]).to(torch.bfloat16)
            perm = fused_row_perm(c, name, self.device)
            return w[perm].contiguous() if perm is not None else w.contiguous() if name.endswith("_norm") else w

        return [entry(e.name, e.layer) for e in ops.WeightTable(self.dims(), weight_format=self.weight_dtype)]

    def dims(self) -> ops.LlamaDims:
        """The fused step's dims of this model: one cache slot per sequence and the scratch slot."""
        return llama_dims(self.cfg, self.max_batch + 1, self.kv_dtype == "fp8")

    def fused_decoder(self) -> ops.FusedLlamaDecoder:
        if self._fused is None:
            self._fused = ops.FusedLlamaDecoder(self.dims(), self.fused_weights(), self.k_cache, self.v_cache,
                                                weight_format=self.weight_dtype,
                                                kv_scales=(self.kv_scales.table(self.device)
                                                           if self.kv_scales is not None else None),
                                                windows=self.cfg.windows if self.cfg.windowed else None)
        return self._fused

    def step_rows(self, tokens, pos, slots=None, emit_rows=0, pos_range=None):
        """``decode_step`` without host validation (the fused path: without host
        sync either, so capturable); returns (ids, logits). ``pos_range``: (min,
        max) of ``pos`` for the unfused kernels' bounds check and attention
        grid; None means anything in [0, max_seq), the capture case."""
        B = tokens.shape[0]
        if self.fused and B <= ops.MAX_ROWS:
            tokens, pos = tokens.contiguous(), pos.contiguous()
            slots = slots.contiguous() if slots is not None else None
            logits = torch.empty(B, self.cfg.vocab, dtype=torch.bfloat16, device=self.device)
            ids = torch.empty(B, dtype=torch.int64, device=self.device)
            self.fused_decoder().step(tokens, pos, logits, ids, slots, emit_rows)
            return ids, logits
        if self.kv_dtype != "bf16":
            raise ValueError(f"an {self.kv_dtype} KV cache runs the fused step only (at most {ops.MAX_ROWS} rows, "
                             "fused=True): the unfused kernels read and write bf16 caches")
        if self.weight_dtype != "bf16":
            raise ValueError(f"{self.weight_dtype} weights run the fused step only (at most {ops.MAX_ROWS} rows, "
                             "fused=True): the unfused path multiplies bf16 weights")
        if self.cfg.windowed:
            raise ValueError(f"a sliding window runs the fused step only (at most {ops.MAX_ROWS} rows, fused=True): "
                             "the unfused attention kernel reads every cached position")
        return self._decode_unfused(tokens, pos, pos_range or (0, self.cfg.max_seq - 1))

    def _decode_unfused(self, tokens, pos, pos_range):
        c = self.cfg
        B = tokens.shape[0]
        lens = pos + 1
        x = self.embed.index_select(0, tokens)
        h = ops.rmsnorm(x, self.layers[0]["attn_norm"], c.eps)
        residual = x
        for i, L in enumerate(self.layers):
            kc, vc = self.k_cache[i, :B], self.v_cache[i, :B]
            qkv = F.linear(h, L["wqkv"], L["bqkv"] if c.qkv_bias else None)
            if c.qk_norm:  # per-head norm with the standalone rmsnorm kernel on [B * heads, D] views
                nq, nk = c.n_heads * c.head_dim, c.n_kv_heads * c.head_dim
                qn = ops.rmsnorm(qkv[:, :nq].reshape(-1, c.head_dim), L["q_norm"], c.eps).view(B, nq)
                kn = ops.rmsnorm(qkv[:, nq:nq + nk].reshape(-1, c.head_dim), L["k_norm"], c.eps).view(B, nk)
                qkv = torch.cat([qn, kn, qkv[:, nq + nk:]], 1)
            q = ops.rope_qkv_cache(qkv, pos, kc, vc, c.n_heads, c.n_kv_heads, c.head_dim, c.rope_theta,
                                   pos_range=pos_range, inv_freq=self.rope_inv_freq(), inv_freq_checked=True)
            a = ops.decode_attention(q, kc, vc, lens, max_len=pos_range[1] + 1)
            o = F.linear(a.view(B, -1), L["wo"])
            h, residual = ops.rmsnorm(o, L["ffn_norm"], c.eps, residual=residual)
            m = F.linear(ops.silu_mul(F.linear(h, L["w_gate_up"])), L["w_down"])
            nxt = self.layers[i + 1]["attn_norm"] if i + 1 < len(self.layers) else self.final_norm
            h, residual = ops.rmsnorm(m, nxt, c.eps, residual=residual)
        logits = F.linear(h, self.lm_head)
        return ops.argmax(logits), logits

    # ------------------------------------------------------------------ hipGraph
    def capture_graph(self, rows: int | None = None, emit_rows: int = 0):
        """Capture one step of ``rows`` token rows into a hipGraph (torch.cuda.CUDAGraph).

        Decode at small batch is bound by kernel count; replaying the captured
        graph removes the per-kernel launch cost. One graph serves every step:
        the fused kernels' grids depend on the row count alone and read each
        row's context length from ``pos``; the unfused attention is launched for
        the cache capacity (splits past a row's length exit immediately). Fused
        path: up to 64 rows with a row->slot map (padding rows point at the
        scratch slot); unfused: one row per slot. Several row counts may be
        captured (e.g. 16 for decode-heavy steps, 64 for prefill-heavy ones);
        ``graph_step`` picks the graph by the number of rows it is given.
        ``emit_rows``: rows that get ids (0: all).
        """
        R = rows or (16 if self.fused else self.max_batch)
        g_tok = torch.zeros(R, dtype=torch.int64, device=self.device)
        g_pos = torch.zeros(R, dtype=torch.int32, device=self.device)
        g_slot = (torch.full((R,), self.scratch_slot, dtype=torch.int32, device=self.device)
                  if self.fused else None)
        graph, (g_ids, g_logits) = capture(lambda: self.step_rows(g_tok, g_pos, g_slot, emit_rows), self.device)
        self._graphs[R] = (graph, g_tok, g_pos, g_slot, g_ids, g_logits)
        return self

    @torch.no_grad()
    def graph_step(self, tokens: torch.Tensor, pos: torch.Tensor, slots: torch.Tensor | None = None,
                   return_logits: bool = False):
        """Replay the graph captured for ``tokens.shape[0]`` rows. tokens/pos/slots:
        [rows] (slots default to row b -> slot b); positions must be < max_seq."""
        R = tokens.shape[0]
        graph, g_tok, g_pos, g_slot, g_ids, g_logits = self._graphs[R]
        g_tok.copy_(tokens, non_blocking=True)
        g_pos.copy_(pos, non_blocking=True)
        if g_slot is not None:
            if slots is None:
                slots = torch.arange(R, dtype=torch.int32).clamp_(max=self.scratch_slot)
            g_slot.copy_(slots, non_blocking=True)
        graph.replay()
        return (g_ids, g_logits) if return_logits else g_ids

    # ------------------------------------------------------------------ fp32 reference
    @torch.no_grad()
    def reference_logits(self, seqs: torch.Tensor, kv_round=None) -> torch.Tensor:
        """fp32 forward of full sequences [B, T]; returns logits of the last position [B, V]. ``kv_round``: see
        ``reference_hidden``."""
        return self.reference_hidden(seqs, kv_round)[:, -1] @ self.reference_weight("lm_head").T

    def reference_weight(self, name: str, layer: int | None = None) -> torch.Tensor:
        """GEMM weight ``name`` ("lm_head", or one of a layer's four) in fp32 and plain row order, as the reference
        multiplies it. bf16 weights: the tensor itself. FP8 weights: the dequantised ``q * s`` (the function the
        kernels compute; the quantisation error against the original is a separate quantity), which carries the
        preceding norm's weight folded in, so the reference then norms with a weight of one (``_ref_norm``)."""
        if self.weight_dtype == "bf16":
            return (self.lm_head if layer is None else self.layers[layer][name]).float()
        if layer is None:
            return ops.dequantize_weight_fp8(self.lm_head_q, self.lm_head_s)
        L = self.layers[layer]
        w = dequantize_gemm_weight(L[name + "_q"], L[name + "_s"])
        perm = fused_row_perm(self.cfg, name, w.device)
        if perm is not None:
            w = w[torch.argsort(perm)]
        return w

    def _ref_norm(self, g: torch.Tensor) -> torch.Tensor:
        """The weight the reference's RMSNorm ahead of a folded GEMM applies: g, or one where g is in the weight."""
        return torch.ones_like(g) if self.weight_dtype != "bf16" else g

    @torch.no_grad()
    def reference_hidden(self, seqs: torch.Tensor, kv_round=None) -> torch.Tensor:
        """fp32 forward of full sequences [B, T]; returns the final normed hidden
        state of every position [B, T, dim] (what the LM head multiplies).
        A layer with a sliding window W (``cfg.windows``) masks, besides the future, every key at or below q - W:
        position q attends to (q - W, q], transformers' ``kv_idx > q_idx - sliding_window``.
        ``kv_round``: how K and V rows are stored, a function of the fp32 rows. None: the model's own cache
        format, bf16 rounding or ``e4m3_round`` (one rounding from fp32, not through bf16). With ``kv_scales`` (and
        no ``kv_round``) a row of layer i and KV head h is stored as the kernels store it, e4m3_round(x * fp32(1 / s)),
        and read back times s."""
        scaled = kv_round is None and self.kv_scales is not None
        if kv_round is None:
            kv_round = e4m3_round if self.kv_dtype == "fp8" else (lambda t: t.to(torch.bfloat16).float())

        def kv_store(t, which, layer):  # t: [B, T, Hkv, D]
            if not scaled:
                return kv_round(t)
            s = (self.kv_scales.k if which == "k" else self.kv_scales.v)[layer].to(t.device)[None, None, :, None]
            return e4m3_round(t.float() * (1.0 / s)) * s
        c = self.cfg
        B, T = seqs.shape
        f32 = lambda t: t.float()
        x = f32(self.embed)[seqs]  # [B, T, dim]

        def rms(v, wgt):
            return v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + c.eps) * f32(wgt)

        def bf(v):  # mirror the bf16 storage points of the HIP path
            return v.to(torch.bfloat16).float()

        pos = torch.arange(T, device=seqs.device, dtype=torch.float32)
        if c.rope_scaling is not None:  # the table the kernels read
            inv_freq = rope_mod.inv_freq(c.rope_theta, c.head_dim, c.rope_scaling, seqs.device)
        else:
            inv_freq = torch.exp2(-math.log2(c.rope_theta) * torch.arange(0, c.head_dim // 2, device=seqs.device,
                                                                          dtype=torch.float32) * 2 / c.head_dim)
        ang = pos[:, None] * inv_freq[None, :]
        cos, sin = torch.cos(ang), torch.sin(ang)

        def rope(t):  # [B, T, nh, D]
            half = c.head_dim // 2
            t1, t2 = t[..., :half], t[..., half:]
            cc, ss = cos[None, :, None, :], sin[None, :, None, :]
            return torch.cat([t1 * cc - t2 * ss, t2 * cc + t1 * ss], -1)

        residual = x
        h = bf(rms(x, self._ref_norm(self.layers[0]["attn_norm"])))
        G = c.n_heads // c.n_kv_heads
        causal = torch.full((T, T), float("-inf"), device=seqs.device).triu(1)
        for i, L in enumerate(self.layers):
            mask = causal
            if c.windowed and c.windows[i]:  # keys at or below q - W as well
                mask = causal + torch.full((T, T), float("-inf"), device=seqs.device).tril(-c.windows[i])
            raw = h @ self.reference_weight("wqkv", i).T
            raw = raw + f32(L["bqkv"]) if c.qkv_bias else raw
            qkv = bf(raw)
            q = qkv[..., : c.n_heads * c.head_dim].view(B, T, c.n_heads, c.head_dim)
            k = qkv[..., c.n_heads * c.head_dim: (c.n_heads + c.n_kv_heads) * c.head_dim].view(
                B, T, c.n_kv_heads, c.head_dim)
            # V is stored from the fp32 projection (the bf16 rounding of it is the bf16 store itself; the FP8 store
            # rounds the fp32 value once). A QK-norm model's V passes through the bf16 projection buffer first.
            v = kv_store((qkv if c.qk_norm else raw)[..., (c.n_heads + c.n_kv_heads) * c.head_dim:].view(
                B, T, c.n_kv_heads, c.head_dim), "v", i)
            if c.qk_norm:
                q, k = rms(q, L["q_norm"]), rms(k, L["k_norm"])
            q, k = bf(rope(q)), kv_store(rope(k), "k", i)
            k = k.repeat_interleave(G, dim=2)
            v = v.repeat_interleave(G, dim=2)
            s = torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(c.head_dim) + mask
            a = bf(torch.einsum("bhqk,bkhd->bqhd", s.softmax(-1), v).reshape(B, T, -1))
            o = bf(a @ self.reference_weight("wo", i).T)
            residual = bf(residual + o)
            h = bf(rms(residual, self._ref_norm(L["ffn_norm"])))
            gu = bf(h @ self.reference_weight("w_gate_up", i).T)
            g_, u_ = gu[..., : c.ffn], gu[..., c.ffn:]
            m = bf(bf(F.silu(g_) * u_) @ self.reference_weight("w_down", i).T)
            residual = bf(residual + m)
            nxt = self.layers[i + 1]["attn_norm"] if i + 1 < len(self.layers) else self.final_norm
            h = bf(rms(residual, self._ref_norm(nxt)))
        return h

    @torch.no_grad()
    def generate(self, prompt: list[int], max_new: int) -> list[int]:
        """Greedy single-sequence generation on slot 0 (prefill = sequential decode steps)."""
        out = []
        tok = None
        for p, t in enumerate(prompt + [None] * max_new):
            if p >= self.cfg.max_seq:
                break
            cur = t if t is not None else tok
            ids = self.decode_step(torch.tensor([cur], device=self.device),
                                   torch.tensor([p], dtype=torch.int32, device=self.device), (p, p))
            tok = int(ids.item())
            if p >= len(prompt) - 1:
                out.append(tok)
                if len(out) >= max_new:
                    break
        return out
