"""Weights-only loading of Llama-architecture checkpoints (Hugging Face
layout: ``config.json`` + ``model.safetensors`` or sharded
``model-0000k-of-0000n.safetensors`` with ``model.safetensors.index.json``)
into the endpoint's model (``TinyLlama``), plus the checkpoint's tokenizer.

Only safetensors is read — a flat tensor format with no code in it — through
``safetensors.safe_open`` (memory-mapped, one tensor at a time), so loading a
checkpoint executes nothing from the file and never holds the whole
checkpoint in host memory twice.

Name mapping (HF ``LlamaForCausalLM`` → ours, see ``tiny_llm.py``):

=====================================================  ===========================
``model.embed_tokens.weight``                            ``embed``
``model.layers.i.input_layernorm.weight``                ``layers[i]["attn_norm"]``
``...self_attn.{q,k,v}_proj.weight`` (concatenated)      ``layers[i]["wqkv"]``
``...self_attn.o_proj.weight``                           ``layers[i]["wo"]``
``...post_attention_layernorm.weight``                   ``layers[i]["ffn_norm"]``
``...mlp.{gate,up}_proj.weight`` (concatenated)          ``layers[i]["w_gate_up"]``
``...mlp.down_proj.weight``                              ``layers[i]["w_down"]``
``model.norm.weight``                                    ``final_norm``
``lm_head.weight`` (or the embedding when tied)          ``lm_head``
``...self_attn.q_norm.weight`` (Qwen3 only)              ``layers[i]["q_norm"]``
``...self_attn.k_norm.weight`` (Qwen3 only)              ``layers[i]["k_norm"]``
``...self_attn.{q,k,v}_proj.bias`` (Qwen2, concatenated)  ``layers[i]["bqkv"]``
=====================================================  ===========================

``Qwen3ForCausalLM`` (dense) is the Llama layout plus a per-head RMSNorm over
``head_dim`` on q and k before RoPE (``LlamaConfig.qk_norm``); its ``head_dim``
comes from the config and need not be ``hidden_size / num_attention_heads``.
A Llama or Mistral checkpoint that carries these tensors is refused: loading
it without the norm would compute a different model.

``Qwen2ForCausalLM`` (Qwen2, Qwen2.5 and their Coder, Math and R1-Distill
variants) is the Llama layout plus a bias on the q, k and v projections
(``LlamaConfig.qkv_bias``), and none on ``o_proj`` or the MLP. A checkpoint of
another architecture that carries ``q_proj.bias`` is refused, as is any
checkpoint with an ``o_proj`` or MLP bias.

Llama 3.1 / 3.2 / 3.3 checkpoints (and their distillations) scale the RoPE
frequencies: ``rope_scaling`` of type ``llama3``, or ``linear`` in older
long-context fine-tunes (``LlamaConfig.rope_scaling``, ``models/rope.py``).
Every key the type needs must be in the config; ``yarn``, ``dynamic``,
``longrope`` and any other type are refused.

A checkpoint that declares a sliding attention window (Mistral-7B-v0.1 and its fine-tunes; Qwen2 / Qwen3 configs
with ``use_sliding_window``) is served in one of two ways (docs/SLIDING_WINDOW.md). By default the context is capped
at the window, below which sliding and full attention are the same function, and a ``sliding_attention`` entry in
``layer_types`` is refused. With ``sliding_window=True`` the layers that slide get their window
(``LlamaConfig.windows``) and the context is the usual one.

HF Llama q/k projections are already laid out for the rotate-half RoPE
convention our kernels use (``reference_logits``), so no head permutation is
needed here; the fused decoder applies its own interleaving at setup.
"""
from __future__ import annotations

import json
import os

import torch

from p2p_llm_tunnel_amd.models import rope as rope_mod
from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig, TinyLlama

_SUPPORTED = {"LlamaForCausalLM", "MistralForCausalLM", "Qwen2ForCausalLM", "Qwen3ForCausalLM"}
_QK_NORM = {"Qwen3ForCausalLM"}  # per-head RMSNorm on q and k before RoPE
_QKV_BIAS = {"Qwen2ForCausalLM"}  # bias on q_proj, k_proj and v_proj, always (the config has no flag for it)
_GQA_RATIOS = (1, 2, 4, 5, 6, 7, 8)  # the fused step's attention instantiations (decode_fused.hip: GqaRatios)


_LAYER_TYPES = ("full_attention", "sliding_attention")  # what layer_types may hold with sliding_window=True


def layer_windows(raw: dict) -> tuple:
    """The sliding window of every layer of an HF config that declares one (``read_config(sliding_window=True)``):
    one int per layer, 0 for a layer with full attention. ``layer_types`` decides per layer where the config has
    it; otherwise every layer slides, except that a config with ``use_sliding_window`` (Qwen2, Qwen3) follows
    transformers' ``max_window_layers`` rule: layers with index >= ``max_window_layers`` slide. Refused: a config
    that declares no window (none set, ``use_sliding_window`` false, or no layer that slides), a window below 1, a
    ``layer_types`` list of another length than ``num_hidden_layers`` or with any other entry."""
    n = int(raw["num_hidden_layers"])
    sw = raw.get("sliding_window")
    use = raw.get("use_sliding_window")  # Qwen2 / Qwen3 only; absent (or null) elsewhere
    if sw is None or use is False:
        raise ValueError("sliding_window=True (--sliding-window), but the checkpoint declares no sliding window "
                         "(config.json has no sliding_window, or use_sliding_window is false)")
    if isinstance(sw, bool) or not isinstance(sw, int) or sw < 1:
        raise ValueError(f"sliding_window {sw!r}: a window must be an int >= 1")
    types = raw.get("layer_types")
    if types is not None:
        other = sorted({str(t) for t in types} - set(_LAYER_TYPES))
        if other:
            raise ValueError(f"layer_types {other}: only full_attention and sliding_attention layers are supported "
                             "by the decode kernels")
        if len(types) != n:
            raise ValueError(f"layer_types has {len(types)} entries, but num_hidden_layers is {n}")
        slides = [t == "sliding_attention" for t in types]
    elif use is not None:
        first = int(raw["max_window_layers"]) if raw.get("max_window_layers") is not None else n
        slides = [i >= first for i in range(n)]
    else:
        slides = [True] * n
    if not any(slides):
        raise ValueError("sliding_window=True (--sliding-window), but the checkpoint declares no sliding window: "
                         "none of its layers slides (layer_types / max_window_layers)")
    return tuple(int(sw) if s else 0 for s in slides)


def read_config(path: str, max_seq: int | None = None, sliding_window: bool = False) -> tuple[LlamaConfig, dict]:
    """LlamaConfig from an HF ``config.json`` (file or checkpoint directory);
    also returns the raw dict (tokenizer ids, tie flag). ``sliding_window``: serve the checkpoint's sliding window
    (``layer_windows``) instead of capping the context at it."""
    f = os.path.join(path, "config.json") if os.path.isdir(path) else path
    with open(f) as fh:
        raw = json.load(fh)
    arch = (raw.get("architectures") or ["LlamaForCausalLM"])[0]
    if arch == "Qwen3MoeForCausalLM":
        raise ValueError("unsupported architecture 'Qwen3MoeForCausalLM': mixture-of-experts layers are not "
                         "supported by the decode kernels (dense Qwen3 only)")
    if arch == "Qwen2MoeForCausalLM":
        raise ValueError("unsupported architecture 'Qwen2MoeForCausalLM': mixture-of-experts layers are not "
                         "supported by the decode kernels (dense Qwen2 only)")
    if arch not in _SUPPORTED:
        raise ValueError(f"unsupported architecture {arch!r} (Llama-style decoders only: {sorted(_SUPPORTED)})")
    # transformers >= 5 writes rope_parameters {rope_theta, rope_type}; older
    # files carry rope_theta (+ rope_scaling) at the top level.
    rope = raw.get("rope_parameters") or raw.get("rope_scaling") or {}
    scaling = rope_mod.from_hf(rope)  # None: default RoPE; llama3 or linear; anything else is refused
    theta = rope.get("rope_theta", raw.get("rope_theta", 10000.0))
    if raw.get("hidden_act", "silu") != "silu":
        raise ValueError(f"hidden_act {raw['hidden_act']!r}: only SwiGLU (silu) decoders are supported")
    if raw.get("attention_bias") or raw.get("mlp_bias"):
        raise ValueError("projection biases are not supported by the decode kernels"
                         + (" (Qwen2: on q, k and v only, without a config flag)" if arch in _QKV_BIAS else ""))
    windows = None
    if sliding_window:  # the layers that slide get their window; the context is not capped
        windows = layer_windows(raw)
    else:
        other = sorted({str(t) for t in raw.get("layer_types") or []} - {"full_attention"})
        if other:
            raise ValueError(f"layer_types {other}: only full_attention layers are supported by the decode kernels"
                             + (" (sliding_attention: with sliding_window=True / --sliding-window)"
                                if "sliding_attention" in other else ""))
        sw = raw.get("sliding_window")
        if sw and raw.get("use_sliding_window", True):  # full attention == sliding attention up to the window
            max_seq = min(int(max_seq or sw), int(sw))
    heads = int(raw["num_attention_heads"])
    dim = int(raw["hidden_size"])
    kv_heads = int(raw.get("num_key_value_heads", heads))
    if kv_heads <= 0 or heads % kv_heads or heads // kv_heads not in _GQA_RATIOS:
        raise ValueError(f"GQA ratio {heads}/{kv_heads}"
                         + (f" = {heads // kv_heads}" if kv_heads > 0 and heads % kv_heads == 0 else "")
                         + f" is not supported by the decode kernels (num_attention_heads / num_key_value_heads "
                           f"must be one of {list(_GQA_RATIOS)})")
    cfg = LlamaConfig(
        vocab=int(raw["vocab_size"]), dim=dim, n_layers=int(raw["num_hidden_layers"]), n_heads=heads,
        n_kv_heads=kv_heads, head_dim=int(raw.get("head_dim") or dim // heads),
        ffn=int(raw["intermediate_size"]),
        max_seq=int(max_seq or min(int(raw.get("max_position_embeddings", 2048)), 8192)),
        eps=float(raw.get("rms_norm_eps", 1e-5)), rope_theta=float(theta), qk_norm=arch in _QK_NORM,
        qkv_bias=arch in _QKV_BIAS, rope_scaling=scaling, windows=windows)
    return cfg, raw


def _tensor_files(path: str) -> dict[str, str]:
    """tensor name -> safetensors file, for a single or an index-sharded checkpoint."""
    if os.path.isfile(path):
        files = [path]
    else:
        idx = os.path.join(path, "model.safetensors.index.json")
        if os.path.exists(idx):
            with open(idx) as fh:
                index = json.load(fh)["weight_map"]
            return {k: os.path.join(path, v) for k, v in index.items()}
        files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith(".safetensors"))
        if not files:
            raise FileNotFoundError(f"no .safetensors files in {path}")
    from safetensors import safe_open
    out = {}
    for f in files:
        with safe_open(f, framework="pt", device="cpu") as sf:
            for k in sf.keys():
                out[k] = f
    return out


class _Reader:
    """Tensors by name across the checkpoint's files, opened lazily."""

    def __init__(self, path: str):
        from safetensors import safe_open
        self._open = safe_open
        self.where = _tensor_files(path)
        self._handles = {}

    def has(self, name: str) -> bool:
        return name in self.where

    def get(self, name: str) -> torch.Tensor:
        f = self.where.get(name)
        if f is None:
            raise KeyError(f"checkpoint has no tensor {name!r}")
        h = self._handles.get(f)
        if h is None:
            h = self._handles[f] = self._open(f, framework="pt", device="cpu").__enter__()
        return h.get_tensor(name)

    def close(self):
        for h in self._handles.values():
            h.__exit__(None, None, None)
        self._handles.clear()


def load_llama(path: str, device="cuda", max_batch: int = 8, max_seq: int | None = None,
               fused: bool = True, prefix: str = "model.", kv_dtype: str = "bf16",
               weight_dtype: str = "bf16", kv_scales=None, sliding_window: bool = False) -> TinyLlama:
    """A TinyLlama with the checkpoint's weights (bf16 on ``device``). ``kv_dtype``: "bf16" or "fp8", the KV
    cache's format (``TinyLlama``), for every family alike. ``kv_scales`` ("fp8" only): None (scale 1: ``k_scale`` /
    ``v_scale`` tensors a checkpoint may carry are then not read), a ``KvScales``, or "checkpoint": the per-layer
    ``self_attn.k_scale`` / ``.v_scale`` (or ``kv_scale``) tensors of the checkpoint, each a scalar broadcast over
    the layer's KV heads; a checkpoint that lacks them for any layer is refused. ``weight_dtype``: "bf16", "fp8"
    (docs/WEIGHT_FP8.md) or "mxfp4" (docs/WEIGHT_MXFP4.md: the layers' GEMM weights as MXFP4, the LM head as FP8): each
    layer's GEMM weights are quantised on ``device`` as soon as the layer is read and its bf16 tensors dropped, so
    the device never holds the bf16 and the quantised copies of all layers together. The checkpoint itself is bf16 / fp16
    / fp32 either way: one that is already quantised on disk is treated as before. ``sliding_window``: serve the
    checkpoint's sliding attention window (``read_config``, docs/SLIDING_WINDOW.md), fused step only; a checkpoint
    that declares none is refused."""
    from p2p_llm_tunnel_amd.models.tiny_llm import WEIGHT_DTYPES, quantize_layer_
    if weight_dtype not in WEIGHT_DTYPES:
        raise ValueError(f"weight_dtype must be one of {list(WEIGHT_DTYPES)}, got {weight_dtype!r}")
    from p2p_llm_tunnel_amd.models import kv_scales as kvs
    kv_scales = kvs.parse_kv_scales(kv_scales, kv_dtype)  # refused with a bf16 cache before anything is read
    cfg, raw = read_config(path, max_seq, sliding_window)
    if cfg.windowed and not fused:
        raise ValueError("a sliding window runs the fused step only: load with fused=True")
    c = cfg
    rd = _Reader(path)
    dev = torch.device(device)

    def t(name, shape):
        x = rd.get(name)
        if tuple(x.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(x.shape)} != expected {tuple(shape)}")
        return x.to(torch.bfloat16).to(dev)

    try:
        q_out, kv_out = c.n_heads * c.head_dim, c.n_kv_heads * c.head_dim
        w = {"embed": t(prefix + "embed_tokens.weight", (c.vocab, c.dim)),
             "final_norm": t(prefix + "norm.weight", (c.dim,)), "layers": []}
        if rd.has("lm_head.weight"):
            w["lm_head"] = t("lm_head.weight", (c.vocab, c.dim))
        elif raw.get("tie_word_embeddings", True):
            w["lm_head"] = w["embed"]
        else:
            raise KeyError("checkpoint has no lm_head.weight and does not tie embeddings")
        if kv_scales == kvs.CHECKPOINT:
            kv_scales = kvs.read_checkpoint(rd.has, rd.get, c.n_layers, c.n_kv_heads, prefix)
        for i in range(c.n_layers):
            p = f"{prefix}layers.{i}."
            q = t(p + "self_attn.q_proj.weight", (q_out, c.dim))
            k = t(p + "self_attn.k_proj.weight", (kv_out, c.dim))
            v = t(p + "self_attn.v_proj.weight", (kv_out, c.dim))
            for n in ("self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"):
                if rd.has(p + n + ".bias"):
                    raise ValueError(f"{p}{n}.bias: only q, k and v projection biases are supported by the decode "
                                     "kernels")
            bqkv = None
            if c.qkv_bias:
                bqkv = torch.cat([t(p + "self_attn.q_proj.bias", (q_out,)), t(p + "self_attn.k_proj.bias", (kv_out,)),
                                  t(p + "self_attn.v_proj.bias", (kv_out,))], 0).contiguous()
            elif any(rd.has(f"{p}self_attn.{n}_proj.bias") for n in "qkv"):
                raise ValueError(f"{p}self_attn has q/k/v projection biases, but the architecture "
                                 f"{(raw.get('architectures') or ['LlamaForCausalLM'])[0]!r} applies none: attention "
                                 "projection biases are not supported for it, refusing to load it without them")
            gate = t(p + "mlp.gate_proj.weight", (c.ffn, c.dim))
            up = t(p + "mlp.up_proj.weight", (c.ffn, c.dim))
            w["layers"].append({
                "attn_norm": t(p + "input_layernorm.weight", (c.dim,)),
                "wqkv": torch.cat([q, k, v], 0).contiguous(),
                "wo": t(p + "self_attn.o_proj.weight", (c.dim, q_out)),
                "ffn_norm": t(p + "post_attention_layernorm.weight", (c.dim,)),
                "w_gate_up": torch.cat([gate, up], 0).contiguous(),
                "w_down": t(p + "mlp.down_proj.weight", (c.dim, c.ffn)),
            })
            if bqkv is not None:
                w["layers"][-1]["bqkv"] = bqkv
            if c.qk_norm:
                w["layers"][-1]["q_norm"] = t(p + "self_attn.q_norm.weight", (c.head_dim,))
                w["layers"][-1]["k_norm"] = t(p + "self_attn.k_norm.weight", (c.head_dim,))
            elif rd.has(p + "self_attn.q_norm.weight") or rd.has(p + "self_attn.k_norm.weight"):
                raise ValueError(f"{p}self_attn has q_norm / k_norm weights, but the architecture "
                                 f"{(raw.get('architectures') or ['LlamaForCausalLM'])[0]!r} applies no QK-norm: refusing "
                                 "to load it without them")
            del q, k, v, gate, up
            if weight_dtype != "bf16":  # this layer's bf16 GEMM weights give way to the quantised ones before the next is read
                quantize_layer_(c, w["layers"][-1], weight_dtype)
    finally:
        rd.close()
    return TinyLlama.from_weights(cfg, w, device=dev, max_batch=max_batch, fused=fused, kv_dtype=kv_dtype,
                                  weight_dtype=weight_dtype, kv_scales=kv_scales)


class Detokenizer:
    """Incremental detokenisation of one generated sequence: ``push(id)``
    returns the text that token adds. Decodes a short window (the tokens since
    the last emitted boundary) rather than the whole sequence, so a token costs
    O(window), and holds text back while it ends in an incomplete UTF-8
    sequence (byte-fallback tokens)."""

    __slots__ = ("tok", "ids", "prefix", "read")

    def __init__(self, tok, prompt_ids: list[int]):
        self.tok = tok
        self.ids = list(prompt_ids[-4:])  # a little context: leading-space rules depend on it
        self.prefix = 0
        self.read = len(self.ids)

    def push(self, tid: int) -> str:
        self.ids.append(tid)
        before = self.tok.decode(self.ids[self.prefix:self.read], skip_special_tokens=True)
        after = self.tok.decode(self.ids[self.prefix:], skip_special_tokens=True)
        if len(after) <= len(before) or after.endswith("\ufffd"):
            return ""
        self.prefix, self.read = self.read, len(self.ids)
        return after[len(before):]


class Tokenizer:
    """The checkpoint's ``tokenizer.json`` (Hugging Face ``tokenizers``: a
    Rust library; the file is data, no code from it runs), its special ids and
    its chat template (``tokenizer_config.json``), rendered in jinja2's
    immutable sandbox."""

    def __init__(self, path: str, eos_ids: list[int] | None = None):
        from tokenizers import Tokenizer as _T
        d = path if os.path.isdir(path) else os.path.dirname(path)
        f = os.path.join(path, "tokenizer.json") if os.path.isdir(path) else path
        self.tok = _T.from_file(f)
        self.eos_ids = set(eos_ids or [])
        self.bos = self.eos = ""
        self.template = None
        tc = os.path.join(d, "tokenizer_config.json")
        if os.path.exists(tc):
            with open(tc) as fh:
                conf = json.load(fh)

            def tokstr(v):
                return v.get("content", "") if isinstance(v, dict) else (v or "")
            self.bos, self.eos = tokstr(conf.get("bos_token")), tokstr(conf.get("eos_token"))
            t = conf.get("chat_template")
            if isinstance(t, list):  # [{name, template}, ...]
                t = next((x["template"] for x in t if x.get("name") == "default"), t[0]["template"] if t else None)
            if t:
                from jinja2.sandbox import ImmutableSandboxedEnvironment

                def fail(msg):
                    raise ValueError(msg)
                env = ImmutableSandboxedEnvironment(trim_blocks=True, lstrip_blocks=True)
                env.globals["raise_exception"] = fail
                self.template = env.from_string(t)
            if self.eos and not self.eos_ids:
                e = self.tok.token_to_id(self.eos)
                if e is not None:
                    self.eos_ids.add(e)

    @classmethod
    def for_checkpoint(cls, path: str) -> "Tokenizer | None":
        f = os.path.join(path, "tokenizer.json") if os.path.isdir(path) else None
        if not f or not os.path.exists(f):
            return None
        eos = []
        try:
            _, raw = read_config(path)
            e = raw.get("eos_token_id")
            eos = e if isinstance(e, list) else ([e] if e is not None else [])
        except (OSError, ValueError, KeyError):
            pass
        # generation_config.json may list more (Qwen3: <|im_end|> and <|endoftext|>)
        gc = os.path.join(path, "generation_config.json")
        if os.path.exists(gc):
            try:
                with open(gc) as fh:
                    e = json.load(fh).get("eos_token_id")
                more = e if isinstance(e, list) else ([e] if e is not None else [])
                eos = list(eos) + [int(x) for x in more if isinstance(x, int) and not isinstance(x, bool)
                                   and x not in eos]
            except (OSError, ValueError, AttributeError):
                pass
        return cls(path, eos)

    def encode(self, text: str, special: bool = True) -> list[int]:
        return self.tok.encode(text, add_special_tokens=special).ids

    def decode(self, ids: list[int]) -> str:
        return self.tok.decode(ids, skip_special_tokens=True)

    def chat(self, messages: list[dict], template_kwargs: dict | None = None) -> list[int]:
        """Prompt ids for a chat: the checkpoint's template with the generation
        prompt appended, or plain ``role: content`` lines without one.
        ``template_kwargs``: extra scalar variables for the template (e.g.
        ``enable_thinking`` for Qwen3's); they never override the ones set here."""
        msgs = [{"role": str(m.get("role", "user")), "content": str(m.get("content", ""))} for m in messages]
        if self.template is not None:
            text = self.template.render(**{**(template_kwargs or {}), "messages": msgs, "add_generation_prompt": True,
                                           "bos_token": self.bos, "eos_token": self.eos})
            return self.encode(text, special=False)
        return self.encode("".join(f"{m['role']}: {m['content']}\n" for m in msgs) + "assistant:")

    def detokenizer(self, prompt_ids: list[int]) -> Detokenizer:
        return Detokenizer(self.tok, prompt_ids)

    def token_bytes(self) -> list[bytes]:
        """The bytes every id adds to the text, by id (guided decoding walks
        them through its automaton; ``models/guided.py``). Special (control)
        tokens and ids the vocabulary leaves unused give b"": they never take
        part in a guided completion. Two kinds of vocabulary are understood:
        ByteLevel BPE (Llama 3, Qwen: every character of a token stands for one
        byte, by the GPT-2 byte table, inverted here) and Metaspace /
        byte-fallback vocabularies (Llama 2, Mistral: U+2581 stands for a space,
        ``<0xNN>`` for the byte NN). Any other kind raises ValueError. Computed
        once."""
        got = getattr(self, "_token_bytes", None)
        if got is not None:
            return got
        spec = json.loads(self.tok.to_str())
        model = spec.get("model") or {}

        def kinds(node):
            if not isinstance(node, dict):
                return set()
            out = {node.get("type")}
            for sub in node.get("decoders") or node.get("pretokenizers") or []:
                out |= kinds(sub)
            return out
        used = kinds(spec.get("decoder")) | kinds(spec.get("pre_tokenizer"))
        if model.get("type") == "BPE" and "ByteLevel" in used:
            # The GPT-2 table: printable bytes stand for themselves, the rest are numbered from U+0100 up.
            keep = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
            table, n = {chr(b): b for b in keep}, 0
            for b in range(256):
                if b not in keep:
                    table[chr(256 + n)] = b
                    n += 1

            def to_bytes(text):
                return bytes(table[c] for c in text) if all(c in table for c in text) else None
        elif model.get("type") in ("BPE", "Unigram") and ("Metaspace" in used or model.get("byte_fallback")):
            def to_bytes(text):
                if len(text) == 6 and text.startswith("<0x") and text.endswith(">"):
                    try:
                        return bytes([int(text[3:5], 16)])
                    except ValueError:
                        pass
                return text.replace("▁", " ").encode("utf-8")
        else:
            raise ValueError(f"guided decoding understands ByteLevel BPE and Metaspace / byte-fallback tokenizers; "
                             f"this one is a {model.get('type')!r} model with {sorted(k for k in used if k)}")
        added = {a["id"]: a for a in spec.get("added_tokens") or []}
        vocab = self.tok.get_vocab(with_added_tokens=True)
        out = [b""] * (max(vocab.values()) + 1 if vocab else 0)
        for text, tid in vocab.items():
            a = added.get(tid)
            if a is not None:  # an added token is literal text; a special one is control
                out[tid] = b"" if a.get("special") else a.get("content", "").encode("utf-8")
            else:
                out[tid] = to_bytes(text) or b""
        self._token_bytes = out
        return out
