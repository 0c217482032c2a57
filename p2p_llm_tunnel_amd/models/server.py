"""OpenAI/Ollama-compatible streaming endpoint backed by ``TinyLlama`` on a HIP device.

This is the "local inference endpoint on the MI355X node" that ``tunnel serve
--upstream`` fronts (BASELINE.json configs #2/#5). One engine thread owns the
GPU and runs iteration-level (continuous) batching: every step advances each
active slot by one token — a prompt token while prefilling, the last sampled
token while decoding — so new requests join without waiting for others.

One asyncio thread serves HTTP/1.1 (keep-alive, chunked) for every
connection. The engine hands each step's tokens to it in ONE batch
(``call_soon_threadsafe``) and the I/O thread writes them from pre-rendered
byte templates, so a step costs one thread hand-off instead of one per
stream, and the engine waits for the GPU with the GIL released (event sync on
a pinned output buffer) while the I/O thread writes the previous step's
tokens. (The thread-per-connection server this replaces spent ~1.3 ms of
GIL ping-pong per 8-stream step around a 0.18 ms GPU step;
profiles/bench_gpu_upstream_r01.json.)

  GET  /v1/models, /health, /api/tags
  POST /v1/chat/completions  (SSE when "stream": true; JSON otherwise)
  POST /v1/completions       (same, "prompt" instead of "messages")
  POST /api/generate         (Ollama NDJSON stream)
  POST /v1/embeddings, /api/embed, /api/embeddings  (see "Embeddings" below)

Sampling: temperature / top_p / seed (and the common top_k extension) from an
OpenAI request, or "options" of an Ollama one, drawn on device after the LM
head (ops.sample_, sample.hip: top-k and top-p by radix select, Gumbel-max
draw); temperature 0 — the default unless --default-temperature — keeps the
fused LM head's greedy argmax. Stop sequences (OpenAI "stop": a string or up
to 4; Ollama "options.stop") end a completion at the first match in the
detokenised text, which is left out (finish_reason "stop"); a streamed
response holds back only a tail that could still begin one. Parameters that
would change the output and are not implemented (n > 1, penalties,
logit_bias, Ollama's repeat_penalty, mirostat, ...) are answered
with 400, as is sampling on an engine without the captured HIP step.

Penalties (--penalties, off by default: the 400s above stand): OpenAI
"presence_penalty" and "frequency_penalty" in [-2, 2], the vLLM extension
"repetition_penalty" in (0, 10] and "logit_bias" (an object of up to 300
decimal token ids in [0, vocab) -> a bias in [-100, 100]); Ollama
"options.repeat_penalty" in (0, 10], "presence_penalty" and
"frequency_penalty". They run on device inside the captured step, ahead of
the sampler (ops.penalize_, penalty.hip): a per-slot table counts every
generated id and marks the prompt's, the repetition penalty divides or
multiplies the logit of every id seen in the prompt or generated (HF / vLLM
semantics — NOT Ollama's window of the last 64 tokens: "repeat_last_n" is
accepted only as -1, or 0 = repeat penalty off; anything else is a 400 that
says so), frequency and presence subtract by the generated count, the bias
is added last, and greedy requests take the argmax of the result. n > 1,
best_of, mirostat, tfs_z, typical_p and min_p stay refused. See
docs/PENALTIES.md.

Guided decoding (--guided, off by default: the keys below are then not acted
on): /v1/chat/completions and /v1/completions take "guided_regex" (a string:
the whole completion matches it), "guided_choice" (a non-empty list of
non-empty strings: the completion is one of them) or the newer
"structured_outputs": {"regex": ...} / {"choice": [...]}; more than one of
them, a wrong type, a pattern outside the supported subset, a server without a
tokenizer or with one whose tokens' bytes are not known are answered with 400
and the reason. The pattern is compiled off the I/O thread (an executor; a small
LRU of compiled guides) into a token-level automaton (models/guided.py) whose
table the engine keeps in a device arena; ops.guide_ (guide.hip) walks it
inside the captured step, after the penalties and ahead of the sampler, and
masks every token the automaton's state does not allow. A completion that
reaches a full match with nothing left to add ends through EOS (finish_reason
"stop"); one cut by max_tokens ends with "length" and may be an incomplete
match. "response_format", JSON schemas, Ollama's "format" and grammars that
need a stack are out of scope. See docs/GUIDED.md.

Chat template variables: a chat request's optional "chat_template_kwargs", a
JSON object of scalars, is handed to the checkpoint's chat template
({"enable_thinking": false} for Qwen3's); anything else is answered with 400.

Log-probabilities: /v1/chat/completions takes "logprobs": true with
"top_logprobs" 0..20, /v1/completions the legacy "logprobs" 1..5. They are
computed on device inside the captured step (ops.logprobs_, logprobs.hip: a
log-sum-exp and a deterministic top-N selection per requesting row) and come
back with the sampled ids through pinned memory. The distribution is the
model's own softmax(logits): it does not depend on temperature, top_k or top_p
(vLLM's default too), nor on penalties or logit_bias: the logprobs kernel
reads the raw logits, so a banned token still reports the model's probability. Every delivered token has an entry, the tokens of a
matched stop sequence included (their text is cut, their entries are not); the
EOS token has none. A streamed chat response with logprobs sends exactly one
chunk per token (its "content" is "" when the detokeniser or the stop matcher
holds the text back). Non-finite values are sent as -9999.0. The eager engine
has no logits and answers such a request with 400; /api/generate has no
logprobs.

Prefix cache (--prefix-cache, off by default): a request whose prompt begins
like the K/V rows a cache slot already holds — the next turn of a chat, a
second stream with the same system prompt — takes those rows instead of
prefilling them again: in place when that slot is free, copied slot to slot on
the device (ops.kv_copy_, kv_copy.hip) when it is busy; see ``Engine``.
Non-streamed chat responses then report usage.prompt_tokens_details.cached_tokens.

Embeddings: /v1/embeddings (OpenAI: "input" a string, a list of strings, a
list of token ids or a list of such lists, 1..256 items; "encoding_format"
"float" or "base64" = little-endian float32 bytes; "dimensions" must equal the
model's), /api/embed (Ollama: "input" a string or a list of strings;
"truncate", default true, keeps the first max_seq - 1 tokens) and the legacy
/api/embeddings ("prompt"). The text is tokenised without a chat template;
every item is one engine request that prefills and never samples, and its
final hidden state (after the final norm) is pooled on the device
(ops.embed_pool_, embed_pool.hip: the mean over all positions, or with
--embed-pooling last the last position's; L2-normalised). An empty item, or
one longer than max_seq - 1 tokens where nothing truncates, is answered with
400 naming the item.

Two model sources:

* random-init (``--config tiny|small|micro``, the benchmark default): byte-level
  prompts (bytes mod vocab), generated ids rendered as `` t<id>`` pieces;
* a Hugging Face Llama-architecture checkpoint (``--checkpoint DIR``: config.json,
  safetensors, tokenizer.json; loaded weights-only by ``checkpoint.py``): prompts
  go through the checkpoint's tokenizer and chat template, tokens are
  detokenised incrementally, and generation stops at the EOS token
  (finish_reason "stop").
"""
from __future__ import annotations

import argparse
import asyncio
import functools
import json
import os
import queue
import socket
import sys
import threading
import time
import uuid
from typing import NamedTuple

import torch


class Sampling:
    """How a request picks its tokens: temperature (0 = greedy argmax, the
    fused LM head's own result), then top-k (0 = off) and top-p (1 = off),
    drawn on device by ``ops.sample_`` (sample.hip) from a per-request seed
    and the token's index, so a fixed seed replays the same completion."""
    __slots__ = ("temperature", "top_k", "top_p", "seed")

    def __init__(self, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, seed: int | None = None):
        self.temperature = float(temperature)
        self.top_k = int(top_k)
        self.top_p = float(top_p)
        self.seed = int.from_bytes(os.urandom(8), "little") >> 1 if seed is None else int(seed) & ((1 << 63) - 1)

    @property
    def greedy(self) -> bool:
        return not self.temperature >= 1e-4 or self.top_k == 1  # the kernel's own greedy rule (+ top-1)

    def column(self, counter: int) -> list[int]:
        from p2p_llm_tunnel_amd.ops import pack_sampling
        return pack_sampling(0.0 if self.greedy else self.temperature, self.top_k, self.top_p, self.seed, counter)


class Penalties:
    """What a request does to its logits ahead of the sampler, on device
    (``ops.penalize_``, penalty.hip; an engine built with ``penalties=True``):
    ``repetition`` (HF / vLLM: a seen id's logit x becomes x / r when x > 0,
    else x * r; seen = anywhere in the prompt or generated; 1 = off), then
    ``frequency`` and ``presence`` (OpenAI: x -= f * count and x -= p *
    (count > 0), counts over generated tokens; 0 = off), then ``logit_bias``
    ({id: value in [-100, 100]}, at most 300 ids, added last)."""
    __slots__ = ("repetition", "frequency", "presence", "logit_bias")

    def __init__(self, repetition: float = 1.0, frequency: float = 0.0, presence: float = 0.0, logit_bias=None):
        from p2p_llm_tunnel_amd.ops import MAX_LOGIT_BIAS
        for name, v, ok in (("repetition", repetition, lambda x: 0.0 < x <= 10.0),
                            ("frequency", frequency, lambda x: -2.0 <= x <= 2.0),
                            ("presence", presence, lambda x: -2.0 <= x <= 2.0)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not ok(v):
                raise ValueError(f"{name}={v!r} is out of range (repetition in (0, 10], frequency and presence "
                                 "in [-2, 2])")
        self.repetition, self.frequency, self.presence = float(repetition), float(frequency), float(presence)
        bias = dict(logit_bias or {})
        if len(bias) > MAX_LOGIT_BIAS:
            raise ValueError(f"logit_bias takes at most {MAX_LOGIT_BIAS} entries, got {len(bias)}")
        for k, v in bias.items():
            if type(k) is not int or k < 0 or isinstance(v, bool) or not isinstance(v, (int, float)) or \
                    not -100.0 <= v <= 100.0:
                raise ValueError(f"logit_bias maps token ids (ints >= 0) to values in [-100, 100], got {k!r}: {v!r}")
        self.logit_bias = {k: float(v) for k, v in bias.items()}  # a dict: no id twice

    @property
    def neutral(self) -> bool:
        return self.repetition == 1.0 and self.frequency == 0.0 and self.presence == 0.0 and \
            not any(self.logit_bias.values())

    def column(self) -> list[int]:
        from p2p_llm_tunnel_amd.ops import pack_penalties
        return pack_penalties(self.repetition, self.frequency, self.presence)


class SamplingError(ValueError):
    """A request asks for sampling this server does not implement (answered with 400)."""


def _number(src: dict, key: str, lo: float, hi: float, default, integer=False, lo_open=False):
    v = src.get(key)
    if v is None:
        return default
    if isinstance(v, bool) or not isinstance(v, (int, float)) or (integer and isinstance(v, float) and not v.is_integer()):
        raise SamplingError(f"{key} must be {'an integer' if integer else 'a number'}, got {v!r}")
    if not (lo < v if lo_open else lo <= v) or v > hi:
        raise SamplingError(f"{key} must be in {'(' if lo_open else '['}{lo}, {hi}], got {v!r}")
    return int(v) if integer else float(v)


# Parameters that would change which tokens come out and that this server
# does not implement: neutral values pass, anything else is refused instead of
# being silently ignored.
_OPENAI_NEUTRAL = {"n": (1,), "best_of": (1,), "presence_penalty": (0, 0.0), "frequency_penalty": (0, 0.0),
                   "logprobs": (False, 0), "top_logprobs": (0,), "logit_bias": ({},)}
_OLLAMA_NEUTRAL = {"repeat_penalty": (1, 1.0), "presence_penalty": (0, 0.0), "frequency_penalty": (0, 0.0),
                   "mirostat": (0,), "tfs_z": (1, 1.0), "typical_p": (1, 1.0), "min_p": (0, 0.0)}
_MAX_STOPS = 4  # the OpenAI API's limit


# What --penalties takes out of the two tables above (ops.penalize_ implements them).
_OPENAI_PENALTY_KEYS = ("presence_penalty", "frequency_penalty", "logit_bias")
_OLLAMA_PENALTY_KEYS = ("repeat_penalty", "presence_penalty", "frequency_penalty")


def penalty_params(body: dict, ollama: bool, vocab: int | None = None) -> Penalties | None:
    """Penalties of a request on a server started with --penalties; None when
    every one is absent or neutral. OpenAI: "presence_penalty" and
    "frequency_penalty" in [-2, 2], the vLLM extension "repetition_penalty" in
    (0, 10], "logit_bias": an object of at most 300 entries whose keys are
    decimal token ids in [0, vocab) — two keys that name one id are refused —
    and whose values are numbers in [-100, 100]. Ollama ("options"):
    "repeat_penalty" in (0, 10], "presence_penalty", "frequency_penalty" in
    [-2, 2]. The repeat penalty covers the whole prompt and everything generated
    (HF / vLLM), not Ollama's window of the last 64 tokens, so "repeat_last_n" is
    accepted only as -1 (everything) or 0 (which switches the repeat penalty
    off). Raises SamplingError (answered with 400) naming the parameter."""
    src = body.get("options", {}) if ollama else body
    if src is None:
        src = {}
    if not isinstance(src, dict):
        raise SamplingError("options must be an object")
    presence = _number(src, "presence_penalty", -2.0, 2.0, 0.0)
    frequency = _number(src, "frequency_penalty", -2.0, 2.0, 0.0)
    bias = {}
    if ollama:
        rep = _number(src, "repeat_penalty", 0.0, 10.0, 1.0, lo_open=True)
        last_n = src.get("repeat_last_n")
        if last_n is not None:
            if type(last_n) is not int or last_n not in (-1, 0):
                raise SamplingError(f"repeat_last_n={last_n!r} is not supported: the repeat penalty covers the whole "
                                    "prompt and everything generated; only -1 (everything) and 0 (repeat penalty "
                                    "off) are accepted")
            if last_n == 0:
                rep = 1.0
    else:
        rep = _number(src, "repetition_penalty", 0.0, 10.0, 1.0, lo_open=True)
        raw = src.get("logit_bias")
        if raw is not None:
            from p2p_llm_tunnel_amd.ops import MAX_LOGIT_BIAS
            if not isinstance(raw, dict):
                raise SamplingError(f"logit_bias must be an object of token id: bias, got {raw!r}")
            if len(raw) > MAX_LOGIT_BIAS:
                raise SamplingError(f"logit_bias takes at most {MAX_LOGIT_BIAS} entries, got {len(raw)}")
            for k, v in raw.items():
                if not (isinstance(k, str) and k.isascii() and k.isdigit()):
                    raise SamplingError(f"logit_bias key {k!r} is not a decimal token id")
                tid = int(k)
                if vocab is not None and tid >= vocab:
                    raise SamplingError(f"logit_bias key {k!r} is outside the vocabulary [0, {vocab})")
                if tid in bias:
                    raise SamplingError(f"logit_bias names token id {tid} twice")
                if isinstance(v, bool) or not isinstance(v, (int, float)) or not -100.0 <= v <= 100.0:
                    raise SamplingError(f"logit_bias[{k!r}] must be a number in [-100, 100], got {v!r}")
                bias[tid] = float(v)
    pen = Penalties(rep, frequency, presence, bias)
    return None if pen.neutral else pen


def sampling_params(body: dict, ollama: bool, default_temperature: float = 0.0, penalties: bool = False,
                    vocab: int | None = None) -> Sampling:
    """Sampling of an OpenAI request (top-level temperature / top_p / seed, and
    the common top_k extension) or an Ollama one ("options"). Raises
    SamplingError for values out of range or parameters not implemented.

    "logprobs" and "top_logprobs" are not sampling: this function refuses any
    non-neutral value of either. The OpenAI endpoints parse them first with
    ``logprob_params`` and pass this function the body without the two keys.

    ``penalties`` (a server started with --penalties; ``vocab``: the model's):
    the penalty parameters and logit_bias are then checked by
    ``penalty_params`` — whose result the caller takes from there — instead of
    being refused unless neutral; everything else is as without the switch."""
    src = body.get("options", {}) if ollama else body
    if src is None:
        src = {}
    if not isinstance(src, dict):
        raise SamplingError("options must be an object")
    taken = () if not penalties else _OLLAMA_PENALTY_KEYS if ollama else _OPENAI_PENALTY_KEYS
    for key, neutral in (_OLLAMA_NEUTRAL if ollama else _OPENAI_NEUTRAL).items():
        if key in taken:
            continue
        if key in src and src[key] is not None and not any(src[key] == x and type(src[key]) is type(x)
                                                            for x in neutral):
            raise SamplingError(f"{key}={src[key]!r} is not supported by this server")
    if penalties:
        penalty_params(body, ollama, vocab)
    t = _number(src, "temperature", 0.0, 100.0, default_temperature)
    top_p = _number(src, "top_p", 0.0, 1.0, 1.0, lo_open=True)
    top_k = _number(src, "top_k", 0, 1 << 30, 0, integer=True)
    seed = _number(src, "seed", -(1 << 63), (1 << 64) - 1, None, integer=True)
    return Sampling(t, top_k, top_p, seed)


_GUIDE_KEYS = ("guided_regex", "guided_choice", "structured_outputs")


def guided_params(body: dict):
    """What a request on a server started with --guided asks its completion to
    match: None, or ``(kind, pattern)`` for ``guided.compile_guide``: ("regex",
    a string) from "guided_regex" or "structured_outputs": {"regex": ...},
    ("choice", a tuple of non-empty strings) from "guided_choice" or
    "structured_outputs": {"choice": [...]}. A null value counts as absent.
    More than one of them, or a wrong type, raises SamplingError (answered with
    400) naming the key. The pattern itself is checked by the compiler."""
    found = []
    v = body.get("guided_regex")
    if v is not None:
        found.append(("guided_regex", "regex", v))
    v = body.get("guided_choice")
    if v is not None:
        found.append(("guided_choice", "choice", v))
    so = body.get("structured_outputs")
    if so is not None:
        if not isinstance(so, dict):
            raise SamplingError(f"structured_outputs must be an object, got {so!r}")
        other = sorted(k for k, x in so.items() if k not in ("regex", "choice") and x is not None)
        if other:
            raise SamplingError(f"structured_outputs.{other[0]} is not supported by this server: it takes "
                                '"regex" and "choice"')
        for k in ("regex", "choice"):
            if so.get(k) is not None:
                found.append((f"structured_outputs.{k}", k, so[k]))
    if not found:
        return None
    if len(found) > 1:
        raise SamplingError(f"{found[0][0]} and {found[1][0]} cannot be combined: a request takes one guide")
    name, kind, v = found[0]
    if kind == "regex":
        if not isinstance(v, str):
            raise SamplingError(f"{name} must be a string, got {v!r}")
        return kind, v
    if not isinstance(v, list) or not v or not all(isinstance(c, str) and c for c in v):
        raise SamplingError(f"{name} must be a non-empty list of non-empty strings, got {v!r}")
    return kind, tuple(v)


_LEGACY_MAX_LOGPROBS = 5  # /v1/completions: the OpenAI API's limit for the legacy integer form
_LOGPROB_KEYS = ("logprobs", "top_logprobs")


def logprob_params(body: dict, kind: str) -> int | None:
    """How many top log-probabilities a request wants beside each chosen
    token's own: None = no logprobs at all, N in 0..20 = the chosen token's plus
    the top N. ``kind`` is the endpoint: "chat" takes "logprobs": true with
    "top_logprobs" in 0..20 (default 0; a non-zero "top_logprobs" without
    "logprobs": true is refused), "text" the legacy integer "logprobs" in 1..5
    (null, false and 0 are off), "ollama" has none. Raises SamplingError
    (answered with 400) naming the offending field."""
    if kind == "ollama":
        return None
    lp = body.get("logprobs")
    if kind == "chat":
        if lp is not None and not isinstance(lp, bool) and not (type(lp) is int and lp == 0):  # 0: off, as before
            raise SamplingError(f"logprobs must be a boolean, got {lp!r}")
        from p2p_llm_tunnel_amd.ops import MAX_TOP_LOGPROBS
        top = _number(body, "top_logprobs", 0, MAX_TOP_LOGPROBS, None, integer=True)
        if not lp:
            if top:
                raise SamplingError(f"top_logprobs={top!r} needs logprobs: true")
            return None
        return top or 0
    top = body.get("top_logprobs")
    if top is not None and not (top == 0 and type(top) is int):
        raise SamplingError(f"top_logprobs={top!r} belongs to /v1/chat/completions; /v1/completions takes "
                            f"logprobs: 1..{_LEGACY_MAX_LOGPROBS}")
    if lp is None or lp is False:
        return None
    n = _number(body, "logprobs", 0, _LEGACY_MAX_LOGPROBS, None, integer=True)
    return n or None


def _finite(x: float) -> float:
    """JSON has no -inf: a non-finite logprob is sent as -9999.0, as the OpenAI API does."""
    return x if -float("inf") < x < float("inf") else -9999.0


def chat_logprob_entry(token: int, record, text_of) -> dict:
    """One element of a chat response's ``logprobs.content``: ``record`` is
    ``(chosen_logprob, [(id, logprob), ...])`` as the engine appends it to
    ``Request.lp``, ``text_of(id)`` the token's text."""
    def one(tid, lp):
        text = text_of(tid)
        return {"token": text, "logprob": _finite(lp), "bytes": list(text.encode("utf-8"))}
    chosen, top = record
    entry = one(token, chosen)
    entry["top_logprobs"] = [one(tid, lp) for tid, lp in top]
    return entry


def chat_logprobs(tokens: list[int], records: list, text_of) -> dict:
    """``choices[0].logprobs`` of a chat completion."""
    return {"content": [chat_logprob_entry(t, r, text_of) for t, r in zip(tokens, records)]}


def completion_logprobs(tokens: list[int], records: list, text_of, offset: int = 0) -> dict:
    """``choices[0].logprobs`` of a legacy completion: four lists of one length.
    ``text_offset`` counts characters of the tokens' own texts from the start
    of the completion (``offset``: where the first of ``tokens`` starts, for a
    streamed chunk); ``top_logprobs`` maps token text to logprob (of two ids
    with the same text the more probable one stays)."""
    out = {"tokens": [], "token_logprobs": [], "top_logprobs": [], "text_offset": []}
    for t, (chosen, top) in zip(tokens, records):
        text = text_of(t)
        out["tokens"].append(text)
        out["token_logprobs"].append(_finite(chosen))
        tops = {}
        for tid, lp in top:
            tops.setdefault(text_of(tid), _finite(lp))
        out["top_logprobs"].append(tops)
        out["text_offset"].append(offset)
        offset += len(text)
    return out


def stop_sequences(body: dict, ollama: bool) -> list[str]:
    """Stop sequences of an OpenAI request ("stop": null, a string, or a list
    of up to 4 strings) or an Ollama one ("options.stop": a list of strings).
    Empty strings are dropped (they would match at once); anything else that
    is not a string is refused."""
    src = body.get("options", {}) if ollama else body
    if not isinstance(src, dict):
        return []
    v = src.get("stop")
    if v is None:
        return []
    if isinstance(v, str):
        v = [v]
    if not isinstance(v, list) or not all(isinstance(x, str) for x in v):
        raise SamplingError(f"stop must be a string or a list of strings, got {v!r}")
    if len(v) > _MAX_STOPS and not ollama:
        raise SamplingError(f"stop takes at most {_MAX_STOPS} sequences, got {len(v)}")
    return [x for x in v if x]


class StopMatcher:
    """Finds the first stop sequence in a completion's text as pieces arrive.

    ``push(piece)`` returns the text that is safe to emit and whether a stop
    sequence ended the completion (the text up to the match is emitted, the
    match and everything after it are not). A tail that could still be the
    start of a stop sequence is held back until the next piece decides it;
    ``flush()`` releases it when the completion ends for another reason."""
    __slots__ = ("stops", "buf")

    def __init__(self, stops: list[str]):
        self.stops = stops
        self.buf = ""

    def push(self, piece: str) -> tuple[str, bool]:
        buf = self.buf + piece
        hit = -1
        for s in self.stops:
            i = buf.find(s)
            if i >= 0 and (hit < 0 or i < hit):
                hit = i
        if hit >= 0:
            self.buf = ""
            return buf[:hit], True
        keep = 0
        for s in self.stops:
            for k in range(min(len(s) - 1, len(buf)), keep, -1):
                if buf.endswith(s[:k]):
                    keep = k
                    break
        self.buf = buf[len(buf) - keep:] if keep else ""
        return (buf[:len(buf) - keep] if keep else buf), False

    def flush(self) -> str:
        out, self.buf = self.buf, ""
        return out


class Request:
    """A generation request. Tokens go to ``out`` (a queue ending with None)
    unless ``batched`` is set: then the engine's ``deliver`` hook receives them
    together with every other batched request's tokens of the same step.
    ``logprobs``: None is off; N in 0..20 asks for each token's log-probability
    and the top N: the engine appends ``(chosen_logprob, [(id, logprob), ...])``
    to ``lp`` before it hands the token over.
    ``embed``: None generates; "mean" or "last" makes it an embedding request,
    which prefills the prompt's first ``max_seq - 1`` tokens and samples
    nothing: no token is delivered, and when the terminating None arrives
    ``embedding`` holds the pooled, L2-normalised final hidden state (float32,
    ``dim`` values; the mean over all positions, or the last position's).
    ``penalties``: a ``Penalties`` (None, or a neutral one, is off); needs an
    engine built with ``penalties=True``, and an embedding request takes none.
    ``guide``: a ``guided.Guide`` compiled for the model's vocabulary (None is
    off): every token is then one the guide's automaton allows; needs an engine
    built with ``guided=True``, and an embedding request takes none."""

    def __init__(self, prompt_ids: list[int], max_new: int, batched: bool = False, sampling: Sampling | None = None,
                 logprobs: int | None = None, embed: str | None = None, penalties: Penalties | None = None,
                 guide=None):
        if embed not in (None, "mean", "last"):
            raise ValueError(f'embed must be None, "mean" or "last", got {embed!r}')
        if guide is not None:
            from p2p_llm_tunnel_amd.models.guided import Guide
            if not isinstance(guide, Guide):
                raise TypeError(f"guide must be a guided.Guide, got {guide!r}")
            if embed is not None:
                raise ValueError("an embedding request samples nothing and takes no guide")
        self.guide = guide
        if penalties is not None and not isinstance(penalties, Penalties):
            raise TypeError(f"penalties must be a Penalties, got {penalties!r}")
        if penalties is not None and penalties.neutral:
            penalties = None
        if penalties is not None and embed is not None:
            raise ValueError("an embedding request samples nothing and takes no penalties")
        self.penalties = penalties
        self.embed = embed
        self.embedding = None
        if logprobs is not None:
            from p2p_llm_tunnel_amd.ops import MAX_TOP_LOGPROBS
            if isinstance(logprobs, bool) or not isinstance(logprobs, int) or not 0 <= logprobs <= MAX_TOP_LOGPROBS:
                raise ValueError(f"logprobs must be None or an integer in 0..{MAX_TOP_LOGPROBS}, got {logprobs!r}")
        self.logprobs = logprobs
        self.lp: list = []
        self.prompt = prompt_ids
        self.max_new = max_new
        self.out: queue.Queue = queue.Queue()
        self.generated = 0
        self.cancelled = False
        self.batched = batched
        self.sampling = sampling or Sampling()
        self.state = None  # front-end bookkeeping for batched requests
        self.cached_tokens = 0  # prompt rows taken from the prefix cache (set at admission)
        self.kv = None  # the engine's slot state of this request (prefix cache: drained ids are recorded there)


_MAX_COPY_JOBS = 8  # jobs per ``model.kv_copy`` call (ops.MAX_KV_COPY_JOBS)
_MAX_EMBED_JOBS = 16  # jobs per ``model.embed_pool`` call (ops.MAX_EMBED_JOBS)


def _common_prefix(a: list, b: list) -> int:
    """Length of the longest common prefix of two lists (slices compare at C speed)."""
    n, i = min(len(a), len(b)), 0
    while i < n and a[i:min(i + 64, n)] == b[i:min(i + 64, n)]:
        i = min(i + 64, n)
    while i < n and a[i] == b[i]:
        i += 1
    return i


# One token row of a planned step (a decode row's token is read on the device).
_Row = NamedTuple("_Row", [("slot", int), ("token", int), ("pos", int), ("decode", int), ("emit", bool)])

# Rows of the staging buffer, one column per token row: token (prompt rows),
# position, cache slot, decode flag, slot to record the sampled id under
# (scratch for rows that emit nothing), then the sampler's column
# (temperature bits, top_k, top_p bits, seed, counter; temperature 0 = greedy),
# then what the row wants of ops.logprobs_ (0 = nothing, 1 + N = the chosen
# token's logprob and the top N).
_TOK, _POS, _SLOT, _DEC, _REC = range(5)
_SMP = slice(5, 10)
_LP = 10
_IN_ROWS = _LP + 1
# An engine built with penalties=True stages four more rows, ops.penalize_'s
# column: repetition, frequency and presence bits, flags (0 = the row is off).
_PEN = slice(_IN_ROWS, _IN_ROWS + 4)


class _StepBuf:
    """Host staging of one in-flight step (two alternate: step k+1 is planned
    and launched while step k runs); ``h_in`` has the rows named above.
    ``h_lp`` / ``h_lp_ids`` receive ops.logprobs_'s outputs of the rows that
    asked (steps that replay a graph with the logprobs kernel)."""

    def __init__(self, rows: int, cuda: bool, device=None, in_rows: int = _IN_ROWS):
        from p2p_llm_tunnel_amd.ops import MAX_TOP_LOGPROBS
        self.rows = rows
        self.h_in = torch.zeros((in_rows, rows), dtype=torch.int64, pin_memory=cuda)
        self.np = self.h_in.numpy()
        self.h_out = torch.zeros(rows, dtype=torch.int64, pin_memory=cuda)
        self.h_lp = torch.zeros((rows, MAX_TOP_LOGPROBS + 1), dtype=torch.float32, pin_memory=cuda)
        self.h_lp_ids = torch.zeros((rows, MAX_TOP_LOGPROBS), dtype=torch.int32, pin_memory=cuda)
        # Device twins (captured engines only: the eager step has no logits).
        self.d_lp = self.d_lp_ids = None
        if device is not None:
            self.d_lp = torch.zeros(self.h_lp.shape, dtype=torch.float32, device=device)
            self.d_lp_ids = torch.zeros(self.h_lp_ids.shape, dtype=torch.int32, device=device)
        self.ev = torch.cuda.Event() if cuda else None
        self.n = 0
        self.emits = []  # (row, req, finished, token index)
        # Embedding requests that finish in this step: (req, row of h_emb). The
        # buffers ([max_batch, dim] fp32, device and pinned) come with the first such step.
        self.embeds = []
        self.d_emb = self.h_emb = None


class Engine:
    """Continuous batching with chunked prefill over the fused decode step,
    one step in flight ahead of the host.

    Every step packs up to ``rows`` (64) token rows: first one decode row per
    generating sequence, then prompt chunks of prefilling sequences, each row
    tagged with its cache slot and position (``TinyLlama.decode_step(slots=)``).
    A 512-byte prompt is thus prefilled in 8 steps instead of 512, while
    generating sequences keep emitting a token every step. Steps of up to 16
    rows replay a 16-row graph, larger ones a 64-row graph; padding rows point
    at the model's scratch slot.

    The schedule never depends on token values (no stop tokens; lengths are
    known), so the host plans step k+1 while step k runs: a decode row's input
    token is read on the device from ``last[slot]``, which every emitting row
    updates after the step, and the sampled ids come back through a pinned
    buffer and an event per step. The host waits on step k (GIL released, so
    the HTTP thread writes meanwhile) only after step k+1 is queued behind it.
    Each step is one hipGraph replay: input copy from pinned staging, decode
    token gather, the fused step, (the sampler, the logprobs kernel,)
    last-token scatter, ids (and logprobs) back to pinned memory.

    ``model`` injects a model object (tests use a CPU stand-in with the same
    ``decode_step`` / ``cfg`` / ``scratch_slot`` / ``device`` surface). One
    with ``TinyLlama.step_rows`` on a HIP device runs captured; any other runs
    the same step eagerly through ``decode_step``, without the sampler.

    ``prefix_cache`` (off by default: admission, planning and the slot order
    are then exactly as described above) reuses K/V rows across requests. Per
    slot the engine keeps the token ids whose rows at positions 0..n-1 are valid
    once the work already queued on the stream has run (``_resident``): a row
    counts from the moment its step is launched, a token once it is a prompt id
    or a drained output, and the last generated token is never fed back, so it
    is never resident. A slot keeps its residency after its request finishes,
    is cancelled or stops, until a new request takes the slot. A new request
    is matched against every slot's residency (longest common prefix, capped at
    its length - 1 since the last prompt token must still run to sample, and
    ignored below ``prefix_min``); the longest match wins, ties go to a free
    slot. If that slot is free the request is admitted into it at position m
    (in place, nothing moves); if it is busy the request goes to the
    least-recently-freed free slot (never-used slots first) and the rows are
    copied there on the device (``model.kv_copy``: kv_copy.hip, one launch per
    up to 8 jobs, on the engine's stream between two graph replays, never
    captured). A request takes what is resident at that moment; it never waits
    for another request's prefill. The scratch slot never takes part.
    ``Request.cached_tokens``, ``prefix_hits``, ``cached_tokens`` and
    ``kv_copies`` (jobs) count the reuse; ``prefill_tokens`` still counts only
    rows that ran.

    Embedding requests (``Request(embed="mean" | "last")``) prefill and never
    sample: their rows emit nothing, take no LM-head rows and never touch
    ``last``, and the slot is freed in the step that runs the last prompt row.
    After every fused step the decoder's ``resid`` buffer holds the final
    residual of all rows of the step, so right after the replay of a step with
    embed rows, before anything else is queued on the stream, the engine
    launches ``model.embed_pool`` (embed_pool.hip; never captured, one launch
    per up to 16 jobs, one job per slot: a slot's rows are contiguous and in
    position order, since non-emitting rows keep their order in the sort). A
    sequence that spans several steps carries its fp32 sum in the model's
    ``acc`` row of its slot; the sequences that finish are normalised into the
    step buffer's ``d_emb`` and come back through one copy into its pinned
    ``h_emb``, which ``_drain`` hands over after the step's event. With the
    prefix cache on, an embed request takes no cached prefix (mean pooling needs
    every row); its own rows become resident like any other request's. Steps
    without embed rows launch exactly what they launched before.

    ``penalties`` (off by default: the engine then allocates, captures, stages
    and replays exactly what is described above) serves ``Request(penalties=)``.
    The engine keeps, per cache slot and vocabulary id, how often the id was
    generated and whether it occurs in the prompt (``_pen_state``, int32
    [max_batch + 1, V]; the scratch slot's row serves capture and padding) and
    the slot's logit_bias list, and captures a fourth ``post`` per (R, par): 3
    runs ``ops.penalize_`` (penalty.hip) from the raw logits into a ``work``
    buffer and replaces the greedy ids by the argmax of that buffer, then the
    sampler on ``work``, then the logprobs kernel on the RAW logits (so
    log-probabilities stay the model's own). A step replays post 3 when an
    emitting row's request has penalties, otherwise the graph it replayed
    before; rows of other requests in a post-3 step are off (``work`` is a copy
    of their logits, their ids stand). The count of the token a step samples
    exists only on the device when the next step is queued, so the kernel
    counts a decode row's input token itself, one step late and in time.
    Admission of such a request queues ``ops.penalty_reset_`` for its slot
    ahead of its first step (``_pen_reset``), whether its prompt's head runs,
    is reused in place or is copied: the prompt bits come from the prompt ids.

    ``guided`` (off by default, like ``penalties``) serves ``Request(guide=)``:
    guided decoding, see docs/GUIDED.md. The engine keeps one device arena of
    ``guided_states`` token-table rows (int16 [guided_states, V]), per cache
    slot the arena row its request's table starts at (``_gd_base``, -1 = not
    guided) and the automaton's state (``_gd_cur``), and captures one more
    ``post`` per (R, par): 4 runs ``ops.penalize_`` (an engine with penalties),
    then ``ops.guide_`` (guide.hip), which advances the slot's state by the
    row's input token, masks what the state does not allow to -inf in ``work``
    and replaces the greedy id by the argmax of the masked row, then the sampler
    on ``work`` and the logprobs kernel on the RAW logits. A step replays post 4
    when an emitting row's request is guided; rows of other requests are off
    there. Tables are shared between requests with the same pattern, stay
    resident after their last request and are evicted least recently used when
    room is needed; a request whose table does not fit while others are in use
    waits at the head of the admission queue. Admission queues
    ``ops.guide_reset_`` for the slot ahead of the request's first step
    (``_gd_bind``), and also when a request without a guide takes a slot whose
    last request had one.
    """

    def __init__(self, device="cuda:0", config="tiny", max_batch=8, seed=0, use_graph=True, rows=64, model=None,
                 small_rows=16, prefix_cache=False, prefix_min=16, penalties=False, kv_dtype="bf16",
                 guided=False, guided_states=1024):
        if model is None:
            from p2p_llm_tunnel_amd.models.tiny_llm import TinyLlama
            model = TinyLlama(config, device=device, max_batch=max_batch, seed=seed, fused=True, kv_dtype=kv_dtype)
        elif kv_dtype != "bf16" and getattr(model, "kv_dtype", "bf16") != kv_dtype:
            raise ValueError(f"kv_dtype={kv_dtype!r}, but the injected model was built with "
                             f"{getattr(model, 'kv_dtype', 'bf16')!r} caches")
        if prefix_cache and not callable(getattr(model, "kv_copy", None)):
            raise ValueError("prefix_cache needs a model with kv_copy(jobs) (slot-to-slot K/V row copy)")
        # hipGraphs need a model with the capturable step on a HIP device (a
        # loaded checkpoint qualifies; CPU stand-ins in tests run eagerly).
        use_graph = use_graph and model.device.type == "cuda" and hasattr(model, "step_rows")
        max_batch = getattr(model, "max_batch", max_batch)
        if not (1 <= max_batch <= rows and 1 <= small_rows <= rows):
            raise ValueError("need 1 <= max_batch <= rows and small_rows <= rows")
        self.model = model
        self.device = self.model.device
        self.rows = rows
        self.small_rows = small_rows
        self.use_graph = use_graph
        cuda = self.device.type == "cuda"
        self._k = 0
        self._d_last = torch.zeros(max_batch + 1, dtype=torch.int64, device=self.device)
        # Two row counts under graphs: steps of up to 16 rows replay the 16-row
        # graphs, larger ones (prefill-heavy, or more than 16 generating slots)
        # the 64-row graphs (4 MFMA row tiles), whose LM head covers only the
        # leading rows that sample (at most one per slot: max_batch rows).
        sizes = [small_rows] + ([rows] if rows > small_rows else []) if use_graph else [rows]
        lp_dev = self.device if use_graph else None
        if penalties and not use_graph:
            raise ValueError("penalties need the graph-captured HIP step; this engine runs eagerly")
        # An FP8 cache is read and written by the fused HIP step alone: refused on the eager engine, like sampling.
        if getattr(model, "kv_dtype", "bf16") != "bf16" and not use_graph:
            raise ValueError("an fp8 KV cache needs the graph-captured HIP step; this engine runs eagerly")
        if guided and not use_graph:
            raise ValueError("guided decoding needs the graph-captured HIP step; this engine runs eagerly")
        self.penalties = bool(penalties)
        self.guided = bool(guided)
        self._held = None  # a guided request that waits for room in the arena (the head of the admission queue)
        in_rows = _PEN.stop if self.penalties else _IN_ROWS
        self._bufs = {R: [_StepBuf(R, cuda, lp_dev, in_rows), _StepBuf(R, cuda, lp_dev, in_rows)] for R in sizes}
        self._d_in = {R: torch.zeros((in_rows, R), dtype=torch.int64, device=self.device) for R in sizes}
        if self.penalties:
            self._pen_alloc(max_batch, {R: (R if R == small_rows else max_batch) for R in sizes})
        if self.guided:
            self._gd_alloc(max_batch, {R: (R if R == small_rows else max_batch) for R in sizes}, guided_states)
        # Each graph holds the whole step (_step_body), one per staging buffer
        # of the pair, so a step is one replay. What follows the fused step is
        # the graph's ``post``: 0 nothing (all-greedy steps), 1 the sampler
        # (some row samples), 2 the sampler, then the logprobs kernel and its
        # two copies back (some emitting row's request has logprobs set); with
        # ``penalties`` also 3: penalize_, the sampler on its output, logprobs_;
        # with ``guided`` also 4: (penalize_,) guide_, the sampler on its
        # output, logprobs_.
        self._graphs = {(R, par, post): self._capture(self._bufs[R][par], 0 if R == small_rows else max_batch, post)
                        for R in sizes if use_graph for par in (0, 1)
                        for post in (0, 1, 2) + ((3,) if self.penalties else ()) + ((4,) if self.guided else ())}
        self.max_batch = max_batch
        self.pending: queue.Queue = queue.Queue()
        self.slots: list[dict | None] = [None] * max_batch
        self.deliver = None  # callable(list[(Request, int | None)]) for batched requests
        self._wake = threading.Event()
        self._stop = threading.Event()
        self.steps = 0
        self.tokens_out = 0
        self.prefill_tokens = 0
        self.prefix_cache = bool(prefix_cache)
        self.prefix_min = max(1, int(prefix_min))
        self.prefix_hits = 0  # requests admitted with cached rows
        self.cached_tokens = 0  # prompt rows not run, over all requests
        self.kv_copies = 0  # slot-to-slot copy jobs issued
        self.can_embed = callable(getattr(model, "embed_pool", None))
        self.embeddings = 0  # embedding requests finished
        self._pools = []  # _plan -> _launch: the step's (slot, first row, rows, first piece, req when it finishes)
        # Prefix cache: per slot the state of the request that last took it (its
        # residency; kept after the slot is freed), whether the slot was busy at
        # the last admission pass, and the pass-ordered tick at which it was
        # seen free (least recently freed = smallest).
        self._kv: list[dict | None] = [None] * max_batch
        self._was_busy = [False] * max_batch
        self._freed = [0] * max_batch
        self._tick = 0
        self.thread = threading.Thread(target=self._loop, daemon=True, name="engine")
        self.thread.start()

    def submit(self, req: Request) -> Request:
        if req.logprobs is not None and not self.use_graph:
            raise ValueError("logprobs need the graph-captured HIP step; this engine runs eagerly")
        if req.embed is not None and not self.can_embed:
            raise ValueError("embeddings need a model with embed_pool(jobs, out) (pooling of the final hidden state)")
        if req.penalties is not None and not self.penalties:
            raise ValueError("penalties and logit_bias need an engine built with penalties=True (--penalties) on the "
                             "graph-captured HIP step")
        if req.penalties is not None and any(t >= self.model.cfg.vocab for t in req.penalties.logit_bias):
            raise ValueError(f"logit_bias ids must be in [0, {self.model.cfg.vocab})")
        if req.guide is not None:
            if not self.guided:
                raise ValueError("a guide needs an engine built with guided=True (--guided) on the graph-captured "
                                 "HIP step")
            if req.guide.vocab != self.model.cfg.vocab:
                raise ValueError(f"the guide was compiled for a vocabulary of {req.guide.vocab}, the model has "
                                 f"{self.model.cfg.vocab}")
            if req.guide.n_states > self._gd_arena.shape[0]:
                raise ValueError(f"the guide has {req.guide.n_states} states, the arena holds "
                                 f"{self._gd_arena.shape[0]} (--guided-states)")
        self.pending.put(req)
        self._wake.set()
        return req

    def stop(self):
        self._stop.set()
        self._wake.set()
        self.thread.join(timeout=10)

    def _pen_alloc(self, max_batch: int, sample_rows: dict):
        """Device state of ``penalties`` and the stagings of ``_pen_reset``."""
        from p2p_llm_tunnel_amd.ops import MAX_LOGIT_BIAS
        cfg, dev = self.model.cfg, self.device
        self._pen_state = torch.zeros((max_batch + 1, cfg.vocab), dtype=torch.int32, device=dev)
        self._pen_bias_n = torch.zeros(max_batch + 1, dtype=torch.int32, device=dev)
        self._pen_bias_ids = torch.zeros((max_batch + 1, MAX_LOGIT_BIAS), dtype=torch.int32, device=dev)
        self._pen_bias_val = torch.zeros((max_batch + 1, MAX_LOGIT_BIAS), dtype=torch.float32, device=dev)
        self._work = {R: torch.zeros((n, cfg.vocab), dtype=torch.bfloat16, device=dev) for R, n in sample_rows.items()}
        # A reset's input: the prompt ids, then [2, k] bias ids and value bits,
        # written into pinned memory and copied to ONE device twin (the copy and
        # the kernel that reads the twin are ordered on the stream, so one is
        # enough). The pinned side must not be rewritten while a queued copy may
        # still read it, and a slot can be taken again before its previous
        # request's only step has drained (one-chunk prompt, max_new = 1: freed
        # at plan time). Two alternating stagings per slot, no event: a slot is
        # freed only by a pass of ``_plan`` that ran rows of it or that follows
        # such a pass, so between two admissions into one slot a step is launched
        # behind the first one's copy, and ``_loop`` has drained every step
        # launched two passes back (the step's event covers the copy queued ahead
        # of it). The third admission is at least two passes after the first:
        # the staging it rewrites is no longer read.
        n = cfg.max_seq + 2 * MAX_LOGIT_BIAS
        self._pen_stage = [[torch.zeros(n, dtype=torch.int32, pin_memory=True) for _ in (0, 1)]
                           for _ in range(max_batch)]
        self._pen_turn = [0] * max_batch
        self._pen_dev = torch.zeros(n, dtype=torch.int32, device=dev)

    def _pen_reset(self, slot: int, req: Request, ids: list):
        """Queue ``ops.penalty_reset_`` for a request with penalties admitted
        into ``slot``: ``ids`` is its whole prompt as admitted, cached rows
        included."""
        if req.penalties is None:
            return
        import numpy as np
        from p2p_llm_tunnel_amd import ops
        V = self.model.cfg.vocab
        h = self._pen_stage[slot][self._pen_turn[slot]]
        self._pen_turn[slot] ^= 1
        hn = h.numpy()
        n = len(ids)
        hn[:n] = np.asarray(ids, dtype=np.int64) % V
        bias = [(t, v) for t, v in req.penalties.logit_bias.items() if v != 0.0]  # submit checked the ids
        k = len(bias)
        if k:
            hn[n:n + k] = [t for t, _ in bias]
            hn[n + k:n + 2 * k] = np.asarray([v for _, v in bias], dtype=np.float32).view(np.int32)
        d = self._pen_dev[:n + 2 * k]
        d.copy_(h[:n + 2 * k], non_blocking=True)
        ops.penalty_reset_(self._pen_state, slot, d[:n], self._pen_bias_n, self._pen_bias_ids, self._pen_bias_val,
                           d[n:].view(2, k) if k else None)

    _GD_STAGE_BYTES = 4 << 20  # pinned staging of a table upload, two of them

    def _gd_alloc(self, max_batch: int, sample_rows: dict, states: int):
        """Device state of ``guided`` and the staging of table uploads."""
        from p2p_llm_tunnel_amd.models.guided import MAX_STATES
        cfg, dev = self.model.cfg, self.device
        if isinstance(states, bool) or not isinstance(states, int) or not 1 <= states <= MAX_STATES:
            raise ValueError(f"guided_states must be an integer in 1..{MAX_STATES}, got {states!r}")
        self._gd_arena = torch.full((states, cfg.vocab), -1, dtype=torch.int16, device=dev)
        self._gd_base = torch.full((max_batch + 1,), -1, dtype=torch.int32, device=dev)
        self._gd_cur = torch.zeros(max_batch + 1, dtype=torch.int32, device=dev)
        if not hasattr(self, "_work"):  # an engine with penalties masks their output in place
            self._work = {R: torch.zeros((n, cfg.vocab), dtype=torch.bfloat16, device=dev)
                          for R, n in sample_rows.items()}
        # Uploads go through pinned memory in pieces of whole table rows. The
        # pinned side must not be rewritten while a queued copy may still read
        # it. Unlike a penalty reset, an upload is rare (only a pattern that is
        # not resident) and large, so nothing is derived from the order of the
        # loop's passes here: each of the two stagings has an event, recorded
        # behind the copy that reads it, and the engine waits for it before it
        # writes that staging again. The wait is for copies queued behind at
        # most the two steps in flight.
        per = max(1, self._GD_STAGE_BYTES // (2 * cfg.vocab))
        self._gd_stage = [torch.zeros((per, cfg.vocab), dtype=torch.int16, pin_memory=True) for _ in (0, 1)]
        self._gd_stage_ev = [None, None]
        self._gd_turn = 0
        self._gd_tables: dict = {}  # key -> [first arena row, rows, requests holding it, tick of last use]
        self._gd_slot: list = [None] * max_batch  # (key, req) of the guided request a slot holds
        self._gd_on = [False] * max_batch  # the device's base[slot] is >= 0
        self._gd_tick = 0
        self.guide_uploads = 0  # tables copied into the arena
        self.guide_shared = 0  # guided requests that found their table resident

    def _gd_release(self):
        """Give back the tables of slots whose guided request has left."""
        for i, held in enumerate(self._gd_slot):
            if held is not None and (self.slots[i] is None or self.slots[i]["req"] is not held[1]):
                self._gd_tables[held[0]][2] -= 1
                self._gd_slot[i] = None

    def _gd_room(self, n: int, held_only: bool = False):
        """First arena row of a gap of ``n`` rows between the resident tables
        (``held_only``: between those a request holds, as if every idle one
        were gone), or None."""
        at = 0
        for first, rows, held, _ in sorted(self._gd_tables.values()):
            if held_only and not held:
                continue
            if first - at >= n:
                return at
            at = first + rows
        return at if self._gd_arena.shape[0] - at >= n else None

    def _gd_reserve(self, req: Request) -> bool:
        """Make ``req``'s table resident and count the request as holding it;
        False when it does not fit beside the tables that requests hold now.
        Tables nobody holds are evicted least recently used first, and only
        when evicting them can make the room. What a new
        table overwrites was last read by steps queued ahead of the upload."""
        g = req.guide
        self._gd_tick += 1
        t = self._gd_tables.get(g.key)
        if t is not None:
            t[2] += 1
            t[3] = self._gd_tick
            self.guide_shared += 1
            return True
        at = self._gd_room(g.n_states)
        if at is None and self._gd_room(g.n_states, held_only=True) is None:
            return False  # not even without the idle tables: they stay resident for the requests that come back
        while at is None:
            idle = [k for k, v in self._gd_tables.items() if v[2] == 0]
            del self._gd_tables[min(idle, key=lambda k: self._gd_tables[k][3])]
            at = self._gd_room(g.n_states)
        per = self._gd_stage[0].shape[0]
        for r0 in range(0, g.n_states, per):
            n = min(per, g.n_states - r0)
            turn = self._gd_turn
            self._gd_turn ^= 1
            if self._gd_stage_ev[turn] is not None:
                self._gd_stage_ev[turn].synchronize()
            h = self._gd_stage[turn]
            h.numpy()[:n] = g.next[r0:r0 + n]
            self._gd_arena[at + r0:at + r0 + n].copy_(h[:n], non_blocking=True)
            ev = self._gd_stage_ev[turn] = self._gd_stage_ev[turn] or torch.cuda.Event()
            ev.record()
        self._gd_tables[g.key] = [at, g.n_states, 1, self._gd_tick]
        self.guide_uploads += 1
        return True

    def _gd_bind(self, slot: int, req: Request):
        """Queue ``ops.guide_reset_`` for a request admitted into ``slot``:
        its table's first row and state 0, or -1 when the request has no guide
        and the slot's last one had."""
        from p2p_llm_tunnel_amd import ops
        if req.guide is None:
            if self._gd_on[slot]:
                ops.guide_reset_(self._gd_base, self._gd_cur, self._gd_arena, slot, -1)
                self._gd_on[slot] = False
            return
        self._gd_slot[slot] = (req.guide.key, req)
        ops.guide_reset_(self._gd_base, self._gd_cur, self._gd_arena, slot, self._gd_tables[req.guide.key][0])
        self._gd_on[slot] = True

    def _take(self):
        """The next request to admit, or None: the queue is empty, or its head
        is a guided request whose table has no room yet (it stays the head)."""
        if self._held is not None:
            req, self._held = self._held, None
        else:
            try:
                req = self.pending.get_nowait()
            except queue.Empty:
                return None
        if req.guide is not None and not self._gd_reserve(req):
            self._held = req
            return None
        return req

    @staticmethod
    def _resident(s: dict) -> list:
        """Token ids of the rows of ``s``'s slot that are valid once the queued
        work has run: the known ids (prompt, then drained outputs) as far as rows
        were launched."""
        return s["known"][:min(s["pos"], len(s["known"]))]

    def _admit_prefix(self):
        """``_admit`` with the prefix cache on (see the class docstring)."""
        for i, s in enumerate(self.slots):
            if s is None and self._was_busy[i]:
                self._was_busy[i] = False
                self._tick += 1
                self._freed[i] = self._tick
        free = [i for i, s in enumerate(self.slots) if s is None]
        jobs = []
        max_seq, V = self.model.cfg.max_seq, self.model.cfg.vocab
        if self.guided:
            self._gd_release()
        while free:
            req = self._take()
            if req is None:
                break
            req.max_new = max(1, min(req.max_new, max_seq - 2))  # as in _admit
            if req.embed is not None:  # the prompt's head, as in _admit
                ids = [t % V for t in req.prompt[:max_seq - 1]] or [0]
            else:
                ids = [t % V for t in req.prompt[-(max_seq - req.max_new - 1):]] or [0]
            m, src = 0, None
            for i, s in enumerate(self._kv):
                if s is None or req.embed is not None:  # an embed request pools every row: it takes no prefix
                    continue
                n = min(_common_prefix(ids, self._resident(s)), len(ids) - 1)
                if n >= self.prefix_min and (n > m or (n == m and self.slots[i] is None and self.slots[src] is not None)):
                    m, src = n, i
            if src is not None and self.slots[src] is None:
                slot = src  # in place
            else:
                slot = min(free, key=lambda i: (self._kv[i] is not None, self._freed[i]))
                if src is not None:
                    jobs.append((src, slot, m))
            free.remove(slot)
            s = {"req": req, "pos": m, "ids": ids, "gen": 0, "known": list(ids), "embed": req.embed}
            self.slots[slot] = self._kv[slot] = req.kv = s
            self._was_busy[slot] = True
            req.cached_tokens = m
            if self.penalties:
                self._pen_reset(slot, req, ids)
            if self.guided:
                self._gd_bind(slot, req)
            if m:
                self.prefix_hits += 1
                self.cached_tokens += m
        # One launch per up to MAX_KV_COPY_JOBS jobs, in admission order; a job
        # that reads a slot an earlier job of the launch writes (or the reverse)
        # starts the next launch, so within one no slot is source and destination.
        launch: list = []
        for job in jobs + [None]:
            if launch and (job is None or len(launch) >= _MAX_COPY_JOBS or
                           any(job[0] == d or job[1] in (a, d) for a, d, _ in launch)):
                self.model.kv_copy(launch)
                self.kv_copies += len(launch)
                launch = []
            if job is not None:
                launch.append(job)

    def _admit(self):
        if self.prefix_cache:
            return self._admit_prefix()
        if self.guided:
            self._gd_release()
        for i in range(self.max_batch):
            if self.slots[i] is None:
                req = self._take()
                if req is None:
                    return
                # max_new is clamped so prompt + generated rows fit max_seq; a
                # prompt too long for the rest keeps its end (for a chat, the
                # latest turns and the generation prompt).
                max_seq = self.model.cfg.max_seq
                req.max_new = max(1, min(req.max_new, max_seq - 2))
                ids = req.prompt[-(max_seq - req.max_new - 1):] or [0]
                if req.embed is not None:  # nothing is generated: the prompt's head, up to the cache's rows
                    ids = req.prompt[:max_seq - 1] or [0]
                self.slots[i] = {"req": req, "pos": 0, "ids": ids, "gen": 0, "embed": req.embed}
                if self.penalties:
                    self._pen_reset(i, req, ids)
                if self.guided:
                    self._gd_bind(i, req)

    def _plan(self, batch: list):
        """Rows of the next step (``_Row``), with the host-side state advanced
        past them (it does not depend on the tokens) and the emitting rows'
        (row, req, finished, token index) list."""
        V = self.model.cfg.vocab
        rows, emits = [], []
        for i, s in enumerate(self.slots):  # decode rows first: one token each
            if s is None or s["pos"] < len(s["ids"]):
                continue
            if s["req"].cancelled:
                self._emit(s["req"], None, batch)
                self.slots[i] = None
                continue
            rows.append(_Row(i, 0, s["pos"], 1, True))
        for i, s in enumerate(self.slots):  # then prompt chunks
            if s is None or s["pos"] >= len(s["ids"]):
                continue
            if s["embed"] and s["req"].cancelled:  # it never reaches a decode row: dropped here
                self._emit(s["req"], None, batch)
                self.slots[i] = None
                continue
            take = min(self.rows - len(rows), len(s["ids"]) - s["pos"])
            for p in range(s["pos"], s["pos"] + take):
                rows.append(_Row(i, s["ids"][p] % V, p, 0, p == len(s["ids"]) - 1 and not s["embed"]))
            if len(rows) >= self.rows:
                break
        # Rows that sample go first: the 64-row graph's LM head covers only the
        # first max_batch rows (each slot samples at most once per step).
        rows.sort(key=lambda r: not r.emit)
        # Embed slots: all their rows are non-emitting, so after the (stable)
        # sort they are still contiguous and in position order.
        self._pools = pools = []
        for r, row in enumerate(rows):
            s = self.slots[row.slot]
            if s["embed"]:
                if pools and pools[-1][0] == row.slot:
                    pools[-1][2] += 1
                else:
                    pools.append([row.slot, r, 1, row.pos == 0, None])
        # Advance every row's slot first: after the sort a slot's sampling row
        # can precede its other prompt rows, so slots are only freed once all
        # rows of the step are accounted for.
        max_seq = self.model.cfg.max_seq
        for row in rows:
            self.slots[row.slot]["pos"] += 1
            if not row.emit:
                self.prefill_tokens += 1
        done = []
        for r, row in enumerate(rows):
            if not row.emit:
                continue
            i = row.slot
            s = self.slots[i]
            s["gen"] += 1
            fin = s["gen"] >= s["req"].max_new or s["pos"] >= max_seq - 1
            emits.append((r, s["req"], fin, s["gen"] - 1))  # the token's index: the sampler's counter
            if fin:
                done.append(i)
        for pool in pools:  # an embed request is done with its last prompt row
            s = self.slots[pool[0]]
            if s["pos"] >= len(s["ids"]):
                pool[4] = s["req"]
                done.append(pool[0])
        for i in done:
            self.slots[i] = None
        return rows, emits

    def _step_body(self, b: _StepBuf, n: int, run, sample_rows: int = 0, logprobs: bool = False,
                   penalize: bool = False, guide: bool = False):
        """One step on the first ``n`` rows of ``b``: staging -> device, decode
        rows' tokens gathered from ``last``, the model through ``run(tokens, pos,
        slots) -> (ids, logits)``, (the sampler over the leading ``sample_rows``
        rows' logits; with ``logprobs``, the logprobs kernel over the same rows
        and the sampled ids, and its outputs -> pinned staging,) last-token
        scatter, ids -> pinned staging. With ``penalize`` the sampler reads what
        ``ops.penalize_`` made of those rows' logits; the logprobs kernel still
        reads the raw ones. With ``guide`` ``ops.guide_`` masks those rows (the
        penalised ones in place) ahead of the sampler."""
        din = self._d_in[b.rows]
        din.copy_(b.h_in, non_blocking=True)
        d = din[:, :n]
        tok = torch.where(d[_DEC] != 0, self._d_last[d[_SLOT]], d[_TOK])
        ids, logits = run(tok, d[_POS].to(torch.int32), d[_SLOT].to(torch.int32))
        if sample_rows:
            from p2p_llm_tunnel_amd import ops
            drawn = logits[:sample_rows]
            if penalize:
                drawn = ops.penalize_(drawn, self._work[b.rows], ids[:sample_rows], tok[:sample_rows], din[_DEC],
                                      din[_SLOT], din[_PEN], self._pen_state, self._pen_bias_n, self._pen_bias_ids,
                                      self._pen_bias_val)
            if guide:
                drawn = ops.guide_(drawn, self._work[b.rows], ids[:sample_rows], tok[:sample_rows], din[_DEC],
                                   din[_SLOT], self._gd_base, self._gd_cur, self._gd_arena)
            ops.sample_(drawn, ids[:sample_rows], din[_SMP])
            if logprobs:
                ops.logprobs_(logits[:sample_rows], ids[:sample_rows], din[_LP], b.d_lp[:sample_rows],
                              b.d_lp_ids[:sample_rows])
                b.h_lp.copy_(b.d_lp, non_blocking=True)
                b.h_lp_ids.copy_(b.d_lp_ids, non_blocking=True)
        self._d_last.index_copy_(0, d[_REC], ids)
        b.h_out[:n].copy_(ids, non_blocking=True)

    def _capture(self, b: _StepBuf, emit_rows: int, post: int):
        """The step on all of ``b``'s rows through ``step_rows``, as a hipGraph;
        ``post``: what follows the fused step (see ``_graphs``)."""
        from p2p_llm_tunnel_amd.models.tiny_llm import capture
        b.np[:] = 0
        b.np[_SLOT, :] = b.np[_REC, :] = self.model.scratch_slot  # warm-up and capture touch the scratch slot only
        run = functools.partial(self.model.step_rows, emit_rows=emit_rows)
        sample_rows = (emit_rows or b.rows) if post else 0
        graph, _ = capture(lambda: self._step_body(b, b.rows, run, sample_rows, post >= 2,
                                                   post == 3 or (post == 4 and self.penalties), post == 4),
                           self.device)
        torch.cuda.synchronize(self.device)
        return graph

    def _launch(self, rows, emits) -> _StepBuf:
        n, scratch = len(rows), self.model.scratch_slot
        R = self.small_rows if self.use_graph and n <= self.small_rows else self.rows
        par = self._k % 2
        self._k += 1
        b = self._bufs[R][par]
        h = b.np
        h[_TOK, :n] = [r.token for r in rows]
        h[_POS, :n] = [r.pos for r in rows]
        h[_SLOT, :n] = [r.slot for r in rows]
        h[_DEC, :n] = [r.decode for r in rows]
        h[_REC, :n] = [r.slot if r.emit else scratch for r in rows]
        h[_SMP, :] = 0  # greedy unless an emitting row samples
        h[_LP, :] = 0  # no logprobs unless an emitting row's request asks
        post = 0
        for r, req, _, ctr in emits:
            if not req.sampling.greedy:
                h[_SMP, r] = req.sampling.column(ctr)
                post = max(post, 1)
            if req.logprobs is not None:
                h[_LP, r] = 1 + req.logprobs
                post = 2
        if self.penalties:
            h[_PEN, :] = 0  # every row off unless its request has penalties
            for r, req, _, _ in emits:
                if req.penalties is not None:
                    h[_PEN, r] = req.penalties.column()
                    post = 3
        if self.guided and any(req.guide is not None for _, req, _, _ in emits):
            post = 4
        if n < R:  # padding rows: scratch slot, nothing recorded
            h[_TOK, n:R] = h[_POS, n:R] = h[_DEC, n:R] = 0
            h[_SLOT, n:R] = h[_REC, n:R] = scratch
        b.n, b.emits = n, emits
        if self.use_graph:
            self._graphs[(R, par, post)].replay()
        else:  # injected model (tests): the same step, eagerly, on its n rows; no sampler
            rng = (min(r.pos for r in rows), max(r.pos for r in rows))
            self._step_body(b, n, lambda tok, pos, slots: (
                self.model.decode_step(tok, pos, rng, slots=slots).to(torch.int64), None))
        b.embeds = []
        if self._pools:
            self._pool(b, self._pools)
        if b.ev is not None:
            b.ev.record()
        self.steps += 1
        return b

    def _pool(self, b: _StepBuf, pools):
        """Pool the embed rows of the step just queued (see the class docstring)."""
        if b.h_emb is None:
            shape = (self.max_batch, self.model.cfg.dim)
            b.h_emb = torch.zeros(shape, dtype=torch.float32, pin_memory=self.device.type == "cuda")
            b.d_emb = torch.zeros(shape, dtype=torch.float32, device=self.device)
        jobs = []
        for slot, row0, n, first, req in pools:
            if req is None:  # more rows to come: "mean" carries its sum in acc[slot], "last" waits for the last row
                if self.slots[slot]["embed"] == "mean":
                    jobs.append((slot, row0, n, 1 if first else 0, -1))
                continue
            if req.embed == "last":
                row0, n, first = row0 + n - 1, 1, True
            jobs.append((slot, row0, n, (1 if first else 0) | 2, len(b.embeds)))
            b.embeds.append((req, len(b.embeds)))
        for k in range(0, len(jobs), _MAX_EMBED_JOBS):
            self.model.embed_pool([(row0, n, slot, flags, out_row)
                                   for slot, row0, n, flags, out_row in jobs[k:k + _MAX_EMBED_JOBS]], b.d_emb)
        if b.embeds:
            b.h_emb[:len(b.embeds)].copy_(b.d_emb[:len(b.embeds)], non_blocking=True)

    def _drain(self, b: _StepBuf, batch: list):
        if b.ev is not None:
            b.ev.synchronize()  # GIL released: the HTTP thread writes meanwhile
        out = b.h_out[: b.n].tolist() if b.emits else []
        for r, req, fin, _ in b.emits:
            if self.prefix_cache:  # drained: the id is known (a cancelled request's too: its row may have been fed)
                req.kv["known"].append(out[r])
            if req.cancelled:
                continue
            if req.logprobs is not None:  # the record first: the token's consumer finds it there
                lps = b.h_lp[r, :1 + req.logprobs].tolist()
                req.lp.append((lps[0], list(zip(b.h_lp_ids[r, :req.logprobs].tolist(), lps[1:]))))
            self._emit(req, out[r], batch)
            req.generated += 1
            self.tokens_out += 1
            if fin:
                self._emit(req, None, batch)
        for req, row in b.embeds:
            req.embedding = b.h_emb[row].numpy().copy()
            self.embeddings += 1
            self._emit(req, None, batch)

    def _loop(self):
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)
        inflight: list[_StepBuf] = []
        with torch.no_grad():
            while not self._stop.is_set():
                batch = []
                self._admit()
                rows, emits = self._plan(batch)
                if rows:
                    inflight.append(self._launch(rows, emits))
                if inflight and (len(inflight) >= 2 or not rows):
                    self._drain(inflight.pop(0), batch)
                if batch:
                    self._flush(batch)
                # Hand the GIL over once per step: when the host is the slower
                # side the event wait above returns at once, and the HTTP thread
                # (accepting a burst of new connections, say) would otherwise get
                # the GIL only at the interpreter's forced-switch interval.
                time.sleep(0)
                if not rows and not inflight:
                    self._wake.wait(0.05)
                    self._wake.clear()

    def _emit(self, req: Request, tok, batch: list):
        if req.batched and self.deliver is not None:
            batch.append((req, tok))
        else:
            req.out.put(tok)

    def _flush(self, batch: list):
        if self.deliver is not None:
            self.deliver(batch)


def chat_template_kwargs(body: dict) -> dict | None:
    """The request's optional ``chat_template_kwargs``: a JSON object of scalars
    handed to the chat-template render (``{"enable_thinking": false}`` for
    Qwen3's template). Anything else raises SamplingError (answered with 400)
    naming the field."""
    kw = body.get("chat_template_kwargs")
    if kw is None:
        return None
    if not isinstance(kw, dict):
        raise SamplingError(f"chat_template_kwargs must be a JSON object, got {kw!r}")
    for k, v in kw.items():
        if v is not None and not isinstance(v, (bool, int, float, str)):
            raise SamplingError(f"chat_template_kwargs[{k!r}] must be a scalar (string, number, boolean or null), "
                                f"got {v!r}")
    return kw


def _prompt_ids(body: dict, tok=None, template_kwargs: dict | None = None) -> list[int]:
    msgs = body.get("messages")
    if tok is not None:
        if isinstance(msgs, list):
            msgs = [m for m in msgs if isinstance(m, dict)]
            # the keyword only when the request carries the field: any tokenizer with chat(messages) still serves
            return (tok.chat(msgs, template_kwargs=template_kwargs) if template_kwargs else tok.chat(msgs)) or [0]
        return tok.encode(str(body.get("prompt", ""))) or [0]
    if "messages" in body:
        text = "\n".join(str(m.get("content", "")) for m in body.get("messages", []) if isinstance(m, dict))
    else:
        text = str(body.get("prompt", ""))
    return list(text.encode("utf-8"))[:512] or [1]


def _piece(text: str) -> bytes:
    """A text piece as the inside of a JSON string."""
    return json.dumps(text, ensure_ascii=False)[1:-1].encode()


def _chunk(data: bytes) -> bytes:
    return b"%x\r\n%s\r\n" % (len(data), data)


class _Stream:
    """Per-request output state on the I/O thread: the writer and the byte
    template around each token piece (token ids render as " t<id>": no JSON
    escaping needed)."""
    __slots__ = ("writer", "stream", "kind", "rid", "pre", "post", "toks", "done", "detok", "reason", "stop",
                 "stop_hit", "lp_toks", "lp_off")

    def __init__(self, writer, stream, kind, rid, model, detok=None, stop=None, logprobs=False):
        self.lp_toks = [] if logprobs else None  # with logprobs: the delivered ids; Request.lp[k] belongs to the k-th
        self.lp_off = 0  # legacy completions, streamed: text_offset of the next token
        self.writer = writer
        self.stream = stream
        self.kind = kind  # "chat" | "text" | "ollama"
        self.rid = rid
        self.toks = []  # non-streamed: rendered pieces (bytes, JSON-escaped when detokenised)
        self.detok = detok  # checkpoint tokenizer: incremental text of this request
        self.reason = "length"
        self.stop = stop  # StopMatcher, or None without stop sequences
        self.stop_hit = False  # a stop sequence matched (its held-back text is the match, never emitted)
        self.done = asyncio.get_running_loop().create_future()
        m = json.dumps(model)
        if kind == "chat":
            self.pre = ('data: {"id": "%s", "object": "chat.completion.chunk", "model": %s, "choices": '
                        '[{"index": 0, "delta": {"content": "' % (rid, m)).encode()
            self.post = b'"}, "finish_reason": null}]}\n\n'
        elif kind == "text":
            self.pre = ('data: {"id": "%s", "object": "text_completion", "model": %s, "choices": '
                        '[{"index": 0, "text": "' % (rid, m)).encode()
            self.post = b'", "finish_reason": null}]}\n\n'
        else:
            self.pre = ('{"model": %s, "response": "' % m).encode()
            self.post = b'", "done": false}\n'


class _EmbedBatch:
    """The items of one embeddings HTTP request on the I/O thread: one engine
    request each; ``done`` resolves when the last has arrived (True) or the
    client has gone (False)."""
    __slots__ = ("writer", "reader", "reqs", "left", "done")

    def __init__(self, writer, reader, reqs):
        self.writer = writer
        self.reader = reader
        self.reqs = reqs
        self.left = len(reqs)
        self.done = asyncio.get_running_loop().create_future()

    def gone(self) -> bool:
        """The client closed the connection. Nothing is written before the last
        item has arrived, so its end of stream is the only sign there is."""
        return self.writer.transport.is_closing() or (self.reader is not None and self.reader.at_eof())


_MAX_EMBED_INPUTS = 256  # items per embeddings request
_EMBED_PATHS = ("/v1/embeddings", "/embeddings", "/api/embed", "/api/embeddings")


class FrontEnd:
    """HTTP/1.1 server on one asyncio thread (see the module docstring)."""

    def __init__(self, engine: Engine, host: str, port: int, model_name: str, tokenizer=None,
                 default_temperature: float = 0.0, embed_pooling: str = "mean"):
        if embed_pooling not in ("mean", "last"):
            raise ValueError(f'embed_pooling must be "mean" or "last", got {embed_pooling!r}')
        self.embed_pooling = embed_pooling
        self.engine = engine
        self.model_name = model_name
        # Temperature of requests that give none. 0 (greedy) by default — the
        # OpenAI API's nominal default is 1 — so unparameterised completions
        # stay deterministic; --default-temperature sets it.
        self.default_temperature = default_temperature
        self.tok = tokenizer
        self.eos = tokenizer.eos_ids if tokenizer is not None else frozenset()
        # Compiled guides, most recently used last (--guided): compilation runs in an executor, off the I/O thread.
        self._guides: dict = {}
        self._guides_lock = threading.Lock()
        self._guide_pool = None  # one worker: compilations run one at a time (they hold the GIL the engine needs)
        self.loop = asyncio.new_event_loop()
        self._ready = threading.Event()
        self._err = None
        self.thread = threading.Thread(target=self._run, args=(host, port), daemon=True, name="http")
        self.thread.start()
        self._ready.wait(30)
        if self._err:
            raise self._err
        engine.deliver = lambda batch: self.loop.call_soon_threadsafe(self._on_batch, batch)

    # ---------------------------------------------------------------- lifecycle
    def _run(self, host, port):
        asyncio.set_event_loop(self.loop)
        try:
            self.server = self.loop.run_until_complete(
                asyncio.start_server(self._conn, host, port, backlog=1024, limit=1 << 20))
            self.server_address = self.server.sockets[0].getsockname()[:2]
        except Exception as e:  # noqa: BLE001 - re-raised by the constructor
            self._err = e
            self._ready.set()
            return
        self._ready.set()
        self.loop.run_forever()
        # Stopped: cancel the keep-alive connection tasks still parked in a
        # read and let them unwind, so none is destroyed while pending.
        pending = [t for t in asyncio.all_tasks(self.loop) if not t.done()]
        for t in pending:
            t.cancel()
        if pending:
            self.loop.run_until_complete(asyncio.gather(*pending, return_exceptions=True))

    def shutdown(self):
        def stop():
            self.server.close()
            self.loop.stop()
        self.loop.call_soon_threadsafe(stop)
        self.thread.join(timeout=10)
        if self._guide_pool is not None:
            self._guide_pool.shutdown(wait=False, cancel_futures=True)

    # ---------------------------------------------------------------- tokens
    def _on_batch(self, batch):
        for req, tok in batch:
            st = req.state
            if st is None or st.done.done():
                continue
            if req.embed is not None:  # st is the _EmbedBatch of its HTTP request; tok is the terminating None
                if st.gone():  # client went away: drop the items still queued or running
                    for r in st.reqs:
                        r.cancelled = True
                    st.done.set_result(False)
                    continue
                st.left -= 1
                if st.left == 0:
                    st.done.set_result(True)
                continue
            if st.writer.transport.is_closing():  # client went away: free the slot
                req.cancelled = True
                st.done.set_result(False)
                continue
            if tok is None:
                self._finish(req, st)
                continue
            if tok in self.eos:  # stop: the engine frees the slot on its next step
                req.cancelled = True
                st.reason = "stop"
                self._finish(req, st)
                continue
            if st.lp_toks is not None:
                self._on_token_logprobs(req, st, tok)
                continue
            if st.stop is not None:
                piece = st.detok.push(tok) if st.detok is not None else " t%d" % tok
                text, stopped = st.stop.push(piece)
                if text:
                    self._emit_piece(st, _piece(text))
                if stopped:  # the engine frees the slot on its next step
                    req.cancelled = True
                    st.reason = "stop"
                    st.stop_hit = True
                    self._finish(req, st)
                continue
            if st.detok is not None:
                piece = st.detok.push(tok)
                if not piece:
                    continue
                body = _piece(piece)
            else:
                body = b" t%d" % tok
            self._emit_piece(st, body)

    def _token_text(self, tid: int) -> str:
        return self.tok.decode([tid]) if self.tok is not None else " t%d" % tid

    def _on_token_logprobs(self, req, st, tok):
        """A token of a request with logprobs: its entry goes out with it. A
        streamed response gets exactly one chunk per token, rendered here
        (``content`` is "" while the detokeniser or the stop matcher holds the
        text back); the tokens of a matched stop sequence keep their entries."""
        record = req.lp[len(st.lp_toks)]  # appended by the engine before it delivered the token
        st.lp_toks.append(tok)
        piece = st.detok.push(tok) if st.detok is not None else " t%d" % tok
        stopped = False
        if st.stop is not None:
            piece, stopped = st.stop.push(piece)
        if st.stream:
            if st.kind == "chat":
                choice = {"index": 0, "delta": {"content": piece},
                          "logprobs": {"content": [chat_logprob_entry(tok, record, self._token_text)]},
                          "finish_reason": None}
                obj = {"id": st.rid, "object": "chat.completion.chunk", "model": self.model_name, "choices": [choice]}
            else:
                lp = completion_logprobs([tok], [record], self._token_text, st.lp_off)
                st.lp_off += len(lp["tokens"][0])
                obj = {"id": st.rid, "object": "text_completion", "model": self.model_name,
                       "choices": [{"index": 0, "text": piece, "logprobs": lp, "finish_reason": None}]}
            st.writer.write(_chunk(f"data: {json.dumps(obj, ensure_ascii=False)}\n\n".encode()))
        elif piece:
            st.toks.append(_piece(piece))
        if stopped:  # the engine frees the slot on its next step
            req.cancelled = True
            st.reason = "stop"
            st.stop_hit = True
            self._finish(req, st)

    @staticmethod
    def _emit_piece(st, body: bytes):
        if st.stream:
            st.writer.write(_chunk(st.pre + body + st.post))
        else:
            st.toks.append(body)

    def _finish(self, req, st):
        w = st.writer
        if st.stop is not None and not st.stop_hit:
            # A held-back tail that never became a stop sequence: the completion
            # ended otherwise (length, EOS — also finish_reason "stop"), so it is
            # real text.
            held = st.stop.flush()
            if held:
                self._emit_piece(st, _piece(held))
        if st.stream:
            if st.kind == "ollama":
                tail = _chunk((json.dumps({"model": self.model_name, "response": "", "done": True}) + "\n").encode())
            else:
                fin = {"index": 0, "delta": {}, "finish_reason": st.reason} if st.kind == "chat" else \
                    {"index": 0, "text": "", "finish_reason": st.reason}
                obj = {"id": st.rid, "object": "chat.completion.chunk" if st.kind == "chat" else "text_completion",
                       "choices": [fin]}
                tail = _chunk(f"data: {json.dumps(obj)}\n\n".encode()) + _chunk(b"data: [DONE]\n\n")
            w.write(tail + b"0\r\n\r\n")
        else:
            text = json.loads(b'"' + b"".join(st.toks) + b'"')
            if st.kind == "ollama":
                obj = {"model": self.model_name, "response": text, "done": True}
            elif st.kind == "chat":
                obj = {"id": st.rid, "object": "chat.completion", "model": self.model_name,
                       "choices": [{"index": 0, "message": {"role": "assistant", "content": text},
                                    "finish_reason": st.reason}],
                       "usage": {"prompt_tokens": len(req.prompt), "completion_tokens": req.generated,
                                 "total_tokens": len(req.prompt) + req.generated}}
                if self.engine.prefix_cache:  # the OpenAI field; absent with the cache off
                    obj["usage"]["prompt_tokens_details"] = {"cached_tokens": req.cached_tokens}
            else:
                obj = {"id": st.rid, "object": "text_completion", "model": self.model_name,
                       "choices": [{"index": 0, "text": text, "finish_reason": st.reason}]}
            if st.lp_toks is not None:  # (never an Ollama request)
                render = chat_logprobs if st.kind == "chat" else completion_logprobs
                obj["choices"][0]["logprobs"] = render(st.lp_toks, req.lp[:len(st.lp_toks)], self._token_text)
            w.write(self._json_response(obj))
        st.done.set_result(True)

    # ---------------------------------------------------------------- HTTP
    @staticmethod
    def _response(status: int, ctype: str, body: bytes, reason: str = "OK") -> bytes:
        return (b"HTTP/1.1 %d %s\r\nContent-Type: %s\r\nContent-Length: %d\r\n\r\n"
                % (status, reason.encode(), ctype.encode(), len(body))) + body

    def _json_response(self, obj, status=200) -> bytes:
        reason = {200: "OK", 400: "Bad Request", 404: "Not Found"}.get(status, "Error")
        return self._response(status, "application/json", json.dumps(obj).encode(), reason)

    async def _conn(self, reader: asyncio.StreamReader, writer: asyncio.StreamWriter):
        sock = writer.get_extra_info("socket")
        if sock is not None:
            try:  # one small write per token: never hold it back for an ACK
                sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
            except OSError:
                pass
        try:
            while True:
                try:
                    head = await reader.readuntil(b"\r\n\r\n")
                except (asyncio.IncompleteReadError, asyncio.LimitOverrunError, ConnectionError):
                    break
                lines = head.decode("latin-1").split("\r\n")
                parts = lines[0].split(" ")
                if len(parts) != 3:
                    writer.write(self._response(400, "text/plain", b"bad request", "Bad Request"))
                    break
                method, target, version = parts
                hdrs = {}
                for line in lines[1:]:
                    if ":" in line:
                        k, v = line.split(":", 1)
                        hdrs[k.strip().lower()] = v.strip()
                try:
                    if "chunked" in hdrs.get("transfer-encoding", "").lower():
                        body = await self._read_chunked(reader)
                    else:
                        n = int(hdrs.get("content-length", "0") or 0)
                        body = await reader.readexactly(n) if n else b""
                except (asyncio.IncompleteReadError, asyncio.LimitOverrunError, ValueError, ConnectionError):
                    break
                conn = hdrs.get("connection", "").lower()
                keep = (version == "HTTP/1.1" and conn != "close") or (version == "HTTP/1.0" and conn == "keep-alive")
                ok = await self._dispatch(method, target.split("?")[0], body, writer, reader)
                if not ok or not keep:
                    break
                await writer.drain()
        except ConnectionError:
            pass
        finally:
            try:
                writer.close()
            except RuntimeError:
                pass

    @staticmethod
    async def _read_chunked(reader) -> bytes:
        out = bytearray()
        while True:
            size = int((await reader.readuntil(b"\r\n")).split(b";")[0].strip() or b"0", 16)
            if size == 0:
                while (await reader.readuntil(b"\r\n")) != b"\r\n":  # trailers
                    pass
                return bytes(out)
            out += await reader.readexactly(size)
            await reader.readexactly(2)

    def _embed_inputs(self, path: str, body: dict) -> tuple[list[list[int]], str]:
        """Token ids of every item of an embeddings request and the response's
        encoding ("float" | "base64"); raises SamplingError (answered with 400)
        naming the offending field or item."""
        openai = path in ("/v1/embeddings", "/embeddings")
        cfg = self.engine.model.cfg
        limit = cfg.max_seq - 1
        fmt = "float"
        if openai:
            fmt = body.get("encoding_format") or "float"
            if fmt not in ("float", "base64"):
                raise SamplingError(f'encoding_format must be "float" or "base64", got {fmt!r}')
            dims = body.get("dimensions")
            if dims is not None and (isinstance(dims, bool) or dims != cfg.dim):
                raise SamplingError(f"dimensions={dims!r} is not supported: this model's embeddings have {cfg.dim}")
        key = "prompt" if path == "/api/embeddings" else "input"
        raw = body.get(key)
        is_ids = lambda v: isinstance(v, list) and bool(v) and all(type(t) is int for t in v)
        single = isinstance(raw, str) or (openai and is_ids(raw)) or path == "/api/embeddings"
        if single:
            raw = [raw]
        if not isinstance(raw, list) or not 1 <= len(raw) <= _MAX_EMBED_INPUTS:
            raise SamplingError(f"{key} must be a string or a list of 1..{_MAX_EMBED_INPUTS} items")
        truncate = True if openai else body.get("truncate", True)
        if not isinstance(truncate, bool):
            raise SamplingError(f"truncate must be a boolean, got {truncate!r}")
        items = []
        for n, item in enumerate(raw):
            name = key if single else f"{key}[{n}]"
            if isinstance(item, str):
                ids = self.tok.encode(item) if self.tok is not None else list(item.encode("utf-8"))
            elif openai and isinstance(item, list) and all(type(t) is int for t in item):
                if not all(0 <= t < cfg.vocab for t in item):
                    raise SamplingError(f"{name}: token ids must be in [0, {cfg.vocab})")
                ids = list(item)
            else:
                raise SamplingError(f"{name} must be a string" + (" or a list of token ids" if openai else ""))
            if not ids:
                raise SamplingError(f"{name} is empty")
            if len(ids) > limit:
                if openai or not truncate:
                    raise SamplingError(f"{name} has {len(ids)} tokens; this model takes at most {limit}")
                ids = ids[:limit]
            items.append(ids)
        return items, fmt

    async def _embeddings(self, path, body, writer, reader=None) -> bool:
        """POST /v1/embeddings (+ /embeddings), /api/embed and /api/embeddings:
        every item is one engine request (``Request(embed=)``), and the response
        is written when all have arrived."""
        t0 = time.perf_counter_ns()

        def refuse(msg):
            writer.write(self._json_response({"error": {"message": msg, "type": "invalid_request_error"}}, 400))
            return True
        try:
            req_body = json.loads(body or b"{}")
        except ValueError:
            return refuse("the request body is not JSON")
        if not isinstance(req_body, dict):
            return refuse("the request body must be a JSON object")
        if not self.engine.can_embed:
            return refuse("embeddings need a model with embed_pool (pooling of the final hidden state)")
        try:
            items, fmt = self._embed_inputs(path, req_body)
        except SamplingError as e:
            return refuse(str(e))
        reqs = [Request(ids, 1, batched=True, embed=self.embed_pooling) for ids in items]
        group = _EmbedBatch(writer, reader, reqs)
        for r in reqs:
            r.state = group
            self.engine.submit(r)
        if not await group.done:
            return False
        n_tok = sum(len(ids) for ids in items)
        if fmt == "base64":
            import base64
            vecs = [base64.b64encode(r.embedding.astype("<f4").tobytes()).decode() for r in reqs]
        else:
            vecs = [r.embedding.tolist() for r in reqs]
        if path == "/api/embed":
            obj = {"model": self.model_name, "embeddings": vecs, "prompt_eval_count": n_tok,
                   "total_duration": time.perf_counter_ns() - t0}
        elif path == "/api/embeddings":
            obj = {"embedding": vecs[0]}
        else:
            obj = {"object": "list", "data": [{"object": "embedding", "index": i, "embedding": v}
                                               for i, v in enumerate(vecs)],
                   "model": self.model_name, "usage": {"prompt_tokens": n_tok, "total_tokens": n_tok}}
        writer.write(self._json_response(obj))
        return True

    _GUIDE_CACHE = 32  # compiled guides kept by the front end

    def _guide(self, kind: str, pattern):
        """The compiled ``Guide`` of a request's pattern (runs in an executor
        thread); raises SamplingError (answered with 400) with the reason."""
        from p2p_llm_tunnel_amd.models.guided import compile_guide
        with self._guides_lock:
            g = self._guides.pop((kind, pattern), None)
            if g is not None:
                self._guides[(kind, pattern)] = g
                return g
        if self.tok is None:
            raise SamplingError("guided decoding needs a tokenizer: this server has none (it serves a random-init "
                                "model whose ids have no text)")
        V = self.engine.model.cfg.vocab
        try:
            tb = self.tok.token_bytes()
        except (ValueError, AttributeError) as e:
            raise SamplingError(f"guided decoding is not available with this tokenizer: {e}") from None
        if len(tb) > V:
            raise SamplingError(f"the tokenizer has {len(tb)} ids, the model's vocabulary {V}")
        tb = list(tb) + [b""] * (V - len(tb))
        states = self.engine._gd_arena.shape[0]
        g = compile_guide(kind, list(pattern) if kind == "choice" else pattern, tb,
                          [e for e in self.eos if 0 <= e < V], states)
        with self._guides_lock:
            self._guides[(kind, pattern)] = g
            while len(self._guides) > self._GUIDE_CACHE:
                self._guides.pop(next(iter(self._guides)))
        return g

    async def _dispatch(self, method, path, body, writer, reader=None) -> bool:
        name = self.model_name
        if method in ("GET", "HEAD"):
            if path in ("/v1/models", "/models"):
                resp = self._json_response({"object": "list", "data": [
                    {"id": name, "object": "model", "owned_by": "p2p_llm_tunnel_amd"}]})
            elif path == "/health":
                resp = self._response(200, "text/plain", b"ok")
            elif path == "/api/tags":
                resp = self._json_response({"models": [{"name": name, "model": name}]})
            else:
                resp = self._json_response({"error": "not found"}, 404)
            if method == "HEAD":
                resp = resp[: resp.index(b"\r\n\r\n") + 4]
            writer.write(resp)
            return True
        if method == "POST" and path in _EMBED_PATHS:
            return await self._embeddings(path, body, writer, reader)
        if method != "POST" or path not in ("/v1/chat/completions", "/chat/completions", "/v1/completions",
                                            "/api/generate"):
            writer.write(self._json_response({"error": "not found"}, 404))
            return True
        try:
            req_body = json.loads(body or b"{}")
            if not isinstance(req_body, dict):
                req_body = {}
        except ValueError:
            req_body = {}
        raw_max = req_body.get("max_tokens", req_body.get("num_predict", 16))
        try:
            max_new = int(raw_max if raw_max is not None else 16)
        except (TypeError, ValueError):
            writer.write(self._json_response({"error": f"max_tokens must be an integer, got {raw_max!r}"}, 400))
            return True
        ollama = path == "/api/generate"
        kind = "ollama" if ollama else ("chat" if "chat" in path else "text")
        try:
            # Logprobs first; sampling_params refuses both keys, so the OpenAI
            # endpoints hand it the body without them.
            logprobs = logprob_params(req_body, kind)
            if logprobs is not None and not self.engine.use_graph:
                raise SamplingError("logprobs need the graph-captured HIP step; this engine runs eagerly")
            rest = req_body if ollama else {k: v for k, v in req_body.items() if k not in _LOGPROB_KEYS}
            pen_on = getattr(self.engine, "penalties", False)
            sampling = sampling_params(rest, ollama, self.default_temperature, penalties=pen_on,
                                       vocab=self.engine.model.cfg.vocab)
            penalties = penalty_params(rest, ollama, self.engine.model.cfg.vocab) if pen_on else None
            stops = stop_sequences(req_body, ollama)
            template_kwargs = chat_template_kwargs(req_body)
            guide = None
            if getattr(self.engine, "guided", False) and not ollama:
                want = guided_params(req_body)
                if want is not None:
                    if self._guide_pool is None:
                        from concurrent.futures import ThreadPoolExecutor
                        self._guide_pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="guide")
                    guide = await asyncio.get_running_loop().run_in_executor(self._guide_pool, self._guide, *want)
            if not sampling.greedy and not self.engine.use_graph:
                # The eager step (CPU stand-ins, injected models) has no sampler:
                # refuse rather than answer a sampled request greedily.
                raise SamplingError("sampling (temperature > 0) needs the graph-captured HIP step; "
                                    "this engine runs eagerly")
        except SamplingError as e:
            writer.write(self._json_response({"error": {"message": str(e), "type": "invalid_request_error"}}, 400))
            return True
        stream = bool(req_body.get("stream", ollama))
        rid = ("chatcmpl-" if kind == "chat" else "cmpl-") + uuid.uuid4().hex[:12]
        prompt = _prompt_ids(req_body, self.tok, template_kwargs)
        req = Request(prompt, max(1, min(max_new, 1024)), batched=True, sampling=sampling, logprobs=logprobs,
                      penalties=penalties, guide=guide)
        st = _Stream(writer, stream, kind, rid, name, self.tok.detokenizer(prompt) if self.tok is not None else None,
                     StopMatcher(stops) if stops else None, logprobs is not None)
        req.state = st
        if stream:
            writer.write(b"HTTP/1.1 200 OK\r\nContent-Type: %s\r\nCache-Control: no-cache\r\n"
                         b"Transfer-Encoding: chunked\r\n\r\n"
                         % (b"application/x-ndjson" if ollama else b"text/event-stream"))
        self.engine.submit(req)
        return await st.done


def start_server(host="127.0.0.1", port=0, device="cuda:0", config="tiny", max_batch=8, model_name=None,
                 engine: Engine | None = None, checkpoint: str | None = None, max_seq: int | None = None,
                 tokenizer=None, default_temperature: float = 0.0, prefix_cache: bool = False, prefix_min: int = 16,
                 embed_pooling: str = "mean", penalties: bool = False, kv_dtype: str = "bf16",
                 guided: bool = False, guided_states: int = 1024):
    """Engine + HTTP front-end; returns (server, port, engine). ``server.shutdown()``
    stops the HTTP side, ``engine.stop()`` the GPU side. ``checkpoint``: serve a
    Hugging Face Llama checkpoint directory (weights + tokenizer) instead of
    the random-init ``config``. ``tokenizer`` (a ``checkpoint.Tokenizer``)
    overrides the checkpoint's own or gives an injected engine a text side.
    ``prefix_cache`` / ``prefix_min``: the engine's prefix cache (``Engine``);
    an injected ``engine`` brings its own setting, which must not contradict.
    ``embed_pooling``: how the embedding routes pool the final hidden state
    ("mean" over all positions, or the "last" position's). ``penalties``: the
    engine's on-device penalties and logit_bias (``Engine``); the endpoint then
    takes the parameters ``penalty_params`` describes instead of answering 400,
    and an injected ``engine`` must have been built with them too. ``kv_dtype``:
    "bf16" or "fp8", the KV cache's format (``TinyLlama``; docs/KV_FP8.md): fp8 halves
    its bytes, needs the graph-captured HIP step (refused on an eager engine) and must
    not contradict an injected ``engine``'s model. ``guided`` / ``guided_states``: the
    engine's guided decoding and the rows of its table arena (``Engine``; docs/GUIDED.md);
    /v1/chat/completions and /v1/completions then act on "guided_regex", "guided_choice" and
    "structured_outputs" (``guided_params``), which are ignored without the switch, and an
    injected ``engine`` must have been built with it too."""
    kv_dtype = parse_kv_dtype(kv_dtype)
    if engine is not None and guided and not getattr(engine, "guided", False):
        raise ValueError("guided=True, but the injected engine was built without it")
    if engine is not None and getattr(engine.model, "kv_dtype", "bf16") != kv_dtype:
        raise ValueError(f"kv_dtype={kv_dtype!r}, but the injected engine's model has "
                         f"{getattr(engine.model, 'kv_dtype', 'bf16')!r} caches")
    if engine is not None and prefix_cache and not engine.prefix_cache:
        raise ValueError("prefix_cache=True, but the injected engine was built without it")
    if engine is not None and penalties and not getattr(engine, "penalties", False):
        raise ValueError("penalties=True, but the injected engine was built without them")
    sys.setswitchinterval(0.0005)  # two busy threads: bound a GIL wait at 0.5 ms, not 5
    tok = tokenizer
    if checkpoint and engine is None:
        import os
        from p2p_llm_tunnel_amd.models.checkpoint import Tokenizer, load_llama
        model = load_llama(checkpoint, device=device, max_batch=max_batch, max_seq=max_seq, kv_dtype=kv_dtype)
        tok = tok or Tokenizer.for_checkpoint(checkpoint)
        engine = Engine(device=device, max_batch=max_batch, model=model, prefix_cache=prefix_cache,
                        prefix_min=prefix_min, penalties=penalties, guided=guided, guided_states=guided_states)
        model_name = model_name or os.path.basename(os.path.normpath(checkpoint))
    engine = engine or Engine(device=device, config=config, max_batch=max_batch, prefix_cache=prefix_cache,
                              prefix_min=prefix_min, penalties=penalties, kv_dtype=kv_dtype, guided=guided,
                              guided_states=guided_states)
    srv = FrontEnd(engine, host, port, model_name or f"p2pt-{config}", tokenizer=tok,
                   default_temperature=default_temperature, embed_pooling=embed_pooling)
    return srv, srv.server_address[1], engine


KV_DTYPE_CHOICES = ("bf16", "fp8")


def parse_kv_dtype(v) -> str:
    """--kv-dtype / ``start_server(kv_dtype=)``: "bf16" (the default) or "fp8"; anything else is refused."""
    if v not in KV_DTYPE_CHOICES:
        raise ValueError(f"kv_dtype must be one of {list(KV_DTYPE_CHOICES)}, got {v!r}")
    return v


def kv_cache_line(model, kv_dtype: str) -> str:
    """The start-up log line with the KV cache's size."""
    k, v = getattr(model, "k_cache", None), getattr(model, "v_cache", None)
    nbytes = sum(t.numel() * t.element_size() for t in (k, v) if t is not None)
    shape = "x".join(str(n) for n in k.shape) if k is not None else "?"
    return f"kv cache: {nbytes} bytes ({kv_dtype}, K and V of {shape})"


def replica_cmd(a, i: int) -> list[str]:
    """The command line of replica ``i`` of ``--gpus``: this process's own switches, on device ``cuda:i`` and port
    ``a.port + i``."""
    cmd = [sys.executable, "-m", "p2p_llm_tunnel_amd.models.server", "--host", a.host, "--port", str(a.port + i),
           "--device", f"cuda:{i}", "--config", a.config, "--max-batch", str(a.max_batch)]
    if a.checkpoint:
        cmd += ["--checkpoint", a.checkpoint] + (["--max-seq", str(a.max_seq)] if a.max_seq else [])
    cmd += ["--default-temperature", str(a.default_temperature)]
    if a.prefix_cache:
        cmd += ["--prefix-cache", "--prefix-min", str(a.prefix_min)]
    if getattr(a, "embed_pooling", "mean") != "mean":
        cmd += ["--embed-pooling", a.embed_pooling]
    if getattr(a, "penalties", False):
        cmd += ["--penalties"]
    if getattr(a, "kv_dtype", "bf16") != "bf16":
        cmd += ["--kv-dtype", a.kv_dtype]
    if getattr(a, "guided", False):
        cmd += ["--guided", "--guided-states", str(a.guided_states)]
    return cmd


def _replicas(a) -> int:
    """--gpus N: one endpoint process per GPU on ports port..port+N-1 (data-
    parallel replicas: the model fits one MI355X many times over, so replicas
    scale throughput with no cross-GPU traffic). `tunnel serve --upstream`
    takes the printed comma-separated list and balances requests over them by
    fewest in flight. Each child is a fresh interpreter pinned to its device;
    the parent never touches the GPU and exits with the first child that dies."""
    import subprocess
    base = a.port
    procs = []
    for i in range(a.gpus):
        procs.append(subprocess.Popen(replica_cmd(a, i)))
    ups = ",".join(f"http://{a.host}:{base + i}" for i in range(a.gpus))
    print(f"{a.gpus} inference endpoints; use: tunnel serve --upstream {ups}", flush=True)
    try:
        while True:
            for p in procs:
                rc = p.poll()
                if rc is not None:
                    for q in procs:
                        if q.poll() is None:
                            q.terminate()
                    return rc
            time.sleep(0.5)
    except KeyboardInterrupt:
        for p in procs:
            p.terminate()
        return 0


def arg_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="GPU-backed OpenAI/Ollama-compatible endpoint")
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=11434)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--config", default="tiny")
    ap.add_argument("--max-batch", type=int, default=8)
    ap.add_argument("--checkpoint", default=None,
                    help="Hugging Face Llama checkpoint directory (config.json, *.safetensors, tokenizer.json)")
    ap.add_argument("--max-seq", type=int, default=None, help="KV-cache length per slot (checkpoint default: "
                    "min(max_position_embeddings, 8192))")
    ap.add_argument("--gpus", type=int, default=0,
                    help="spawn one endpoint per GPU (cuda:0..N-1) on consecutive ports instead of serving here")
    ap.add_argument("--default-temperature", type=float, default=0.0,
                    help="temperature of requests that set none (0: greedy; requests may set temperature, top_p, "
                         "top_k, seed)")
    ap.add_argument("--prefix-cache", action="store_true",
                    help="reuse the K/V rows of a prompt prefix a cache slot already holds (multi-turn chats, "
                         "shared system prompts) instead of prefilling them again")
    ap.add_argument("--prefix-min", type=int, default=16, metavar="N",
                    help="shortest common prefix, in tokens, worth reusing (with --prefix-cache)")
    ap.add_argument("--embed-pooling", choices=("mean", "last"), default="mean",
                    help="how /v1/embeddings, /api/embed and /api/embeddings pool the final hidden state: the mean "
                         "over all positions, or the last position's (both L2-normalised)")
    ap.add_argument("--penalties", action="store_true",
                    help="apply presence_penalty, frequency_penalty, repetition_penalty and logit_bias (OpenAI) and "
                         "repeat_penalty, presence_penalty, frequency_penalty (Ollama options) on the device ahead "
                         "of the sampler instead of answering 400; the repeat penalty covers the whole prompt and "
                         "everything generated (repeat_last_n: only -1, or 0 = off). Costs a [max_batch + 1, vocab] "
                         "int32 count table and four more captured graphs")
    ap.add_argument("--kv-dtype", choices=KV_DTYPE_CHOICES, default="bf16",
                    help="format of the KV cache: bf16, or fp8 (OCP e4m3, scale 1, no calibration): half the bytes "
                         "per cached token, so the same memory holds twice the context or slots; values beyond "
                         "+-448 saturate (docs/KV_FP8.md)")
    ap.add_argument("--guided", action="store_true",
                    help="guided decoding on the device: /v1/chat/completions and /v1/completions act on "
                         "guided_regex, guided_choice and structured_outputs {regex | choice} (a checkpoint with a "
                         "ByteLevel or Metaspace tokenizer). Costs the table arena and four more captured graphs "
                         "(docs/GUIDED.md)")
    ap.add_argument("--guided-states", type=int, default=1024, metavar="N",
                    help="rows of the guided-decoding arena, 2 x vocab bytes each: the token-level states of all "
                         "resident patterns together (with --guided)")
    return ap


def main(argv=None):
    a = arg_parser().parse_args(argv)
    if a.gpus > 0:
        raise SystemExit(_replicas(a))
    srv, port, engine = start_server(a.host, a.port, a.device, a.config, a.max_batch, checkpoint=a.checkpoint,
                                     max_seq=a.max_seq, default_temperature=a.default_temperature,
                                     prefix_cache=a.prefix_cache, prefix_min=a.prefix_min,
                                     embed_pooling=a.embed_pooling, penalties=a.penalties, kv_dtype=a.kv_dtype,
                                     guided=a.guided, guided_states=a.guided_states)
    print(kv_cache_line(engine.model, a.kv_dtype), flush=True)
    print(f"inference endpoint on http://{a.host}:{port} ({a.checkpoint or a.config}, {a.device})", flush=True)
    try:
        threading.Event().wait()
    except KeyboardInterrupt:
        engine.stop()


if __name__ == "__main__":
    main()
