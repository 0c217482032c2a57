"""Request parameters of the inference endpoint (models/server.py): request body
to values (``Sampling``, ``Penalties``, a guide's pattern, logprobs, stops) and
back (the logprob renderers). No torch: ``ops`` is imported where the engine calls."""
from __future__ import annotations

import os


class Sampling:
    """How a request picks its tokens: temperature (0 = greedy argmax, the
    fused LM head's own result), then top-k (0 = off) and top-p (1 = off),
    drawn on device by ``ops.sample_`` (sample.hip) from a per-request seed
    and the token's index, so a fixed seed replays the same completion.
    ``min_p`` (0 = off; an engine built with ``min_p=True``, docs/MIN_P.md)
    then drops every token less likely than min_p times the most likely one
    (``ops.sample_minp_``)."""
    __slots__ = ("temperature", "top_k", "top_p", "seed", "min_p")

    def __init__(self, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, seed: int | None = None,
                 min_p: float = 0.0):
        self.temperature = float(temperature)
        self.top_k = int(top_k)
        self.top_p = float(top_p)
        self.seed = int.from_bytes(os.urandom(8), "little") >> 1 if seed is None else int(seed) & ((1 << 63) - 1)
        if isinstance(min_p, bool) or not isinstance(min_p, (int, float)) or not 0.0 <= min_p <= 1.0:
            raise ValueError(f"min_p must be a number in [0, 1], got {min_p!r}")
        self.min_p = float(min_p)

    @property
    def greedy(self) -> bool:
        return not self.temperature >= 1e-4 or self.top_k == 1  # the kernel's own greedy rule (+ top-1)

    def column(self, counter: int, min_p: bool = False) -> list[int]:
        """The sampler's params column: five values, or six for an engine built with ``min_p=True``."""
        from p2p_llm_tunnel_amd.ops import pack_sampling
        return pack_sampling(0.0 if self.greedy else self.temperature, self.top_k, self.top_p, self.seed, counter,
                             self.min_p if min_p else None)


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
                    vocab: int | None = None, min_p: bool = False) -> Sampling:
    """Sampling of an OpenAI request (top-level temperature / top_p / seed, and
    the common top_k extension) or an Ollama one ("options"). Raises
    SamplingError for values out of range or parameters not implemented,
    "logprobs" and "top_logprobs" among them: the OpenAI endpoints parse those
    first with ``logprob_params`` and pass this function the body without them.

    ``penalties`` (a server started with --penalties; ``vocab``: the model's):
    the penalty parameters and logit_bias are then checked by
    ``penalty_params`` — whose result the caller takes from there — instead of
    being refused unless neutral; everything else is as without the switch.

    ``min_p`` (a server started with --min-p): Ollama's "options.min_p" and
    the top-level "min_p" of an OpenAI request (vLLM's extension) are taken, a
    number in [0, 1], 0 = off. Without the switch an Ollama value other than 0
    is refused like the other unimplemented options, and the OpenAI key, which
    is no part of that API, is not looked at."""
    src = body.get("options", {}) if ollama else body
    if src is None:
        src = {}
    if not isinstance(src, dict):
        raise SamplingError("options must be an object")
    taken = () if not penalties else _OLLAMA_PENALTY_KEYS if ollama else _OPENAI_PENALTY_KEYS
    if min_p:
        taken += ("min_p",)
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
    return Sampling(t, top_k, top_p, seed, _number(src, "min_p", 0.0, 1.0, 0.0) if min_p else 0.0)


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
