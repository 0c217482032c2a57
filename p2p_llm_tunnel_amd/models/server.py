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
  POST /api/chat             (Ollama chat: NDJSON stream, or one JSON object; see "Ollama chat" below)
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
logit_bias, Ollama's repeat_penalty, min_p, mirostat, ...) are answered
with 400, as is sampling on an engine without the captured HIP step.

min_p (--min-p, off by default: Ollama's "options.min_p" other than 0 is then
answered with 400 and a top-level "min_p" of an OpenAI request, which that API
does not have, is not looked at): Ollama "options.min_p" and the vLLM extension
"min_p" on the OpenAI routes, a number in [0, 1]. Tokens less likely than min_p
times the most likely one are dropped after top-k and top-p (HF's order), on
device inside the captured step (ops.sample_minp_, sample.hip). See
docs/MIN_P.md.

Ollama chat: /api/chat takes "model", "messages" ("role" system / user /
assistant, string "content"), "stream" (default true), "options" (the sampling
options, "num_predict" and "stop" of /api/generate) and "keep_alive", which is
ignored. The messages go through the chat template of /v1/chat/completions. A
streamed response is NDJSON, one {"model", "created_at", "message": {"role":
"assistant", "content": piece}, "done": false} per token batch from a byte
template rendered once per request (so "created_at" is the request's), then a
final object with an empty content, "done": true, "done_reason" ("stop" or
"length"), "prompt_eval_count", "eval_count" and "total_duration",
"prompt_eval_duration" (up to the first token) and "eval_duration" in ns; a
non-streamed one is that final object with the whole content. Non-empty
"tools" or "format", "images" on a message, a content that is no string, an
unknown role and an empty "messages" are answered with 400.

Penalties (--penalties, off by default: the 400s above stand): OpenAI
"presence_penalty", "frequency_penalty", "logit_bias" and the vLLM extension
"repetition_penalty"; Ollama "options.repeat_penalty", "presence_penalty" and
"frequency_penalty" (ranges and refusals: ``params.penalty_params``). They run
on device inside the captured step, ahead of the sampler (ops.penalize_,
penalty.hip; the arithmetic: ``params.Penalties``). The repetition penalty has
HF / vLLM semantics — every id seen in the prompt or generated, NOT Ollama's
window of the last 64 tokens: "repeat_last_n" is accepted only as -1, or 0 =
repeat penalty off. n > 1, best_of, mirostat, tfs_z and typical_p stay
refused (min_p too, unless --min-p). See docs/PENALTIES.md.

Guided decoding (--guided, off by default: the keys below are then not acted
on): /v1/chat/completions and /v1/completions take "guided_regex" (the whole
completion matches it), "guided_choice" (the completion is one of the strings)
or the newer "structured_outputs": {"regex": ...} / {"choice": [...]}
(``params.guided_params``); more than one of them, a wrong type, a pattern
outside the supported subset, a server without a tokenizer or with one whose
tokens' bytes are not known are answered with 400 and the reason. The pattern
is compiled off the I/O thread (an executor; a small LRU of compiled guides)
into a token-level automaton (models/guided.py) that ops.guide_ (guide.hip)
walks inside the captured step, masking every token its state does not allow.
A completion that reaches a full match with nothing left to add ends through
EOS (finish_reason "stop"); one cut by max_tokens ends with "length" and may
be an incomplete match. "response_format", JSON schemas, Ollama's "format" and
grammars that need a stack are out of scope. See docs/GUIDED.md.

Chat template variables: a chat request's optional "chat_template_kwargs", a
JSON object of scalars, is handed to the checkpoint's chat template
({"enable_thinking": false} for Qwen3's); anything else is answered with 400.

Log-probabilities: /v1/chat/completions takes "logprobs": true with
"top_logprobs" 0..20, /v1/completions the legacy "logprobs" 1..5
(``params.logprob_params``). They are computed on device inside the captured
step (ops.logprobs_, logprobs.hip: a log-sum-exp and a deterministic top-N
selection per requesting row) from the model's own softmax(logits): they do not
depend on temperature, top_k or top_p (vLLM's default too), nor on penalties or
logit_bias, so a banned token still reports the model's probability. Every
delivered token has an entry, the tokens of a matched stop sequence included
(their text is cut, their entries are not); the EOS token has none. A streamed
chat response with logprobs sends exactly one chunk per token (its "content"
is "" when the detokeniser or the stop matcher holds the text back).
Non-finite values are sent as -9999.0. The eager engine has no logits and
answers such a request with 400; /api/generate has no logprobs.

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
import json
import socket
import sys
import threading
import time
import uuid

# The engine and the request parameters live in their own modules; their public
# names stay importable from here.
from p2p_llm_tunnel_amd.models.engine import Engine, Request
from p2p_llm_tunnel_amd.models.params import (_LOGPROB_KEYS, Penalties, Sampling, SamplingError,  # noqa: F401
                                              StopMatcher, chat_logprob_entry, chat_logprobs, completion_logprobs,
                                              guided_params, logprob_params, penalty_params, sampling_params,
                                              stop_sequences)


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


_OLLAMA_ROLES = ("system", "user", "assistant")


def ollama_chat_body(body: dict) -> None:
    """What /api/chat refuses of a request body, beside its sampling options:
    raises SamplingError (answered with 400) naming the field. "messages" is a
    non-empty list of objects with a "role" of system, user or assistant and a
    string "content"; "images" on a message, non-empty "tools" and a non-empty
    "format" (tool calls, vision and JSON output are not served) are refused,
    not ignored."""
    if body.get("tools"):
        raise SamplingError("tools are not supported by this server")
    if body.get("format"):
        raise SamplingError(f"format={body['format']!r} is not supported by this server")
    msgs = body.get("messages")
    if not isinstance(msgs, list) or not msgs:
        raise SamplingError("messages must be a non-empty list")
    for n, m in enumerate(msgs):
        if not isinstance(m, dict):
            raise SamplingError(f"messages[{n}] must be an object")
        if m.get("role") not in _OLLAMA_ROLES:
            raise SamplingError(f"messages[{n}].role must be one of {list(_OLLAMA_ROLES)}, got {m.get('role')!r}")
        if m.get("images"):
            raise SamplingError(f"messages[{n}].images is not supported by this server")
        if not isinstance(m.get("content"), str):
            raise SamplingError(f"messages[{n}].content must be a string, got {m.get('content')!r}")


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
                 "stop_hit", "lp_toks", "lp_off", "t0", "t_first", "created", "n_tok")

    def __init__(self, writer, stream, kind, rid, model, detok=None, stop=None, logprobs=False):
        self.t0 = time.perf_counter_ns()  # /api/chat's durations: the request's start, and its first token's arrival
        self.t_first = 0
        self.n_tok = 0  # tokens taken from the engine (the EOS token or a matched stop's included)
        self.created = None  # /api/chat: "created_at", one per request
        self.lp_toks = [] if logprobs else None  # with logprobs: the delivered ids; Request.lp[k] belongs to the k-th
        self.lp_off = 0  # legacy completions, streamed: text_offset of the next token
        self.writer = writer
        self.stream = stream
        self.kind = kind  # "chat" | "text" | "ollama" (/api/generate) | "ollama_chat" (/api/chat)
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
        elif kind == "ollama_chat":
            now = time.time()
            self.created = time.strftime("%Y-%m-%dT%H:%M:%S", time.gmtime(now)) + ".%06dZ" % (now % 1 * 1e6)
            self.pre = ('{"model": %s, "created_at": "%s", "message": {"role": "assistant", "content": "'
                        % (m, self.created)).encode()
            self.post = b'"}, "done": false}\n'
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
            if not st.t_first:
                st.t_first = time.perf_counter_ns()
            if tok is None:
                self._finish(req, st)
                continue
            st.n_tok += 1
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

    def _ollama_chat_final(self, req, st, content: str) -> dict:
        """The last object of an /api/chat response (the only one when it is not streamed)."""
        now = time.perf_counter_ns()
        first = st.t_first or now
        return {"model": self.model_name, "created_at": st.created,
                "message": {"role": "assistant", "content": content}, "done": True, "done_reason": st.reason,
                "total_duration": now - st.t0, "prompt_eval_count": len(req.prompt),
                "prompt_eval_duration": first - st.t0, "eval_count": st.n_tok, "eval_duration": now - first}

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
            elif st.kind == "ollama_chat":
                tail = _chunk((json.dumps(self._ollama_chat_final(req, st, "")) + "\n").encode())
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
            elif st.kind == "ollama_chat":
                obj = self._ollama_chat_final(req, st, text)
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
        g = compile_guide(kind, list(pattern) if kind == "choice" else pattern, tb,
                          [e for e in self.eos if 0 <= e < V], self.engine._gd.tables.states)
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
                                            "/api/generate", "/api/chat"):
            writer.write(self._json_response({"error": "not found"}, 404))
            return True
        try:
            req_body = json.loads(body or b"{}")
            if not isinstance(req_body, dict):
                req_body = {}
        except ValueError:
            req_body = {}
        raw_max = req_body.get("max_tokens", req_body.get("num_predict", 16))
        if path == "/api/chat":
            try:
                ollama_chat_body(req_body)
            except SamplingError as e:
                writer.write(self._json_response({"error": {"message": str(e), "type": "invalid_request_error"}}, 400))
                return True
            opts = req_body.get("options")
            if isinstance(opts, dict) and opts.get("num_predict") is not None:  # where Ollama's clients put it
                raw_max = opts["num_predict"]
        try:
            max_new = int(raw_max if raw_max is not None else 16)
        except (TypeError, ValueError):
            writer.write(self._json_response({"error": f"max_tokens must be an integer, got {raw_max!r}"}, 400))
            return True
        ollama = path in ("/api/generate", "/api/chat")
        kind = ("ollama_chat" if path == "/api/chat" else "ollama") if ollama else \
            ("chat" if "chat" in path else "text")
        try:
            # Logprobs first; sampling_params refuses both keys, so the OpenAI
            # endpoints hand it the body without them.
            logprobs = logprob_params(req_body, "ollama" if ollama else kind)
            if logprobs is not None and not self.engine.use_graph:
                raise SamplingError("logprobs need the graph-captured HIP step; this engine runs eagerly")
            rest = req_body if ollama else {k: v for k, v in req_body.items() if k not in _LOGPROB_KEYS}
            pen_on = getattr(self.engine, "penalties", False)
            sampling = sampling_params(rest, ollama, self.default_temperature, penalties=pen_on,
                                       vocab=self.engine.model.cfg.vocab,
                                       min_p=getattr(self.engine, "min_p", False))
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
                 guided: bool = False, guided_states: int = 1024, weight_dtype: str = "bf16", kv_scales=None,
                 sliding_window: bool = False, min_p: bool = False):
    """Engine + HTTP front-end; returns (server, port, engine). ``server.shutdown()``
    stops the HTTP side, ``engine.stop()`` the GPU side. ``checkpoint``: serve a
    Hugging Face Llama checkpoint directory (weights + tokenizer) instead of
    the random-init ``config``. ``tokenizer`` (a ``checkpoint.Tokenizer``)
    overrides the checkpoint's own or gives an injected engine a text side.
    ``embed_pooling``: how the embedding routes pool the final hidden state
    ("mean" over all positions, or the "last" position's). ``prefix_cache`` /
    ``prefix_min``, ``penalties``, ``guided`` / ``guided_states`` and ``kv_dtype``
    ("bf16" or "fp8", the KV cache's format: docs/KV_FP8.md) are ``Engine``'s; an
    injected ``engine`` brings its own settings, which these must not contradict.
    With ``penalties`` the endpoint takes the parameters ``penalty_params``
    describes instead of answering 400; with ``guided`` /v1/chat/completions and
    /v1/completions act on what ``guided_params`` describes, which is ignored
    without the switch. ``weight_dtype`` ("bf16", "fp8" or "mxfp4", the format of the GEMM weights:
    docs/WEIGHT_FP8.md, docs/WEIGHT_MXFP4.md) is ``Engine``'s and ``load_llama``'s, and an injected engine's model must have it.
    ``kv_scales`` (``kv_dtype="fp8"`` only): a ``KvScales``, the path of a JSON file ``{"k": [[..]], "v": [[..]]}``
    or "checkpoint" (the checkpoint's own ``k_scale`` / ``v_scale`` tensors): per-layer, per-KV-head scales of the
    FP8 cache (docs/KV_FP8.md); an injected engine's model must carry the same.
    ``sliding_window``: serve the checkpoint's sliding attention window instead of capping the context at it
    (``load_llama``, docs/SLIDING_WINDOW.md); it needs a checkpoint that declares one, or an injected engine whose
    model has windowed layers.
    ``min_p`` is ``Engine``'s: the endpoint then takes Ollama's "options.min_p" and a top-level "min_p" on the OpenAI
    routes (``sampling_params``, docs/MIN_P.md) instead of refusing the first and ignoring the second; an injected
    engine must have been built with it."""
    if engine is not None and min_p and not getattr(engine, "min_p", False):
        raise ValueError("min_p=True, but the injected engine was built without it")
    if sliding_window and engine is None and not checkpoint:
        raise ValueError("sliding_window=True (--sliding-window) needs a checkpoint that declares a sliding window")
    if sliding_window and engine is not None and not getattr(getattr(engine.model, "cfg", None), "windowed", False):
        raise ValueError("sliding_window=True, but the injected engine's model has no windowed layer")
    kv_dtype = parse_kv_dtype(kv_dtype)
    from p2p_llm_tunnel_amd.models import kv_scales as kvs
    kv_scales = kvs.parse_kv_scales(kv_scales, kv_dtype)
    if kv_scales == kvs.CHECKPOINT and not (checkpoint and engine is None):
        raise ValueError("kv_scales='checkpoint' (--kv-scales checkpoint) needs a checkpoint to read them from")
    if engine is not None and kv_scales is not None and getattr(engine.model, "kv_scales", None) != kv_scales:
        raise ValueError("kv_scales given, but the injected engine's model was built with other scales or none")
    weight_dtype = parse_weight_dtype(weight_dtype)
    if engine is not None and getattr(engine.model, "weight_dtype", "bf16") != weight_dtype:
        raise ValueError(f"weight_dtype={weight_dtype!r}, but the injected engine's model has "
                         f"{getattr(engine.model, 'weight_dtype', 'bf16')!r} weights")
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
        model = load_llama(checkpoint, device=device, max_batch=max_batch, max_seq=max_seq, kv_dtype=kv_dtype,
                           weight_dtype=weight_dtype, kv_scales=kv_scales, sliding_window=sliding_window)
        tok = tok or Tokenizer.for_checkpoint(checkpoint)
        engine = Engine(device=device, max_batch=max_batch, model=model, prefix_cache=prefix_cache,
                        prefix_min=prefix_min, penalties=penalties, guided=guided, guided_states=guided_states,
                        min_p=min_p)
        model_name = model_name or os.path.basename(os.path.normpath(checkpoint))
    engine = engine or Engine(device=device, config=config, max_batch=max_batch, prefix_cache=prefix_cache,
                              prefix_min=prefix_min, penalties=penalties, kv_dtype=kv_dtype, guided=guided,
                              guided_states=guided_states, weight_dtype=weight_dtype, kv_scales=kv_scales,
                              min_p=min_p)
    srv = FrontEnd(engine, host, port, model_name or f"p2pt-{config}", tokenizer=tok,
                   default_temperature=default_temperature, embed_pooling=embed_pooling)
    return srv, srv.server_address[1], engine


KV_DTYPE_CHOICES = ("bf16", "fp8")


def parse_kv_dtype(v) -> str:
    """--kv-dtype / ``start_server(kv_dtype=)``: "bf16" (the default) or "fp8"; anything else is refused."""
    if v not in KV_DTYPE_CHOICES:
        raise ValueError(f"kv_dtype must be one of {list(KV_DTYPE_CHOICES)}, got {v!r}")
    return v


WEIGHT_DTYPE_CHOICES = ("bf16", "fp8", "mxfp4")


def parse_weight_dtype(v) -> str:
    """--weight-dtype / ``start_server(weight_dtype=)``: "bf16" (the default), "fp8" or "mxfp4"; anything else is refused."""
    if v not in WEIGHT_DTYPE_CHOICES:
        raise ValueError(f"weight_dtype must be one of {list(WEIGHT_DTYPE_CHOICES)}, got {v!r}")
    return v


def weights_line(model, weight_dtype: str) -> str:
    """The start-up log line with the weights' size."""
    sizes = getattr(model, "weight_bytes", None)
    if not callable(sizes):
        return f"weights: ? bytes ({weight_dtype})"
    b = sizes()
    return (f"weights: {b['total']} bytes ({weight_dtype} GEMM weights {b['gemm']}, bf16 embedding {b['embed']})")


def kv_cache_line(model, kv_dtype: str) -> str:
    """The start-up log line with the KV cache's size."""
    k, v = getattr(model, "k_cache", None), getattr(model, "v_cache", None)
    nbytes = sum(t.numel() * t.element_size() for t in (k, v) if t is not None)
    shape = "x".join(str(n) for n in k.shape) if k is not None else "?"
    scales = getattr(model, "kv_scales", None)
    return (f"kv cache: {nbytes} bytes ({kv_dtype}, K and V of {shape})"
            + (f"; scales in use: {scales.describe()}" if scales is not None else ""))


def min_p_line(engine) -> str:
    """The start-up log line of ``--min-p``."""
    if getattr(engine, "min_p", False):
        return "min_p: on (options.min_p and min_p are applied on the device after top-k and top-p)"
    return "min_p: off (options.min_p other than 0 is answered with 400; start with --min-p)"


def window_line(model) -> str:
    """The start-up log line of ``--sliding-window``: the window, how many layers have one, and the context."""
    cfg = model.cfg
    windows = [w for w in (cfg.windows or ()) if w]
    sizes = sorted(set(windows))
    return (f"sliding window: {'/'.join(str(w) for w in sizes) or 'none'} tokens on {len(windows)} of {cfg.n_layers} "
            f"layers; context {cfg.max_seq} tokens (the cache keeps every row: no ring buffer)")


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
    if getattr(a, "kv_scales", None):
        cmd += ["--kv-scales", a.kv_scales]
    if getattr(a, "guided", False):
        cmd += ["--guided", "--guided-states", str(a.guided_states)]
    if getattr(a, "weight_dtype", "bf16") != "bf16":
        cmd += ["--weight-dtype", a.weight_dtype]
    if getattr(a, "sliding_window", False):
        cmd += ["--sliding-window"]
    if getattr(a, "min_p", False):
        cmd += ["--min-p"]
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
                    help="format of the KV cache: bf16, or fp8 (OCP e4m3; scale 1 unless --kv-scales gives scales): half "
                         "the bytes per cached token, so the same memory holds twice the context or slots; values "
                         "beyond +-448 times the scale saturate (docs/KV_FP8.md)")
    ap.add_argument("--kv-scales", default=None, metavar="checkpoint|FILE",
                    help="per-layer, per-KV-head scales of the fp8 KV cache (with --kv-dtype fp8): 'checkpoint' reads "
                         "the checkpoint's self_attn.k_scale / .v_scale (or kv_scale) tensors; FILE is JSON "
                         '{"k": [[...]], "v": [[...]]}, one row per layer and one number per KV head, as '
                         "scripts/calibrate_kv.py writes it (docs/KV_FP8.md)")
    ap.add_argument("--weight-dtype", choices=WEIGHT_DTYPE_CHOICES, default="bf16",
                    help="format of the GEMM weights (QKV, O, gate/up, down and the LM head): bf16, or fp8 (OCP e4m3 "
                         "with one fp32 scale per output row, per-row absmax, no calibration; the activations stay "
                         "bf16): half the weight bytes per decode step; the embedding table stays bf16 "
                         "(docs/WEIGHT_FP8.md); or mxfp4 (OCP Microscaling FP4 for the four GEMM weights of every "
                         "layer: e2m1 values in blocks of 32 with a power-of-two scale, round to nearest, no "
                         "calibration; the LM head is fp8): about a quarter of their bytes (docs/WEIGHT_MXFP4.md)")
    ap.add_argument("--sliding-window", action="store_true",
                    help="serve the checkpoint's sliding attention window (Mistral-7B-v0.1 and its fine-tunes; Qwen2 / "
                         "Qwen3 with use_sliding_window) instead of capping the context at it: the layers that slide "
                         "attend to their last sliding_window tokens and the context follows --max-seq / "
                         "max_position_embeddings. Needs --checkpoint; one that declares no window is refused "
                         "(docs/SLIDING_WINDOW.md)")
    ap.add_argument("--min-p", action="store_true",
                    help="take min_p (Ollama options.min_p; a top-level min_p on the OpenAI routes, vLLM's extension) "
                         "instead of answering 400 / ignoring it: tokens less likely than min_p times the most likely "
                         "one are dropped on the device after top-k and top-p. Costs one more staged row per step; "
                         "the number of captured graphs stays (docs/MIN_P.md)")
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
    if a.kv_scales and a.kv_dtype != "fp8":
        raise SystemExit("--kv-scales needs --kv-dtype fp8: a bf16 KV cache has no scales")
    if a.sliding_window and not a.checkpoint:
        raise SystemExit("--sliding-window needs --checkpoint: the window is the checkpoint's own")
    if a.gpus > 0:
        raise SystemExit(_replicas(a))
    srv, port, engine = start_server(a.host, a.port, a.device, a.config, a.max_batch, checkpoint=a.checkpoint,
                                     max_seq=a.max_seq, default_temperature=a.default_temperature,
                                     prefix_cache=a.prefix_cache, prefix_min=a.prefix_min,
                                     embed_pooling=a.embed_pooling, penalties=a.penalties, kv_dtype=a.kv_dtype,
                                     guided=a.guided, guided_states=a.guided_states, weight_dtype=a.weight_dtype,
                                     kv_scales=a.kv_scales, sliding_window=a.sliding_window, min_p=a.min_p)
    print(weights_line(engine.model, a.weight_dtype), flush=True)
    print(kv_cache_line(engine.model, a.kv_dtype), flush=True)
    if a.sliding_window:
        print(window_line(engine.model), flush=True)
    print(min_p_line(engine), flush=True)
    print(f"inference endpoint on http://{a.host}:{port} ({a.checkpoint or a.config}, {a.device})", flush=True)
    try:
        threading.Event().wait()
    except KeyboardInterrupt:
        engine.stop()


if __name__ == "__main__":
    main()
