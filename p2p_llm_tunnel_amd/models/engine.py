"""The continuous-batching ``Engine`` behind models/server.py: one thread that
owns the GPU, admits ``Request`` objects into cache slots and advances every
active slot by one token per captured step."""
from __future__ import annotations

import functools
import queue
import threading
import time
from typing import NamedTuple

import torch

from p2p_llm_tunnel_amd.models.guided import MAX_STATES, Guide
from p2p_llm_tunnel_amd.models.params import Penalties, Sampling


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


def _layout(min_p: bool) -> tuple:
    """(sampler rows, logprobs row, penalty rows) of the staging block. An engine built with min_p=True stages
    one more sampler row, the float32 bits of ln(min_p), right behind the five (ops.sample_minp_ reads its six
    rows as one block), and what follows moves down by one; without it, the rows named above."""
    return (slice(5, 11), _LP + 1, slice(_PEN.start + 1, _PEN.stop + 1)) if min_p else (_SMP, _LP, _PEN)


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


# What follows the fused step inside a captured graph, its ``post``, is described here and nowhere else. The stages,
# in the order they run: ops.penalize_ writes the penalised logits of the rows that sample into ``work`` and replaces
# their greedy ids by its argmax; ops.guide_ advances each slot's automaton by the row's input token, masks what the
# state does not allow to -inf in ``work`` (a copy of the logits when nothing was penalised) and takes the argmax
# again; ops.sample_ (ops.sample_minp_ in an engine built with min_p=True) draws from ``work`` when either ran, else
# from the logits; ops.logprobs_ reads the RAW logits
# (log-probabilities stay the model's own) and its outputs go back to pinned memory. A step replays the lowest post
# that runs every stage an emitting row needs; rows that need less are off in their staging columns (``work`` is a
# copy of their logits, their ids stand).
_SAMPLE, _LOGPROBS, _PENALIZE, _GUIDE = 1, 2, 4, 8


def _posts(penalties: bool, guided: bool) -> dict:
    """post -> the mask of stages it runs: 0 none (all-greedy steps), 1, 2, with
    ``penalties`` 3, with ``guided`` 4, which penalises exactly when 3 exists."""
    posts = {0: 0, 1: _SAMPLE, 2: _SAMPLE | _LOGPROBS}
    if penalties:
        posts[3] = _SAMPLE | _LOGPROBS | _PENALIZE
    if guided:
        posts[4] = _SAMPLE | _LOGPROBS | _GUIDE | (_PENALIZE if penalties else 0)
    return posts


class _PenaltyState:
    """Device state of ``Engine(penalties=True)``: per cache slot and
    vocabulary id how often the id was generated and whether it occurs in the
    prompt (``state``, int32 [max_batch + 1, V]; the scratch slot's row serves
    capture and padding), the slots' logit_bias lists (``bias_*``) and the
    stagings of ``reset``. The count of the token a step samples exists only on
    the device when the next step is queued, so ``ops.penalize_`` counts a
    decode row's input token itself, one step late and in time."""

    def __init__(self, cfg, device, max_batch: int):
        from p2p_llm_tunnel_amd.ops import MAX_LOGIT_BIAS
        self.state = torch.zeros((max_batch + 1, cfg.vocab), dtype=torch.int32, device=device)
        self.bias_n = torch.zeros(max_batch + 1, dtype=torch.int32, device=device)
        self.bias_ids = torch.zeros((max_batch + 1, MAX_LOGIT_BIAS), dtype=torch.int32, device=device)
        self.bias_val = torch.zeros((max_batch + 1, MAX_LOGIT_BIAS), dtype=torch.float32, device=device)
        # A reset's input: the prompt ids, then [2, k] bias ids and value bits, written into pinned memory and copied
        # to ONE device twin (the copy and the kernel that reads the twin are ordered on the stream, so one is
        # enough). The pinned side must not be rewritten while a queued copy may still read it, and a slot can be
        # taken again before its previous request's only step has drained (one-chunk prompt, max_new = 1: freed at
        # plan time). Two alternating stagings per slot, no event: a slot is freed only by a pass of ``Engine._plan``
        # that ran rows of it or that follows such a pass, so between two admissions into one slot a step is launched
        # behind the first one's copy, and ``Engine._loop`` has drained every step launched two passes back (the
        # step's event covers the copy queued ahead of it). The third admission is at least two passes after the
        # first: the staging it rewrites is no longer read.
        n = cfg.max_seq + 2 * MAX_LOGIT_BIAS
        self._stage = [[torch.zeros(n, dtype=torch.int32, pin_memory=True) for _ in (0, 1)] for _ in range(max_batch)]
        self._turn = [0] * max_batch
        self._dev = torch.zeros(n, dtype=torch.int32, device=device)

    def reset(self, slot: int, req: Request, ids: list):
        """Queue ``ops.penalty_reset_`` for a request with penalties admitted
        into ``slot``, whether its prompt's head runs, is reused in place or is
        copied: ``ids`` is its whole prompt as admitted, cached rows included."""
        if req.penalties is None:
            return
        import numpy as np
        from p2p_llm_tunnel_amd import ops
        h = self._stage[slot][self._turn[slot]]
        self._turn[slot] ^= 1
        hn = h.numpy()
        n = len(ids)
        hn[:n] = ids
        bias = [(t, v) for t, v in req.penalties.logit_bias.items() if v != 0.0]  # submit checked the ids
        k = len(bias)
        if k:
            hn[n:n + k] = [t for t, _ in bias]
            hn[n + k:n + 2 * k] = np.asarray([v for _, v in bias], dtype=np.float32).view(np.int32)
        d = self._dev[:n + 2 * k]
        d.copy_(h[:n + 2 * k], non_blocking=True)
        ops.penalty_reset_(self.state, slot, d[:n], self.bias_n, self.bias_ids, self.bias_val,
                           d[n:].view(2, k) if k else None)


class GuideTables:
    """Which guide tables are resident in an arena of ``states`` rows, and
    where: host bookkeeping only, no device. ``tables`` maps a guide's key to
    ``[first row, rows, holders, tick of last use]``. The contract:

    * requests with the same key share one table; ``reserve`` counts a holder,
      ``release`` gives one back, and a table without holders is idle;
    * a new table goes first-fit into the gaps between the resident ones;
    * idle tables stay resident; they are evicted least recently used first, and
      only when that can make the room: a table that would not fit even with
      every idle one gone evicts nothing and has no room now;
    * a held table is never evicted and never moved."""

    def __init__(self, states: int):
        if isinstance(states, bool) or not isinstance(states, int) or not 1 <= states <= MAX_STATES:
            raise ValueError(f"guided_states must be an integer in 1..{MAX_STATES}, got {states!r}")
        self.states = states
        self.tables: dict = {}
        self.tick = 0  # one per reserve: the order of last use

    def _room(self, n: int, held_only: bool = False):
        """First row of a gap of ``n`` rows between the resident tables
        (``held_only``: as if every idle one were gone), or None."""
        at = 0
        for first, rows, held, _ in sorted(self.tables.values()):
            if held_only and not held:
                continue
            if first - at >= n:
                return at
            at = first + rows
        return at if self.states - at >= n else None

    def reserve(self, key, n_states: int):
        """Count one more holder of ``key``'s table of ``n_states`` rows:
        ``(first row, upload)``, where ``upload`` says the table is new there
        and must be copied in, or None when it does not fit now."""
        self.tick += 1
        t = self.tables.get(key)
        if t is not None:
            t[2] += 1
            t[3] = self.tick
            return t[0], False
        at = self._room(n_states)
        if at is None and self._room(n_states, held_only=True) is None:
            return None  # not even without the idle tables: they stay resident for the requests that come back
        while at is None:
            idle = [k for k, v in self.tables.items() if v[2] == 0]
            del self.tables[min(idle, key=lambda k: self.tables[k][3])]
            at = self._room(n_states)
        self.tables[key] = [at, n_states, 1, self.tick]
        return at, True

    def release(self, key):
        self.tables[key][2] -= 1


class _GuideState:
    """Device state of ``Engine(guided=True)`` around a ``GuideTables``: the
    arena of token-table rows (int16 [guided_states, V]), per cache slot the
    arena row its request's table starts at (``base``, -1 = not guided) and the
    automaton's state (``cur``), and the staging of table uploads. ``uploads``:
    tables copied into the arena; ``shared``: requests that found theirs there."""

    _STAGE_BYTES = 4 << 20  # pinned staging of a table upload, two of them

    def __init__(self, cfg, device, max_batch: int, states: int):
        self.tables = GuideTables(states)
        self.arena = torch.full((states, cfg.vocab), -1, dtype=torch.int16, device=device)
        self.base = torch.full((max_batch + 1,), -1, dtype=torch.int32, device=device)
        self.cur = torch.zeros(max_batch + 1, dtype=torch.int32, device=device)
        # Uploads go through pinned memory in pieces of whole table rows. The pinned side must not be rewritten while
        # a queued copy may still read it. Unlike a penalty reset, an upload is rare (only a pattern that is not
        # resident) and large, so nothing is derived from the order of the loop's passes here: each of the two
        # stagings has an event, recorded behind the copy that reads it, and the engine waits for it before it writes
        # that staging again. The wait is for copies queued behind at most the two steps in flight.
        per = max(1, self._STAGE_BYTES // (2 * cfg.vocab))
        self._stage = [torch.zeros((per, cfg.vocab), dtype=torch.int16, pin_memory=True) for _ in (0, 1)]
        self._stage_ev = [None, None]
        self._turn = 0
        self._slot: list = [None] * max_batch  # (key, req) of the guided request a slot holds
        self._on = [False] * max_batch  # the device's base[slot] is >= 0
        self.uploads = self.shared = 0

    def release(self, slots: list):
        """Give back the tables of slots whose guided request has left."""
        for i, held in enumerate(self._slot):
            if held is not None and (slots[i] is None or slots[i]["req"] is not held[1]):
                self.tables.release(held[0])
                self._slot[i] = None

    def reserve(self, req: Request) -> bool:
        """Make ``req``'s table resident, held by ``req``; False when it has no room
        now. What an upload overwrites was last read by steps queued ahead of it."""
        g = req.guide
        got = self.tables.reserve(g.key, g.n_states)
        if got is None:
            return False
        at, upload = got
        if not upload:
            self.shared += 1
            return True
        per = self._stage[0].shape[0]
        for r0 in range(0, g.n_states, per):
            n = min(per, g.n_states - r0)
            turn = self._turn
            self._turn ^= 1
            if self._stage_ev[turn] is not None:
                self._stage_ev[turn].synchronize()
            h = self._stage[turn]
            h.numpy()[:n] = g.next[r0:r0 + n]
            self.arena[at + r0:at + r0 + n].copy_(h[:n], non_blocking=True)
            ev = self._stage_ev[turn] = self._stage_ev[turn] or torch.cuda.Event()
            ev.record()
        self.uploads += 1
        return True

    def bind(self, slot: int, req: Request):
        """Queue ``ops.guide_reset_`` for a request admitted into ``slot``: its table's
        first row and state 0, or -1 when it has no guide and the slot's last one had."""
        from p2p_llm_tunnel_amd import ops
        if req.guide is None:
            if self._on[slot]:
                ops.guide_reset_(self.base, self.cur, self.arena, slot, -1)
                self._on[slot] = False
            return
        self._slot[slot] = (req.guide.key, req)
        ops.guide_reset_(self.base, self.cur, self.arena, slot, self.tables.tables[req.guide.key][0])
        self._on[slot] = True


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
    every row); its own rows become resident like any other request's.

    ``penalties`` and ``guided`` (both off by default: the engine then allocates,
    captures, stages and replays exactly what is described above) serve
    ``Request(penalties=)`` and ``Request(guide=)`` (docs/PENALTIES.md,
    docs/GUIDED.md) from a ``_PenaltyState`` (``_pen``) and a ``_GuideState``
    (``_gd``), each None when off and each with one more captured ``post`` per
    (R, par): what a post runs, and which one a step replays, is described once,
    above ``_posts``. Admission resets the slot's device state ahead of the
    request's first step (``_PenaltyState.reset``, ``_GuideState.bind``); a
    guided request whose table has no room yet waits at the head of the
    admission queue (``_take``, ``GuideTables``).

    ``min_p`` (off by default, and then nothing above changes): the staging
    block holds a sixth sampler row (``_layout``), every captured post that
    samples launches ``ops.sample_minp_`` in place of ``ops.sample_``, and
    ``Sampling(min_p=)`` is honoured (docs/MIN_P.md). The number of graphs is
    what it is without the switch.
    """

    def __init__(self, device="cuda:0", config="tiny", max_batch=8, seed=0, use_graph=True, rows=64, model=None,
                 small_rows=16, prefix_cache=False, prefix_min=16, penalties=False, kv_dtype="bf16",
                 guided=False, guided_states=1024, weight_dtype="bf16", kv_scales=None, min_p=False):
        if kv_scales is not None and kv_dtype != "fp8" and getattr(model, "kv_dtype", "bf16") != "fp8":
            raise ValueError("kv_scales need kv_dtype='fp8' (--kv-dtype fp8): a bf16 KV cache has no scales")
        if model is None:
            from p2p_llm_tunnel_amd.models.tiny_llm import TinyLlama
            model = TinyLlama(config, device=device, max_batch=max_batch, seed=seed, fused=True, kv_dtype=kv_dtype,
                              weight_dtype=weight_dtype, kv_scales=kv_scales)
        elif kv_scales is not None and getattr(model, "kv_scales", None) != kv_scales:
            raise ValueError("kv_scales given, but the injected model was built with other scales or none")
        elif kv_dtype != "bf16" and getattr(model, "kv_dtype", "bf16") != kv_dtype:
            raise ValueError(f"kv_dtype={kv_dtype!r}, but the injected model was built with "
                             f"{getattr(model, 'kv_dtype', 'bf16')!r} caches")
        elif weight_dtype != "bf16" and getattr(model, "weight_dtype", "bf16") != weight_dtype:
            raise ValueError(f"weight_dtype={weight_dtype!r}, but the injected model was built with "
                             f"{getattr(model, 'weight_dtype', 'bf16')!r} weights")
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
        # Two row counts under graphs: the 64-row graphs (4 MFMA row tiles) serve prefill-heavy steps and more than
        # 16 generating slots; their LM head covers only the leading rows that sample (one per slot at most).
        sizes = [small_rows] + ([rows] if rows > small_rows else []) if use_graph else [rows]
        lp_dev = self.device if use_graph else None
        fp8 = getattr(model, "kv_dtype", "bf16") != "bf16"  # read and written by the fused HIP step alone
        w8 = getattr(model, "weight_dtype", "bf16") != "bf16"  # multiplied by the fused HIP step alone
        windowed = bool(getattr(getattr(model, "cfg", None), "windowed", False))  # attended by the fused HIP step alone
        for on, what in ((penalties, "penalties need"), (fp8, "an fp8 KV cache needs"), (w8, f"{getattr(model, 'weight_dtype', 'bf16')} weights need"),
                         (guided, "guided decoding needs"), (windowed, "a sliding window needs"),
                         (min_p, "min_p needs")):
            if on and not use_graph:
                raise ValueError(f"{what} the graph-captured HIP step; this engine runs eagerly")
        self.penalties = bool(penalties)
        self.guided = bool(guided)
        self._held = None  # a guided request that waits for room in the arena (the head of the admission queue)
        self.min_p = bool(min_p)
        self._smp, self._lp, self._pen_rows = _layout(self.min_p)
        in_rows = self._pen_rows.stop if self.penalties else self._lp + 1
        self._bufs = {R: [_StepBuf(R, cuda, lp_dev, in_rows), _StepBuf(R, cuda, lp_dev, in_rows)] for R in sizes}
        self._d_in = {R: torch.zeros((in_rows, R), dtype=torch.int64, device=self.device) for R in sizes}
        cfg = model.cfg
        self._pen = _PenaltyState(cfg, self.device, max_batch) if penalties else None
        self._gd = _GuideState(cfg, self.device, max_batch, guided_states) if guided else None
        # What penalize_ and guide_ write and the sampler then reads, over the rows that sample.
        self._work = {R: torch.zeros((R if R == small_rows else max_batch, cfg.vocab), dtype=torch.bfloat16,
                                     device=self.device) for R in sizes} if penalties or guided else None
        # Each graph holds the whole step (_step_body), one per staging buffer
        # of the pair and per ``post`` (see ``_posts``), so a step is one replay.
        self._posts = _posts(self.penalties, self.guided)
        # stages an emitting row can need (a mask) -> the lowest post that runs them all
        self._post_for = [min((p for p, st in self._posts.items() if st & need == need), default=None)
                          for need in range(16)]
        self._graphs = {(R, par, post): self._capture(self._bufs[R][par], 0 if R == small_rows else max_batch, post)
                        for R in sizes if use_graph for par in (0, 1) for post in self._posts}
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
        # Prefix cache: per slot the state of the request that last took it (its residency; kept after the slot is
        # freed), whether the slot was busy at the last admission pass, and the pass-ordered tick at which it was seen
        # free (least recently freed = smallest).
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
        if req.penalties is not None and self._pen is None:
            raise ValueError("penalties and logit_bias need an engine built with penalties=True (--penalties) on the "
                             "graph-captured HIP step")
        if req.penalties is not None and any(t >= self.model.cfg.vocab for t in req.penalties.logit_bias):
            raise ValueError(f"logit_bias ids must be in [0, {self.model.cfg.vocab})")
        if req.sampling.min_p > 0.0 and not self.min_p:
            raise ValueError("min_p needs an engine built with min_p=True (--min-p) on the graph-captured HIP step")
        if req.guide is not None:
            if self._gd is None:
                raise ValueError("a guide needs an engine built with guided=True (--guided) on the graph-captured "
                                 "HIP step")
            if req.guide.vocab != self.model.cfg.vocab:
                raise ValueError(f"the guide was compiled for a vocabulary of {req.guide.vocab}, the model has "
                                 f"{self.model.cfg.vocab}")
            if req.guide.n_states > self._gd.tables.states:
                raise ValueError(f"the guide has {req.guide.n_states} states, the arena holds "
                                 f"{self._gd.tables.states} (--guided-states)")
        self.pending.put(req)
        self._wake.set()
        return req

    def stop(self):
        self._stop.set()
        self._wake.set()
        self.thread.join(timeout=10)

    guide_uploads = property(lambda self: self._gd.uploads)  # tables copied into the arena
    guide_shared = property(lambda self: self._gd.shared)  # guided requests that found their table resident

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
        if req.guide is not None and not self._gd.reserve(req):
            self._held = req
            return None
        return req

    @staticmethod
    def _resident(s: dict) -> list:
        """Token ids of the rows of ``s``'s slot that are valid once the queued
        work has run: the known ids (prompt, then drained outputs) as far as rows
        were launched."""
        return s["known"][:min(s["pos"], len(s["known"]))]

    def _choose(self, free: list, ids: list, req: Request):
        """Where ``_admit`` puts ``req``: (slot, cached rows, slot to copy them from or
        None). With the prefix cache the rule of the class docstring."""
        if not self.prefix_cache:
            return free[0], 0, None
        m, src = 0, None
        for i, s in enumerate(self._kv):
            if s is None or req.embed is not None:  # an embed request pools every row: it takes no prefix
                continue
            n = min(_common_prefix(ids, self._resident(s)), len(ids) - 1)
            if n >= self.prefix_min and (n > m or (n == m and self.slots[i] is None and self.slots[src] is not None)):
                m, src = n, i
        if src is not None and self.slots[src] is None:
            return src, m, None  # in place
        return min(free, key=lambda i: (self._kv[i] is not None, self._freed[i])), m, src

    def _admit(self):
        """Queued requests into free slots, in queue order, until either runs out."""
        if self.prefix_cache:
            for i, s in enumerate(self.slots):
                if s is None and self._was_busy[i]:
                    self._was_busy[i] = False
                    self._tick += 1
                    self._freed[i] = self._tick
        free = [i for i, s in enumerate(self.slots) if s is None]
        jobs = []
        max_seq, V = self.model.cfg.max_seq, self.model.cfg.vocab
        if self._gd is not None:
            self._gd.release(self.slots)
        while free:
            req = self._take()
            if req is None:
                break
            # max_new is clamped so prompt + generated rows fit max_seq; a prompt too long for the rest keeps its end
            # (for a chat, the latest turns and the generation prompt). An embed request generates nothing: the
            # prompt's head, up to the cache's rows.
            req.max_new = max(1, min(req.max_new, max_seq - 2))
            cut = req.prompt[:max_seq - 1] if req.embed is not None else req.prompt[-(max_seq - req.max_new - 1):]
            ids = [t % V for t in cut] or [0]
            slot, m, src = self._choose(free, ids, req)
            free.remove(slot)
            if src is not None:
                jobs.append((src, slot, m))
            self.slots[slot] = s = {"req": req, "pos": m, "ids": ids, "gen": 0, "embed": req.embed}
            if self.prefix_cache:  # the slot's residency (``_resident``): ``_drain`` adds the outputs to ``known``
                s["known"] = list(ids)
                self._kv[slot] = req.kv = s
                self._was_busy[slot] = True
            req.cached_tokens = m
            if self._pen is not None:
                self._pen.reset(slot, req, ids)
            if self._gd is not None:
                self._gd.bind(slot, req)
            if m:
                self.prefix_hits += 1
                self.cached_tokens += m
        # One launch per up to MAX_KV_COPY_JOBS jobs, in admission order; a job that reads a slot an earlier job of
        # the launch writes (or the reverse) starts the next launch, so within one no slot is source and destination.
        launch: list = []
        for job in jobs + [None]:
            if launch and (job is None or len(launch) >= _MAX_COPY_JOBS or
                           any(job[0] == d or job[1] in (a, d) for a, d, _ in launch)):
                self.model.kv_copy(launch)
                self.kv_copies += len(launch)
                launch = []
            if job is not None:
                launch.append(job)

    def _plan(self, batch: list):
        """Rows of the next step (``_Row``), with the host-side state advanced
        past them (it does not depend on the tokens) and the emitting rows'
        (row, req, finished, token index) list."""
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
                rows.append(_Row(i, s["ids"][p], p, 0, p == len(s["ids"]) - 1 and not s["embed"]))
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
        slots) -> (ids, logits)``, the stages of ``_posts`` that the flags name
        over the leading ``sample_rows`` rows, last-token scatter, ids -> pinned
        staging."""
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
                                      din[_SLOT], din[self._pen_rows], self._pen.state, self._pen.bias_n, self._pen.bias_ids,
                                      self._pen.bias_val)
            if guide:
                drawn = ops.guide_(drawn, self._work[b.rows], ids[:sample_rows], tok[:sample_rows], din[_DEC],
                                   din[_SLOT], self._gd.base, self._gd.cur, self._gd.arena)
            (ops.sample_minp_ if self.min_p else ops.sample_)(drawn, ids[:sample_rows], din[self._smp])
            if logprobs:
                ops.logprobs_(logits[:sample_rows], ids[:sample_rows], din[self._lp], b.d_lp[:sample_rows],
                              b.d_lp_ids[:sample_rows])
                b.h_lp.copy_(b.d_lp, non_blocking=True)
                b.h_lp_ids.copy_(b.d_lp_ids, non_blocking=True)
        self._d_last.index_copy_(0, d[_REC], ids)
        b.h_out[:n].copy_(ids, non_blocking=True)

    def _capture(self, b: _StepBuf, emit_rows: int, post: int):
        """The step on all of ``b``'s rows through ``step_rows``, as a hipGraph;
        ``post``: what follows the fused step (see ``_posts``)."""
        from p2p_llm_tunnel_amd.models.tiny_llm import capture
        b.np[:] = 0
        b.np[_SLOT, :] = b.np[_REC, :] = self.model.scratch_slot  # warm-up and capture touch the scratch slot only
        run = functools.partial(self.model.step_rows, emit_rows=emit_rows)
        st = self._posts[post]
        sample_rows = (emit_rows or b.rows) if st & _SAMPLE else 0
        graph, _ = capture(lambda: self._step_body(b, b.rows, run, sample_rows, bool(st & _LOGPROBS),
                                                   bool(st & _PENALIZE), bool(st & _GUIDE)), self.device)
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
        smp, lp = self._smp, self._lp
        h[smp, :] = 0  # greedy unless an emitting row samples
        h[lp, :] = 0  # no logprobs unless an emitting row's request asks
        need = 0  # the stages this step's emitting rows need: its post is the lowest that runs them all
        for r, req, _, ctr in emits:
            if not req.sampling.greedy:
                h[smp, r] = req.sampling.column(ctr, self.min_p)
                need |= _SAMPLE
            if req.logprobs is not None:
                h[lp, r] = 1 + req.logprobs
                need |= _LOGPROBS
        if self._pen is not None:
            h[self._pen_rows, :] = 0  # every row off unless its request has penalties
            for r, req, _, _ in emits:
                if req.penalties is not None:
                    h[self._pen_rows, r] = req.penalties.column()
                    need |= _PENALIZE
        if self._gd is not None and any(req.guide is not None for _, req, _, _ in emits):
            need |= _GUIDE
        if n < R:  # padding rows: scratch slot, nothing recorded
            h[_TOK, n:R] = h[_POS, n:R] = h[_DEC, n:R] = 0
            h[_SLOT, n:R] = h[_REC, n:R] = scratch
        b.n, b.emits = n, emits
        if self.use_graph:
            self._graphs[(R, par, self._post_for[need])].replay()
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
                if batch and self.deliver is not None:
                    self.deliver(batch)
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
