"""Streaming inference: ``DialogueStream`` labels the utterance that has just arrived, for many live dialogues at once.

Under a causal context band ``(past, 0)`` (``M2FNet(config, context=(past, 0))``) the K and V rows of an utterance at every attention
site - both modality encoders, every fusion layer - depend on earlier utterances only and never change once computed.  A stream keeps
them in per-site caches on the device, so one step costs one row per dialogue where ``forward`` over the prefix costs the whole prefix
again.  The arithmetic runs in the gfx950 kernels behind ``runtime.StreamPlan`` (``csrc/attention_stream.hip`` for the attention, the
eval plan's own GEMM / LayerNorm / classifier launches for the rest); this module is plumbing.  The reference has no counterpart.

A history - a dialogue joined in progress, a session moved to another process, the refill after ``reset()`` - is loaded with
``prefill``: up to ``max_chunk`` utterances per slot and call through ``runtime.StreamChunkPlan`` (``csrc/attention_stream_chunk.hip``),
which writes the same cache rows as that many steps at the cost of one forward over the chunk.

PAGED CACHES (``model.stream(..., pages=N, page_rows=16)``): a dense stream reserves ``capacity`` rows per slot and site whether or not
the dialogue ever fills them.  A paged stream allocates cache rows in pages of ``page_rows`` from one pool of N pages per site through
a per-slot page table, so memory follows the utterances actually cached and ``max_streams`` can be in the thousands.  The allocation
lives here on the host (``PageAllocator``), next to the mirrored lengths; the table travels to the device with the inputs, only when it
changed.  The kernels are the paged forms in the same two files and give the dense stream's bits.
"""
from __future__ import annotations

import heapq
from typing import List, Optional, Sequence

import torch

from . import runtime
from .layout import M2FConfig

MAX_CAPACITY = 512
MAX_CHUNK = 64
PAGE_ROWS = (16, 32, 64)


def resolve_max_chunk(max_chunk) -> int:
    """1 (no chunk plan: ``prefill`` goes through ``step``) or 2 .. 64 utterances per slot and chunk call; ValueError otherwise."""
    if isinstance(max_chunk, bool) or not isinstance(max_chunk, int) or not 1 <= max_chunk <= MAX_CHUNK:
        raise ValueError(f"stream: max_chunk must be an integer in 1 .. {MAX_CHUNK}, got {max_chunk!r}")
    return max_chunk


def chunk_schedule(counts: Sequence[int], T: int) -> List[List[int]]:
    """How ``prefill`` feeds ``counts[s]`` utterances per slot in chunks of at most T: ceil(max(counts) / T) calls, call i giving slot s
    clamp(counts[s] - i * T, 0, T) rows.  Every entry is <= T and the entries of a slot sum to its count."""
    if T < 1:
        raise ValueError(f"chunk_schedule: T >= 1 required, got {T}")
    counts = [int(c) for c in counts]
    if any(c < 0 for c in counts):
        raise ValueError(f"chunk_schedule: counts must be >= 0, got {counts}")
    calls = (max(counts, default=0) + T - 1) // T
    return [[min(max(c - i * T, 0), T) for c in counts] for i in range(calls)]


def check_prefill_fits(lengths: Sequence[int], counts: Sequence[int], capacity: int, past: Optional[int]) -> None:
    """A stream without a window holds at most ``capacity`` utterances per slot: RuntimeError if a slot's history would pass it -
    checked for the whole call before anything is launched."""
    if past is not None:
        return
    full = [s for s, (n, c) in enumerate(zip(lengths, counts)) if c > 0 and n + c > capacity]
    if full:
        raise RuntimeError(f"DialogueStream.prefill: slot(s) {full} would pass {capacity} utterances, the capacity of a stream without a "
                           "window (context past=None); reset() the slot, or stream under a window (past, 0)")


def prefix_counts(valid: torch.Tensor) -> Optional[List[int]]:
    """valid bool [B, L] (True = an utterance): the per-dialogue lengths if every row is a valid prefix followed by padding (the collate
    layout), else None."""
    n = valid.sum(1)
    L = valid.shape[1]
    if torch.equal(valid, torch.arange(L)[None, :] < n[:, None]):
        return n.tolist()
    return None


def resolve_capacity(past: Optional[int], capacity: Optional[int]) -> int:
    """Rows per slot and site: ``past + 1`` for a window (a given value below it is raised to it), 512 without one; ValueError outside
    1 .. 512."""
    if capacity is None:
        capacity = MAX_CAPACITY if past is None else past + 1
    if isinstance(capacity, bool) or not isinstance(capacity, int):
        raise ValueError(f"stream: capacity must be an integer in 1 .. {MAX_CAPACITY}, got {capacity!r}")
    if past is not None and 1 <= capacity < past + 1:
        capacity = past + 1
    if not 1 <= capacity <= MAX_CAPACITY:
        raise ValueError(f"stream: capacity must be in 1 .. {MAX_CAPACITY} rows per slot, got {capacity}"
                         + (f" (a window of past = {past} needs {past + 1})" if past is not None else ""))
    return capacity


def cache_bytes(cfg: M2FConfig, max_streams: int, capacity: int, bf16: bool = False) -> int:
    """2 * sum over attention sites of pad(d_site) * S * C * element size: K and V, every encoder layer of every stack and every
    fusion layer; pad(d_site) = heads * head dim padded to 4 floats (fp32 caches, 4 B) or 8 bf16 values (bf16 mode, 2 B)."""
    q, esize = (8, 2) if bf16 else (4, 4)
    pad = lambda d, h: h * ((d // h + q - 1) // q * q)          # noqa: E731
    width = 0
    if cfg.audio_enabled:
        width += cfg.ntrans_audio * cfg.nlayers_audio * pad(cfg.d_audio, cfg.nhead_audio)
    if cfg.text_enabled:
        width += cfg.ntrans_text * cfg.nlayers_text * pad(cfg.d_text, cfg.nhead_text)
    if cfg.fam_enabled:
        width += cfg.nlayers_fam * pad(cfg.d_fam, cfg.nhead_fam)
    return 2 * width * max_streams * capacity * esize


def resolve_pages(pages, page_rows):
    """(None, page_rows): a dense stream; (pages >= 1, page_rows in 16 / 32 / 64): a paged one; ValueError otherwise."""
    if isinstance(page_rows, bool) or page_rows not in PAGE_ROWS:
        raise ValueError(f"stream: page_rows must be one of {PAGE_ROWS}, got {page_rows!r}")
    if pages is None:
        return None, page_rows
    if isinstance(pages, bool) or not isinstance(pages, int) or pages < 1:
        raise ValueError(f"stream: pages must be None (dense caches) or an integer >= 1, got {pages!r}")
    return pages, page_rows


def _pages_of(rows: int, page_rows: int) -> int:
    return (rows + page_rows - 1) // page_rows


def pages_needed(lengths: Sequence[int], new: Sequence[int], capacity: int, page_rows: int, ring: bool) -> List[int]:
    """Pages each slot GAINS when it takes ``new[s]`` utterances on top of ``lengths[s]``: a slot holds ceil(rows / page_rows) pages for
    its rows = min(utterances, capacity) live cache rows - on a ring the rows are recycled once ``capacity`` are in use, so a slot never
    holds more than ceil(capacity / page_rows).  A plain cache cannot pass its capacity: ValueError."""
    out = []
    for s, (n, a) in enumerate(zip(lengths, new)):
        if not ring and n + a > capacity:
            raise ValueError(f"pages_needed: slot {s} would hold {n + a} utterances, past the capacity {capacity} of a plain cache")
        out.append(_pages_of(min(n + a, capacity), page_rows) - _pages_of(min(n, capacity), page_rows))
    return out


def cache_bytes_paged(cfg: M2FConfig, pages: int, page_rows: int, bf16: bool = False) -> int:
    """Bytes of every site's K and V pools: ``cache_bytes`` with ``pages * page_rows`` rows in place of ``max_streams * capacity``."""
    return cache_bytes(cfg, pages, page_rows, bf16)


class PageAllocator:
    """Which page holds which rows, on the host.  ``pages`` ids 0 .. pages - 1, shared by every attention site; the lowest free id is
    handed out first, so a run is reproducible.  ``slot_pages[s]`` lists slot s's pages in logical order - entry e holds its cache rows
    e * page_rows .. - and ``table`` (CPU int32 [slots, ceil(capacity / page_rows)]) carries the same ids for the device; entries past a
    slot's list are stale and never read.  ``dirty`` is set whenever the table changed since it was last cleared."""

    def __init__(self, pages: int, slots: int, capacity: int, page_rows: int):
        self.pages, self.slots, self.capacity, self.page_rows = int(pages), int(slots), int(capacity), int(page_rows)
        self._free = list(range(self.pages))               # a heap: the lowest id first
        self.slot_pages: List[List[int]] = [[] for _ in range(self.slots)]
        self.table = torch.zeros(self.slots, _pages_of(self.capacity, self.page_rows), dtype=torch.int32)
        self.dirty = False

    @property
    def pages_free(self) -> int:
        return len(self._free)

    def shortfall(self, need: Sequence[int]) -> List[int]:
        """The slots that would go without a page if ``need[s]`` pages were taken in slot order ([]: everything fits)."""
        left, short = len(self._free), []
        for s, n in enumerate(need):
            if n > left:
                short.append(s)
            left -= min(n, left)
        return short

    def take(self, need: Sequence[int], what: str = "PageAllocator.take") -> None:
        """Gives slot s ``need[s]`` more pages.  All or nothing: RuntimeError naming the slots left short, nothing changed."""
        need = [int(n) for n in need]
        if len(need) != self.slots or any(n < 0 for n in need):
            raise ValueError(f"{what}: one count >= 0 per slot required")
        width = self.table.shape[1]
        over = [s for s, n in enumerate(need) if len(self.slot_pages[s]) + n > width]
        if over:
            raise ValueError(f"{what}: slot(s) {over} would hold more than {width} pages, the {self.capacity} rows of a slot")
        short = self.shortfall(need)
        if short:
            raise RuntimeError(f"{what}: slot(s) {short} need a cache page and the pool has {len(self._free)} free of {self.pages} "
                               f"({sum(need)} needed); reset() finished dialogues or open the stream with more pages")
        for s, n in enumerate(need):
            for _ in range(n):
                page = heapq.heappop(self._free)
                self.table[s, len(self.slot_pages[s])] = page
                self.slot_pages[s].append(page)
                self.dirty = True

    def release(self, slots: Optional[Sequence[int]] = None) -> None:
        """Returns the pages of those slots (None: of every slot) to the pool."""
        for s in range(self.slots) if slots is None else slots:
            for page in self.slot_pages[s]:
                heapq.heappush(self._free, page)
            self.slot_pages[s] = []


class DialogueStream:
    """``model.stream(max_streams, capacity=None, use_graph=True, max_chunk=1, pages=None, page_rows=16)``: ``max_streams``
    slots, each one live dialogue.

    ``step(text [S, d_t], audio [S, d_a], active=None) -> logits [S, C_out]`` takes ONE new utterance per active slot and returns a
    fresh tensor with its logits (zero rows at inactive slots).  ``active`` is a host-side bool sequence or CPU tensor (None: every
    slot); the lengths are mirrored on the host (``lengths``), so nothing waits for the device.  With ``use_graph`` a step is one
    captured hipGraph, replayed unchanged while the dialogues grow: inputs, mask and counts live in device buffers.

    Caches: per attention site K and V as ``[S][H][capacity][pad(hd)]`` (fp32; bf16 mode: bf16, rounded once), together
    ``2 * sum_sites pad(d_site) * S * capacity * 4 B`` (``cache_bytes``; bf16 mode: 2 B) - at C3 width, S = 64, capacity 512 that is
    3.8 GB in fp32.  With a window ``(past, 0)`` the cache is a ring of ``past + 1`` rows and a dialogue has no length limit; with
    ``past=None`` a slot holds at most ``capacity`` (<= 512) utterances and the step that would pass it raises RuntimeError before
    anything is launched.

    ``reset(slots=None)`` starts new dialogues in those slots (stale rows are never read: the live count comes from the length).
    THE CACHES BELONG TO THE WEIGHTS THAT WROTE THEM: after ``load_state_dict``, an optimizer step or ``averaged_parameters()`` call
    ``reset()`` before the next step.

    ``prefill(text [S, n, d_t], audio [S, n, d_a], counts=None) -> logits [S, n, C_out]`` loads a history: slot s takes its first
    ``counts[s]`` rows (None: n for every slot, 0: the slot is untouched) and is left exactly as ``counts[s]`` steps would leave it -
    same cache rows, same length - ready for ``step``; logits are zero at rows past the count.  With ``max_chunk = T`` in 2 .. 64 the
    rows go through the chunk plan in ceil(n / T) calls of at most T rows per slot (``chunk_schedule``), each one captured graph of a
    forward over S * T rows; with the default ``max_chunk = 1`` it goes through ``step``.  On a stream without a window a history that
    would pass the capacity raises RuntimeError before anything is launched.  ``run`` feeds T columns per call when the batch has
    the collate layout (every dialogue a valid prefix followed by padding).

    PAGED: with ``pages = N`` every site holds pools ``[N][H][page_rows][pad(hd)]`` instead (``cache_bytes_paged``) and a slot takes a
    page from the shared pool whenever its next row crosses a page boundary (``PageAllocator``; ``pages_free`` tells what is left);
    ``reset`` returns a slot's pages.  Everything above holds unchanged and the logits are the dense stream's bits.  A ``step``,
    ``prefill`` or ``run`` that would need more pages than are free raises RuntimeError naming the slots before anything is launched
    or allocated, and leaves the stream exactly as it was."""

    def __init__(self, model, max_streams: int, capacity: int, use_graph: bool = True, max_chunk: int = 1,
                 pages: Optional[int] = None, page_rows: int = 16):
        self.model, self.use_graph = model, bool(use_graph)
        self.max_streams, self.capacity = int(max_streams), int(capacity)
        self.max_chunk = resolve_max_chunk(max_chunk)
        self.past = model.context[0]
        eng = model.engine()
        self._eng = eng
        cfg = eng.cfg
        if cfg.dropout != 0.0:
            cfg = M2FConfig(**{**cfg.__dict__, "dropout": 0.0})
        self.pages, self.page_rows = resolve_pages(pages, page_rows)
        self.plan = runtime.StreamPlan(cfg, self.max_streams, self.capacity, self.past, eng.precision, eng.flat, eng.wshadow,
                                       self.pages, self.page_rows)
        self.allocator = PageAllocator(self.pages, self.max_streams, self.capacity, self.page_rows) if self.pages else None
        self.chunk_plan = runtime.StreamChunkPlan(self.plan, self.max_chunk, eng.flat, eng.wshadow) if self.max_chunk > 1 else None
        self.lengths: List[int] = [0] * self.max_streams
        self._active_host: Optional[List[bool]] = None        # what the device's mask holds (None: not written yet)
        self._new_host: Optional[List[int]] = None            # ... and the chunk plan's per-slot row counts

    # -- plumbing ----------------------------------------------------------------------------------------------------------------
    def _on_stream(self, body):
        eng = self._eng
        cur = torch.cuda.current_stream(eng.device)
        eng.stream.wait_stream(cur)                        # (hipGraph capture is illegal on the default stream)
        with torch.cuda.stream(eng.stream):
            out = body()
        cur.wait_stream(eng.stream)
        return out

    def _mask(self, active, n: int) -> List[bool]:
        if active is None:
            return [True] * n
        if isinstance(active, torch.Tensor):
            if active.is_cuda:
                raise ValueError("stream.step: `active` is a host-side mask (a bool sequence or a CPU tensor)")
            active = active.reshape(-1).tolist()
        act = [bool(a) for a in active]
        if len(act) != n:
            raise ValueError(f"stream.step: `active` needs {n} entries, got {len(act)}")
        return act

    def _refuse_training(self, what: str) -> None:
        if self.model.training and self.model.m2f_config.dropout > 0.0:
            raise RuntimeError(f"DialogueStream.{what}: the model is in training mode with dropout > 0; a stream scores the model "
                               "without dropout - call model.eval() first")

    @property
    def pages_free(self) -> Optional[int]:
        """Free pages of a paged stream's pool (None: a dense stream)."""
        return None if self.allocator is None else self.allocator.pages_free

    def _reserve(self, new: Sequence[int], what: str) -> None:
        """Paged: the pages the slots need for ``new[s]`` more utterances each, beyond what they hold - all of them or RuntimeError."""
        al = self.allocator
        if al is None:
            return
        gain = pages_needed(self.lengths, new, self.capacity, self.page_rows, self.past is not None)
        held = pages_needed([0] * self.max_streams, self.lengths, self.capacity, self.page_rows, True)
        al.take([max(0, h + g - len(p)) for h, g, p in zip(held, gain, al.slot_pages)], f"DialogueStream.{what}")

    def _send_table(self) -> None:
        """(inside _on_stream) the page table travels with the inputs, only when it changed"""
        al = self.allocator
        if al is not None and al.dirty:
            self.plan.table.copy_(al.table, non_blocking=True)
            al.dirty = False

    def _step(self, text, audio, act: List[bool]) -> torch.Tensor:
        """act: one entry per slot (rows of text / audio may be fewer: the leading slots)."""
        self._refuse_training("step")
        if self.past is None:
            full = [s for s, a in enumerate(act) if a and self.lengths[s] >= self.capacity]
            if full:
                raise RuntimeError(f"DialogueStream.step: slot(s) {full} already hold {self.capacity} utterances, the capacity of a "
                                   "stream without a window (context past=None); reset() the slot, or stream under a window (past, 0)")
        self._reserve([int(a) for a in act], "step")
        pl, cfg, eng = self.plan, self.plan.cfg, self._eng

        def body():
            self._send_table()
            for buf, x, on, name in ((pl.text_in, text, cfg.text_enabled, "text"), (pl.audio_in, audio, cfg.audio_enabled, "audio")):
                if not on:
                    continue
                if x is None:
                    raise ValueError(f"stream.step: {name} is enabled in this model and must be given")
                buf[: x.shape[0]].copy_(x.detach().reshape(x.shape[0], -1), non_blocking=True)
            if act != self._active_host:                   # the mask travels with the inputs (only when it changes)
                pl.active.copy_(torch.tensor(act, dtype=torch.uint8), non_blocking=True)
                self._active_host = list(act)
            fresh = eng.shadows_fresh()
            pl.params_fresh(fresh)
            pl.step(self.use_graph)
            if pl.shared_shadow and not fresh:
                eng.mark_shadows_fresh()                   # (a step that ran the parameter casts leaves the shared shadows current)
            if all(act):
                return pl.logits.clone()
            return torch.where(pl.active[:, None] != 0, pl.logits, torch.zeros((), dtype=pl.logits.dtype, device=pl.logits.device))

        out = self._on_stream(body)
        for s, a in enumerate(act):
            if a:
                self.lengths[s] += 1
        return out

    # -- public surface ----------------------------------------------------------------------------------------------------------
    def step(self, text: Optional[torch.Tensor], audio: Optional[torch.Tensor], active: Optional[Sequence[bool]] = None) -> torch.Tensor:
        S = self.max_streams
        for x, name in ((text, "text"), (audio, "audio")):
            if x is not None and (x.dim() != 2 or x.shape[0] != S):
                raise ValueError(f"stream.step: {name} must be [max_streams = {S}, d], got {tuple(x.shape)}")
        return self._step(text, audio, self._mask(active, S))

    def _chunk(self, text, audio, new: List[int], first: int) -> torch.Tensor:
        """One chunk call: slot s takes rows first .. first + new[s] - 1 of text / audio ([B, n, d], B <= S leading slots).  Returns the
        chunk plan's logits [S, T, C_out] as a fresh tensor, zeros at the rows past new[s]."""
        pl, cfg, eng, T = self.chunk_plan, self.chunk_plan.cfg, self._eng, self.max_chunk
        width = max(new)

        self._reserve(new, "prefill")

        def body():
            self._send_table()
            if new != self._new_host:                       # the counts travel with the inputs (only when they change)
                pl.new.copy_(torch.tensor(new, dtype=torch.int32), non_blocking=True)
                self._new_host = list(new)
            for buf, x, on in ((pl.text_in, text, cfg.text_enabled), (pl.audio_in, audio, cfg.audio_enabled)):
                if not on:
                    continue
                B = x.shape[0]
                buf.zero_()                                 # rows past a slot's count, slots not given: zeros whatever the caller holds there
                xs = x[:, first: first + width].detach().to(buf.device, non_blocking=True)
                rows = torch.arange(width, device=buf.device)[None, :] < pl.new[:B, None]
                buf[:B, :width].copy_(torch.where(rows[:, :, None], xs, torch.zeros((), dtype=xs.dtype, device=buf.device)), non_blocking=True)
            fresh = eng.shadows_fresh()
            pl.params_fresh(fresh)
            pl.prefill(self.use_graph)
            if pl.shared_shadow and not fresh:
                eng.mark_shadows_fresh()
            keep = torch.arange(T, device=pl.logits.device)[None, :] < pl.new[:, None]
            return torch.where(keep[:, :, None], pl.logits, torch.zeros((), dtype=pl.logits.dtype, device=pl.logits.device))

        out = self._on_stream(body)
        for s, n in enumerate(new):
            self.lengths[s] += n
        return out

    def prefill(self, text: Optional[torch.Tensor], audio: Optional[torch.Tensor], counts: Optional[Sequence[int]] = None) -> torch.Tensor:
        S = self.max_streams
        self._refuse_training("prefill")
        cfg = self.plan.cfg
        n = None
        for x, on, name in ((text, cfg.text_enabled, "text"), (audio, cfg.audio_enabled, "audio")):
            if not on:
                continue
            if x is None:
                raise ValueError(f"stream.prefill: {name} is enabled in this model and must be given")
            if x.dim() != 3 or x.shape[0] != S or (n is not None and x.shape[1] != n):
                raise ValueError(f"stream.prefill: {name} must be [max_streams = {S}, n, d], got {tuple(x.shape)}")
            n = x.shape[1]
        if counts is None:
            counts = [n] * S
        else:
            if isinstance(counts, torch.Tensor):
                if counts.is_cuda:
                    raise ValueError("stream.prefill: `counts` is host-side (an int sequence or a CPU tensor)")
                counts = counts.reshape(-1).tolist()
            counts = [int(c) for c in counts]
            if len(counts) != S or any(not 0 <= c <= n for c in counts):
                raise ValueError(f"stream.prefill: `counts` needs {S} entries in 0 .. {n}, got {counts}")
        check_prefill_fits(self.lengths, counts, self.capacity, self.past)
        self._reserve(counts, "prefill")                   # (the whole call's pages, before its first launch)
        return self._feed(text, audio, counts, n)

    def _feed(self, text, audio, counts: List[int], n: int) -> torch.Tensor:
        """counts: one entry per slot; text / audio [B, n, d] hold the leading B slots.  Returns logits [S, n, C_out]."""
        S, T = self.max_streams, self.max_chunk
        cfg = self.plan.cfg
        for x, on, name in ((text, cfg.text_enabled, "text"), (audio, cfg.audio_enabled, "audio")):
            if on and x is None:
                raise ValueError(f"stream: {name} is enabled in this model and must be given")
        out = torch.zeros(S, n, self.plan.cfg.cls_out, dtype=torch.float32, device=self._eng.device)
        if T == 1:
            for i in range(max(counts, default=0)):
                act = [c > i for c in counts]
                out[:, i] = self._step(None if text is None else text[:, i], None if audio is None else audio[:, i], act)
            return out
        for i, new in enumerate(chunk_schedule(counts, T)):
            w = max(new)
            out[:, i * T: i * T + w] = self._chunk(text, audio, new, i * T)[:, :w]
        return out

    def reset(self, slots: Optional[Sequence[int]] = None) -> None:
        S = self.max_streams
        if slots is None:
            self._on_stream(lambda: self.plan.reset(None))
            self.lengths = [0] * S
            if self.allocator is not None:
                self.allocator.release()
            return
        slots = [int(s) for s in slots]
        if any(not 0 <= s < S for s in slots):
            raise ValueError(f"stream.reset: slots must be in 0 .. {S - 1}")
        host = torch.zeros(S, dtype=torch.uint8)
        host[slots] = 1
        dev = self._eng.device

        def body():
            mask = host.to(dev)
            self.plan.reset(mask)
            mask.record_stream(torch.cuda.current_stream(dev))
        self._on_stream(body)
        for s in slots:
            self.lengths[s] = 0
        if self.allocator is not None:
            self.allocator.release(set(slots))

    def run(self, text: Optional[torch.Tensor], audio: Optional[torch.Tensor], mask: torch.Tensor) -> torch.Tensor:
        """A padded batch (text [B, L, d_t], audio [B, L, d_a], mask bool [B, L], True = pad; B <= max_streams) through the stream:
        resets the first B slots and feeds the batch column by column with ``active = ~mask[:, i]`` - or, on a stream with
        ``max_chunk = T > 1`` and a batch in the collate layout (every row a valid prefix followed by padding), T columns per call.
        Returns logits [B, L, C_out] with zeros at pad slots - what ``forward`` gives at the valid slots under the model's band.  Reads
        ``mask`` on the host once."""
        B, L = mask.shape
        S = self.max_streams
        if B > S:
            raise ValueError(f"stream.run: {B} dialogues do not fit {S} stream slots")
        self.reset(range(B))
        valid = (~mask.bool()).cpu()
        counts = prefix_counts(valid) if self.max_chunk > 1 else None
        if counts is not None:
            self._refuse_training("run")
            counts = counts + [0] * (S - B)
            check_prefill_fits(self.lengths, counts, self.capacity, self.past)
            self._reserve(counts, "run")
            return self._feed(text, audio, counts, L)[:B]
        if self.allocator is not None:                      # (the whole batch's pages, before its first step)
            rows = valid.sum(1).tolist() + [0] * (S - B)
            if self.past is None:
                check_prefill_fits(self.lengths, rows, self.capacity, self.past)
            self._reserve(rows, "run")
        out = torch.zeros(B, L, self.plan.cfg.cls_out, dtype=torch.float32, device=self._eng.device)
        for i in range(L):
            act = valid[:, i].tolist() + [False] * (S - B)
            if not any(act):
                continue
            logits = self._step(None if text is None else text[:, i], None if audio is None else audio[:, i], act)
            out[:, i] = logits[:B]
        return out

    def close(self) -> None:
        if self.plan is not None:
            torch.cuda.synchronize(self._eng.device)
            if self.chunk_plan is not None:                 # (it borrows the stream plan's caches: it goes first)
                self.chunk_plan.close()
                self.chunk_plan = None
            self.plan.close()
            self.plan = None
