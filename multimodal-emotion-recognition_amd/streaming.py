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

SNAPSHOTS (``snapshot`` / ``restore`` / ``evict`` / ``fork``): the caches are a dialogue's whole state and never change once written,
so its live cache rows plus its length are an exact checkpoint - restoring it gives the bits an uninterrupted stream gives, where a
``prefill`` recomputes (and under a window is not even exact from a truncated history).  A ``StreamSnapshot`` is one packed 1-D tensor
of the caches' element type (float32, or bfloat16 in bf16 mode) plus host-side lists.  Entry e holds the ``rows_e = min(length_e, C)``
live PHYSICAL cache rows 0 .. rows_e - 1 of its slot (a ring keeps its phase), laid out as the dense cache with C replaced by rows_e:

    [site in plan order][K, V][H][rows_e][pad(hd)]

and starts at element ``row_offsets[e] * W``, ``W = sum_sites 2 * H * pad(hd)`` (``cache_bytes(cfg, 1, 1, bf16)`` over the element size);
pad columns travel as they are (zeros) and every segment starts 16-byte aligned.  The format does not depend on dense or paged caches,
``page_rows``, ``max_streams`` or the slot number, so a dialogue moves freely between streams of the same model and window.  The rows
are copied by the gfx950 kernels of ``csrc/stream_cache.hip``, one launch for all sites and slots.
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


def logical_columns(length: int, capacity: int, ring: bool):
    """(first, count) of the columns of a stream's attention row once a slot has taken ``length`` utterances: column t is utterance
    ``first + t``, t < count, the last one the utterance that has just arrived.  A plain cache keeps every utterance (first = 0, count =
    length <= capacity); a ring keeps the last ``capacity`` of them.  Host arithmetic: what the logical order of the weights-emitting
    kernel (``csrc/attention_stream.hip``) means."""
    if isinstance(length, bool) or not isinstance(length, int) or length < 0:
        raise ValueError(f"logical_columns: length must be an integer >= 0, got {length!r}")
    if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
        raise ValueError(f"logical_columns: capacity must be an integer >= 1, got {capacity!r}")
    if not ring and length > capacity:
        raise ValueError(f"logical_columns: a plain cache of {capacity} rows cannot hold {length} utterances")
    count = min(length, capacity)
    return length - count, count


class StreamAttention:
    """What ``DialogueStream.attention`` returns: ``weights[name]`` - fp32 ``[S, C]`` (heads averaged) or ``[S, H, C]`` per attention
    site, column t of slot s = the weight of utterance ``first[s] + t`` in the prediction the last ``step`` made for slot s - with
    ``first`` (utterance index of column 0) and ``count`` (live columns; 0 for a slot that took no utterance in that step, whose row is
    zeros) per slot, both host lists.  Columns behind ``count`` are zeros."""

    def __init__(self, weights, first, count):
        self.weights, self.first, self.count = weights, list(first), list(count)


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

    def state(self) -> tuple:
        """A copy of the allocation (``set_state`` puts it back and marks the table as changed)."""
        return list(self._free), [list(p) for p in self.slot_pages], self.table.clone()

    def set_state(self, state: tuple) -> None:
        free, pages, table = state
        self._free, self.slot_pages = list(free), [list(p) for p in pages]
        self.table.copy_(table)
        self.dirty = True

    def replace_shortfall(self, slots: Sequence[int], need: Sequence[int]) -> List[int]:
        """The slots of ``slots`` that would go without a page if they returned the pages they hold and then took ``need[e]`` each, in
        the order given ([]: everything fits)."""
        left, short = len(self._free) + sum(len(self.slot_pages[s]) for s in slots), []
        for s, n in zip(slots, need):
            if n > left:
                short.append(s)
            left -= min(n, left)
        return short

    def replace(self, slots: Sequence[int], need: Sequence[int], what: str = "PageAllocator.replace") -> None:
        """Slot ``slots[e]`` (each listed once) gives up its pages and takes ``need[e]`` new ones, the lowest free id first.  All or
        nothing, decided before anything is released: free pages plus the pages those slots hold must cover the need, otherwise
        RuntimeError naming the slots left short and nothing changed."""
        slots, need = [int(s) for s in slots], [int(n) for n in need]
        width = self.table.shape[1]
        if len(slots) != len(need) or len(set(slots)) != len(slots) or any(not 0 <= s < self.slots for s in slots) \
                or any(not 0 <= n <= width for n in need):
            raise ValueError(f"{what}: distinct slots in 0 .. {self.slots - 1} with 0 .. {width} pages each required")
        short = self.replace_shortfall(slots, need)
        if short:
            held = sum(len(self.slot_pages[s]) for s in slots)
            raise RuntimeError(f"{what}: slot(s) {short} need cache pages the pool cannot give: {sum(need)} needed, {len(self._free)} free "
                               f"of {self.pages} and {held} held by the target slots; reset() finished dialogues, evict() idle ones or "
                               "open the stream with more pages")
        self.release(slots)
        full = [0] * self.slots
        for s, n in zip(slots, need):
            full[s] = n
        self.take(full, what)


def config_sites(cfg: M2FConfig) -> List[tuple]:
    """(H, hd) of every attention site of the model, encoders first (audio, text), then the fusion layers.  The ORDER of a snapshot's
    segments is the plan's (``runtime.StreamPlan.snapshot_sites``: launches are merged across the encoders); this list is the same sites
    and serves the sums that do not depend on the order."""
    sites = []
    if cfg.audio_enabled:
        sites += [(cfg.nhead_audio, cfg.d_audio // cfg.nhead_audio)] * (cfg.ntrans_audio * cfg.nlayers_audio)
    if cfg.text_enabled:
        sites += [(cfg.nhead_text, cfg.d_text // cfg.nhead_text)] * (cfg.ntrans_text * cfg.nlayers_text)
    if cfg.fam_enabled:
        sites += [(cfg.nhead_fam, cfg.d_fam // cfg.nhead_fam)] * cfg.nlayers_fam
    return sites


def _pad_hd(hd: int, bf16: bool) -> int:
    q = 8 if bf16 else 4
    return (hd + q - 1) // q * q


def snapshot_row_elems(sites: Sequence[Sequence[int]], bf16: bool) -> int:
    """W: the elements one cached utterance takes in a snapshot - K and V of every site, heads padded as in the caches."""
    return sum(2 * H * _pad_hd(hd, bf16) for H, hd in sites)


def snapshot_rows(lengths: Sequence[int], ring: Optional[int]) -> List[int]:
    """Live cache rows per entry: the length itself on a plain cache, min(length, ring capacity) on a ring."""
    return [int(n) if ring is None else min(int(n), ring) for n in lengths]


def snapshot_row_offsets(rows: Sequence[int]) -> List[int]:
    """First packed row of each entry: the exclusive running sum of the entries' rows."""
    out, at = [], 0
    for r in rows:
        out.append(at)
        at += r
    return out


def snapshot_segments(sites: Sequence[Sequence[int]], bf16: bool, rows: Sequence[int]) -> List[List[tuple]]:
    """segments[e][i] = (start, elements) of the i-th (site, K / V, head) segment of entry e in the packed tensor, i running over
    [site][K, V][H]: each holds rows[e] * pad(hd) elements, rows major."""
    W = snapshot_row_elems(sites, bf16)
    out = []
    for r, off in zip(rows, snapshot_row_offsets(rows)):
        at, segs = off * W, []
        for H, hd in sites:
            for _ in range(2 * H):
                segs.append((at, r * _pad_hd(hd, bf16)))
                at += r * _pad_hd(hd, bf16)
        out.append(segs)
    return out


def make_signature(sites, bf16: bool, past: Optional[int], capacity: int) -> tuple:
    """What a snapshot and the stream that takes it must share: the (H, hd) of every site in plan order, the precision, the window and -
    under a window - the ring capacity (None for a plain cache, whose snapshots fit any capacity that holds them)."""
    return (tuple((int(H), int(hd)) for H, hd in sites), bool(bf16), None if past is None else int(past),
            None if past is None else int(capacity))


def check_restore_slots(slots: Sequence[int], entries: int, max_streams: int) -> List[int]:
    """One target slot per entry, each in range and listed once: ValueError otherwise."""
    slots = [int(s) for s in slots]
    if len(slots) != entries:
        raise ValueError(f"stream.restore: {entries} snapshot entries need {entries} slots, got {len(slots)}")
    if any(not 0 <= s < max_streams for s in slots):
        raise ValueError(f"stream.restore: slots must be in 0 .. {max_streams - 1}, got {slots}")
    if len(set(slots)) != len(slots):
        raise ValueError(f"stream.restore: a slot is listed twice in {slots}")
    return slots


def check_restore_fits(lengths: Sequence[int], slots: Sequence[int], capacity: int, past: Optional[int]) -> None:
    """A plain cache holds at most ``capacity`` utterances: RuntimeError naming the slots whose entry is longer."""
    if past is not None:
        return
    full = [s for s, n in zip(slots, lengths) if n > capacity]
    if full:
        raise RuntimeError(f"DialogueStream.restore: the entries for slot(s) {full} hold more than {capacity} utterances, the capacity of "
                           "this stream without a window (context past=None)")


class StreamSnapshot:
    """The cached state of some dialogues, out of a ``DialogueStream`` (module docstring: the format).  ``data``: the packed tensor;
    ``lengths``: the true utterance counts (a ring: the unwrapped count); ``row_offsets``: first packed row of each entry;
    ``signature``: ``make_signature`` of the stream that wrote it.  ``len(snap)`` entries, ``nbytes`` of payload, ``entry(e)`` its (K, V) views per site.  ``select(indices)``
    picks entries into a new snapshot, ``cpu(pin=False)`` / ``to(device)`` move the payload, ``state_dict()`` /
    ``StreamSnapshot.from_state_dict(d)`` hold tensors, ints and lists only (``torch.save`` / ``torch.load``).
    A SNAPSHOT BELONGS TO THE WEIGHTS THAT WROTE IT, like the caches it came from."""

    def __init__(self, data: torch.Tensor, lengths: Sequence[int], row_offsets: Sequence[int], signature: tuple, _ready=None,
                 speakers: Optional[torch.Tensor] = None, crf: Optional[torch.Tensor] = None):
        sites, bf16, past, ring = signature
        self.signature = make_signature(sites, bf16, past, 0 if ring is None else ring)
        self.lengths = [int(n) for n in lengths]
        self.row_offsets = [int(o) for o in row_offsets]
        rows = self.rows
        if any(n < 0 for n in self.lengths) or self.row_offsets != snapshot_row_offsets(rows):
            raise ValueError("StreamSnapshot: lengths must be >= 0 and row_offsets the running sum of the entries' rows")
        want = torch.bfloat16 if self.signature[1] else torch.float32
        if data.dim() != 1 or data.dtype != want or data.numel() != sum(rows) * self.row_elems:
            raise ValueError(f"StreamSnapshot: data must be a 1-D {want} tensor of {sum(rows) * self.row_elems} elements, "
                             f"got {data.dtype} {tuple(data.shape)}")
        self._data, self._ready = data, _ready
        # speaker ids of the cached utterances (a stream of a model with speaker heads; None otherwise): uint8 [sum(rows)], entry e's
        # rows at row_offsets[e] in the order of its packed rows - the slot's cache rows 0 .. rows_e - 1
        if speakers is not None and (speakers.dim() != 1 or speakers.dtype != torch.uint8 or speakers.numel() != sum(rows)):
            raise ValueError(f"StreamSnapshot: speakers must be a 1-D uint8 tensor of {sum(rows)} entries, got {speakers.dtype} {tuple(speakers.shape)}")
        self._speakers = speakers
        # the CRF filter's state of every entry (a stream made with crf=; None otherwise): fp32 [entries, C]
        if crf is not None and (crf.dim() != 2 or crf.dtype != torch.float32 or crf.shape[0] != len(self.lengths)):
            raise ValueError(f"StreamSnapshot: crf must be an fp32 tensor [{len(self.lengths)}, C], got {crf.dtype} {tuple(crf.shape)}")
        self._crf = crf

    @property
    def crf(self) -> Optional[torch.Tensor]:
        """The CRF filter's state of every entry, fp32 [entries, C] (None: the stream ran without crf=)."""
        if self._crf is not None and self._ready is not None:
            self._ready.synchronize()
            self._ready = None
        return self._crf

    @property
    def speakers(self) -> Optional[torch.Tensor]:
        if self._speakers is not None and self._ready is not None:
            self._ready.synchronize()
            self._ready = None
        return self._speakers

    @property
    def data(self) -> torch.Tensor:
        if self._ready is not None:                        # (an evicted snapshot: its copy to the host may still be under way)
            self._ready.synchronize()
            self._ready = None
        return self._data

    @property
    def rows(self) -> List[int]:
        return snapshot_rows(self.lengths, self.signature[3])

    @property
    def row_elems(self) -> int:
        return snapshot_row_elems(self.signature[0], self.signature[1])

    @property
    def nbytes(self) -> int:
        return self._data.numel() * self._data.element_size()

    def __len__(self) -> int:
        return len(self.lengths)

    def entry(self, e: int) -> List[tuple]:
        """Entry e as the caches see it: per site in plan order (K, V), each a view [H, rows_e, pad(hd)] of ``data``."""
        if not 0 <= int(e) < len(self):
            raise ValueError(f"StreamSnapshot.entry: entries are 0 .. {len(self) - 1}, got {e}")
        sites, bf16 = self.signature[0], self.signature[1]
        rows, data = self.rows, self.data
        segs = snapshot_segments(sites, bf16, rows)[int(e)]
        out, i = [], 0
        for H, hd in sites:
            kv = []
            for _ in range(2):
                start = segs[i][0]
                kv.append(data[start: start + H * segs[i][1]].view(H, rows[int(e)], _pad_hd(hd, bf16)))
                i += H
            out.append(tuple(kv))
        return out

    def select(self, indices: Sequence[int]) -> "StreamSnapshot":
        idx = [int(i) for i in indices]
        if any(not 0 <= i < len(self) for i in idx):
            raise ValueError(f"StreamSnapshot.select: indices must be in 0 .. {len(self) - 1}, got {idx}")
        W, rows, data = self.row_elems, self.rows, self.data
        parts = [data[self.row_offsets[i] * W: (self.row_offsets[i] + rows[i]) * W] for i in idx]
        picked = torch.cat(parts) if parts else data[:0]
        spk = self.speakers
        if spk is not None:
            sp = [spk[self.row_offsets[i]: self.row_offsets[i] + rows[i]] for i in idx]
            spk = torch.cat(sp) if sp else spk[:0]
        crf = self.crf
        if crf is not None:
            crf = crf[idx] if idx else crf[:0]
        return StreamSnapshot(picked, [self.lengths[i] for i in idx], snapshot_row_offsets([rows[i] for i in idx]), self.signature, speakers=spk,
                              crf=crf)

    def to(self, device) -> "StreamSnapshot":
        spk = self.speakers
        crf = self.crf
        return StreamSnapshot(self.data.to(device), self.lengths, self.row_offsets, self.signature, speakers=None if spk is None else spk.to(device),
                              crf=None if crf is None else crf.to(device))

    def cpu(self, pin: bool = False) -> "StreamSnapshot":
        data = self.data
        if pin and not data.is_pinned():
            host = torch.empty(data.shape, dtype=data.dtype, pin_memory=True)
            host.copy_(data)
            data = host
        else:
            data = data.cpu()
        spk = self.speakers
        crf = self.crf
        return StreamSnapshot(data, self.lengths, self.row_offsets, self.signature, speakers=None if spk is None else spk.cpu(),
                              crf=None if crf is None else crf.cpu())

    def state_dict(self) -> dict:
        sites, bf16, past, ring = self.signature
        d = {"data": self.data, "lengths": list(self.lengths), "row_offsets": list(self.row_offsets),
             "sites": [[H, hd] for H, hd in sites], "bf16": int(bf16), "past": -1 if past is None else past,
             "ring": -1 if ring is None else ring}
        if self._speakers is not None:                     # (only a snapshot WITH speakers extends the dictionary)
            d["speakers"] = self.speakers
        if self._crf is not None:                          # (likewise)
            d["crf"] = self.crf
        return d

    @classmethod
    def from_state_dict(cls, d: dict) -> "StreamSnapshot":
        past = None if int(d["past"]) < 0 else int(d["past"])
        ring = None if int(d["ring"]) < 0 else int(d["ring"])
        if (past is None) != (ring is None):
            raise ValueError("StreamSnapshot.from_state_dict: a window and a ring capacity come together")
        return cls(d["data"], d["lengths"], d["row_offsets"], (tuple((int(H), int(hd)) for H, hd in d["sites"]), bool(d["bf16"]), past, ring),
                   speakers=d.get("speakers"), crf=d.get("crf"))


class DialogueStream:
    """``model.stream(max_streams, capacity=None, use_graph=True, max_chunk=1, pages=None, page_rows=16, attention=False)``:
    ``max_streams`` slots, each one live dialogue.

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
    or allocated, and leaves the stream exactly as it was.

    SNAPSHOTS: ``snapshot(slots=None) -> StreamSnapshot`` copies the live cache rows and lengths of those slots (None: every slot; a
    slot of length 0 gives an empty entry) into one packed device tensor, sized from the host-mirrored lengths; the stream is unchanged.
    ``restore(snap, slots=None)`` puts entry e into ``slots[e]`` (None: slots 0 .. len(snap) - 1), which are then exactly as the source
    slots were - same cache rows, same ``lengths``, same device counts - whatever they held before; an empty entry resets its slot.
    The source may have been dense or paged, of another ``max_streams``, ``page_rows`` or slot, and - without a window - of another
    capacity that holds the dialogue.  Refused before anything is released or launched: a snapshot of another site geometry,
    precision, ``past`` or ring capacity (ValueError), duplicate or out-of-range slots (ValueError), on a plain cache a length above
    the capacity (RuntimeError), and on a paged stream a need the free pages plus the target slots' own pages cannot cover
    (RuntimeError naming the slots; the stream is left exactly as it was).  ``evict(slots)`` is ``snapshot(slots)`` copied to pinned
    host memory on the engine's stream, then ``reset(slots)``: on a paged stream the pages are free when it returns, and the copy is
    ordered before any later write of the stream.  ``fork(src, dst)`` is ``restore(snapshot([src]), [dst])``.  A SNAPSHOT BELONGS TO THE
    WEIGHTS THAT WROTE IT: the rule above for the caches holds for what was copied out of them.

    POSITION BIAS: the stream, and its chunk plan, take the model's distance-decay gain (``M2FNet.position_bias``) when they are created;
    ``position_bias`` reports it (the applied value, or None).  The new utterance is at distance 0 from itself, the cached ones at
    their distance in utterances; the caches of deeper layers depend on the gain as they depend on the weights.  After
    ``model.set_position_bias`` to another gain ``step`` / ``prefill`` / ``run`` / ``restore`` raise RuntimeError: ``reset()`` of the whole
    stream adopts the model's gain (every dialogue starts over), or build a new stream.  The snapshot format and its signature do
    not carry the gain: A SNAPSHOT BELONGS TO THE WEIGHTS AND THE GAIN THAT WROTE IT, and neither is checked.

    SPEAKER HEADS: a stream of a model with ``speaker_heads`` keeps, beside the K / V caches, ONE ``uint8 [S, capacity]`` array of the cached
    utterances' speaker ids for all sites, indexed by logical cache row (row ``u % capacity`` of a ring; dense on a paged stream too:
    1 B per row).  ``step(..., speakers=[S])``, ``prefill(..., speakers=[S, n])`` and ``run(..., speakers=[B, L])`` then REQUIRE the new
    utterances' ids (``runtime.speaker_ids``; a stream without the setting refuses them).  The new ids are stored inside the step /
    prefill graph by the launch that advances the counters, BEHIND the last attention launch: on a ring that store overwrites the id
    of the utterance that has just left the window, and every attention launch of the step - none reads the row the new utterance
    takes - has seen the old row set, the order the K / V rows have.  ``reset`` needs nothing new (stale ids are never read: the live
    count rules).  Snapshots carry the ids (``StreamSnapshot.speakers``); a snapshot with ids into a stream without, or the reverse,
    raises RuntimeError and leaves the stream untouched.  After ``model.set_speaker_heads`` to another setting the stream refuses to
    run until ``reset()`` of the whole stream, as after ``set_position_bias``.

    ATTENTION ROWS (``attention=True``): every step's attention launches run the weights-emitting form of their kernel and keep, per
    site, slot and head, the new utterance's row of probabilities over the cached ones (``sum_sites H * S * capacity * 4 B``; the same
    logits bit for bit, the step still one replayed graph).  ``attention(average_heads=True, sites=None)`` after a ``step`` returns
    them as a ``StreamAttention`` (``weights[site]`` ``[S, C]`` or ``[S, H, C]``, ``first``, ``count``): which cached utterances the
    prediction used."""

    def __init__(self, model, max_streams: int, capacity: int, use_graph: bool = True, max_chunk: int = 1,
                 pages: Optional[int] = None, page_rows: int = 16, attention: bool = False, crf=None):
        crf_block = None
        if crf is not None:                                 # (refused before anything is created)
            from .crf import check_step_args
            check_step_args("M2FNet.stream", crf, model.m2f_config.cls_out)
            crf_block = crf.block(model.engine().device).detach()
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
        self._bias: Optional[float] = model.position_bias     # (the applied gain or None; the chunk plan below takes the step plan's)
        if self._bias:
            self.plan.attention_bias(self._bias)
        self._spk = model.speaker_heads                        # (the chunk plan below takes the step plan's setting and cached ids)
        if self._spk:
            self.plan.stream_speakers(True)
            self.plan.attention_speakers(self._spk)
        self.allocator = PageAllocator(self.pages, self.max_streams, self.capacity, self.page_rows) if self.pages else None
        self.chunk_plan = runtime.StreamChunkPlan(self.plan, self.max_chunk, eng.flat, eng.wshadow) if self.max_chunk > 1 else None
        self.lengths: List[int] = [0] * self.max_streams
        self._active_host: Optional[List[bool]] = None        # what the device's mask holds (None: not written yet)
        self._new_host: Optional[List[int]] = None            # ... and the chunk plan's per-slot row counts
        self._signature: Optional[tuple] = None               # what a snapshot of this stream carries (read from the plan once)
        # attention rows (model.stream(..., attention=True)): the step's attention launches also store their probabilities
        self.attention_on = bool(attention)
        self._attn_act: Optional[List[bool]] = None           # the mask of the last step, while its rows are what the buffer holds
        if self.attention_on:
            self.plan.stream_attention(True)
        # the CRF's forward filter (model.stream(..., crf=module)): C floats per slot, whatever the window
        self.crf = crf
        self._phi: Optional[torch.Tensor] = None
        if crf is not None:
            self._phi = torch.zeros(self.max_streams, cfg.cls_out, dtype=torch.float32, device=eng.device)
            block = crf_block
            torch.cuda.current_stream(eng.device).synchronize()          # (the zero-fill, before the engine's stream reads it)
            for pl in (self.plan, self.chunk_plan):
                if pl is not None:
                    pl.stream_crf(block, self._phi)

    def crf_posterior(self) -> torch.Tensor:
        """``phi`` fp32 [S, C] (a copy): log P(label of the slot's LAST utterance | its dialogue so far) under the stream's CRF - the
        forward filter, run inside every step / prefill behind the classifier; the ``end`` term is not applied online.  Rows of slots
        that hold no utterance are zeros.  Needs a stream made with ``crf=``."""
        if self._phi is None:
            raise RuntimeError("DialogueStream.crf_posterior: this stream was made without a CRF (model.stream(..., crf=module))")
        return self._on_stream(lambda: self._phi.clone())

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
    def position_bias(self) -> Optional[float]:
        """The gain of the distance-decay attention bias this stream runs under (the applied value; None: off)."""
        return self._bias

    @property
    def speaker_heads(self):
        """(n_same, n_other) this stream runs under, or None."""
        return self._spk

    @property
    def speaker_cache(self) -> Optional[torch.Tensor]:
        """The cached speaker ids, uint8 [S, capacity] by logical cache row (None: a stream without speaker heads)."""
        return self.plan.spk_cache

    def _speakers(self, what: str, speakers, shape) -> Optional[torch.Tensor]:
        """The new utterances' ids as uint8 of `shape` ([rows] / [rows, n]; rows <= max_streams leading slots), or None without the setting."""
        if self._spk is None:
            if speakers is not None:
                raise ValueError(f"stream.{what}: speakers were given, but this stream's model has no speaker heads; it would ignore them")
            return None
        if speakers is None:
            raise ValueError(f"stream.{what}: this stream runs speaker_heads={self._spk}; pass speakers= (one id per new utterance)")
        ids = runtime.speaker_ids(speakers, f"stream.{what}: speakers")
        if tuple(ids.shape) != tuple(shape):
            raise ValueError(f"stream.{what}: speakers must be {tuple(shape)}, got {tuple(ids.shape)}")
        return ids

    def _refuse_bias(self, what: str) -> None:
        if self.model.speaker_heads != self._spk:
            raise RuntimeError(f"DialogueStream.{what}: the model's speaker heads are now {self.model.speaker_heads!r}, this stream's caches "
                               f"were written under {self._spk!r}; reset() the whole stream (it then takes the model's setting) or "
                               "build a new one with model.stream(...)")
        if self.model.position_bias != self._bias:
            raise RuntimeError(f"DialogueStream.{what}: the model's position bias is now {self.model.position_bias!r}, this stream's caches "
                               f"were written under {self._bias!r}; reset() the whole stream (it then takes the model's gain) or "
                               "build a new one with model.stream(...)")

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

    def _step(self, text, audio, act: List[bool], ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """act: one entry per slot (rows of text / audio may be fewer: the leading slots).  ids: `_speakers` of the call."""
        self._refuse_training("step")
        self._refuse_bias("step")
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
            if ids is not None:                            # the ids travel with the inputs
                pl.speakers_in[: ids.shape[0]].copy_(ids, non_blocking=True)
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
        self._attn_act = list(act)
        return out

    # -- public surface ----------------------------------------------------------------------------------------------------------
    def step(self, text: Optional[torch.Tensor], audio: Optional[torch.Tensor], active: Optional[Sequence[bool]] = None,
             speakers: Optional[torch.Tensor] = None) -> torch.Tensor:
        S = self.max_streams
        for x, name in ((text, "text"), (audio, "audio")):
            if x is not None and (x.dim() != 2 or x.shape[0] != S):
                raise ValueError(f"stream.step: {name} must be [max_streams = {S}, d], got {tuple(x.shape)}")
        return self._step(text, audio, self._mask(active, S), self._speakers("step", speakers, (S,)))

    def _chunk(self, text, audio, new: List[int], first: int, ids: Optional[torch.Tensor] = None) -> torch.Tensor:
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
            if ids is not None:                             # ([B, n] ids: the chunk's columns; rows past a count are never read)
                pl.speakers_in[: ids.shape[0], :width].copy_(ids[:, first: first + width], non_blocking=True)
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
        self._attn_act = None
        return out

    def prefill(self, text: Optional[torch.Tensor], audio: Optional[torch.Tensor], counts: Optional[Sequence[int]] = None,
                speakers: Optional[torch.Tensor] = None) -> torch.Tensor:
        S = self.max_streams
        self._refuse_training("prefill")
        self._refuse_bias("prefill")
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
        ids = self._speakers("prefill", speakers, (S, n))
        self._reserve(counts, "prefill")                   # (the whole call's pages, before its first launch)
        return self._feed(text, audio, counts, n, ids)

    def _feed(self, text, audio, counts: List[int], n: int, ids: Optional[torch.Tensor] = None) -> torch.Tensor:
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
                out[:, i] = self._step(None if text is None else text[:, i], None if audio is None else audio[:, i], act,
                                       None if ids is None else ids[:, i].contiguous())
            self._attn_act = None                           # (a history, however it was loaded: `attention` answers for a `step`)
            return out
        for i, new in enumerate(chunk_schedule(counts, T)):
            w = max(new)
            out[:, i * T: i * T + w] = self._chunk(text, audio, new, i * T, ids)[:, :w]
        return out

    def reset(self, slots: Optional[Sequence[int]] = None) -> None:
        S = self.max_streams
        self._attn_act = None
        if slots is None:
            if self.model.position_bias != self._bias:     # (every dialogue starts over: the stream follows the model's gain)
                self._bias = self.model.position_bias
                for pl in (self.plan, self.chunk_plan):
                    if pl is not None:
                        pl.attention_bias(self._bias)
            if self.model.speaker_heads != self._spk:      # (likewise: the stream follows the model's speaker heads)
                self._spk = self.model.speaker_heads
                if self._spk:
                    self.plan.stream_speakers(True)
                    self.plan.attention_speakers(self._spk)
                else:
                    self.plan.attention_speakers(None)
                if self.chunk_plan is not None:
                    self.chunk_plan.follow_speakers()
                if not self._spk:
                    self.plan.stream_speakers(False)
            self._on_stream(lambda: (self.plan.reset(None), self._phi.zero_() if self._phi is not None else None))
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
            if self._phi is not None:
                self._phi.masked_fill_(mask.bool()[:, None], 0.0)
            mask.record_stream(torch.cuda.current_stream(dev))
        self._on_stream(body)
        for s in slots:
            self.lengths[s] = 0
        if self.allocator is not None:
            self.allocator.release(set(slots))

    def run(self, text: Optional[torch.Tensor], audio: Optional[torch.Tensor], mask: torch.Tensor,
            speakers: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A padded batch (text [B, L, d_t], audio [B, L, d_a], mask bool [B, L], True = pad; B <= max_streams) through the stream:
        resets the first B slots and feeds the batch column by column with ``active = ~mask[:, i]`` - or, on a stream with
        ``max_chunk = T > 1`` and a batch in the collate layout (every row a valid prefix followed by padding), T columns per call.
        Returns logits [B, L, C_out] with zeros at pad slots - what ``forward`` gives at the valid slots under the model's band.  Reads
        ``mask`` on the host once."""
        B, L = mask.shape
        S = self.max_streams
        if B > S:
            raise ValueError(f"stream.run: {B} dialogues do not fit {S} stream slots")
        self._refuse_bias("run")
        ids = self._speakers("run", speakers, (B, L))
        self.reset(range(B))
        valid = (~mask.bool()).cpu()
        counts = prefix_counts(valid) if self.max_chunk > 1 else None
        if counts is not None:
            self._refuse_training("run")
            counts = counts + [0] * (S - B)
            check_prefill_fits(self.lengths, counts, self.capacity, self.past)
            self._reserve(counts, "run")
            return self._feed(text, audio, counts, L, ids)[:B]
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
            logits = self._step(None if text is None else text[:, i], None if audio is None else audio[:, i], act,
                                None if ids is None else ids[:, i].contiguous())
            out[:, i] = logits[:B]
        self._attn_act = None                               # (a whole batch, by steps or by chunks: `attention` answers for a `step`)
        return out

    # -- snapshots ---------------------------------------------------------------------------------------------------------------
    @property
    def signature(self) -> tuple:
        if self._signature is None:
            sites = self.plan.snapshot_sites()
            if sorted(sites) != sorted(config_sites(self.plan.cfg)):
                raise RuntimeError(f"stream: the plan reports attention sites {sites}, the configuration has {config_sites(self.plan.cfg)}")
            self._signature = make_signature(sites, self._eng.precision == runtime.BF16, self.past, self.capacity)
        return self._signature

    def _entries(self, slots: Sequence[int], lengths: Sequence[int], row_offsets: Sequence[int]):
        """(inside _on_stream) the per-entry arrays of a gather / scatter, uploaded without waiting for the device"""
        dev = self._eng.device
        idx = torch.tensor([list(slots), list(lengths)], dtype=torch.int32).to(dev, non_blocking=True)
        off = torch.tensor(list(row_offsets), dtype=torch.int64).to(dev, non_blocking=True)
        return idx[0], idx[1], off

    def _snapshot(self, slots, pinned: bool) -> StreamSnapshot:
        S = self.max_streams
        slots = list(range(S)) if slots is None else [int(s) for s in slots]
        if any(not 0 <= s < S for s in slots):
            raise ValueError(f"stream.snapshot: slots must be in 0 .. {S - 1}, got {slots}")
        sig = self.signature
        lengths = [self.lengths[s] for s in slots]
        rows = [min(n, self.capacity) for n in lengths]
        offsets = snapshot_row_offsets(rows)
        dev = self._eng.device
        data = torch.empty(sum(rows) * snapshot_row_elems(sig[0], sig[1]), dtype=torch.bfloat16 if sig[1] else torch.float32, device=dev)
        host = torch.empty(data.shape, dtype=data.dtype, pin_memory=True) if pinned else None
        ready = None
        spk_c, spk = self.plan.spk_cache, None              # speaker heads: the ids of the same rows (plain indexing: tiny and not hot)
        spk_host = torch.empty(sum(rows), dtype=torch.uint8, pin_memory=True) if (pinned and spk_c is not None) else None
        phi, phi_host = None, None                          # the CRF filter's state of the same slots
        if self._phi is not None and pinned:
            phi_host = torch.empty(len(slots), self._phi.shape[1], dtype=torch.float32, pin_memory=True)

        def body():
            nonlocal ready, phi
            if self._phi is not None:
                phi = self._phi[slots] if slots else self._phi[:0].clone()
                if phi_host is not None:
                    phi_host.copy_(phi, non_blocking=True)
            self._send_table()                              # (every path that changes the table sends it; a gather must never depend on that)
            nonlocal spk
            if data.numel():
                self.plan.gather(*self._entries(slots, lengths, offsets), data)
            if spk_c is not None:
                parts = [spk_c[s, :r] for s, r in zip(slots, rows)]
                spk = torch.cat(parts) if parts else spk_c.new_zeros(0)
                if spk_host is not None:
                    spk_host.copy_(spk, non_blocking=True)
            if host is not None:
                host.copy_(data, non_blocking=True)
                ready = torch.cuda.Event()
                ready.record(torch.cuda.current_stream(dev))
        self._on_stream(body)
        return StreamSnapshot(data if host is None else host, lengths, offsets, sig, _ready=ready,
                              speakers=spk if spk_host is None else spk_host, crf=phi if phi_host is None else phi_host)

    def snapshot(self, slots: Optional[Sequence[int]] = None) -> StreamSnapshot:
        return self._snapshot(slots, pinned=False)

    def restore(self, snap: StreamSnapshot, slots: Optional[Sequence[int]] = None) -> None:
        self._refuse_bias("restore")
        if (snap.speakers is None) != (self._spk is None):  # (before anything is released or launched: the stream stays as it is)
            raise RuntimeError("stream.restore: the snapshot " + ("carries no speaker ids" if snap.speakers is None else "carries speaker ids") +
                               ", this stream runs " + ("without speaker heads" if self._spk is None else f"speaker_heads={self._spk}"))
        if (snap.crf is None) != (self._phi is None):      # (likewise)
            raise RuntimeError("stream.restore: the snapshot " + ("carries no CRF filter state" if snap.crf is None else "carries a CRF filter state") +
                               ", this stream runs " + ("without a CRF" if self._phi is None else "with crf="))
        if snap.crf is not None and snap.crf.shape[1] != self._phi.shape[1]:
            raise ValueError(f"stream.restore: the snapshot's CRF state is {tuple(snap.crf.shape)}, this stream's [*, {self._phi.shape[1]}]")
        if snap.signature != self.signature:
            raise ValueError(f"stream.restore: the snapshot was written under (sites (H, hd), bf16, past, ring capacity) = {snap.signature}, "
                             f"this stream runs {self.signature}")
        slots = check_restore_slots(range(len(snap)) if slots is None else slots, len(snap), self.max_streams)
        check_restore_fits(snap.lengths, slots, self.capacity, self.past)
        data = snap.data
        if data.device != self._eng.device:
            raise ValueError(f"stream.restore: the snapshot lives on {data.device}, the stream on {self._eng.device}; snap.to(device) first")
        spk = snap.speakers
        if spk is not None and spk.device != self._eng.device:
            raise ValueError(f"stream.restore: the snapshot's speakers live on {spk.device}, the stream on {self._eng.device}; snap.to(device) first")
        rows = snap.rows
        if not slots:
            return
        al = self.allocator
        if al is not None:                                  # (all the pages or nothing, before anything is released or launched)
            before = al.state()
            al.replace(slots, [_pages_of(r, self.page_rows) for r in rows], "DialogueStream.restore")
        src = data if data.numel() else torch.zeros(8, dtype=data.dtype, device=data.device)      # (every entry empty: nothing is read)

        def body():
            self._send_table()                              # the table goes first: the scatter writes through it
            self.plan.scatter(*self._entries(slots, snap.lengths, snap.row_offsets), src)
            if spk is not None:
                for s_, o_, r_ in zip(slots, snap.row_offsets, rows):
                    if r_:
                        self.plan.spk_cache[s_, :r_].copy_(spk[o_: o_ + r_], non_blocking=True)
            if snap.crf is not None:                        # (C floats per entry: a host copy is uploaded here, as nothing else is)
                self._phi[slots] = snap.crf.to(self._eng.device, non_blocking=True)
        try:
            self._on_stream(body)
        except Exception:                                   # a launch that was refused: the host keeps describing the device -
            if al is not None:                              # the old pages and lengths; the old table is sent again with the next call
                al.set_state(before)
            raise
        for s, n in zip(slots, snap.lengths):
            self.lengths[s] = n
        self._attn_act = None

    # -- attention rows ----------------------------------------------------------------------------------------------------------
    def attention(self, average_heads: bool = True, sites: Optional[Sequence[str]] = None) -> StreamAttention:
        """Which cached utterances did the predictions of the last ``step`` use: a ``StreamAttention`` with, per attention site (named
        as ``M2FNet.last_attention`` names them; `sites`: a selection, default all), fresh tensors ``[S, C]`` - the heads averaged by
        the rule of ``last_attention``, on the device - or ``[S, H, C]``, column t of slot s being utterance ``first[s] + t`` of the
        slot's dialogue, ``t < count[s]``.  One eager launch outside the step graph; nothing waits for the device.  Needs a stream made
        with ``attention=True`` and a ``step`` as the last call: after ``prefill`` (the chunk kernel stores no rows), ``restore``,
        ``reset`` or ``run`` it raises RuntimeError."""
        if not self.attention_on:
            raise RuntimeError("DialogueStream.attention: this stream was made without attention rows (model.stream(..., attention=True))")
        if self._attn_act is None:
            raise RuntimeError("DialogueStream.attention: the last call was not a step (prefill, restore, reset and run leave no "
                               "attention rows): call step first")
        names = [n for (n, _, _) in self.plan.attention_sites()]
        want = names if sites is None else list(sites)
        unknown = [n for n in want if n not in names]
        if unknown:
            raise ValueError(f"DialogueStream.attention: unknown attention site(s) {unknown}; this model has {names}")
        maps = self._on_stream(lambda: self.plan.attention_rows([names.index(n) for n in want], not average_heads))
        ring = self.past is not None
        cols = [logical_columns(n, self.capacity, ring) if a else (0, 0) for n, a in zip(self.lengths, self._attn_act)]
        return StreamAttention(dict(zip(want, maps)), [c[0] for c in cols], [c[1] for c in cols])

    def evict(self, slots: Sequence[int]) -> StreamSnapshot:
        slots = [int(s) for s in slots]
        snap = self._snapshot(slots, pinned=True)
        self.reset(slots)
        return snap

    def fork(self, src: int, dst: int) -> None:
        self.restore(self.snapshot([src]), [dst])

    def close(self) -> None:
        if self.plan is not None:
            torch.cuda.synchronize(self._eng.device)
            if self.chunk_plan is not None:                 # (it borrows the stream plan's caches: it goes first)
                self.chunk_plan.close()
                self.chunk_plan = None
            self.plan.close()
            self.plan = None
