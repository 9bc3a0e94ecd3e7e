"""Streaming inference: ``DialogueStream`` labels the utterance that has just arrived, for many live dialogues at once.

Under a causal context band ``(past, 0)`` (``M2FNet(config, context=(past, 0))``) the K and V rows of an utterance at every attention
site - both modality encoders, every fusion layer - depend on earlier utterances only and never change once computed.  A stream keeps
them in per-site caches on the device, so one step costs one row per dialogue where ``forward`` over the prefix costs the whole prefix
again.  The arithmetic runs in the gfx950 kernels behind ``runtime.StreamPlan`` (``csrc/attention_stream.hip`` for the attention, the
eval plan's own GEMM / LayerNorm / classifier launches for the rest); this module is plumbing.  The reference has no counterpart.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from . import runtime
from .layout import M2FConfig

MAX_CAPACITY = 512


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


class DialogueStream:
    """``model.stream(max_streams, capacity=None, use_graph=True)``: ``max_streams`` slots, each one live dialogue.

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
    ``reset()`` before the next step.  A history is fed utterance by utterance (no batched prefill)."""

    def __init__(self, model, max_streams: int, capacity: int, use_graph: bool = True):
        self.model, self.use_graph = model, bool(use_graph)
        self.max_streams, self.capacity = int(max_streams), int(capacity)
        self.past = model.context[0]
        eng = model.engine()
        self._eng = eng
        cfg = eng.cfg
        if cfg.dropout != 0.0:
            cfg = M2FConfig(**{**cfg.__dict__, "dropout": 0.0})
        self.plan = runtime.StreamPlan(cfg, self.max_streams, self.capacity, self.past, eng.precision, eng.flat, eng.wshadow)
        self.lengths: List[int] = [0] * self.max_streams
        self._active_host: Optional[List[bool]] = None        # what the device's mask holds (None: not written yet)

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

    def _step(self, text, audio, act: List[bool]) -> torch.Tensor:
        """act: one entry per slot (rows of text / audio may be fewer: the leading slots)."""
        if self.model.training and self.model.m2f_config.dropout > 0.0:
            raise RuntimeError("DialogueStream.step: the model is in training mode with dropout > 0; a stream scores the model "
                               "without dropout - call model.eval() first")
        if self.past is None:
            full = [s for s, a in enumerate(act) if a and self.lengths[s] >= self.capacity]
            if full:
                raise RuntimeError(f"DialogueStream.step: slot(s) {full} already hold {self.capacity} utterances, the capacity of a "
                                   "stream without a window (context past=None); reset() the slot, or stream under a window (past, 0)")
        pl, cfg, eng = self.plan, self.plan.cfg, self._eng

        def body():
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

    def reset(self, slots: Optional[Sequence[int]] = None) -> None:
        S = self.max_streams
        if slots is None:
            self._on_stream(lambda: self.plan.reset(None))
            self.lengths = [0] * S
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

    def run(self, text: Optional[torch.Tensor], audio: Optional[torch.Tensor], mask: torch.Tensor) -> torch.Tensor:
        """A padded batch (text [B, L, d_t], audio [B, L, d_a], mask bool [B, L], True = pad; B <= max_streams) through the stream:
        resets the first B slots and feeds the batch column by column with ``active = ~mask[:, i]``.  Returns logits [B, L, C_out]
        with zeros at pad slots - what ``forward`` gives at the valid slots under the model's band.  Reads ``mask`` on the host once."""
        B, L = mask.shape
        S = self.max_streams
        if B > S:
            raise ValueError(f"stream.run: {B} dialogues do not fit {S} stream slots")
        self.reset(range(B))
        valid = (~mask.bool()).cpu()
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
            self.plan.close()
            self.plan = None
