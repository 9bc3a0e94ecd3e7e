"""The model watch of the reference's train loop (src/train.py:132-138: ``wandb.watch(model, log="all", log_freq=100)``) on the buffers
the kernels really use.  wandb's watch hangs hooks on the parameters; here the gradients are written by the plan's kernels into one flat
buffer behind autograd's back - and in the fastest modes (bf16 gradients, an accumulation group's sum, the reduced data-parallel buffer)
they never reach ``.grad`` - so those hooks see nothing.  ``ModelWatch`` instead has the optimizer hand the buffers THIS step reads to
``csrc/tensor_stats.hip``: per parameter tensor the counts of finite / NaN / infinite / zero values, min, max, sum and sum of squares
(float64) and a ``bins``-bin histogram by ``torch.histc``'s rule, two reads of the buffer, nothing on the step path waits for the host.

    w = ModelWatch(model, log="all", log_freq=100, bins=64)
    optimizer = FusedAdam(model, ..., watch=w)            # or optimizer.watch = w; None detaches
    ...
    if w.pending:                                          # a due step has run since the last read
        rec = w.read()                                     # the one synchronising call
        wandb.log({k: wandb.Histogram(np_histogram=v) for k, v in w.wandb_payload(rec).items()})
"""
from __future__ import annotations

import json
import math
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import runtime

KINDS = ("gradients", "parameters", "updates", "exp_avg", "exp_avg_sq", "ema")
_WANDB = {"gradients": ("gradients",), "parameters": ("parameters",), "all": ("gradients", "parameters")}
SCALARS = ("numel", "finite", "nan", "inf", "zeros", "min", "max", "mean", "l2", "rms")


class TensorStats(NamedTuple):
    numel: int
    finite: int
    nan: int
    inf: int
    zeros: int
    min: float          # over the finite values; NaN when there is none (as mean, l2, rms)
    max: float
    mean: float
    l2: float           # sqrt(sum of squares)
    rms: float
    hist: np.ndarray    # int64 [bins]: torch.histc(x[isfinite], bins, min, max)
    edges: np.ndarray   # float64 [bins + 1]


def check_kinds(log) -> Tuple[str, ...]:
    """``log``: "gradients", "parameters", "all" (wandb's three values) or an iterable of KINDS -> the kinds, in KINDS order."""
    if isinstance(log, str):
        if log not in _WANDB:
            raise ValueError(f"ModelWatch: log must be gradients, parameters, all or a list drawn from {list(KINDS)} (got {log!r})")
        return _WANDB[log]
    try:
        kinds = list(log)
    except TypeError:
        raise ValueError(f"ModelWatch: log must be gradients, parameters, all or a list drawn from {list(KINDS)} (got {log!r})") from None
    bad = [k for k in kinds if not isinstance(k, str) or k not in KINDS]
    if bad or not kinds:
        raise ValueError(f"ModelWatch: log must be gradients, parameters, all or a non-empty list drawn from {list(KINDS)} (got {log!r})")
    if len(set(kinds)) != len(kinds):
        raise ValueError(f"ModelWatch: log names a kind twice ({log!r})")
    return tuple(k for k in KINDS if k in kinds)


def check_log_freq(log_freq) -> int:
    if isinstance(log_freq, bool) or not isinstance(log_freq, int) or log_freq < 1:
        raise ValueError(f"ModelWatch: log_freq must be an integer >= 1 (got {log_freq!r})")
    return log_freq


def check_bins(bins) -> int:
    if isinstance(bins, bool) or not isinstance(bins, int) or not 2 <= bins <= runtime.TSTATS_MAX_BINS:
        raise ValueError(f"ModelWatch: bins must be an integer in [2, {runtime.TSTATS_MAX_BINS}] (got {bins!r})")
    return bins


def stats_from_row(row: np.ndarray, counts: np.ndarray, den: float = 1.0) -> TensorStats:
    """One record row (float64 [9]: numel, finite, nan, inf, zeros, min, max, sum, sumsq) and its int64 counts -> TensorStats, the value
    fields and the edges divided by `den` in float64."""
    numel, finite, nan, inf, zeros = (int(v) for v in row[:5])
    lo, hi, s, q = (float(v) for v in row[5:9])
    bins = len(counts)
    if finite > 0:
        mean, l2, rms = s / finite / den, math.sqrt(q) / den, math.sqrt(q / finite) / den
        a, b = np.float32(lo), np.float32(hi)
        if a == b:                                          # the kernel's rule, in fp32 as there
            a, b = a - np.float32(1.0), b + np.float32(1.0)
        edges = (float(a) + (float(b) - float(a)) * np.arange(bins + 1, dtype=np.float64) / bins) / den
    else:
        mean = l2 = rms = float("nan")
        edges = np.full(bins + 1, np.nan)
    return TensorStats(numel, finite, nan, inf, zeros, lo / den, hi / den, mean, l2, rms, counts.astype(np.int64, copy=True), edges)


class ModelWatch:
    """Per-tensor statistics and histograms of a model's flat buffers every ``log_freq`` optimizer steps.

    ``log``: "gradients", "parameters", "all" (both), or an iterable drawn from ``gradients, parameters, updates, exp_avg, exp_avg_sq,
    ema``.  Attached to a ``FusedAdam`` (``watch=`` / ``optimizer.watch``), step ``n`` (from 0, the optimizer's own count) is due when
    ``n % log_freq == 0``; on a due step the optimizer enqueues one collection per kind on the buffers that step uses - ``gradients``:
    the buffer the Adam kernel is about to read (fp32, the bf16 buffer of ``set_grad_bf16``, an accumulation group's sum, the reduced
    data-parallel buffer), with ``den`` = ``grad_scale``; ``parameters``, ``exp_avg``, ``exp_avg_sq``, ``ema``: as they are before the
    update (``ema`` once an average exists); ``updates``: new parameters minus a snapshot taken before the update kernels (one device
    copy of the flat buffer, on due steps only).  ``read()`` is the one call that waits for the device."""

    def __init__(self, model, log="all", log_freq: int = 100, bins: int = 64):
        if not hasattr(model, "engine") or not hasattr(model, "named_parameters"):
            raise TypeError(f"ModelWatch watches an M2FNet (its flat buffers); got {type(model).__name__}")
        self.model = model
        self.kinds = check_kinds(log)
        self.log_freq = check_log_freq(log_freq)
        self.bins = check_bins(bins)
        self.file: Optional[str] = None                    # the drop-in loop appends one JSON line per due step here
        self.pending = False                               # a record has been begun since the last read()
        self._engine = None
        self._names = None
        self._records: Optional[torch.Tensor] = None       # float64 [len(kinds) * row]: every kind's record, read with ONE copy
        self._scratch: Dict[str, torch.Tensor] = {}
        self._snapshot: Optional[torch.Tensor] = None
        self._step = 0
        self._collected = []

    def due(self, n: int) -> bool:
        return n % self.log_freq == 0

    # ---- device side ----------------------------------------------------------------------------------------------------------------
    def _bind(self):
        eng = self.model.engine()
        if eng is not self._engine:
            first = {}
            for name, p in self.model.named_parameters():
                first.setdefault(id(p), name)
            self._names = [first[id(p)] for (p, _, _, _) in eng.items]
            self._scratch = {}
            for k in self.kinds:
                self._scratch[k], rec = runtime.tensor_stats_buffers(eng.cfg, self.bins, eng.flat.device)
            self._rec_len = rec.numel()
            self._records = torch.zeros(len(self.kinds) * self._rec_len, dtype=torch.float64, device=eng.flat.device)
            self._snapshot = None
            self._engine = eng
            self._collected = []
        return eng

    def begin(self, step: int) -> None:
        """Starts the record of optimizer step `step`: what is collected from here on belongs to it."""
        self._bind()
        self._step, self._collected, self.pending = int(step), [], True

    def collect(self, kind: str, buffer: torch.Tensor, den: Optional[torch.Tensor] = None, other: Optional[torch.Tensor] = None) -> None:
        """Enqueues the collection of one flat buffer of the model's layout (``model.flat_gradients()``, the engine's parameter buffer,
        an optimizer's moments: the WHOLE buffer, fp32 or bf16) as `kind` of the current record, on the current stream; nothing waits.
        `den`: one-element fp32 device tensor the host divides the value fields by in ``read()``; `other` (fp32): the statistics are
        those of ``buffer - other``.  For loops that step with a torch optimizer: ``w.begin(step); w.collect("gradients",
        model.flat_gradients()); rec = w.read()``."""
        if kind not in self.kinds:
            raise ValueError(f"ModelWatch.collect: {kind!r} is not one of the watched kinds {list(self.kinds)}")
        eng = self._bind()
        n = eng.flat.numel()
        for what, t in (("buffer", buffer), ("other", other)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
                raise ValueError(f"ModelWatch.collect: {what} must be a contiguous flat device tensor of the model's {n} elements")
        if buffer.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"ModelWatch.collect: buffer must be fp32 or bf16 (got {buffer.dtype})")
        if other is not None and (other.dtype != torch.float32 or buffer.dtype != torch.float32):
            raise ValueError("ModelWatch.collect: the difference form takes two fp32 buffers")
        if den is not None and (den.dtype != torch.float32 or not den.is_cuda or den.numel() != 1):
            raise ValueError("ModelWatch.collect: den must be a one-element fp32 device tensor")
        i = self.kinds.index(kind)
        runtime.tensor_stats(eng.cfg, buffer, self._scratch[kind], self._records[i * self._rec_len: (i + 1) * self._rec_len], self.bins,
                             b=other, den=den)
        if kind not in self._collected:
            self._collected.append(kind)
        self.pending = True

    def snapshot(self, flat: torch.Tensor) -> torch.Tensor:
        """A device copy of `flat` (the parameters before the update kernels), kept until ``updates`` is collected against it."""
        if self._snapshot is None or self._snapshot.shape != flat.shape or self._snapshot.device != flat.device:
            self._snapshot = torch.empty_like(flat)
        self._snapshot.copy_(flat)
        return self._snapshot

    # ---- host side ------------------------------------------------------------------------------------------------------------------
    def read(self) -> dict:
        """``{"step": n, "den": d, kind: {name: TensorStats}}`` of the last record: ONE device-to-host copy, the one synchronising call.
        `name`: the names of ``model.named_parameters()`` (a shared tensor once, under its first name).  ``gradients`` are divided by
        ``den`` (min, max, mean, l2, rms and the edges, in float64): the gradient the optimizer uses, before clipping - what
        ``clip_grad_norm_`` would measure; counts stay as they are."""
        if self._records is None:
            raise RuntimeError("ModelWatch.read: nothing has been collected yet")
        host = self._records.cpu().numpy()
        self.pending = False
        out = {"step": self._step, "den": 1.0}
        H, Fd, row_len = runtime.TSTATS_HEADER, runtime.TSTATS_FIELDS, runtime.TSTATS_FIELDS + self.bins
        for i, kind in enumerate(self.kinds):
            if kind not in self._collected:
                continue
            rec = host[i * self._rec_len: (i + 1) * self._rec_len]
            den = float(rec[0]) if kind == "gradients" else 1.0
            if kind == "gradients":
                out["den"] = den
            assert int(rec[1]) == len(self._names) and int(rec[2]) == self.bins
            rows = rec[H:].reshape(len(self._names), row_len)
            counts = rows[:, Fd:].view(np.int64)
            out[kind] = {name: stats_from_row(rows[t, :Fd], counts[t], den) for t, name in enumerate(self._names)}
        return out

    @staticmethod
    def kinds_of(rec: dict):
        return [k for k in KINDS if k in rec]

    def wandb_payload(self, rec: dict) -> dict:
        """``{"gradients/<name>": (counts list, edges list), "parameters/<name>": ...}``, each value ready for
        ``wandb.Histogram(np_histogram=...)``."""
        return {f"{kind}/{name}": (st.hist.tolist(), st.edges.tolist()) for kind in self.kinds_of(rec) for name, st in rec[kind].items()}

    def summary(self, rec: dict):
        """One line per kind and tensor, for a log file."""
        return [f"step {rec['step']} {kind}/{name}: numel {st.numel} finite {st.finite} nan {st.nan} inf {st.inf} zeros {st.zeros} "
                f"min {st.min:.6e} max {st.max:.6e} mean {st.mean:.6e} rms {st.rms:.6e} l2 {st.l2:.6e}"
                for kind in self.kinds_of(rec) for name, st in rec[kind].items()]

    def json_line(self, rec: dict) -> str:
        """The record as one JSON line: step, den and per kind and tensor the scalar fields and the counts (``json.loads`` gives them
        back; a field without a value is NaN)."""
        out = {"step": rec["step"], "den": rec["den"]}
        for kind in self.kinds_of(rec):
            out[kind] = {name: {**{f: getattr(st, f) for f in SCALARS}, "hist": st.hist.tolist()} for name, st in rec[kind].items()}
        return json.dumps(out)
