"""``DeviceScores``: the reference's per-batch evaluation rule (src/train.py:245-272, src/test.py:51-74 - sklearn's accuracy and
weighted F1 on the utterances whose label is not -1, averaged unweighted over the batches, and the mean of the per-batch criterion
losses) kept in ONE device-resident record that the gfx950 kernels of ``csrc/metrics.hip`` add to batch by batch.  Scoring a batch
never waits for the device; the host reads the record when it wants the numbers."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import runtime
from .runtime import check, lib, ptr, stream_ptr

HEAD = 8                   # doubles in front of the confusion matrix: loss_sum, acc_sum, f1_sum, n_batches, last loss / acc / f1, unused
MAX_CLASSES = 16


def batch_scores(cm) -> Tuple[float, float]:
    """(accuracy, weighted F1) of ONE batch from its confusion matrix ``cm[true][predicted]`` (any nested sequence of integers), in
    float64 and in the kernel's operation order - the rule include/m2fnet_hip.h states; ``(nan, nan)`` for an empty batch."""
    C = len(cm)
    cm = [[int(v) for v in row] for row in cm]
    n = sum(sum(row) for row in cm)
    trace, f1w = 0, 0.0
    for c in range(C):
        support = sum(cm[c])
        predicted = sum(cm[j][c] for j in range(C))
        trace += cm[c][c]
        d = support + predicted
        f = float(2 * cm[c][c]) / float(d) if d else 0.0
        f1w += f * float(support)
    if n == 0:
        return float("nan"), float("nan")
    return float(trace) / float(n), f1w / float(n)


def class_report(cm) -> Dict[str, list]:
    """Per-class precision / recall / F1 / support from a confusion matrix ``cm[true][predicted]`` (host arithmetic, zero where a
    denominator is zero - sklearn's default)."""
    C = len(cm)
    cm = [[int(v) for v in row] for row in cm]
    out = {"precision": [], "recall": [], "f1": [], "support": []}
    for c in range(C):
        tp, support = cm[c][c], sum(cm[c])
        predicted = sum(cm[j][c] for j in range(C))
        out["precision"].append(tp / predicted if predicted else 0.0)
        out["recall"].append(tp / support if support else 0.0)
        out["f1"].append(2 * tp / (support + predicted) if support + predicted else 0.0)
        out["support"].append(support)
    return out


class DeviceScores:
    """The surface of the drop-in's ``BatchScores`` (``update`` / ``sums`` / ``result`` / ``n_batches``) with the sums on the device,
    plus what the device makes cheap: the mean batch loss, the confusion matrix of the whole pass and a per-class report.
    ``update`` and ``M2FNet.eval_step`` only queue launches; ``sums`` / ``result`` / ``mean_loss`` / ``n_batches`` / ``confusion`` /
    ``report`` copy the record to the host (one copy each)."""

    def __init__(self, n_classes: int, device):
        runtime.require_gpu()
        if not 1 <= int(n_classes) <= MAX_CLASSES:
            raise ValueError(f"DeviceScores: 1 .. {MAX_CLASSES} classes (got {n_classes})")
        self.n_classes = int(n_classes)
        self.device = torch.device(device)
        n = lib().m2f_eval_record_bytes(self.n_classes)
        if n < 0:
            raise runtime.HipError(lib().m2f_last_error().decode())
        self.record = torch.zeros(n // 8, dtype=torch.float64, device=self.device)
        self._scratch: Optional[torch.Tensor] = None

    def reset(self) -> None:
        self.record.zero_()

    def update(self, logits: torch.Tensor, emotion: torch.Tensor, class_weights: Optional[torch.Tensor] = None,
               label_smoothing: float = 0.1, focal_gamma: Optional[float] = None) -> None:
        """Score one batch: logits ``[B, L, C]`` (or ``[T, C]``) fp32 on the device, emotion ``[B, L]`` (-1 = not scored).
        focal_gamma (a finite number in [0, 8]): the loss is the focal criterion's (m2f_eval_scores_focal); None: the plain one."""
        gamma = None if focal_gamma is None else runtime.check_focal_gamma(focal_gamma, "focal_gamma", "DeviceScores.update")
        C = self.n_classes
        if logits.shape[-1] != C or logits.dtype != torch.float32 or logits.device != self.record.device:
            raise ValueError(f"DeviceScores.update: fp32 logits [..., {C}] on {self.record.device} expected, got "
                             f"{tuple(logits.shape)} {logits.dtype} on {logits.device}")
        rows = logits.reshape(-1, C).contiguous()
        labels = emotion.reshape(-1).to(device=rows.device, dtype=torch.int64).contiguous()
        T = rows.shape[0]
        if labels.numel() != T:
            raise ValueError(f"DeviceScores.update: {T} logit rows but {labels.numel()} labels")
        if T == 0:
            raise ValueError("DeviceScores.update: a batch needs at least one row (an all-unlabelled one scores NaN)")
        need = lib().m2f_eval_scratch_bytes(T, C)
        if need < 0:
            raise runtime.HipError(lib().m2f_last_error().decode())
        if self._scratch is None or self._scratch.numel() * 8 < need:
            self._scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=rows.device)
        cw = None
        if class_weights is not None:
            cw = class_weights.to(device=rows.device, dtype=torch.float32).contiguous()
            if cw.numel() != C:
                raise ValueError(f"DeviceScores.update: {C} class weights expected, got {cw.numel()}")
        if gamma is not None:
            g = torch.tensor([gamma], dtype=torch.float32).to(rows.device, non_blocking=True)
            check(lib().m2f_eval_scores_focal(T, C, ptr(rows), ptr(labels), ptr(cw), float(label_smoothing), ptr(g), ptr(self._scratch),
                                              ptr(self.record), stream_ptr()), "m2f_eval_scores_focal")
            return
        check(lib().m2f_eval_scores(T, C, ptr(rows), ptr(labels), ptr(cw), float(label_smoothing), ptr(self._scratch),
                                    ptr(self.record), stream_ptr()), "m2f_eval_scores")

    # -- device views (no sync) ------------------------------------------------------------------------
    def last(self) -> torch.Tensor:
        """Device view ``(loss, accuracy, weighted_f1)`` of the batch scored last (float64)."""
        return self.record[4:7]

    # -- host reads (one copy of the record each) ------------------------------------------------------
    def _host(self) -> torch.Tensor:
        return self.record.cpu()

    def totals(self) -> Tuple[float, float, float, float]:
        """(loss_sum, acc_sum, f1_sum, n_batches) in one read - what ranks add up under data parallelism."""
        h = self._host()
        return float(h[0]), float(h[1]), float(h[2]), float(h[3])

    def sums(self) -> Tuple[float, float]:
        h = self._host()
        return float(h[1]), float(h[2])

    @property
    def n_batches(self) -> int:
        return int(self._host()[3])

    def result(self) -> Tuple[float, float]:
        """(accuracy, weighted_f1), each the plain mean of the per-batch scores."""
        h = self._host()
        n = max(float(h[3]), 1.0)
        return float(h[1]) / n, float(h[2]) / n

    def mean_loss(self) -> float:
        h = self._host()
        return float(h[0]) / max(float(h[3]), 1.0)

    def confusion(self) -> torch.Tensor:
        """int64 ``[C, C]`` host tensor, ``[true][predicted]``, summed over every batch since the last ``reset``."""
        C = self.n_classes
        return self._host()[HEAD:].view(torch.int64).view(C, C).clone()

    def report(self) -> Dict[str, list]:
        """Per-class precision / recall / F1 / support of the whole pass (from ``confusion()``, on the host)."""
        return class_report(self.confusion().tolist())
