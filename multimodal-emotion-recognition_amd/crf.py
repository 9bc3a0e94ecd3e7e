"""Linear-chain CRF over a dialogue's emotion labels (csrc/crf.hip behind m2f_crf_nll / m2f_crf_viterbi / m2f_crf_filter).

Every utterance is otherwise scored and decoded on its own; the CRF adds what the classifier's rows cannot say: emotions persist from
turn to turn and shift in typical ways.  For a dialogue whose chain rows are t_1 < ... < t_n, emissions e = logits and labels y:

    score(y) = start[y_1] + sum_k e[t_k, y_k] + sum_{k>=2} transitions[y_{k-1}, y_k] + end[y_n]
    logZ     = log sum_paths exp(score)
    loss     = sum_dialogues (logZ - score(y)) / sum_dialogues n            (pytorch-crf's ``token_mean``)

The chain of the loss is the rows whose label is not -1, in row order (a -1 in the middle links its neighbours); the chain of ``decode``
is the rows whose mask is False.  A dialogue without a chain row contributes nothing.

The parameters are ONE flat fp32 block of C*C + 2*C elements, [transitions row-major C x C | start C | end C].  It is deliberately not
part of ``M2FNet``'s flat parameter buffer, its ``state_dict`` or ``m2f_config``: the kernels read it as an input, the way they read
class weights, and its gradient goes to a buffer of its own.  At zeros (the default) the CRF is the independent softmax.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn as nn

MIN_CLASSES, MAX_CLASSES = 2, 16


def param_count(num_classes: int) -> int:
    return num_classes * num_classes + 2 * num_classes


def check_num_classes(num_classes, who: str = "LinearChainCRF") -> int:
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not MIN_CLASSES <= num_classes <= MAX_CLASSES:
        raise ValueError(f"{who}: num_classes must be an integer in [{MIN_CLASSES}, {MAX_CLASSES}] (got {num_classes!r})")
    return num_classes


def label_count_params(labels, lengths, num_classes: int, smoothing: float = 1.0) -> np.ndarray:
    """The parameter block of a label set's log bigram, start and end frequencies (numpy, on the host): ``labels`` is the dialogues'
    labels one after the other (-1 = unlabelled: skipped, its neighbours linked, as the loss links them), ``lengths`` the utterances
    per dialogue.  Every count gets ``smoothing`` added; each row of exp(transitions), exp(start) and exp(end) sums to 1."""
    C = check_num_classes(num_classes, "from_label_counts")
    if not smoothing >= 0.0:
        raise ValueError(f"from_label_counts: smoothing must be >= 0 (got {smoothing!r})")
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lengths.sum() != labels.size or (lengths < 0).any():
        raise ValueError(f"from_label_counts: lengths sum to {int(lengths.sum())} but there are {labels.size} labels")
    if ((labels < -1) | (labels >= C)).any():
        raise ValueError(f"from_label_counts: labels must be -1 or in [0, {C})")
    trans = np.full((C, C), float(smoothing))
    start = np.full(C, float(smoothing))
    end = np.full(C, float(smoothing))
    at = 0
    for n in lengths:
        chain = labels[at: at + n]
        chain = chain[chain >= 0]
        at += n
        if chain.size == 0:
            continue
        start[chain[0]] += 1.0
        end[chain[-1]] += 1.0
        np.add.at(trans, (chain[:-1], chain[1:]), 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        block = np.concatenate([np.log(trans / trans.sum(1, keepdims=True)).reshape(-1), np.log(start / start.sum()),
                                np.log(end / end.sum())])
    return block.astype(np.float32)


def check_step_args(who: str, crf, num_classes: int) -> "LinearChainCRF":
    """``crf=`` of a step or a stream: ValueError unless it is a LinearChainCRF over the classifier's classes.  What the CRF criterion is
    refused beside is criterion.RULES' business.  A host function: no GPU needed."""
    if not isinstance(crf, LinearChainCRF):
        raise ValueError(f"{who}: crf= must be a LinearChainCRF (got {type(crf).__name__})")
    if crf.num_classes != num_classes:
        raise ValueError(f"{who}: crf= has {crf.num_classes} classes, the model's classifier has {num_classes}")
    return crf


class _CRFFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits2d, target1d, params, batch):
        from . import functional as F
        # only what a backward can ask for: no gradient at all (torch.no_grad, inference_mode, detached inputs) runs the forward sweep alone
        want_dl, want_dp = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        out, dl, dp, _ = F.crf_nll(logits2d, target1d, params, batch=batch, normalise=True, param_grad=want_dp,
                                   logit_grad=want_dl or want_dp)
        ctx.save_for_backward(dl, dp)
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        dl, dp = ctx.saved_tensors
        return (dl * grad_out if ctx.needs_input_grad[0] else None), None, (dp * grad_out if dp is not None else None), None


class LinearChainCRF(nn.Module):
    """``LinearChainCRF(num_classes)``: the criterion (``forward``), the Viterbi decoder (``decode``) and the parameter block the fused
    step, the eval step and the streams take as ``crf=``.  ``crf.params.requires_grad_(False)`` makes it a pure input."""

    def __init__(self, num_classes: int):
        super().__init__()
        self.num_classes = C = check_num_classes(num_classes)
        self.params = nn.Parameter(torch.zeros(param_count(C), dtype=torch.float32))

    @classmethod
    def from_label_counts(cls, labels, lengths, smoothing: float = 1.0, *, num_classes: Optional[int] = None) -> "LinearChainCRF":
        """A prior usable without training: log bigram, start and end frequencies of a label set (`label_count_params`).
        num_classes (keyword only): the classifier's classes; None takes the highest label + 1 - pass it whenever the set may lack
        its highest class."""
        if num_classes is None:
            num_classes = max(int(np.asarray(labels).max()) + 1, MIN_CLASSES)
        crf = cls(num_classes)
        with torch.no_grad():
            crf.params.copy_(torch.from_numpy(label_count_params(labels, lengths, num_classes, smoothing)))
        return crf

    @property
    def transitions(self) -> torch.Tensor:
        C = self.num_classes
        return self.params[: C * C].view(C, C)

    @property
    def start(self) -> torch.Tensor:
        C = self.num_classes
        return self.params[C * C: C * C + C]

    @property
    def end(self) -> torch.Tensor:
        C = self.num_classes
        return self.params[C * C + C:]

    @property
    def trainable(self) -> bool:
        return bool(self.params.requires_grad)

    def step_buffers(self, device, want_grad: bool = True):
        """(params, grad) as a fused step takes them: the block on `device`, and - trainable and wanted - the gradient buffer the step
        overwrites (kept by the module; ``publish_grad`` makes ``params.grad`` a view of it), else None."""
        p = self.block(device)
        if not (want_grad and self.trainable):
            return p.detach(), None
        g = getattr(self, "_grad_buf", None)
        if g is None or g.device != p.device:
            g = self._grad_buf = torch.zeros_like(p.detach())
        return p.detach(), g

    def publish_grad(self) -> None:
        """After a fused step: ``params.grad`` is the gradient buffer itself (overwritten by the next step)."""
        g = getattr(self, "_grad_buf", None)
        if self.trainable and g is not None and self.params.grad is not g:
            self.params.grad = g

    def block(self, device=None) -> torch.Tensor:
        """The parameter block as the kernels take it: fp32, contiguous, 16-byte aligned, on `device` (ValueError otherwise)."""
        p = self.params
        if device is not None and p.device != torch.device(device):
            raise ValueError(f"LinearChainCRF: the parameters are on {p.device}, the step runs on {device}: move the module first")
        if not p.is_contiguous() or p.data_ptr() % 16:
            raise ValueError("LinearChainCRF: the parameter block must be contiguous and 16-byte aligned")
        return p

    def _rows(self, input: torch.Tensor, target: torch.Tensor, who: str) -> torch.Tensor:
        """input [B, C, L] (the criterion's 3-D form) or [B, L, C] against target [B, L] -> [B, L, C]."""
        C = self.num_classes
        if input.dim() != 3 or target.dim() != 2 or input.shape[0] != target.shape[0]:
            raise ValueError(f"{who}: input [B, C, L] or [B, L, C] and target / mask [B, L] required "
                             f"(got {tuple(input.shape)}, {tuple(target.shape)})")
        L = target.shape[1]
        if input.shape[1] == C and input.shape[2] == L:
            return input.permute(0, 2, 1)
        if input.shape[1] == L and input.shape[2] == C:
            return input
        raise ValueError(f"{who}: input {tuple(input.shape)} is neither [B, {C}, {L}] nor [B, {L}, {C}]")

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        rows = self._rows(input, target, "LinearChainCRF.forward")
        B, L, C = rows.shape
        return _CRFFunction.apply(rows.reshape(B * L, C).contiguous().float(), target.reshape(-1).contiguous(),
                                  self.block(rows.device), B)

    @torch.no_grad()
    def decode(self, logits: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        """The Viterbi path of logits [B, L, C] over the rows whose mask [B, L] is False: int64 [B, L], -1 at masked slots.  The lowest
        class index wins every tie."""
        from . import functional as F
        C = self.num_classes
        if logits.dim() != 3 or logits.shape[2] != C or tuple(mask.shape) != tuple(logits.shape[:2]):
            raise ValueError(f"LinearChainCRF.decode: logits [B, L, {C}] and mask [B, L] required "
                             f"(got {tuple(logits.shape)}, {tuple(mask.shape)})")
        B, L, _ = logits.shape
        pred, _ = F.crf_viterbi(logits.reshape(B * L, C).contiguous().float(), mask.reshape(-1), self.block(logits.device), batch=B)
        return pred.view(B, L).long()
