"""Auxiliary label head: a second linear classifier over the classifier's last hidden activation, trained against a second label per
utterance (csrc/aux_head.hip behind m2f_aux_head / m2f_aux_head_forward / m2f_aux_head_backward / m2f_plan_aux_head).

MELD labels every utterance twice, with an emotion and a sentiment.  ``M2FNet.train_step(aux=(head, aux_labels, weight))`` adds, for
every utterance with an emotion label AND an auxiliary label,

    u = W h + b,    a = label-smoothed cross entropy of u against the auxiliary label,    numerator += weight * w_y * a

over ``h`` = ``last_features()`` (post-ReLU, post-dropout in train mode) and the criterion's one denominator, inside the one replayed
step graph; the gradient reaches the trunk through the hidden activation's gradient.

The parameters are ONE flat fp32 block of A*D + A elements, [W row-major A x D | b A].  Like the CRF's block it is deliberately not part
of ``M2FNet``'s flat parameter buffer, its ``state_dict`` or ``m2f_config``: the kernels read it as an input and its gradient goes to a
buffer of its own, which an optimizer of the caller's steps beside ``FusedAdam``.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn as nn

MIN_CLASSES, MAX_CLASSES = 2, 16
MAX_FEATURES = 1024


def param_count(in_features: int, num_classes: int) -> int:
    return num_classes * in_features + num_classes


def check_num_classes(num_classes, who: str = "AuxiliaryHead") -> int:
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not MIN_CLASSES <= num_classes <= MAX_CLASSES:
        raise ValueError(f"{who}: num_classes must be an integer in [{MIN_CLASSES}, {MAX_CLASSES}] (got {num_classes!r})")
    return num_classes


def check_pair(weight, label_smoothing, who: str = "train_step") -> Tuple[float, float]:
    """(weight, label smoothing) of the auxiliary term as floats; ValueError naming the argument unless weight is a finite number >= 0
    and the smoothing a finite number in [0, 1).  A host function: no GPU needed."""
    for name, v in (("weight", weight), ("aux_label_smoothing", label_smoothing)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{who}: aux {name} must be a finite number, got {v!r}")
    if weight < 0.0:
        raise ValueError(f"{who}: aux weight must be >= 0, got {weight!r}")
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"{who}: aux_label_smoothing must lie in [0, 1), got {label_smoothing!r}")
    return float(weight), float(label_smoothing)


def check_step_args(who: str, aux, in_features: int, mask_shape=None, label_smoothing: float = 0.0, device=None):
    """``aux=`` of a step -> (head, aux_labels, weight, label_smoothing); ValueError unless it is a triple of an AuxiliaryHead over
    `in_features`, int64 labels of `mask_shape` on `device` (where the step runs; None: not checked) and a valid weight.  What the
    auxiliary head is refused beside is criterion.RULES' business.  A host function: no GPU needed."""
    if not isinstance(aux, (tuple, list)) or len(aux) != 3:
        raise ValueError(f"{who}: aux= must be a triple (head, aux_labels, weight), got {type(aux).__name__}")
    head, labels, weight = aux
    if not isinstance(head, AuxiliaryHead):
        raise ValueError(f"{who}: aux= needs an AuxiliaryHead first (got {type(head).__name__})")
    if head.in_features != in_features:
        raise ValueError(f"{who}: aux= head has in_features {head.in_features}, the model's classifier hidden width is {in_features}")
    if in_features > MAX_FEATURES:
        raise ValueError(f"{who}: aux= needs a classifier hidden width <= {MAX_FEATURES} (got {in_features})")
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or (mask_shape is not None and tuple(labels.shape) != tuple(mask_shape)):
        got = f"{tuple(labels.shape)} {labels.dtype}" if isinstance(labels, torch.Tensor) else type(labels).__name__
        raise ValueError(f"{who}: aux= labels must be int64 {list(mask_shape) if mask_shape is not None else '[B, L]'}, laid out like emotion (got {got})")
    if device is not None and labels.device != torch.device(device):
        raise ValueError(f"{who}: aux= labels are on {labels.device}, the step runs on {device} (move them as emotion is moved)")
    return (head, labels) + check_pair(weight, label_smoothing, who)


class _HeadFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat2d, params, num_classes):
        from . import functional as F
        ctx.save_for_backward(feat2d, params)
        ctx.num_classes = num_classes
        return F.aux_head_forward(feat2d, params, num_classes)

    @staticmethod
    def backward(ctx, grad_out):
        from . import functional as F
        feat2d, params = ctx.saved_tensors
        dfeat, dparams = F.aux_head_backward(feat2d, params, grad_out.contiguous().float(), ctx.num_classes,
                                             want_features=ctx.needs_input_grad[0], want_params=ctx.needs_input_grad[1])
        return dfeat, dparams, None


class AuxiliaryHead(nn.Module):
    """``AuxiliaryHead(in_features, num_classes)``: the linear head ``train_step(aux=)`` trains inside the step, and - called on features
    ``[..., in_features]`` - its logits ``[..., num_classes]`` through the same kernels, under autograd with respect to the features and
    the block.  ``weight`` / ``bias`` are views of the one fp32 block ``params``; ``state_dict`` holds them under those two keys.
    Initialised as ``nn.Linear(in_features, num_classes)`` is, in the same order under the caller's seed.
    ``head.params.requires_grad_(False)`` makes it a pure input."""

    def __init__(self, in_features: int, num_classes: int):
        super().__init__()
        if isinstance(in_features, bool) or not isinstance(in_features, int) or not 1 <= in_features <= MAX_FEATURES:
            raise ValueError(f"AuxiliaryHead: in_features must be an integer in [1, {MAX_FEATURES}] (got {in_features!r})")
        self.in_features = D = in_features
        self.num_classes = A = check_num_classes(num_classes)
        self.params = nn.Parameter(torch.empty(param_count(D, A), dtype=torch.float32))
        with torch.no_grad():              # nn.Linear.reset_parameters: the weight, then the bias
            nn.init.kaiming_uniform_(self.params[: A * D].view(A, D), a=math.sqrt(5))
            bound = 1.0 / math.sqrt(D)
            nn.init.uniform_(self.params[A * D:], -bound, bound)

    @property
    def weight(self) -> torch.Tensor:
        return self.params[: self.num_classes * self.in_features].view(self.num_classes, self.in_features)

    @property
    def bias(self) -> torch.Tensor:
        return self.params[self.num_classes * self.in_features:]

    @property
    def trainable(self) -> bool:
        return bool(self.params.requires_grad)

    # state_dict: `weight` and `bias`, as an nn.Linear's
    def _save_to_state_dict(self, destination, prefix, keep_vars):
        w, b = self.weight, self.bias
        destination[prefix + "weight"] = w if keep_vars else w.detach().clone()
        destination[prefix + "bias"] = b if keep_vars else b.detach().clone()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        for name, view in (("weight", self.weight), ("bias", self.bias)):
            key = prefix + name
            if key not in state_dict:
                if strict:
                    missing_keys.append(key)
                continue
            src = state_dict[key]
            if tuple(src.shape) != tuple(view.shape):
                error_msgs.append(f"size mismatch for {key}: copying a param with shape {tuple(src.shape)} from checkpoint, the shape in "
                                  f"current model is {tuple(view.shape)}.")
                continue
            with torch.no_grad():
                view.copy_(src)
        if strict:
            for key in state_dict:
                if key.startswith(prefix) and key[len(prefix):] not in ("weight", "bias") and "." not in key[len(prefix):]:
                    unexpected_keys.append(key)

    def block(self, device=None) -> torch.Tensor:
        """The parameter block as the kernels take it: fp32, contiguous, 16-byte aligned, on `device` (ValueError otherwise)."""
        p = self.params
        if device is not None and p.device != torch.device(device):
            raise ValueError(f"AuxiliaryHead: the parameters are on {p.device}, the step runs on {device}: move the module first")
        if not p.is_contiguous() or p.data_ptr() % 16:
            raise ValueError("AuxiliaryHead: the parameter block must be contiguous and 16-byte aligned")
        return p

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

    def forward(self, features: torch.Tensor) -> torch.Tensor:
        if features.dim() < 1 or features.shape[-1] != self.in_features:
            raise ValueError(f"AuxiliaryHead: features [..., {self.in_features}] expected, got {tuple(features.shape)}")
        lead = features.shape[:-1]
        rows = features.reshape(-1, self.in_features).float()
        if rows.shape[0] == 0:
            return rows.new_zeros(*lead, self.num_classes)
        out = _HeadFunction.apply(rows, self.block(features.device), self.num_classes)
        return out.view(*lead, self.num_classes)

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, num_classes={self.num_classes}"
