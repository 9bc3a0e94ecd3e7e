"""float64 restatement of gradient clipping by global L2 norm (torch.nn.utils.clip_grad_norm_, norm_type 2) as the fused optimizer
applies it: the reference values of tests/test_grad_clip_gpu.py, checked against torch itself in tests/test_grad_clip_cpu.py.

    norm    = sqrt(sum over parameter tensors of sum(g^2)) / den
    coef    = min(1, max_norm / (norm + 1e-6))                       torch/nn/utils/clip_grad.py
    divisor = den if coef == 1 else den / coef                       the optimizer computes g / divisor = g / den * coef

Everything here is Python float / float64 tensors; nothing is rounded to fp32."""
import math
from typing import Iterable, Sequence, Tuple

import torch


def sum_of_squares(tensors: Iterable[torch.Tensor]) -> float:
    """float64 sum of squares, tensor by tensor (any dtype: fp32 and bf16 values are exact in float64, and so are their squares)."""
    total = 0.0
    for t in tensors:
        total += float(t.detach().double().pow(2).sum())
    return total


def tensors_of(flat: torch.Tensor, items: Sequence[Tuple[int, int]]):
    """The parameter tensors' elements of a flat buffer: items = (offset, numel) per tensor.  The pads between them are skipped."""
    return [flat[o: o + n] for (o, n) in items]


def norm(tensors: Iterable[torch.Tensor], den: float = 1.0) -> float:
    return math.sqrt(sum_of_squares(tensors)) / float(den)


def coef(norm_value: float, max_norm: float) -> float:
    c = float(max_norm) / (float(norm_value) + 1e-6)
    return c if c < 1.0 else 1.0


def divisor(den: float, coef_value: float) -> float:
    return float(den) if coef_value == 1.0 else float(den) / float(coef_value)


def clip_(tensors: Sequence[torch.Tensor], max_norm: float) -> float:
    """In place on float64 gradient tensors, as clip_grad_norm_ does; returns the norm before clipping."""
    n = norm(tensors)
    c = coef(n, max_norm)
    for t in tensors:
        t.mul_(c)
    return n
