"""Sharpness-aware minimisation (Foret et al., ICLR 2021) restated in float64 plain torch: the reference of tests/test_sam_cpu.py and
tests/test_sam_model_gpu.py.

    e = rho * g / (||g||_2 + 1e-12)        the norm over every element of every UNIQUE tensor of the state dict
    SAM gradient   = the oracle's gradient (oracle.loss_and_grads) at w + e
    SAM trajectory = that gradient fed to oracle.adam_step at w

A state dict may hold one tensor under several names (shared LayerNorms): a tensor counts once in the norm and moves once."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import torch

from oracle import m2fnet_oracle as O

EPS = 1e-12


def unique_names(sd: Dict[str, torch.Tensor]) -> List[str]:
    """The first name of every unique tensor, in the state dict's order."""
    seen, out = set(), []
    for k, v in sd.items():
        if id(v) not in seen:
            seen.add(id(v))
            out.append(k)
    return out


def as_float64(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A float64 copy that keeps the aliasing."""
    made, out = {}, {}
    for k, v in sd.items():
        if id(v) not in made:
            made[id(v)] = v.detach().double().clone()
        out[k] = made[id(v)]
    return out


def grad_norm(sd, grads: Dict[str, torch.Tensor]) -> float:
    return float(torch.sqrt(sum((grads[k].double() ** 2).sum() for k in unique_names(sd))))


def perturbation(sd, grads: Dict[str, torch.Tensor], rho: float) -> Tuple[Dict[str, torch.Tensor], float]:
    """-> ({first name: e} over the unique tensors, ||g||)."""
    n = grad_norm(sd, grads)
    return {k: grads[k].double() * (rho / (n + EPS)) for k in unique_names(sd)}, n


def perturbed(sd, grads, rho: float) -> Tuple[Dict[str, torch.Tensor], float]:
    """-> (float64 state dict of w + e with sd's aliasing, ||g||)."""
    e, n = perturbation(sd, grads, rho)
    out = as_float64(sd)
    for k, d in e.items():
        out[k].add_(d)
    return out, n


def loss_and_grads(sd, cfg, batch, class_weight=None, rounding=None, criterion: Optional[Callable] = None):
    """oracle.loss_and_grads; with `criterion` (logits [B, L, C], target [B, L]) -> loss, the same over that criterion instead of the
    cross entropy (float64 autograd through the oracle's forward)."""
    text, audio, key_pad, target = batch
    if criterion is None:
        return O.loss_and_grads(sd, cfg, text, audio, key_pad, target, class_weight, rounding=rounding)
    leaves, sd2 = {}, {}
    for k, v in sd.items():
        if id(v) not in leaves:
            leaves[id(v)] = v.detach().clone().requires_grad_(True)
        sd2[k] = leaves[id(v)]
    logits = O.forward(sd2, cfg, text, audio, key_pad)
    loss = criterion(logits, target)
    loss.backward()
    return logits.detach(), loss.detach(), {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in sd2.items()}


def _as_bf16(grads):
    """Every gradient rounded to bf16 (nearest even, from its fp32 value) as the bf16 gradient buffer holds it; aliasing kept."""
    made, out = {}, {}
    for k, v in grads.items():
        if id(v) not in made:
            made[id(v)] = v.float().bfloat16().double()
        out[k] = made[id(v)]
    return out


def sam_gradient(sd, cfg, batch, rho: float, class_weight=None, rounding=None, criterion=None, to_fp32: bool = False,
                 grad_bf16: bool = False):
    """-> dict(loss = the loss at w, plain = the gradient at w, norm = ||plain||, at = the state dict w + e, loss_at = the loss there,
    logits_at, sam = the gradient there).  sd and the batch in float64 give a float64 reference; with `rounding` (oracle.Bf16Rounding)
    both passes emulate bf16 mode.  to_fp32: w + e is rounded to fp32 before the second pass, as a fp32 master copy holds it.
    grad_bf16: both gradients are rounded to bf16 where they are stored (M2FNet.set_grad_bf16): the norm and e come from the ROUNDED
    first gradient, the buffer the optimizer reads."""
    _, loss, g1 = loss_and_grads(sd, cfg, batch, class_weight, rounding, criterion)
    if grad_bf16:
        g1 = _as_bf16(g1)
    at, n = perturbed(sd, g1, rho)
    if to_fp32:
        made, at32 = {}, {}
        for k, v in at.items():
            if id(v) not in made:
                made[id(v)] = v.float()
            at32[k] = made[id(v)]
        at = at32
    logits2, loss2, g2 = loss_and_grads(at, cfg, batch, class_weight, rounding, criterion)
    if grad_bf16:
        g2 = _as_bf16(g2)
    return dict(loss=loss, plain=g1, norm=n, at=at, loss_at=loss2, logits_at=logits2, sam=g2)


def trajectory(sd, cfg, batch, rho: float, steps: int, lr: float, weight_decay: float, class_weight=None):
    """`steps` SAM steps of torch.optim.Adam (coupled decay: oracle.adam_step) in float64 on one batch -> (losses at w, final state dict)."""
    w = as_float64(sd)
    names = unique_names(w)
    m = [torch.zeros_like(w[k]) for k in names]
    v = [torch.zeros_like(w[k]) for k in names]
    losses = []
    for t in range(1, steps + 1):
        r = sam_gradient(w, cfg, batch, rho, class_weight)
        losses.append(float(r["loss"]))
        O.adam_step([w[k] for k in names], [r["sam"][k].double() for k in names], m, v, t, lr=lr, weight_decay=weight_decay)
    return losses, w
