"""Criterion and optimizer of the reference's train loop as HIP-backed drop-ins.

* ``M2FCrossEntropyLoss``  = ``torch.nn.CrossEntropyLoss(weight, ignore_index=-1, label_smoothing=0.1)`` as the
  reference builds it (src/train.py:41-52), computed by the fused CE kernel (value + gradient in one pass).
* ``M2FFocalLoss``         = the same with every labelled row's term scaled by ``(1 - p_y)^gamma`` (focal loss; its own kernel).
* ``M2FRDropLoss``         = the same over a batch given twice, plus the symmetric KL divergence between each utterance's two predictions
  (R-Drop; its own kernel).
* ``M2FSupConLoss``        = the supervised contrastive loss over utterance features (Khosla et al. 2020; its own exact-fp32 kernels).
* ``M2FAuxiliaryLoss``     = the cross entropy of an ``aux_head.AuxiliaryHead`` over utterance features against a second label, per unit
  of the emotion criterion's labelled weight (the term ``train_step(aux=)`` adds; its own exact-fp32 kernels).
* ``FusedAdam``            = ``torch.optim.Adam(model.parameters(), lr, weight_decay)`` (src/train.py:56): coupled
  L2, bias-corrected; ONE kernel over the flat parameter / gradient / moment buffers instead of ~130 per-tensor
  updates.  ``state_dict()`` keeps torch.optim.Adam's format (per-parameter ``step`` / ``exp_avg`` /
  ``exp_avg_sq`` indexed in reference parameter order), so reference checkpoints load and vice versa.
  ``FusedAdam(model, params=[...])`` takes torch's parameter groups (own lr / betas / eps / weight_decay per group, parameters in no
  group left alone); ``decoupled_weight_decay=True`` / ``FusedAdamW`` = ``torch.optim.AdamW``.
"""
from __future__ import annotations

import contextlib
import ctypes
from typing import Optional

import torch
import torch.nn as nn

from . import functional as F
from . import runtime
from .layout import param_specs

# what torch.optim.Adam / AdamW accept and this optimizer does not: refused by name when set, never ignored
_TORCH_ONLY = ("amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused")
MAX_GROUPS = runtime.ADAM_MAX_GROUPS


def check_ema_decay(decay) -> Optional[float]:
    """``ema_decay``: None, or a number in [0, 1] (-> float); anything else is a ValueError."""
    if decay is None:
        return None
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= decay <= 1.0:
        raise ValueError(f"FusedAdam.ema_decay must be None or a number in [0, 1] (got {decay!r})")
    return float(decay)


def ema_decay_at(decay: float, n: int, warmup: bool = False) -> float:
    """The decay of update `n` (from 0): ``decay``, with warm-up ``min(decay, (1 + n) / (10 + n))``."""
    return min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay


class _CEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits2d, target1d, weight, label_smoothing):
        out, dl = F.cross_entropy(logits2d, target1d, weight, label_smoothing, True)
        ctx.save_for_backward(dl)
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        (dl,) = ctx.saved_tensors
        return dl * grad_out, None, None, None


class M2FCrossEntropyLoss(nn.Module):
    def __init__(self, weight: Optional[torch.Tensor] = None, ignore_index: int = -1, label_smoothing: float = 0.1):
        super().__init__()
        if ignore_index != -1:
            raise ValueError("the fused criterion implements ignore_index=-1 (reference src/train.py:48-50)")
        self.register_buffer("weight", weight)
        self.label_smoothing = float(label_smoothing)

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        # reference call: criterion(outputs.permute(0, 2, 1), emotion) with input [B, C, L], target [B, L]
        if input.dim() == 3:
            C = input.shape[1]
            logits = input.permute(0, 2, 1).reshape(-1, C)
        else:
            logits = input
        w = self.weight.to(device=logits.device, dtype=torch.float32) if self.weight is not None else None
        return _CEFunction.apply(logits.contiguous().float(), target.reshape(-1).contiguous(), w, self.label_smoothing)


class _DistillFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits2d, teacher2d, target1d, weight, label_smoothing, alpha, temperature):
        out, dl = F.cross_entropy_distill(logits2d, teacher2d, target1d, weight, label_smoothing, alpha, temperature, True)
        ctx.save_for_backward(dl)
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        (dl,) = ctx.saved_tensors
        return dl * grad_out, None, None, None, None, None, None


class M2FDistillationLoss(nn.Module):
    """``(1 - alpha) * M2FCrossEntropyLoss + alpha * temperature^2 * KL(softmax(teacher / temperature) || softmax(input / temperature))``
    over the labelled rows, one kernel (``functional.cross_entropy_distill``; the criterion ``M2FNet.train_step(teacher_logits=,
    distill=)`` runs inside the step) on the autograd surface.  ``forward(input, target, teacher_logits)``: input and teacher_logits
    ``[B, C, L]`` or ``[T, C]``, target ``[B, L]`` or ``[T]``; the teacher gets no gradient."""

    def __init__(self, weight: Optional[torch.Tensor] = None, ignore_index: int = -1, label_smoothing: float = 0.1,
                 alpha: float = 0.5, temperature: float = 2.0):
        super().__init__()
        if ignore_index != -1:
            raise ValueError("the fused criterion implements ignore_index=-1 (reference src/train.py:48-50)")
        from .distill import check_distill
        self.alpha, self.temperature = check_distill((alpha, temperature), "M2FDistillationLoss")
        self.register_buffer("weight", weight)
        self.label_smoothing = float(label_smoothing)

    def forward(self, input: torch.Tensor, target: torch.Tensor, teacher_logits: torch.Tensor) -> torch.Tensor:
        from .distill import check_distill
        alpha, temperature = check_distill((self.alpha, self.temperature), "M2FDistillationLoss")
        if teacher_logits.shape != input.shape:
            raise ValueError(f"M2FDistillationLoss: teacher_logits {tuple(teacher_logits.shape)} must have the input's shape "
                             f"{tuple(input.shape)}")
        if input.dim() == 3:
            C = input.shape[1]
            logits = input.permute(0, 2, 1).reshape(-1, C)
            teacher = teacher_logits.permute(0, 2, 1).reshape(-1, C)
        else:
            logits, teacher = input, teacher_logits
        w = self.weight.to(device=logits.device, dtype=torch.float32) if self.weight is not None else None
        return _DistillFunction.apply(logits.contiguous().float(), teacher.detach().contiguous().float(), target.reshape(-1).contiguous(),
                                      w, self.label_smoothing, alpha, temperature)


class _FocalFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits2d, target1d, weight, label_smoothing, gamma):
        out, dl = F.cross_entropy_focal(logits2d, target1d, weight, label_smoothing, gamma, True)
        ctx.save_for_backward(dl)
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        (dl,) = ctx.saved_tensors
        return dl * grad_out, None, None, None, None


class M2FFocalLoss(M2FCrossEntropyLoss):
    """Focal loss (Lin et al. 2017) over ``M2FCrossEntropyLoss``: every labelled row's term scaled by ``(1 - p_y)^gamma``, the sum
    divided by the sum of the labels' class weights as ever - without weights and smoothing ``mean(-(1 - p_y)^gamma log p_y)``.  One
    kernel (``functional.cross_entropy_focal``; the criterion ``M2FNet.train_step(focal_gamma=)`` runs inside the step) on the autograd
    surface of its base class, which it IS: the train loop's fused step accepts it and hands ``gamma`` on.  ``gamma`` (a finite number in
    [0, 8]; 0 = the base class's bits) is a plain attribute, read at every call: a schedule may change it."""

    def __init__(self, weight: Optional[torch.Tensor] = None, ignore_index: int = -1, label_smoothing: float = 0.1, gamma: float = 2.0):
        super().__init__(weight, ignore_index, label_smoothing)
        self.gamma = runtime.check_focal_gamma(gamma, "gamma", "M2FFocalLoss")

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        gamma = runtime.check_focal_gamma(self.gamma, "gamma", "M2FFocalLoss")
        if input.dim() == 3:
            C = input.shape[1]
            logits = input.permute(0, 2, 1).reshape(-1, C)
        else:
            logits = input
        w = self.weight.to(device=logits.device, dtype=torch.float32) if self.weight is not None else None
        return _FocalFunction.apply(logits.contiguous().float(), target.reshape(-1).contiguous(), w, self.label_smoothing, gamma)


class _RDropFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits2d, partner, target1d, weight, label_smoothing, alpha):
        out, dl = F.cross_entropy_rdrop(logits2d, partner, target1d, weight, label_smoothing, alpha, True)
        ctx.save_for_backward(dl)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, grad_out, _):
        (dl,) = ctx.saved_tensors
        return dl * grad_out, None, None, None, None, None


class M2FRDropLoss(M2FCrossEntropyLoss):
    """R-Drop (Liang et al. 2021) over ``M2FCrossEntropyLoss``: the input holds every dialogue TWICE - logits ``[2B, L, C]`` (or the
    reference's ``[2B, C, L]``), view 1 behind view 0, two forwards of one batch under independent dropout masks; the target is the
    doubled ``[2B, L]`` labels.  The loss is the cross entropy over all ``2B``
    dialogues' labelled utterances plus ``alpha * w_y * 0.5 * (KL(p || q) + KL(q || p))`` between each utterance's two predictions,
    over the one denominator - without class weights ``0.5 * (CE(view 0) + CE(view 1)) + alpha * 0.5 * (kl_div(v0, v1, 'batchmean') +
    kl_div(v1, v0, 'batchmean'))``.  One kernel (``functional.cross_entropy_rdrop``; the criterion ``M2FNet.train_step(rdrop=)`` runs
    inside the step) on the autograd surface of its base class.  ``alpha`` (a finite number >= 0; 0 = the base class's bits) is a plain
    attribute, read at every call: a warm-up may change it.  ``last_terms`` holds ``(loss, den, num, kl)`` of the last call on the device
    (kl = sum of w_y * s without alpha).  ``channels_last`` (None: told apart by the target's L; where L == C the reference's layout)
    names the layout outright."""

    def __init__(self, weight: Optional[torch.Tensor] = None, ignore_index: int = -1, label_smoothing: float = 0.1, alpha: float = 1.0,
                 channels_last: Optional[bool] = None):
        super().__init__(weight, ignore_index, label_smoothing)
        self.alpha = runtime.check_rdrop_alpha(alpha, "alpha", "M2FRDropLoss")
        self.channels_last = channels_last    # True: [2B, L, C]; False: [2B, C, L]; None: told apart by the target's L
        self.last_terms = None

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        alpha = runtime.check_rdrop_alpha(self.alpha, "alpha", "M2FRDropLoss")
        if input.dim() != 3:
            raise ValueError(f"M2FRDropLoss: logits [2B, L, C] or [2B, C, L] expected, got {tuple(input.shape)}")
        n = input.shape[0]
        if n % 2:
            raise ValueError(f"M2FRDropLoss: the input holds every dialogue twice (view 0, then view 1), got {n} dialogues")
        if target.dim() != 2 or target.shape[0] != n:
            raise ValueError(f"M2FRDropLoss: target [{n}, L] expected (the labels of both views), got {tuple(target.shape)}")
        Lt = target.shape[1]
        cl = self.channels_last
        if cl is None:                                              # (L == C: the reference's layout)
            cl = input.shape[1] == Lt and input.shape[2] != Lt
        if input.shape[1 if cl else 2] != Lt:
            raise ValueError(f"M2FRDropLoss: logits {tuple(input.shape)} do not match target {tuple(target.shape)}")
        logits = input if cl else input.permute(0, 2, 1)            # [2B, L, C] / the reference's [2B, C, L]
        C = logits.shape[2]
        partner = runtime.rdrop_partner(n // 2, Lt, n * Lt, L=Lt, device=logits.device)
        w = self.weight.to(device=logits.device, dtype=torch.float32) if self.weight is not None else None
        loss, self.last_terms = _RDropFunction.apply(logits.reshape(-1, C).contiguous().float(), partner, target.reshape(-1).contiguous(), w,
                                                     self.label_smoothing, alpha)
        return loss


class _SupConFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat2d, target1d, weight, temperature, n_classes):
        rows, dfeat = F.supcon(feat2d, target1d, weight, 1.0, temperature, n_classes)
        w = torch.ones(n_classes, dtype=torch.float32, device=feat2d.device) if weight is None else weight
        ok = (target1d >= 0) & (target1d < n_classes)
        den = (w[target1d.clamp(0, n_classes - 1)] * ok).sum()
        ctx.save_for_backward(dfeat, den)
        ctx.mark_non_differentiable(rows)
        return rows[:, 3].sum() / den, rows

    @staticmethod
    def backward(ctx, grad_out, _):
        dfeat, den = ctx.saved_tensors
        return dfeat * (grad_out / den), None, None, None, None


class M2FSupConLoss(nn.Module):
    """Supervised contrastive loss (Khosla et al. 2020) over utterance features, the term ``M2FNet.train_step(supcon=)`` adds inside
    the step, on the autograd surface: features ``[N, D]`` or ``[B, L, D]`` (fp32), targets ``[N]`` or ``[B, L]`` with ``ignore_index``
    (-1, the padding label) for rows that are not contrasted.  With V = the labelled rows of a non-zero norm, ``z = h / ||h||``:
    ``l_i = logsumexp_{a in V, a != i}(z_i . z_a / temperature) - mean_{p in V, p != i, y_p = y_i}(z_i . z_p / temperature)`` (0 without a
    positive), and the loss is ``sum_i w_{y_i} l_i / sum_i w_{y_i}`` over the LABELLED rows - the criterion's own denominator, so
    ``M2FCrossEntropyLoss(...)(logits, y) + weight * M2FSupConLoss(...)(h, y)`` is the step's loss.  One family of exact-fp32 kernels
    (``functional.supcon``).  ``temperature`` (finite, > 0) is a plain attribute, read at every call.  ``last_terms`` holds the per-row
    ``(lse, n, l, w l)`` of the last call on the device.  n_classes: the weight's length, else 1 + the largest target (one host read);
    pass it to avoid the read."""

    def __init__(self, weight: Optional[torch.Tensor] = None, ignore_index: int = -1, temperature: float = 0.1,
                 n_classes: Optional[int] = None):
        super().__init__()
        if ignore_index != -1:
            raise ValueError("M2FSupConLoss: ignore_index must be -1 (the padding label the kernels skip)")
        self.register_buffer("weight", weight)
        self.ignore_index = ignore_index
        self.temperature = runtime.check_supcon_pair((0.0, temperature), "temperature", "M2FSupConLoss")[1]
        self.n_classes = n_classes
        self.last_terms = None

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        t = runtime.check_supcon_pair((0.0, self.temperature), "temperature", "M2FSupConLoss")[1]
        if input.dim() not in (2, 3) or target.shape != input.shape[:-1]:
            raise ValueError(f"M2FSupConLoss: features [N, D] / [B, L, D] with targets [N] / [B, L] expected, got {tuple(input.shape)} "
                             f"and {tuple(target.shape)}")
        w = self.weight.to(device=input.device, dtype=torch.float32) if self.weight is not None else None
        tgt = target.reshape(-1).contiguous()
        C = self.n_classes if self.n_classes is not None else (w.numel() if w is not None else max(int(tgt.max()) + 1, 1))
        loss, self.last_terms = _SupConFunction.apply(input.reshape(-1, input.shape[-1]).contiguous().float(), tgt, w, t, C)
        return loss


class _AuxHeadLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat2d, params, target1d, aux1d, weight, eps, n_classes):
        logits, rows, dfeat, dparams = F.aux_head(feat2d, target1d, aux1d, params, (1.0, eps), weight, n_classes)
        w = torch.ones(n_classes, dtype=torch.float32, device=feat2d.device) if weight is None else weight
        ok = (target1d >= 0) & (target1d < n_classes)
        den = (w[target1d.clamp(0, n_classes - 1)] * ok).sum()
        # (no row with an emotion label: den = 0 - the term and its gradient are 0, as the step's are; a select, no 0 / 0)
        inv = torch.where(den > 0, 1.0 / den.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(den))
        ctx.save_for_backward(dfeat, dparams, inv)
        ctx.mark_non_differentiable(logits, rows)
        return rows.sum() * inv, logits, rows

    @staticmethod
    def backward(ctx, grad_out, _l, _r):
        dfeat, dparams, inv = ctx.saved_tensors
        k = grad_out * inv
        return (dfeat * k if ctx.needs_input_grad[0] else None), (dparams * k if ctx.needs_input_grad[1] else None), None, None, None, None, None


class M2FAuxiliaryLoss(nn.Module):
    """The auxiliary label head's term, the one ``M2FNet.train_step(aux=)`` adds inside the step, on the autograd surface:
    ``loss(features, head, emotion, aux_labels)`` with features ``[N, D]`` or ``[B, L, D]`` (fp32), an ``aux_head.AuxiliaryHead`` over
    ``D``, and the two targets ``[N]`` or ``[B, L]`` with ``ignore_index`` (-1, the padding label).  For every row with both labels valid,
    ``a_i`` = the cross entropy (``label_smoothing``, no class weights of its own) of ``head``'s logits against the auxiliary label; the
    loss is ``sum_i w_{y_i} a_i / sum_i w_{y_i}``, the denominator over the rows with an EMOTION label - the criterion's own, so
    ``M2FCrossEntropyLoss(...)(logits, y) + weight * M2FAuxiliaryLoss(...)(h, head, y, s)`` is the step's loss.  ``weight``: the
    emotion classes' weights or None.  Differentiable with respect to the features and the head's block: the kernels give the gradient
    at unit weight and torch scales it by ``grad_out / den``, where the step scales by ``(1 / den) * weight`` inside its reduce launch -
    the two agree to a few fp32 eps, bit equality with the step is NOT offered.  No row with an emotion label: the loss and its
    gradients are 0, as the step's.  ``last_logits`` /
    ``last_terms`` hold the head's logits and the per-row ``w_y a_i`` of the last call on the device.  n_classes: the weight's length,
    else 1 + the largest emotion target (one host read); pass it to avoid the read."""

    def __init__(self, weight: Optional[torch.Tensor] = None, ignore_index: int = -1, label_smoothing: float = 0.0,
                 n_classes: Optional[int] = None):
        super().__init__()
        from .aux_head import check_pair
        if ignore_index != -1:
            raise ValueError("M2FAuxiliaryLoss: ignore_index must be -1 (the padding label the kernels skip)")
        self.register_buffer("weight", weight)
        self.ignore_index = ignore_index
        self.label_smoothing = check_pair(0.0, label_smoothing, "M2FAuxiliaryLoss")[1]
        self.n_classes = n_classes
        self.last_logits = self.last_terms = None

    def forward(self, input: torch.Tensor, head, target: torch.Tensor, aux_target: torch.Tensor) -> torch.Tensor:
        from .aux_head import AuxiliaryHead, check_pair
        eps = check_pair(0.0, self.label_smoothing, "M2FAuxiliaryLoss")[1]
        if not isinstance(head, AuxiliaryHead) or input.dim() not in (2, 3) or input.shape[-1] != head.in_features:
            raise ValueError(f"M2FAuxiliaryLoss: features [N, D] / [B, L, D] and an AuxiliaryHead over D expected, got {tuple(input.shape)} "
                             f"and {head!r}")
        if target.shape != input.shape[:-1] or aux_target.shape != input.shape[:-1]:
            raise ValueError(f"M2FAuxiliaryLoss: targets {tuple(input.shape[:-1])} expected, got {tuple(target.shape)} and {tuple(aux_target.shape)}")
        w = self.weight.to(device=input.device, dtype=torch.float32) if self.weight is not None else None
        tgt = target.reshape(-1).contiguous()
        C = self.n_classes if self.n_classes is not None else (w.numel() if w is not None else max(int(tgt.max()) + 1, 1))
        loss, self.last_logits, self.last_terms = _AuxHeadLossFunction.apply(
            input.reshape(-1, input.shape[-1]).contiguous().float(), head.block(input.device), tgt, aux_target.reshape(-1).contiguous(), w, eps, C)
        return loss


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` (coupled L2 weight decay, reference ``src/train.py:56``) as ONE kernel over the model's flat
    parameter / gradient / moment buffers.  Differences from torch worth knowing: every parameter of the model is updated every
    step - a parameter whose ``.grad`` is None is treated as having a zero gradient (it still receives weight decay and the
    moment decay; torch skips it), which never happens on the M2FNet path, where backward writes every gradient.

    Parameter groups and AdamW (keyword-only).  ``params``: torch's own format - an iterable of parameters, or of dicts with ``params``
    and any of ``lr`` / ``betas`` / ``eps`` / ``weight_decay`` / ``decoupled_weight_decay`` - at most 16 groups, every parameter one of
    ``model``'s and in one group only.  None (the default) = ``model.parameters()`` in one group: with coupled decay that is the optimizer
    described above, kernel for kernel.  ``decoupled_weight_decay=True`` (``FusedAdamW``: the same with ``weight_decay=1e-2``) =
    ``torch.optim.AdamW``: the parameter is multiplied by ``1 - lr * weight_decay`` before Adam's update, and the decay stays out of
    the moments.  A parameter in NO group is neither read nor written by a step - parameter, both moments and both bf16 shadows keep
    their bits, ``engine.shadows_fresh()`` stays true - but its gradient is still computed, and still counts in ``max_grad_norm``'s
    norm (``clip_grad_norm_(model.parameters(), x)``; one divisor for every group).  ``param_groups[i][...]`` are read at every step
    (torch's schedulers work per group), every group counts its own steps (``add_param_group`` starts one at 0), and ``state_dict()``
    / ``load_state_dict()`` keep torch's format with indices running on across the groups: a ``torch.optim.AdamW`` state dict over the
    same parameter lists loads, and back.  ``amsgrad``, ``maximize``, ``foreach``, ``capturable``, ``differentiable`` and ``fused``
    raise when set.  ``step_ranges`` of a grouped optimizer takes ranges of whole tensors only.  All of it runs through one hyper table
    on the device (a row per group, refreshed by one small launch per step) and grouped forms of the same kernels: a coupled group's
    tensors get the bits the single-group kernels give them (tests/test_optimizer_groups_gpu.py).

    ``max_grad_norm`` (constructor argument and plain attribute; may be changed or set to None between steps; not part of
    ``state_dict``): every step first clips the gradient by its global L2 norm, ``torch.nn.utils.clip_grad_norm_(parameters,
    max_grad_norm)``'s rule, on the device - two launches reduce the norm of the gradient buffer THIS step reads (fp32, or the bf16
    buffer of ``M2FNet.set_grad_bf16`` / the data-parallel bf16 exchange) in float64, divided by ``grad_scale`` where one is set, and
    fold ``coef = min(1, max_grad_norm / (norm + 1e-6))`` into the divisor the Adam kernel already applies.  Differences from torch:
    ``.grad`` is NOT scaled - the clip exists only where the optimizer reads; the norm is that of the gradient the optimizer uses
    (after the division by ``grad_scale``: the mean gradient of an accumulation group or of the global batch), which a norm over
    ``.grad`` is not in those modes; ``grad_norm()`` / ``clip_coef()`` are device tensors, nothing on the step path waits for the
    host.  A non-finite norm gives a non-finite divisor and non-finite parameters, as torch's default ``error_if_nonfinite=False``
    does.  None (the default): the step as it was, launch for launch.

    ``ema_decay`` (keyword-only constructor argument and plain attribute; a number in [0, 1] or None; may be changed between steps,
    None stops updating and keeps the buffer) with ``ema_warmup``: an exponential moving average of the weights,
    ``torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay)).update_parameters(model)`` after every
    ``step()``, kept by the optimizer kernels themselves - the kernel that has the new parameter in registers reads, updates and
    writes its average (one fp32 buffer the size of the flat parameter buffer, zeroed at the first averaging step; 8 B of traffic per
    parameter).  ONE update per optimizer step however many micro-batches fed it and however many launches make it up (``step()``,
    ``step_ranges()``, the grouped forms, bf16 gradients: the same bits from all of them); update ``n`` (from 0) uses ``decay``, with
    ``ema_warmup`` ``min(decay, (1 + n) / (10 + n))``; update 0 copies the parameters.  Parameters, moments and shadows are what they
    are without it, bit for bit.  Differences from ``AveragedModel``: no second module - ``with optimizer.averaged_parameters():``
    swaps the average INTO the model (one launch in, one out) for validation, a checkpoint or ``test.py``; a tensor in no parameter
    group is not averaged (its EMA slice is never touched, ``ema_state_dict`` reports its live value); buffers are not averaged
    (M2FNet has none); the average is not part of ``state_dict()`` (torch's format) but of ``ema_state_dict()``.  Refused
    combination: the optimizer inside the weight-gradient launch has no EMA stream - ``prepare_fused`` returns False, as with
    ``max_grad_norm``.  None (the default): the step as it was, launch for launch.

    ``watch`` (keyword-only constructor argument and plain attribute; a ``watch.ModelWatch`` or None): the optimizer counts its own
    steps, and on step ``n`` (from 0) with ``n % watch.log_freq == 0`` it enqueues, before the update kernels, one statistics collection
    per watched kind on the buffers THIS step uses (``ModelWatch``'s docstring; csrc/tensor_stats.hip) and, for ``updates``, one after
    them.  Nothing waits for the host; ``watch.read()`` does.  Clipping and the watch read the same gradient buffer in the same step and
    neither changes the other; a tensor in no parameter group is watched like any other.  ``prepare_fused`` returns False while a watch
    that logs ``gradients`` or ``updates`` is attached (the in-launch optimizer never stores the matrices' gradients); with other kinds
    the in-launch step is counted and the buffers are collected as they are before it.  In ``step_ranges`` on a due step `before_each`
    runs for all ranges first, as with clipping.  Parameters, moments, shadows and the EMA are what they are without it, bit for bit.
    None (the default): the step as it was, launch for launch.

    ``sam_rho`` (keyword-only constructor argument and plain attribute; a finite number > 0 or None; may be changed between steps, so a
    schedule works; not part of ``state_dict``): sharpness-aware minimisation (Foret et al., ICLR 2021), one perturbation per optimizer
    step.  ``first_step()`` reduces the L2 norm of the gradient buffer ``step()`` would read at that moment (fp32, the bf16 buffer of
    ``set_grad_bf16``, or an accumulation group's sum; divided by ``grad_scale`` where one is set) with the clip's launches into a
    record of its own, and one kernel moves every parameter to ``w + rho * g / (||g|| + 1e-12)`` - one fp32 coefficient formed in
    float64 on the device, one fused multiply-add per element - keeping ``w`` in a backup buffer of the flat size and, in bf16 mode,
    writing the bf16 shadows of the moved matrices itself (``engine.shadows_fresh()`` stays true).  An ordinary ``train_step`` on the
    same batch then leaves the gradient at ``w + e`` in the same buffers, and ``step()`` restores ``w`` to its bits before it runs
    today's update on that gradient: clipping, the EMA and the watch see the second gradient, exactly as they see the only one
    without SAM.  ``model.sam_step(...)`` makes the four calls.  ``restore()`` abandons a perturbation; ``sam_norm()`` is the norm
    of the last ``first_step`` on the device.  Nothing waits for the host.  With ``sam_rho`` set, ``step()`` without a pending
    perturbation raises (a loop cannot silently train without SAM); ``first_step()`` while one is pending raises, and so do
    ``averaged_parameters()``, ``ema_state_dict()`` and ``prepare_fused()`` while one is pending.  ``prepare_fused`` returns False (the
    in-launch optimizer cannot wait for a second pass) and ``train_step(optimizer=...)`` refuses by name; ``step_ranges`` and
    ``dp.DataParallelStep`` refuse; a grouped optimizer that leaves a tensor in no group refuses (that tensor must keep every bit,
    and the norm's index set would differ).  A checkpoint, ``model.state_dict()`` or this optimizer's ``state_dict()`` taken WHILE a
    perturbation is pending holds ``w + e``, not ``w``: save after ``step()`` (or ``restore()``).  Under gradient accumulation the
    two passes are two sweeps over the group's micro-batches::

        optimizer.zero_grad()
        for mb in group:
            model.train_step(*mb, normalise=False)
        optimizer.grad_scale = model.loss_terms()[1:2]
        optimizer.first_step()
        optimizer.zero_grad()
        for mb in group:
            model.train_step(*mb, normalise=False)
        optimizer.step()

    None (the default): every launch of the step as it was, bit for bit."""

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_grad_norm: Optional[float] = None, *, params=None, decoupled_weight_decay: bool = False,
                 ema_decay: Optional[float] = None, ema_warmup: bool = False, watch=None, sam_rho: Optional[float] = None,
                 **torch_options):
        for k, v in torch_options.items():
            if k not in _TORCH_ONLY:
                raise TypeError(f"FusedAdam.__init__() got an unexpected keyword argument {k!r}")
            if v:
                raise ValueError(f"FusedAdam does not implement {k}={v!r} (torch.optim.Adam's option; only {k}=False / None is accepted)")
        self.model = model
        self.ema_decay = check_ema_decay(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self._ema: Optional[torch.Tensor] = None           # fp32, the layout of engine.flat; allocated at the first averaging step
        self._n_averaged = 0
        self._averaged_in = False                          # inside averaged_parameters(): model <-> average exchanged
        self.watch = watch                                 # watch.ModelWatch or None
        self._n_steps = 0                                  # optimizer steps taken (every form): the watch's schedule
        self.sam_rho = runtime.check_sam_rho(sam_rho)      # sharpness-aware minimisation: first_step() / step()
        self._sam_saved: Optional[torch.Tensor] = None     # fp32, the layout of engine.flat: w while w + e is in the model
        self._sam_scratch: Optional[torch.Tensor] = None   # float64 partial sums of squares, SAM's own (the clip keeps its own)
        self._sam_record: Optional[torch.Tensor] = None    # 4 fp32 on the device: norm, c, divisor, sqrt(sum of squares)
        self._sam_cfg = None
        self._sam_pending = False                          # between first_step() and step() / restore(): the model holds w + e
        # grouped: anything but ONE coupled group over model.parameters() - the hyper table and the grouped kernels instead of
        # the single-group entries
        self._grouped = params is not None or bool(decoupled_weight_decay)
        self._own_ids = {id(p) for p in model.parameters()}
        self._gsteps = []                                  # grouped: one step count per parameter group
        self._table: Optional[torch.Tensor] = None         # grouped: [16, 8] fp32 on the device (runtime.adam_hyper_groups)
        self._tg = self._tg_key = None                     # tensor -> group map (ctypes int array) and what it was built from
        self.max_grad_norm = max_grad_norm
        self._clip_scratch: Optional[torch.Tensor] = None  # float64 partial sums of squares (runtime.grad_norm_scratch)
        self._clip_record: Optional[torch.Tensor] = None   # 4 fp32 on the device: norm, coef, divisor, sqrt(sum of squares)
        self._clip_cfg = None
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        if self._grouped:
            # torch's own keys too, so that the groups of state_dict() load into torch.optim.Adam / AdamW, whose step() reads them
            defaults.update({k: (None if k in ("foreach", "fused") else False) for k in _TORCH_ONLY})
            defaults["decoupled_weight_decay"] = bool(decoupled_weight_decay)
        super().__init__(list(model.parameters()) if params is None else params, defaults)
        self._engine = None
        self._m = self._v = None
        self._step = 0
        self.grad_scale: Optional[torch.Tensor] = None     # device scalar: g <- g / grad_scale (data parallel)
        self._hyper: Optional[torch.Tensor] = None         # fused steps: lr / bc1, betas, eps, weight decay, 1 / sqrt(bc2) on the device
        self.grads_bf16: Optional[torch.Tensor] = None     # bf16 [n_params]: step() reads THIS instead of the fp32 gradient buffer (a plan
                                                           # armed with runtime.Plan.grad_bf16 left its gradients there, rounded once)

    def add_param_group(self, param_group):
        """torch's ``add_param_group`` with this optimizer's rules: the parameters are ``model``'s, at most 16 groups, no option this
        optimizer does not implement.  Works before and between steps; the new group's step count starts at 0.  A second group turns
        the single coupled group into a grouped optimizer (its count carries over).  With a weight average under way (``n_averaged``
        > 0) the EMA slices of the new group's tensors are seeded with their parameters - the copy a first update makes - so their
        average starts from the weights, not from the zeros of a slice that was never written."""
        self._refuse_averaged("add_param_group()")
        if not isinstance(param_group, dict):
            raise TypeError(f"param_group must be a dict (got {type(param_group).__name__})")
        ps = param_group["params"]
        ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
        foreign = [p for p in ps if id(p) not in self._own_ids]
        if foreign:
            raise ValueError(f"FusedAdam: {len(foreign)} parameter(s) of a group do not belong to the model (first shape: "
                             f"{tuple(foreign[0].shape)}); the optimizer updates the model's flat buffer only")
        if len(self.param_groups) >= MAX_GROUPS:
            raise ValueError(f"FusedAdam takes at most {MAX_GROUPS} parameter groups (the hyper table's rows)")
        for k in _TORCH_ONLY:
            if param_group.get(k):
                raise ValueError(f"FusedAdam does not implement {k}={param_group[k]!r} (parameter group {len(self.param_groups)})")
        if self.param_groups and not self._grouped:
            self._grouped = True
            self._gsteps = [self._step]
            self.param_groups[0].setdefault("decoupled_weight_decay", False)
            self.defaults.setdefault("decoupled_weight_decay", False)
        super().add_param_group({**param_group, "params": ps})
        self._gsteps.append(0)
        self._tg_key = None
        if self._ema is not None and self._n_averaged > 0 and self._engine is not None:
            at = {id(p): (o, n) for (p, o, n, _) in self._engine.items}
            with torch.no_grad():
                for p in ps:
                    if id(p) in at:
                        o, n = at[id(p)]
                        self._ema[o: o + n].copy_(self._engine.flat[o: o + n])

    def _unique_params(self):
        """The model's parameter tensors in parameter-map order (layout.param_specs == param_tables.hip::build_param_map; the engine's items)."""
        named = dict(self.model.named_parameters(remove_duplicate=False))
        seen, out = set(), []
        for sp in param_specs(self.model.m2f_config)[0]:
            p = named[sp.name]
            if sp.alias_of or id(p) in seen:
                continue
            seen.add(id(p))
            out.append(p)
        return out

    def tensor_group_map(self):
        """One int per parameter tensor in parameter-map order: the index of the group that owns it, -1 = none."""
        key = tuple(len(g["params"]) for g in self.param_groups)
        if self._tg_key != key:
            owner = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g["params"]}
            self._tg_list = [owner.get(id(p), -1) for p in self._unique_params()]
            self._tg = (ctypes.c_int * len(self._tg_list))(*self._tg_list)
            self._tg_key = key
        return list(self._tg_list)

    def _hyper_table(self, eng) -> torch.Tensor:
        if self._table is None or self._table.device != eng.flat.device:
            self._table = torch.zeros(MAX_GROUPS, 8, dtype=torch.float32, device=eng.flat.device)
        return self._table

    def _refresh_table(self, eng):
        """This step's row of every group into the device table (one launch, values by value: no sync); -> the tensor -> group map."""
        runtime.adam_hyper_groups(self._hyper_table(eng), [(float(g["lr"]), g["betas"], g["eps"], g["weight_decay"],
                                                 g.get("decoupled_weight_decay", self.defaults.get("decoupled_weight_decay", False)), t)
                                                for g, t in zip(self.param_groups, self._gsteps)])
        self.tensor_group_map()
        return self._tg

    def _owns_everything(self) -> bool:
        return -1 not in self.tensor_group_map()

    def _bind(self):
        eng = self.model.engine()
        if eng is not self._engine:
            old = {id(p): self.state.get(p) for g in self.param_groups for p in g["params"]}
            self._engine = eng
            self._m = torch.zeros_like(eng.flat)
            self._v = torch.zeros_like(eng.flat)
            for (p, o, n, s) in eng.items:
                st = old.get(id(p))
                mv, vv = self._m[o: o + n].view(s), self._v[o: o + n].view(s)
                if st:
                    mv.copy_(st["exp_avg"])
                    vv.copy_(st["exp_avg_sq"])
                    self.state[p] = {"step": st["step"], "exp_avg": mv, "exp_avg_sq": vv}
            if self._ema is not None:                      # (the flat layout is the configuration's: the same on the new engine)
                self._ema = self._ema.to(eng.flat.device) if self._ema.numel() == eng.flat.numel() else None
        return eng

    # ---- exponential moving average of the weights --------------------------------------------------------------------------------
    def _refuse_averaged(self, what: str) -> None:
        if self._averaged_in:
            raise RuntimeError(f"FusedAdam.{what} inside averaged_parameters(): the model holds the averaged weights; leave the context first")

    def _ema_begin(self, eng):
        """-> (average buffer, 1 - decay_t) of the optimizer step that begins, or (None, 0.0) without ``ema_decay``."""
        decay = check_ema_decay(self.ema_decay)
        if decay is None:
            return None, 0.0
        if self._ema is None or self._ema.device != eng.flat.device:
            self._ema = torch.zeros_like(eng.flat)
        w = 1.0 if self._n_averaged == 0 else 1.0 - ema_decay_at(decay, self._n_averaged, self.ema_warmup)
        return self._ema, w

    @property
    def n_averaged(self) -> int:
        """EMA updates so far (one per optimizer step taken with ``ema_decay`` set)."""
        return self._n_averaged

    def ema_parameters(self) -> torch.Tensor:
        """The average: flat fp32 device tensor, indexed like ``model.flat_parameters()`` (pads zero, the slices of tensors in no
        group untouched).  The optimizer's own buffer, not a copy."""
        self._refuse_averaged("ema_parameters()")
        if self._ema is None:
            raise RuntimeError("FusedAdam.ema_parameters: no EMA step has run yet (ema_decay is None, or step() has not been called)")
        return self._ema

    def _owned_ids(self):
        return {id(p) for g in self.param_groups for p in g["params"]}

    def ema_state_dict(self):
        """``{"decay", "warmup", "n_averaged", "parameters": {name: tensor}}``; ``parameters`` has the names and shapes of
        ``model.state_dict()`` and loads into the reference's ``M2FNet``.  A tensor in no parameter group is not averaged: its entry is
        its live value."""
        self._refuse_pending("ema_state_dict()")
        if self._ema is None:
            raise RuntimeError("FusedAdam.ema_state_dict: no EMA step has run yet (ema_decay is None, or step() has not been called)")
        eng = self._bind()
        at = {id(p): (o, n, s) for (p, o, n, s) in eng.items}
        named = dict(self.model.named_parameters(remove_duplicate=False))
        owned = self._owned_ids()
        src = eng.flat if self._averaged_in else self._ema            # (inside the context the model's buffer holds the average)
        out = {}
        for name, t in self.model.state_dict().items():
            p = named.get(name)
            if p is not None and id(p) in owned and id(p) in at:
                o, n, s = at[id(p)]
                out[name] = src[o: o + n].view(s).clone()
            else:
                out[name] = t.detach().clone()
        return {"decay": self.ema_decay, "warmup": self.ema_warmup, "n_averaged": self._n_averaged, "parameters": out}

    @torch.no_grad()
    def load_ema_state_dict(self, d) -> None:
        """Restores ``ema_state_dict()``'s value: strict about the names and shapes of ``parameters`` (those of ``model.state_dict()``).
        ``decay`` / ``warmup`` / ``n_averaged`` are taken over, so the warm-up continues where it was.  Entries of tensors in no group
        are checked and otherwise ignored."""
        self._refuse_averaged("load_ema_state_dict()")
        missing = [k for k in ("decay", "warmup", "n_averaged", "parameters") if k not in d]
        if missing:
            raise KeyError(f"FusedAdam.load_ema_state_dict: missing key(s) {missing}")
        want = self.model.state_dict()
        got = d["parameters"]
        if set(got) != set(want):
            raise KeyError(f"FusedAdam.load_ema_state_dict: parameter names differ (missing {sorted(set(want) - set(got))[:4]}, "
                           f"unexpected {sorted(set(got) - set(want))[:4]})")
        for k, t in want.items():
            if tuple(got[k].shape) != tuple(t.shape):
                raise ValueError(f"FusedAdam.load_ema_state_dict: {k!r} has shape {tuple(got[k].shape)}, the model's is {tuple(t.shape)}")
        decay = check_ema_decay(d["decay"])
        n = int(d["n_averaged"])
        if n < 0:
            raise ValueError(f"FusedAdam.load_ema_state_dict: n_averaged = {n}")
        eng = self._bind()
        at = {id(p): (o, m, s) for (p, o, m, s) in eng.items}
        named = dict(self.model.named_parameters(remove_duplicate=False))
        owned = self._owned_ids()
        ema = torch.zeros_like(eng.flat)
        for name, t in got.items():
            p = named.get(name)
            if p is not None and id(p) in owned and id(p) in at:
                o, m, s = at[id(p)]
                ema[o: o + m].view(s).copy_(t)
        self._ema, self._n_averaged = ema, n
        self.ema_decay, self.ema_warmup = decay, bool(d["warmup"])

    def _exchange(self, eng) -> None:
        self.tensor_group_map()
        runtime.ema_exchange(eng.cfg, eng.flat, self._ema, self._tg)
        eng.invalidate_shadows()                           # (written behind torch's version counters: the next forward re-casts)

    @contextlib.contextmanager
    def averaged_parameters(self):
        """``with optimizer.averaged_parameters():`` - the model's parameters ARE the averaged weights inside: one exchange launch on
        entry swaps every owned tensor with its average in place, the same launch on exit swaps them back, bit for bit.  Inside,
        ``model.state_dict()``, ``forward``, ``eval_step`` and a checkpoint see the average (the bf16 shadows are re-cast by the next
        forward, inside and again after); ``step()``, ``step_ranges()``, ``prepare_fused()`` and a nested entry raise."""
        self._refuse_averaged("averaged_parameters()")
        self._refuse_pending("averaged_parameters()")
        if self._ema is None or self._n_averaged == 0:
            raise RuntimeError("FusedAdam.averaged_parameters: there is no average yet (no step has run with ema_decay set)")
        eng = self._bind()
        self._exchange(eng)
        self._averaged_in = True
        try:
            yield self
        finally:
            self._exchange(eng)
            self._averaged_in = False

    def _materialise_state(self, eng):
        for (p, o, n, s) in eng.items:
            if p not in self.state or not self.state[p]:
                self.state[p] = {"step": torch.tensor(float(self._step)),
                                 "exp_avg": self._m[o: o + n].view(s), "exp_avg_sq": self._v[o: o + n].view(s)}

    # ---- model watch ------------------------------------------------------------------------------------------------------------
    def _watch_due(self):
        """Counts the optimizer step that begins; -> the attached watch when that step is due, else None."""
        n, self._n_steps = self._n_steps, self._n_steps + 1
        w = self.watch
        if w is None or not w.due(n):
            return None
        w.begin(n)
        return w

    def _watch_before(self, w, eng, flat_grad) -> None:
        """The due step's collections on the buffers as they are before the update kernels; `flat_grad` None: no gradient buffer."""
        for kind in w.kinds:
            if kind == "gradients" and flat_grad is not None:
                w.collect(kind, flat_grad, den=self.grad_scale)
            elif kind == "parameters":
                w.collect(kind, eng.flat)
            elif kind == "exp_avg":
                w.collect(kind, self._m)
            elif kind == "exp_avg_sq":
                w.collect(kind, self._v)
            elif kind == "ema" and self._ema is not None and self._n_averaged > 0:
                w.collect(kind, self._ema)
            elif kind == "updates" and flat_grad is not None:
                w.snapshot(eng.flat)

    def _watch_after(self, w, eng) -> None:
        if w is not None and "updates" in w.kinds:
            w.collect("updates", eng.flat, other=w._snapshot)

    def _clip(self, eng, flat_grad) -> Optional[torch.Tensor]:
        """-> the device scalar the Adam kernels divide the gradients by: ``grad_scale`` itself without clipping; with it, the
        divisor of the clip record, written by the two norm launches over `flat_grad` on the current stream."""
        if self.max_grad_norm is None:
            return self.grad_scale
        max_norm = float(self.max_grad_norm)
        if not max_norm > 0.0:
            raise ValueError(f"FusedAdam.max_grad_norm must be a positive number or None (got {self.max_grad_norm!r})")
        if self._clip_record is None or self._clip_record.device != eng.flat.device or self._clip_cfg is not eng.cfg:
            self._clip_scratch = runtime.grad_norm_scratch(eng.cfg, eng.flat.device)
            self._clip_record = torch.zeros(4, dtype=torch.float32, device=eng.flat.device)
            self._clip_cfg = eng.cfg
        runtime.grad_sumsq(eng.cfg, flat_grad, self._clip_scratch)
        runtime.grad_norm_finalize(eng.cfg, self._clip_scratch, self._clip_record, max_norm, self.grad_scale)
        return self._clip_record[2:3]

    def _clip_value(self, i: int, what: str) -> torch.Tensor:
        if self._clip_record is None:
            raise RuntimeError(f"FusedAdam.{what}: no step has clipped yet (max_grad_norm is None, or step() has not run)")
        return self._clip_record[i]

    def grad_norm(self) -> torch.Tensor:
        """Device scalar (a view: the next clipping step overwrites it): global L2 norm of the gradient the last clipping step
        read, divided by ``grad_scale`` - what ``clip_grad_norm_`` returns for the gradients Adam used."""
        return self._clip_value(0, "grad_norm")

    def clip_coef(self) -> torch.Tensor:
        """Device scalar (a view): ``min(1, max_grad_norm / (grad_norm + 1e-6))`` of the last clipping step."""
        return self._clip_value(1, "clip_coef")

    def _grad_buffer(self, eng) -> torch.Tensor:
        """The flat gradient buffer ``step()`` reads: the bf16 buffer where a step left its gradients rounded (M2FNet.set_grad_bf16),
        else the engine's fp32 buffer - after gathering foreign ``.grad`` tensors into it where the engine's views are not published."""
        flat_grad = eng.ensure_grad()
        # fast path: the engine published its flat-buffer views as .grad (checked on the two end parameters);
        # otherwise gather foreign .grad tensors into the flat buffer first
        first, last = eng.items[0][0], eng.items[-1][0]
        if self.grads_bf16 is not None or eng.grad_bf16_buf is not None:      # the step left its gradients rounded to bf16 (M2FNet.set_grad_bf16)
            flat_grad = self.grads_bf16 if self.grads_bf16 is not None else eng.grad_bf16_buf
        elif not (first.grad is eng.grad_views[0] and last.grad is eng.grad_views[-1]):
            for (p, o, n, s), view in zip(eng.items, eng.grad_views):
                if p.grad is None:
                    view.zero_()
                elif p.grad.data_ptr() != view.data_ptr():
                    view.copy_(p.grad)
        return flat_grad

    # ---- sharpness-aware minimisation ---------------------------------------------------------------------------------------------
    def _refuse_pending(self, what: str) -> None:
        if self._sam_pending:
            raise RuntimeError(f"FusedAdam.{what} while a sharpness-aware perturbation is pending: the model holds w + e; call step() "
                               "or restore() first")

    @property
    def sam_pending(self) -> bool:
        """Between ``first_step()`` and ``step()`` / ``restore()``: the model's parameters are ``w + e``."""
        return self._sam_pending

    @torch.no_grad()
    def first_step(self) -> None:
        """SAM's ascent step on the gradient ``step()`` would read now: ``w <- w + sam_rho * g / (||g|| + 1e-12)`` (class docstring).
        Three launches on the current stream - the sum of squares, the record with the coefficient, the perturbation - and no host
        wait.  Run ``train_step`` on the same batch next, then ``step()``."""
        self._refuse_averaged("first_step()")
        rho = runtime.check_sam_rho(self.sam_rho)
        if rho is None:
            raise RuntimeError("FusedAdam.first_step(): sam_rho is None; set it to the perturbation's radius first")
        if self._sam_pending:
            raise RuntimeError("FusedAdam.first_step(): a perturbation is already pending (the model holds w + e); call step() or "
                               "restore() first")
        if self._grouped and not self._owns_everything():
            raise RuntimeError("FusedAdam.first_step(): sharpness-aware minimisation needs parameter groups that cover every tensor of "
                               "the model - a tensor in no group must keep every bit, and the norm would run over another index set")
        eng = self._bind()
        flat_grad = self._grad_buffer(eng)
        if self._sam_record is None or self._sam_record.device != eng.flat.device or self._sam_cfg is not eng.cfg:
            self._sam_scratch = runtime.grad_norm_scratch(eng.cfg, eng.flat.device)
            self._sam_record = torch.zeros(4, dtype=torch.float32, device=eng.flat.device)
            self._sam_saved = torch.zeros_like(eng.flat)
            self._sam_cfg = eng.cfg
        runtime.grad_sumsq(eng.cfg, flat_grad, self._sam_scratch)
        runtime.sam_perturb(eng.cfg, eng.flat, flat_grad, self._sam_saved, eng.wshadow, self._sam_scratch, self._sam_record, rho,
                            self.grad_scale)
        if eng.wshadow is not None:
            eng.mark_shadows_fresh()                         # (the kernel wrote W and W^T of every matrix from w + e)
        self._sam_pending = True

    def _sam_restore(self, eng) -> None:
        runtime.sam_restore(eng.cfg, eng.flat, self._sam_saved)
        eng.invalidate_shadows()                             # (they hold w + e until an optimizer kernel or the forward's casts rewrite them)
        self._sam_pending = False

    @torch.no_grad()
    def restore(self) -> bool:
        """Abandons a pending perturbation: the parameters get their bits from before ``first_step()`` (one launch) and the bf16
        shadows are invalidated (the next forward re-casts them).  Returns whether there was one; without one it does nothing."""
        if not self._sam_pending:
            return False
        self._sam_restore(self._bind())
        return True

    def sam_norm(self) -> torch.Tensor:
        """Device scalar (a view: the next ``first_step()`` overwrites it): L2 norm of the gradient the last ``first_step()`` read,
        divided by ``grad_scale``."""
        if self._sam_record is None:
            raise RuntimeError("FusedAdam.sam_norm: first_step() has not run yet")
        return self._sam_record[0]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._refuse_averaged("step()")
        if not self._sam_pending and runtime.check_sam_rho(self.sam_rho) is not None:
            raise RuntimeError("FusedAdam.step(): sam_rho is set and no perturbation is pending - this step would train without "
                               "sharpness-aware minimisation; call first_step() and a second train_step first (M2FNet.sam_step does), "
                               "or set sam_rho = None")
        eng = self._bind()
        if self._sam_pending:                                # w's bits from before first_step(), then today's step on the second gradient
            self._sam_restore(eng)
        ema, ema_w = self._ema_begin(eng)                    # one average update per optimizer step: every launch gets the same weight
        g = self.param_groups[0]
        flat_grad = self._grad_buffer(eng)
        watch = self._watch_due()
        if watch is not None:
            self._watch_before(watch, eng, flat_grad)
        if self._grouped:
            self._gsteps = [t + 1 for t in self._gsteps]
            scale = self._clip(eng, flat_grad)
            tg = self._refresh_table(eng)
            # the owned tensors with their group's row: shadow-writing kernel (bf16 mode) or slices (fp32 mode).  Tensors of no group are
            # not touched, so their shadows stay what they were: fresh before = fresh after (the version counters do not move)
            runtime.adam_step_grouped(eng.cfg, eng.flat, flat_grad, self._m, self._v, eng.wshadow, tg, self._table, scale,
                                      ema=ema, ema_w=ema_w)
            self._n_averaged += ema is not None
            self._watch_after(watch, eng)
            if eng.wshadow is not None and self._owns_everything():
                eng.mark_shadows_fresh()
            return loss
        self._step += 1
        scale = self._clip(eng, flat_grad)                   # grad_scale, or the clip record's divisor (max_grad_norm)
        if eng.wshadow is not None:
            # bf16 mode: the update and the bf16 shadows (W, W^T) of every 2-D parameter in ONE pass - the forward then skips its
            # parameter casts (engine.shadows_fresh)
            runtime.adam_step_shadowed(eng.cfg, eng.flat, flat_grad, self._m, self._v, eng.wshadow, self._step, g["lr"], g["betas"],
                                       g["eps"], g["weight_decay"], scale, ema=ema, ema_w=ema_w)
            eng.mark_shadows_fresh()
        else:
            runtime.adam_step(eng.flat, flat_grad, self._m, self._v, self._step, g["lr"], g["betas"], g["eps"],
                              g["weight_decay"], scale, ema=ema, ema_w=ema_w)
        self._n_averaged += ema is not None
        self._watch_after(watch, eng)
        return loss

    @torch.no_grad()
    def prepare_fused(self, plan) -> bool:
        """Arms `plan` so that its NEXT ``step()`` is also THIS optimizer's step: the weight-gradient launch applies the update to
        the elements whose gradient it holds in registers, one more launch inside the same graph updates the rest (bf16 mode, one
        process; csrc/gemm_p8.h EPI 3).  Same arithmetic on the same gradients as ``step()`` - bit-identical parameters, moments and
        parameter shadows (tests/test_fused_adam_gpu.py) - but the weight gradients of the table's matrices never reach memory:
        their ``.grad`` keeps whatever it held.  Returns False (and changes nothing) when the plan cannot; call ``finish_fused``
        after the step.  With ``max_grad_norm`` set it returns False: the in-launch optimizer updates elements before the global norm
        can exist, so ``train_step(optimizer=...)`` takes its two-launch branch (the step, then ``step()``).  With ``ema_decay`` set it
        returns False as well: the in-launch optimizer has no EMA stream (its epilogue is at its register budget).  With ``sam_rho`` set
        it returns False too: the in-launch optimizer cannot wait for SAM's second pass."""
        self._refuse_averaged("prepare_fused()")
        self._refuse_pending("prepare_fused()")
        if self.max_grad_norm is not None or self.ema_decay is not None or self.sam_rho is not None:
            return False
        if self.watch is not None and ("gradients" in self.watch.kinds or "updates" in self.watch.kinds):
            return False
        eng = self._bind()
        if eng.wshadow is None or not plan.train or not getattr(plan, "shared_shadow", False):
            return False
        if self._grouped:
            return self._prepare_fused_grouped(eng, plan)
        if plan._fused_bad:
            return False
        if self._hyper is None:
            self._hyper = torch.zeros(8, dtype=torch.float32, device=eng.flat.device)
        key = (self._m.data_ptr(), self._v.data_ptr(), eng.flat.data_ptr(), eng.wshadow.data_ptr(), self._hyper.data_ptr(),
               self.grad_scale.data_ptr() if self.grad_scale is not None else 0)
        if plan._fused_key != key:
            try:
                eng.ensure_grad()
                plan.fused_adam_setup(eng.flat, self._m, self._v, eng.wshadow, self._hyper, self.grad_scale)
            except runtime.HipError as e:
                plan._fused_bad = True                     # (another table form, ...): the caller takes the two-launch path
                plan._fused_err = str(e)
                return False
            plan._fused_key = key
        g = self.param_groups[0]
        self._step += 1
        watch = self._watch_due()
        if watch is not None:
            self._watch_before(watch, eng, None)
        runtime.adam_hyper(self._hyper, self._step, g["lr"], g["betas"], g["eps"], g["weight_decay"])
        plan.fused_adam(True)
        return True

    def _prepare_fused_grouped(self, eng, plan) -> bool:
        # the in-launch form with groups (gemm_p8.h EPI 6): every matrix of the weight-gradient table must be owned - the launch holds
        # its gradient in registers and has nowhere else to put it; otherwise the two-launch branch
        tg = self.tensor_group_map()
        key = ("grouped", tuple(tg), self._m.data_ptr(), self._v.data_ptr(), eng.flat.data_ptr(), eng.wshadow.data_ptr(),
               self._hyper_table(eng).data_ptr(), self.grad_scale.data_ptr() if self.grad_scale is not None else 0)
        if plan._fused_bad_key == key:
            return False
        if plan._fused_key != key:
            try:
                eng.ensure_grad()
                plan.fused_adam_setup_grouped(eng.flat, self._m, self._v, eng.wshadow, self._table, tg, self.grad_scale)
            except runtime.HipError as e:
                plan._fused_key = None                     # (a failed setup leaves the plan without one)
                plan._fused_bad_key = key
                plan._fused_err = str(e)
                return False
            plan._fused_key = key
        self._gsteps = [t + 1 for t in self._gsteps]
        watch = self._watch_due()
        if watch is not None:
            self._watch_before(watch, eng, None)
        self._refresh_table(eng)
        plan.fused_adam(True)
        return True

    def finish_fused(self, plan) -> None:
        """After the armed step: the kernels wrote every parameter and both bf16 shadows of every matrix (grouped: of every owned
        one - the others kept theirs, fresh if they were)."""
        plan.fused_adam(False)
        if not self._grouped or self._owns_everything():
            self._engine.mark_shadows_fresh()

    @torch.no_grad()
    def step_ranges(self, ranges, before_each=None, grads=None):
        """One optimizer step issued as several kernel launches over contiguous element ranges [(lo, hi), ...] of the
        flat buffers (hi clipped to the parameter count; lo, hi multiples of 4).  `before_each(i)` runs before range i
        is launched - the data-parallel path waits there for that range's all-reduce, so the update of one bucket
        overlaps the exchange of the next.  `grads`: gradient buffer to read instead of the engine's (same indexing;
        fp32 or bf16 - the reduced buffer of the bf16 exchange).  Ranges made of whole parameter tensors keep the bf16
        parameter shadows current (m2f_adam_step_shadowed_range); other ranges leave them to the next forward's casts.
        With ``max_grad_norm`` set the global norm needs every range's gradients: `before_each` runs for ALL ranges first, then the
        norm launches over the whole buffer, then the ranges' updates with the clip record's divisor - the updates no longer hide
        under the exchange of the following buckets; that is the price of a global norm.  A due step of an attached ``watch`` does the
        same, on that step only: every range's `before_each` first, then the collections over the whole buffers, then the updates.
        Refused (RuntimeError) with ``sam_rho`` set: sharpness-aware minimisation under data parallelism is not implemented."""
        self._refuse_averaged("step_ranges()")
        self._refuse_pending("step_ranges()")
        if runtime.check_sam_rho(self.sam_rho) is not None:
            raise RuntimeError("FusedAdam.step_ranges(): sharpness-aware minimisation (sam_rho) is not implemented for range-wise steps "
                               "(the data-parallel path); set sam_rho = None")
        eng = self._bind()
        g = self.param_groups[0]
        flat_grad = eng.ensure_grad() if grads is None else grads
        n = eng.flat.numel()
        ranges = [(lo, min(hi, n)) for (lo, hi) in ranges]
        ema, ema_w = self._ema_begin(eng)                    # the SAME weight for every range of this step
        watch = self._watch_due()
        if self._grouped:
            self._step_ranges_grouped(eng, flat_grad, ranges, before_each, n, ema, ema_w, watch)
            self._n_averaged += ema is not None
            self._watch_after(watch, eng)
            return
        self._step += 1
        scale, before_each = self._gather_then_clip(eng, flat_grad, len(ranges), before_each, watch)
        # bf16 mode with the model-wide parameter shadows: ranges that start and end at parameter tensors (dp.GradReducer aligns its
        # buckets that way) go through the shadow-writing kernel, so the next forward needs no parameter casts under data parallelism
        # either; anything else updates the parameters only and the next forward re-casts
        starts = self._tensor_starts(eng)
        shadowed = eng.wshadow is not None and all(lo in starts and (hi >= n or hi in starts) for lo, hi in ranges if hi > lo)
        if not shadowed:
            eng.invalidate_shadows()
        for i, (lo, hi) in enumerate(ranges):
            if before_each is not None:
                before_each(i)
            if hi <= lo:
                continue
            if shadowed:
                runtime.adam_step_shadowed(eng.cfg, eng.flat, flat_grad, self._m, self._v, eng.wshadow, self._step, g["lr"], g["betas"],
                                           g["eps"], g["weight_decay"], scale, first=lo, end=(-1 if hi >= n else hi), ema=ema, ema_w=ema_w)
            else:
                runtime.adam_step(eng.flat[lo:hi], flat_grad[lo:hi], self._m[lo:hi], self._v[lo:hi], self._step, g["lr"],
                                  g["betas"], g["eps"], g["weight_decay"], scale, ema=None if ema is None else ema[lo:hi], ema_w=ema_w)
        self._n_averaged += ema is not None
        self._watch_after(watch, eng)
        if shadowed:
            if self._cover_everything(ranges, n):
                eng.mark_shadows_fresh()
            else:
                eng.invalidate_shadows()

    def _step_ranges_grouped(self, eng, flat_grad, ranges, before_each, n, ema=None, ema_w=0.0, watch=None):
        starts = self._tensor_starts(eng)
        for lo, hi in ranges:
            if hi > lo and not (lo in starts and (hi >= n or hi in starts)):
                raise ValueError(f"FusedAdam.step_ranges: the range [{lo}, {hi}) cuts a parameter tensor; an optimizer with parameter "
                                 "groups / decoupled weight decay takes ranges of whole tensors only (dp.GradReducer's buckets are)")
        self._gsteps = [t + 1 for t in self._gsteps]
        scale, before_each = self._gather_then_clip(eng, flat_grad, len(ranges), before_each, watch)
        tg = self._refresh_table(eng)
        for i, (lo, hi) in enumerate(ranges):
            if before_each is not None:
                before_each(i)
            if hi > lo:
                runtime.adam_step_grouped(eng.cfg, eng.flat, flat_grad, self._m, self._v, eng.wshadow, tg, self._table, scale,
                                          first=lo, end=(-1 if hi >= n else hi), ema=ema, ema_w=ema_w)
        if eng.wshadow is not None:
            if not self._cover_everything(ranges, n):
                eng.invalidate_shadows()
            elif self._owns_everything():
                eng.mark_shadows_fresh()

    def _gather_then_clip(self, eng, flat_grad, n_ranges, before_each, watch):
        """-> (the divisor of this step's updates, the `before_each` the range loop still has to call).  With ``max_grad_norm`` or a due
        watch every range's `before_each` runs first, then the watch's collections and the norm over the whole buffer."""
        if self.max_grad_norm is None and watch is None:
            return self.grad_scale, before_each
        if before_each is not None:
            for i in range(n_ranges):
                before_each(i)
        if watch is not None:
            self._watch_before(watch, eng, flat_grad)
        return self._clip(eng, flat_grad), None

    @staticmethod
    def _cover_everything(ranges, n) -> bool:
        """The non-empty ranges, put in order, tile [0, n) without a gap."""
        covered = sorted((lo, hi) for lo, hi in ranges if hi > lo)
        return bool(covered) and covered[0][0] == 0 and covered[-1][1] >= n and all(a[1] == b[0] for a, b in zip(covered, covered[1:]))

    def _tensor_starts(self, eng):
        if getattr(self, "_starts_of", None) is not eng:
            self._starts = frozenset(int(o) for (_, o, _, _) in eng.items)
            self._starts_of = eng
        return self._starts

    def state_dict(self):
        if self._grouped:
            if self._engine is not None:
                at = {id(p): (o, n, s) for (p, o, n, s) in self._engine.items}
                for g, t in zip(self.param_groups, self._gsteps):
                    for p in (g["params"] if t > 0 else ()):                   # (a group that never stepped has no state, as in torch)
                        o, n, s = at[id(p)]
                        self.state[p] = {"step": torch.tensor(float(t)), "exp_avg": self._m[o: o + n].view(s),
                                         "exp_avg_sq": self._v[o: o + n].view(s)}
            return super().state_dict()
        if self._engine is not None and self._step > 0:
            self._materialise_state(self._engine)
            for p in self.param_groups[0]["params"]:
                self.state[p]["step"] = torch.tensor(float(self._step))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        eng = self.model.engine()
        self._engine = eng
        self._m = torch.zeros_like(eng.flat)
        self._v = torch.zeros_like(eng.flat)
        steps = [int(st["step"]) for st in self.state.values() if st and "step" in st]
        self._step = max(steps) if steps else 0
        if self._grouped:                                  # every group's own count: what its parameters carry
            self._gsteps = [max([int(self.state[p]["step"]) for p in g["params"] if self.state.get(p) and "step" in self.state[p]] or [0])
                            for g in self.param_groups]
            self._tg_key = None
        for (p, o, n, s) in eng.items:
            st = self.state.get(p)
            if st:
                mv, vv = self._m[o: o + n].view(s), self._v[o: o + n].view(s)
                mv.copy_(st["exp_avg"])
                vv.copy_(st["exp_avg_sq"])
                st["exp_avg"], st["exp_avg_sq"] = mv, vv


class FusedAdamW(FusedAdam):
    """``torch.optim.AdamW`` (the reference's stage-1 trainers, feature_extractors/text/train.py:62-63; the M2FNet paper's optimizer):
    ``FusedAdam`` with decoupled weight decay and AdamW's default ``weight_decay=1e-2``.  ``params`` as in ``FusedAdam``."""

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_grad_norm: Optional[float] = None, *, params=None, ema_decay: Optional[float] = None, ema_warmup: bool = False,
                 watch=None, sam_rho: Optional[float] = None, **torch_options):
        super().__init__(model, lr, betas, eps, weight_decay, max_grad_norm, params=params, decoupled_weight_decay=True,
                         ema_decay=ema_decay, ema_warmup=ema_warmup, watch=watch, sam_rho=sam_rho, **torch_options)
