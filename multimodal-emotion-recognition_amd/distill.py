"""Knowledge distillation: train an online (causal or windowed) ``M2FNet`` against the logits of an offline teacher of the same family.

The criterion is one kernel inside the student's train step (``M2FNet.train_step(..., teacher_logits=u, distill=(alpha,
temperature))``; csrc/rowops.hip ``m2f_ce_distill_kernel``): per labelled row

    num = (1 - alpha) * CE numerator + alpha * temperature^2 * w_y * KL(softmax(u / temperature) || softmax(z / temperature))
    den = w_y

and loss = sum num / sum den - the ONE denominator the hard-label criterion has, so gradient accumulation, the data-parallel
division by the global den, bf16 gradients, the optimizer inside the step and clipping work as they do without a teacher.

``Distiller`` holds a student and a frozen teacher and runs the teacher's eval forward in front of the student's step; teacher logits
cached with a dataset go to ``train_step`` directly.  The argument checks below need no device."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch


def check_distill(distill, who: str = "train_step") -> Tuple[float, float]:
    """``distill=(alpha, temperature)`` -> the pair as floats; ValueError unless alpha is a number in [0, 1] and temperature a finite
    number > 0."""
    try:
        alpha, temperature = distill
    except (TypeError, ValueError):
        raise ValueError(f"{who}: distill must be a pair (alpha, temperature), got {distill!r}") from None
    for name, v in (("alpha", alpha), ("temperature", temperature)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"{who}: distill {name} must be a number, got {v!r}")
    if not 0.0 <= alpha <= 1.0:                            # (NaN fails both comparisons)
        raise ValueError(f"{who}: distill alpha must be in [0, 1], got {alpha!r}")
    if not (math.isfinite(temperature) and temperature > 0.0):
        raise ValueError(f"{who}: distill temperature must be finite and > 0, got {temperature!r}")
    return float(alpha), float(temperature)


def _same_device(a: torch.device, b: torch.device) -> bool:
    a, b = torch.device(a), torch.device(b)
    return a.type == b.type and (a.index or 0) == (b.index or 0)


def check_teacher_logits(teacher_logits, B: int, L: int, C: int, device, who: str = "train_step") -> None:
    """ValueError unless `teacher_logits` is an fp32 tensor [B, L, C] on `device`."""
    if not isinstance(teacher_logits, torch.Tensor):
        raise ValueError(f"{who}: teacher_logits must be a tensor, got {type(teacher_logits).__name__}")
    if teacher_logits.dtype != torch.float32:
        raise ValueError(f"{who}: teacher_logits must be float32, got {teacher_logits.dtype}")
    if tuple(teacher_logits.shape) != (B, L, C):
        raise ValueError(f"{who}: teacher_logits must be [B, L, cls_out] = {(B, L, C)}, got {tuple(teacher_logits.shape)}")
    if not _same_device(teacher_logits.device, device):
        raise ValueError(f"{who}: teacher_logits are on {teacher_logits.device}, the model is on {device}")


def resolve_distill_args(teacher_logits, distill, B: int, L: int, C: int, device, who: str = "train_step") -> Optional[Tuple[float, float]]:
    """The two distillation arguments of a step: both None -> None (the plain criterion); both given and valid -> (alpha,
    temperature); anything else is a ValueError - raised before any launch or plan change."""
    if teacher_logits is None and distill is None:
        return None
    if teacher_logits is None or distill is None:
        raise ValueError(f"{who}: teacher_logits and distill=(alpha, temperature) go together (got "
                         f"{'no ' if teacher_logits is None else ''}teacher_logits and {'no ' if distill is None else ''}distill)")
    pair = check_distill(distill, who)
    check_teacher_logits(teacher_logits, B, L, C, device, who)
    return pair


# what student and teacher must share: the label set and the inputs (everything else - widths of the hidden layers, depth, heads,
# context band, precision - may differ)
_SHARED_FIELDS = ("cls_out", "audio_enabled", "text_enabled", "d_audio", "d_text")


def check_pair(student_cfg, teacher_cfg) -> None:
    """ValueError naming the first M2FConfig field in which a teacher may not differ from its student.  The input width of a
    disabled modality is not compared."""
    for f in _SHARED_FIELDS:
        if f == "d_audio" and not student_cfg.audio_enabled or f == "d_text" and not student_cfg.text_enabled:
            continue
        a, b = getattr(student_cfg, f), getattr(teacher_cfg, f)
        if a != b:
            raise ValueError(f"Distiller: student and teacher differ in {f} ({a!r} vs {b!r}); they must agree in "
                             f"{', '.join(_SHARED_FIELDS)}")


class Distiller:
    """``Distiller(student, teacher, alpha=0.5, temperature=2.0)``: the student (an ``M2FNet``, usually ``context=(past, 0)``) trains
    against the logits of ``teacher`` (an ``M2FNet`` of any widths, depth and context - usually the offline ``(None, None)`` - with the
    student's ``cls_out``, enabled modalities and input widths).  The teacher is put in eval mode with ``requires_grad_(False)``; it
    keeps its own engine, plans and precision, and is never written.  Its forward runs under ``torch.inference_mode()``; its engine and
    plans are created outside it, so the teacher can still be scored elsewhere under ``torch.no_grad()``.

    ``train_step(text, audio, mask, emotion, **kw)`` = the teacher's eval forward, then ``student.train_step(..., teacher_logits=,
    distill=(alpha, temperature), **kw)``: no step waits for the host (the first call builds plans and copies the pair from the host, as any first step does).  ``alpha`` and ``temperature`` are plain attributes,
    read at every step (a schedule sets them between steps; captured steps replay, the pair lives on the device)."""

    def __init__(self, student, teacher, alpha: float = 0.5, temperature: float = 2.0):
        check_pair(student.m2f_config, teacher.m2f_config)
        self.alpha, self.temperature = check_distill((alpha, temperature), "Distiller")
        self.student, self.teacher = student, teacher
        teacher.eval()
        teacher.requires_grad_(False)

    def teacher_logits(self, text, audio, mask, speakers=None) -> torch.Tensor:
        """The teacher's logits [B, L, cls_out] of the batch: its eval forward under ``torch.inference_mode()``, no host sync (a
        packed teacher counts the batch's valid utterances on the host, as its forward always does).  speakers: the batch's ids -
        handed on only if the TEACHER has speaker heads (it runs under its own setting)."""
        if self.teacher.training:
            self.teacher.eval()
        if mask.shape[0] == 0:                             # (an empty shard of a data-parallel batch)
            return torch.zeros(0, mask.shape[1], self.teacher.m2f_config.cls_out, dtype=torch.float32, device=mask.device)
        self.teacher.engine(mask.device)                   # (built outside inference mode: its buffers stay ordinary tensors)
        with torch.inference_mode():
            if self.teacher.speaker_heads is not None:
                return self.teacher(text, audio, mask, speakers=speakers)
            return self.teacher(text, audio, mask)

    def train_step(self, text, audio, mask, emotion, speakers=None, **kw) -> torch.Tensor:
        """speakers ([B, L] ids): student and teacher each run under their OWN speaker-head setting, and the batch's ids go to
        whichever of the two has one; needed as soon as either has, refused (ValueError) when neither does.
        focal_gamma= (in ``kw``) goes to the student's step: the focal factor scales its hard-label term, the teacher term stays.
        rdrop=, supcon= and aux= are refused by name: none of them has a distillation form."""
        pair = check_distill((self.alpha, self.temperature), "Distiller")          # (before the teacher runs)
        from .criterion import resolve
        c = self.student.m2f_config
        spec = resolve("Distiller.train_step", num_classes=c.cls_out, cls_hidden=c.cls_hidden, mask_shape=mask.shape, device=mask.device,
                       label_smoothing=None, class_weights=None, distilling=True,       # (neither is looked at before the teacher runs)
                       **{name: kw.get(name) for name in ("focal_gamma", "rdrop", "supcon", "aux")})
        if spec.gamma is not None:
            kw["focal_gamma"] = spec.gamma
        s_on, t_on = self.student.speaker_heads is not None, self.teacher.speaker_heads is not None
        if speakers is not None and not (s_on or t_on):
            raise ValueError("Distiller.train_step: speakers were given, but neither the student nor the teacher has speaker heads")
        if speakers is None and (s_on or t_on):
            raise ValueError("Distiller.train_step: the " + ("student" if s_on else "teacher") + " has speaker heads; pass speakers= ([B, L] ids)")
        u = self.teacher_logits(text, audio, mask, speakers)
        if s_on:
            kw["speakers"] = speakers
        return self.student.train_step(text, audio, mask, emotion, teacher_logits=u, distill=pair, **kw)
