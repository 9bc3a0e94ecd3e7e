"""The criterion arguments of a step as ONE checked value, and the ONE table of what combines with what.

Six criteria live inside the train step: distillation, focal, CRF, R-Drop, supervised contrastive and the auxiliary head.  ``resolve``
turns the keyword arguments of ``M2FNet.train_step`` / ``eval_step``, ``DataParallelStep`` and ``Distiller.train_step`` into a
``Criterion`` - or raises the ValueError that names the pair - and ``runtime.Plan.set_criterion`` turns a ``Criterion`` into the plan's
switches.  A new criterion declares here what it combines with: a field of ``Criterion``, a row of ``RULES`` per argument or
circumstance it is refused beside, an entry of ``COMBINES`` per pair that has a kernel, and its place in ``PRIORITY``.

A host module: nothing here needs a device, and no GPU code is imported until a value checker is called."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional, Tuple

KINDS = ("distill", "focal", "crf", "rdrop", "supcon", "aux")
ARGUMENTS = ("teacher_logits", "distill", "focal_gamma", "crf", "rdrop", "supcon", "aux")


@dataclass(frozen=True, eq=False)
class Criterion:
    """The checked criterion arguments of one step; every field None: the plain cross entropy (``PLAIN``)."""
    distill: Optional[Tuple[float, float]] = None            # (alpha, temperature)
    teacher_logits: Any = None                                # fp32 [B, L, cls_out] on the step's device
    gamma: Optional[float] = None                             # focal
    crf: Any = None                                           # a crf.LinearChainCRF
    rdrop: Optional[float] = None                             # alpha
    supcon: Optional[Tuple[float, float]] = None              # (weight, temperature)
    aux: Optional[tuple] = None                               # (head, labels, weight, label smoothing)

    @property
    def kinds(self) -> Tuple[str, ...]:
        """Which of KINDS are on."""
        on = (self.distill, self.gamma, self.crf, self.rdrop, self.supcon, self.aux)
        return tuple(k for k, v in zip(KINDS, on) if v is not None)

    @property
    def term_weight(self) -> float:
        """The weight of the term whose sum the criterion tail's fourth float holds (R-Drop's alpha, the contrastive or the auxiliary
        weight); 0.0 when no such term is on."""
        for v in (self.rdrop, self.supcon and self.supcon[0], self.aux and self.aux[2]):
            if v is not None:
                return v
        return 0.0


PLAIN = Criterion()

# ---- the rule table ------------------------------------------------------------------------------------------------------------------
# The pairs of KINDS that have a kernel.  Every other pair is refused by a row of RULES (tests/test_criterion_resolve_cpu.py holds the
# two to each other, and csrc/plan.hip's exclusions[] refuses the same pairs on the device side).
COMBINES = frozenset({frozenset({"distill", "focal"}), frozenset({"aux", "focal"})})

_FORM = {"teacher_logits": "distillation", "distill": "distillation", "focal_gamma": "focal", "crf": "CRF", "rdrop": "R-Drop"}


def _no_form(subject: str, owner: str, others) -> list:
    return [(o, f"{subject} and {o} do not combine (the {owner} has no {_FORM[o]} form)") for o in others]


_CRF_DISTILL = "crf= does not combine with teacher_logits / distill (the CRF criterion has no distillation form)"
_AUX_DISTILL = "the auxiliary head has no distillation form"

# subject -> [(beside, refusal)], in the order they are looked at.  `beside` is an argument of ARGUMENTS that was given, or a circumstance:
# "class_weights" (given), "label_smoothing" (!= 0), "accumulating" / "data_parallel", and "trainable ..." = that circumstance with a
# block that requires grad.  Each rule is written once, from the side of the subject that PRIORITY looks at first.
RULES = {
    "rdrop": _no_form("rdrop", "R-Drop criterion", ("teacher_logits", "distill", "focal_gamma", "crf")),
    "supcon": [("data_parallel", "supcon is refused (the supervised contrastive criterion contrasts the whole batch; a per-shard contrast "
                                 "set is a different objective - run it on one device through M2FNet.train_step)")]
    + _no_form("supcon", "supervised contrastive criterion", ("teacher_logits", "distill", "focal_gamma", "crf", "rdrop")),
    "aux": [("teacher_logits", f"aux and teacher_logits do not combine ({_AUX_DISTILL})"),
            ("distill", f"aux and distill do not combine ({_AUX_DISTILL})"),
            ("crf", "aux and crf do not combine (the CRF criterion has no auxiliary form)"),
            ("rdrop", "aux and rdrop do not combine (both write the criterion tail's fourth float)"),
            ("supcon", "aux and supcon do not combine (both join the backward at the hidden activation's gradient)"),
            ("trainable accumulating", "a trainable aux= head does not combine with gradient accumulation (its gradient would need the "
                                       "group's den); freeze it with head.params.requires_grad_(False)"),
            ("trainable data_parallel", "a trainable aux= head does not combine with DataParallelStep (its gradient would need an "
                                        "all-reduce); freeze it with head.params.requires_grad_(False)")],
    "crf": [("class_weights", "crf= does not combine with class_weights (the CRF criterion has no class-weighted form)"),
            ("teacher_logits", _CRF_DISTILL),
            ("distill", _CRF_DISTILL),
            ("focal_gamma", "crf= does not combine with focal_gamma (the CRF criterion has no focal form)"),
            ("label_smoothing", "crf= does not combine with label_smoothing != 0.0 (got {label_smoothing!r}); pass label_smoothing=0.0"),
            ("trainable accumulating", "a trainable crf= does not combine with gradient accumulation (its gradient would need the group's "
                                       "den); freeze it with crf.params.requires_grad_(False)"),
            ("trainable data_parallel", "a trainable crf= does not combine with DataParallelStep (its gradient would need an all-reduce); "
                                        "freeze it with crf.params.requires_grad_(False)")],
}

# Which subject's refusal a caller sees when several apply: the subjects are checked (value, then rules) in this order.  A Distiller
# supplies teacher_logits / distill itself and looks at the three arguments it has no form for, against "distill" alone.
PRIORITY = {"step": ("rdrop", "supcon", "aux", "crf"),
            "data_parallel": ("supcon", "rdrop", "aux", "crf"),
            "distiller": ("supcon", "aux", "rdrop")}

EVAL_TAKES = ("focal_gamma", "crf")                           # the criterion arguments of an evaluation step


def resolve(who: str, *, num_classes: int, cls_hidden: int, mask_shape, device, label_smoothing, class_weights,
            accumulating: bool = False, data_parallel: bool = False, distilling: bool = False, evaluating: bool = False,
            teacher_logits=None, distill=None, focal_gamma=None, crf=None, rdrop=None, supcon=None, aux=None,
            aux_label_smoothing: float = 0.0) -> Criterion:
    """The criterion arguments of a step of `who` -> a ``Criterion``, or the ValueError that names what is wrong - a bad value, or the
    first pair of RULES, by PRIORITY, that does not combine - before any launch or plan change.  mask_shape, device: the batch's [B, L]
    and where the step runs (teacher logits and auxiliary labels must match).  accumulating / data_parallel: gradient accumulation is
    on / the step is a ``DataParallelStep``'s.  distilling: the caller is a ``Distiller``, which refuses what has no distillation form
    before its teacher runs and leaves the rest to the student's step.  evaluating: an evaluation step (EVAL_TAKES; it writes no
    gradient, so accumulation and data parallelism are no circumstances of it: a trainable block is an input there).
    With every argument None: ``PLAIN`` itself."""
    if teacher_logits is None and distill is None and focal_gamma is None and crf is None and rdrop is None and supcon is None and aux is None:
        return PLAIN                                          # (the plain step pays seven comparisons)
    given = {"teacher_logits": teacher_logits, "distill": distill, "focal_gamma": focal_gamma, "crf": crf, "rdrop": rdrop,
             "supcon": supcon, "aux": aux}
    if evaluating:
        for name in ARGUMENTS:
            if given[name] is not None and name not in EVAL_TAKES:
                raise ValueError(f"{who}: {name} is not an argument of an evaluation step (it takes {', '.join(EVAL_TAKES)})")
    from . import aux_head, crf as crf_mod, distill as distill_mod, runtime
    if distilling:
        for subject in PRIORITY["distiller"]:
            if given[subject] is not None:
                raise ValueError(f"{who}: " + dict(RULES[subject])["distill"])
        return Criterion(gamma=None if focal_gamma is None else runtime.check_focal_gamma(focal_gamma, "focal_gamma", who))
    circumstances = (("class_weights", class_weights is not None), ("label_smoothing", label_smoothing != 0.0),
                     ("accumulating", accumulating and not evaluating), ("data_parallel", data_parallel and not evaluating))
    beside = {name for name, v in given.items() if v is not None} | {name for name, on in circumstances if on}
    checked = {}
    for subject in PRIORITY["data_parallel" if data_parallel else "step"]:
        if given[subject] is None:
            continue
        if subject == "rdrop":
            checked[subject] = block = runtime.check_rdrop_alpha(rdrop, "rdrop", who)
        elif subject == "supcon":              # (a data-parallel step refuses the argument whatever it holds: its first rule)
            checked[subject] = block = supcon if data_parallel else runtime.check_supcon_pair(supcon, "supcon", who)
        elif subject == "aux":
            checked[subject] = aux_head.check_step_args(who, aux, cls_hidden, mask_shape, aux_label_smoothing, device)
            block = checked[subject][0]
        else:
            checked[subject] = block = crf_mod.check_step_args(who, crf, num_classes)
        trainable = bool(getattr(block, "trainable", False))
        for other, refusal in RULES[subject]:
            if other in beside or (trainable and other.startswith("trainable ") and other[len("trainable "):] in beside):
                raise ValueError(f"{who}: " + refusal.format(label_smoothing=label_smoothing))
    gamma = None if focal_gamma is None else runtime.check_focal_gamma(focal_gamma, "focal_gamma", who)
    pair = None
    if teacher_logits is not None or distill is not None:
        pair = distill_mod.resolve_distill_args(teacher_logits, distill, mask_shape[0], mask_shape[1], num_classes, device, who)
    return Criterion(distill=pair, teacher_logits=teacher_logits if pair is not None else None, gamma=gamma, **checked)
