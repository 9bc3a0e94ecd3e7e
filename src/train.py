"""Drop-in for the reference's ``src/train.py``: ``main``, ``training_loop``, ``train``, ``validate`` with the same
signatures, batch-dict keys, checkpoint format ({'epoch', 'model_state_dict', 'optimizer_state_dict'}), early
stopping / best-weights protocol and per-batch metric rule.  The model, criterion and optimizer are the HIP-backed
ones (M2FNet plan, fused CE, fused Adam); with ``runtime.fused_step`` the loop body of the reference
(src/train.py:227-231) runs as one hipGraph launch + one Adam kernel."""
import math
import os
import sys
from datetime import datetime

import torch
from sklearn.utils import class_weight

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from dataset import Dataset, DeviceLoader, collate_fn  # noqa: E402
from metrics import BatchScores, move_batch  # noqa: E402
from model import M2FNet  # noqa: E402
from utils import get_config  # noqa: E402
from mer_amd import dp  # noqa: E402
from mer_amd.crf import LinearChainCRF  # noqa: E402
from mer_amd.optim import MAX_GROUPS, FusedAdam, FusedAdamW, M2FCrossEntropyLoss, M2FFocalLoss  # noqa: E402
from mer_amd.watch import ModelWatch, check_bins, check_kinds, check_log_freq  # noqa: E402

try:
    from tqdm import tqdm
except ImportError:                                    # progress bars are cosmetic
    def tqdm(it, **_):
        return it
try:
    import wandb
except ImportError:
    wandb = None

CHECKPOINT_KEYS = ("epoch", "model_state_dict", "optimizer_state_dict")
AUX_KEY = "aux_head_state_dict"                         # present only under runtime.aux_head.enabled (the AuxiliaryHead's weight and bias)
CRF_KEY = "crf_state_dict"                              # present only under solver.loss_fn: CRF (the LinearChainCRF block)
EMA_KEY = "ema_state_dict"                              # present only when runtime.ema is enabled
N_CLASSES = 7


def _runtime(cfg, key, default):
    """Value of the additive ``runtime:`` block of config.yaml (absent in the reference's file -> default)."""
    block = cfg.get("runtime", {}) if isinstance(cfg, dict) else getattr(cfg, "runtime", {})
    return block.get(key, default) if block else default


def grad_accumulation_steps(cfg, world: int = 1) -> int:
    """`runtime.grad_accumulation` = k micro-batches (consecutive DataLoader batches) per optimizer step, checked on the host before
    the GPU is touched: k > 1 needs the fused step (train_step; runtime.fused_step: True), the optimizer outside it
    (runtime.fused_optimizer: False), fp32 gradients on one rank (runtime.grad_bf16: False; several ranks ignore that key) and, with
    several ranks, the whole-step exchange (runtime.grad_overlap: False)."""
    k = _runtime(cfg, "grad_accumulation", 1)
    if isinstance(k, bool) or int(k) != k or int(k) < 1:
        raise ValueError(f"runtime.grad_accumulation must be an integer >= 1 (got {k!r})")
    k = int(k)
    if k > 1:
        if not bool(_runtime(cfg, "fused_step", True)):
            raise ValueError("runtime.grad_accumulation > 1 needs runtime.fused_step: True (the micro-batches run train_step)")
        if bool(_runtime(cfg, "fused_optimizer", False)):
            raise ValueError("runtime.grad_accumulation > 1 does not combine with runtime.fused_optimizer: True "
                             "(the optimizer steps once per group, after the last micro-batch)")
        if world == 1 and bool(_runtime(cfg, "grad_bf16", False)):
            raise ValueError("runtime.grad_accumulation > 1 does not combine with runtime.grad_bf16: True "
                             "(accumulated gradients stay fp32)")
        if world > 1 and bool(_runtime(cfg, "grad_overlap", False)):
            raise ValueError("runtime.grad_accumulation > 1 does not combine with runtime.grad_overlap: True "
                             "(the split step has no accumulate form)")
    return k


def clip_grad_norm(cfg, world: int = 1):
    """`runtime.clip_grad_norm` = null (off) or a positive number: every optimizer step clips the gradient by its global L2 norm
    (torch.nn.utils.clip_grad_norm_'s rule, on the device: FusedAdam.max_grad_norm).  Checked on the host before the GPU is touched:
    the optimizer must run outside the step (runtime.fused_optimizer: False - the in-launch optimizer updates elements before the
    norm exists) and, with several ranks, behind the whole exchange (runtime.grad_overlap: False)."""
    v = _runtime(cfg, "clip_grad_norm", None)
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not v > 0 or v != v or v == float("inf"):
        raise ValueError(f"runtime.clip_grad_norm must be null or a positive finite number (got {v!r})")
    if bool(_runtime(cfg, "fused_optimizer", False)):
        raise ValueError("runtime.clip_grad_norm does not combine with runtime.fused_optimizer: True "
                         "(the optimizer inside the step updates elements before the global norm exists)")
    if world > 1 and bool(_runtime(cfg, "grad_overlap", False)):
        raise ValueError("runtime.clip_grad_norm does not combine with runtime.grad_overlap: True "
                         "(the global norm needs every bucket's reduced gradients before the first update)")
    return float(v)


def ema_settings(cfg):
    """`runtime.ema` = {enabled, decay, warmup, evaluate}: an exponential moving average of the weights kept by the optimizer kernels
    (FusedAdam.ema_decay).  -> None when the block is absent or disabled, else (decay, warmup, evaluate); evaluate: validation, early
    stopping and test.py score the averaged weights.  Checked on the host before the GPU is touched: the optimizer must run outside
    the step (runtime.fused_optimizer: False - the in-launch optimizer has no EMA stream)."""
    block = _runtime(cfg, "ema", None)
    if block is None:
        return None
    if not hasattr(block, "keys"):
        raise ValueError(f"runtime.ema must be a mapping {{enabled, decay, warmup, evaluate}} (got {block!r})")
    unknown = sorted(set(block.keys()) - {"enabled", "decay", "warmup", "evaluate"})
    if unknown:
        raise ValueError(f"runtime.ema: unknown key(s) {unknown} (enabled, decay, warmup, evaluate)")
    flags = {}
    for k, default in (("enabled", False), ("warmup", False), ("evaluate", True)):
        flags[k] = block.get(k, default)
        if not isinstance(flags[k], bool):
            raise ValueError(f"runtime.ema.{k} must be true or false (got {flags[k]!r})")
    decay = block.get("decay", 0.999)
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= decay <= 1.0:
        raise ValueError(f"runtime.ema.decay must be a number in [0, 1] (got {decay!r})")
    if not flags["enabled"]:
        return None
    if bool(_runtime(cfg, "fused_optimizer", False)):
        raise ValueError("runtime.ema.enabled does not combine with runtime.fused_optimizer: True "
                         "(the optimizer inside the step has no EMA stream)")
    return float(decay), flags["warmup"], flags["evaluate"]


def sam_settings(cfg, world: int = 1):
    """`runtime.sam` = {enabled, rho}: sharpness-aware minimisation (FusedAdam.sam_rho; the loop calls M2FNet.sam_step).  -> None when
    the block is absent or disabled, else rho.  Checked on the host before the GPU is touched: the loop body must be the fused step
    (runtime.fused_step: True) with the optimizer outside it (runtime.fused_optimizer: False - the in-launch optimizer cannot wait for
    the second pass), one micro-batch per step (runtime.grad_accumulation: 1) and one process (data parallelism is refused)."""
    block = _runtime(cfg, "sam", None)
    if block is None:
        return None
    if not hasattr(block, "keys"):
        raise ValueError(f"runtime.sam must be a mapping {{enabled, rho}} (got {block!r})")
    unknown = sorted(set(block.keys()) - {"enabled", "rho"})
    if unknown:
        raise ValueError(f"runtime.sam: unknown key(s) {unknown} (enabled, rho)")
    enabled = block.get("enabled", False)
    if not isinstance(enabled, bool):
        raise ValueError(f"runtime.sam.enabled must be true or false (got {enabled!r})")
    rho = block.get("rho", 0.05)
    if isinstance(rho, bool) or not isinstance(rho, (int, float)) or not rho > 0 or rho != rho or rho == float("inf"):
        raise ValueError(f"runtime.sam.rho must be a positive finite number (got {rho!r})")
    if not enabled:
        return None
    if not bool(_runtime(cfg, "fused_step", True)):
        raise ValueError("runtime.sam.enabled needs runtime.fused_step: True (both passes run train_step)")
    if bool(_runtime(cfg, "fused_optimizer", False)):
        raise ValueError("runtime.sam.enabled does not combine with runtime.fused_optimizer: True "
                         "(the optimizer inside the step cannot wait for the second pass)")
    if int(_runtime(cfg, "grad_accumulation", 1) or 1) > 1:
        raise ValueError("runtime.sam.enabled does not combine with runtime.grad_accumulation > 1 in this loop "
                         "(FusedAdam's docstring has the two-sweep form)")
    if world > 1:
        raise ValueError("runtime.sam.enabled does not combine with data-parallel training (DataParallelStep refuses an optimizer "
                         "with sam_rho set); run one process")
    return float(rho)


ADVERSARIAL_DEFAULTS = {"enabled": False, "epsilon": 1.0, "steps": 2, "step_size": None, "norm": "utterance", "modalities": None,
                        "same_dropout": True}


def adversarial_settings(cfg, world: int = 1):
    """`runtime.adversarial` = {enabled, epsilon, steps, step_size, norm, modalities, same_dropout}: adversarial training on the input
    embeddings (the loop calls M2FNet.adversarial_step).  -> None when the block is absent or disabled, else the keyword arguments of
    that call.  Checked on the host before the GPU is touched: the loop body must be the fused step (runtime.fused_step: True) with the
    optimizer outside it (runtime.fused_optimizer: False), one micro-batch per step (runtime.grad_accumulation: 1 - the passes are an
    accumulation group of their own), fp32 gradients (runtime.grad_bf16: False), one process, and neither runtime.sam nor runtime.rdrop."""
    from mer_amd.runtime import ADV_NORMS
    block = _runtime(cfg, "adversarial", None)
    if block is None:
        return None
    keys = ", ".join(ADVERSARIAL_DEFAULTS)
    if not hasattr(block, "keys"):
        raise ValueError(f"runtime.adversarial must be a mapping {{{keys}}} (got {block!r})")
    unknown = sorted(set(block.keys()) - set(ADVERSARIAL_DEFAULTS))
    if unknown:
        raise ValueError(f"runtime.adversarial: unknown key(s) {unknown} ({keys})")
    v = {k: block.get(k, d) for k, d in ADVERSARIAL_DEFAULTS.items()}
    for k in ("enabled", "same_dropout"):
        if not isinstance(v[k], bool):
            raise ValueError(f"runtime.adversarial.{k} must be true or false (got {v[k]!r})")
    for k in ("epsilon", "step_size"):
        x = v[k]
        if k == "step_size" and x is None:
            continue
        if isinstance(x, bool) or not isinstance(x, (int, float)) or x != x or x == float("inf") or x < 0:
            raise ValueError(f"runtime.adversarial.{k} must be a finite number >= 0 (got {x!r})")
    if isinstance(v["steps"], bool) or not isinstance(v["steps"], int) or v["steps"] < 1:
        raise ValueError(f"runtime.adversarial.steps must be an integer >= 1 (got {v['steps']!r})")
    if not isinstance(v["norm"], str) or v["norm"] not in ADV_NORMS:
        raise ValueError(f"runtime.adversarial.norm must be one of {sorted(ADV_NORMS)} (got {v['norm']!r})")
    mods = v["modalities"]
    if mods is not None:
        if isinstance(mods, str) or not hasattr(mods, "__iter__") or not list(mods) or any(m not in ("text", "audio") for m in mods):
            raise ValueError(f"runtime.adversarial.modalities must be null or a non-empty list of text / audio (got {mods!r})")
        mods = list(mods)
    if not v["enabled"]:
        return None
    if not bool(_runtime(cfg, "fused_step", True)):
        raise ValueError("runtime.adversarial.enabled needs runtime.fused_step: True (every pass runs train_step)")
    if bool(_runtime(cfg, "fused_optimizer", False)):
        raise ValueError("runtime.adversarial.enabled does not combine with runtime.fused_optimizer: True "
                         "(the optimizer inside the step cannot wait for the later passes)")
    if int(_runtime(cfg, "grad_accumulation", 1) or 1) > 1:
        raise ValueError("runtime.adversarial.enabled does not combine with runtime.grad_accumulation > 1 "
                         "(the passes are an accumulation group of their own)")
    if bool(_runtime(cfg, "grad_bf16", False)):
        raise ValueError("runtime.adversarial.enabled does not combine with runtime.grad_bf16: True (the passes accumulate fp32 gradients)")
    if world > 1:
        raise ValueError("runtime.adversarial.enabled does not combine with data-parallel training; run one process")
    if sam_settings(cfg, world) is not None:
        raise ValueError("runtime.adversarial.enabled does not combine with runtime.sam.enabled (both re-run the batch)")
    if rdrop_settings(cfg) is not None:
        raise ValueError("runtime.adversarial.enabled does not combine with runtime.rdrop.enabled (the R-Drop step runs every dialogue twice)")
    return {"epsilon": float(v["epsilon"]), "steps": v["steps"], "step_size": None if v["step_size"] is None else float(v["step_size"]),
            "norm": v["norm"], "modalities": mods, "same_dropout": v["same_dropout"]}


def _adv_delta_norm(model, padding_mask):
    """The mean L2 norm of the final perturbation's rows over the valid utterances and the perturbed modalities of the adversarial step
    just taken: a device scalar (read where loss.item() is)."""
    valid = (~padding_mask.bool()).to(torch.float32)
    norms = [(d.norm(dim=-1) * valid).sum() / valid.sum().clamp_min(1.0) for d in model.last_perturbation().values()]
    return sum(norms) / len(norms)


DISTILL_KEYS = ("enabled", "teacher_checkpoint", "teacher_weights", "alpha", "temperature", "teacher_context", "teacher_position_bias")


def resolve_distill(cfg):
    """`runtime.distill` = {enabled, teacher_checkpoint, teacher_weights, alpha, temperature, teacher_context, teacher_position_bias}: train the model against
    the logits of a teacher with the `model:` geometry whose weights come from a checkpoint this loop wrote (mer_amd.distill) - the
    usual case is an online student (runtime.context: {past: ..., future: 0}) under an offline teacher (teacher_context both null).
    teacher_weights: model | ema picks the checkpoint's model_state_dict or the parameters of its ema_state_dict.  -> None when the block
    is absent or disabled, else a dict {checkpoint, weights, alpha, temperature, context} - plus position_bias when teacher_position_bias
    (the teacher's own distance-decay gain; absent or null = none, `position_bias_settings` has the rule) is set.  Checked on the host before the GPU is
    touched: needs runtime.fused_step: True (the criterion lives in the train step)."""
    from mer_amd.distill import check_distill
    block = _runtime(cfg, "distill", None)
    if block is None:
        return None
    if not hasattr(block, "keys"):
        raise ValueError(f"runtime.distill must be a mapping {{{', '.join(DISTILL_KEYS)}}} (got {block!r})")
    unknown = sorted(set(block.keys()) - set(DISTILL_KEYS))
    if unknown:
        raise ValueError(f"runtime.distill: unknown key(s) {unknown} ({', '.join(DISTILL_KEYS)})")
    enabled = block.get("enabled", False)
    if not isinstance(enabled, bool):
        raise ValueError(f"runtime.distill.enabled must be true or false (got {enabled!r})")
    weights = block.get("teacher_weights", "model")
    if weights not in ("model", "ema"):
        raise ValueError(f"runtime.distill.teacher_weights must be model or ema (got {weights!r})")
    try:
        alpha, temperature = check_distill((block.get("alpha", 0.5), block.get("temperature", 2.0)), "runtime.distill")
    except ValueError as e:
        raise ValueError(str(e).replace("distill alpha", "alpha").replace("distill temperature", "temperature")) from None
    ctx = block.get("teacher_context", None)
    ctx = {} if ctx is None else ctx
    if not hasattr(ctx, "keys") or set(ctx.keys()) - {"past", "future"}:
        raise ValueError(f"runtime.distill.teacher_context must be a mapping {{past, future}} (got {ctx!r})")
    band = []
    for k in ("past", "future"):
        v = ctx.get(k, None)
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 0):
            raise ValueError(f"runtime.distill.teacher_context.{k} must be null or an integer >= 0 (got {v!r})")
        band.append(v)
    bias = _position_bias_value(block.get("teacher_position_bias", None), "runtime.distill.teacher_position_bias")
    path = block.get("teacher_checkpoint", None)
    if path is not None and not isinstance(path, str):
        raise ValueError(f"runtime.distill.teacher_checkpoint must be null or a path (got {path!r})")
    if not enabled:
        return None
    if not path:
        raise ValueError("runtime.distill.enabled needs runtime.distill.teacher_checkpoint: a checkpoint written by this loop")
    if not bool(_runtime(cfg, "fused_step", True)):
        raise ValueError("runtime.distill.enabled needs runtime.fused_step: True (the distillation criterion lives in the train step)")
    out = {"checkpoint": path, "weights": weights, "alpha": alpha, "temperature": temperature, "context": (band[0], band[1])}
    if bias is not None:                                   # (only a teacher WITH a bias extends the settings: the others are what they were)
        out["position_bias"] = bias
    return out


def attach_distiller(config, model, device):
    """runtime.distill enabled: builds the teacher (the `model:` geometry, runtime.precision, the block's context band), loads its weights
    from the checkpoint and hangs a mer_amd.distill.Distiller on the model (object.__setattr__: not a sub-module - state_dict, the
    checkpoint, validate() and test.py hold and score the student only).  train() then distils in every branch.  -> the Distiller or None."""
    settings = resolve_distill(config)
    if settings is None:
        return None
    from mer_amd.distill import Distiller
    path = os.path.abspath(settings["checkpoint"])
    state = torch.load(path, map_location=device)
    if settings["weights"] == "ema":
        if EMA_KEY not in state:
            raise ValueError(f"runtime.distill.teacher_weights: ema, but {path} holds no {EMA_KEY} (it was written without runtime.ema)")
        weights = state[EMA_KEY]["parameters"]
    else:
        weights = state["model_state_dict"]
    teacher = M2FNet(config.model, precision=_runtime(config, "precision", "fp32"), context=settings["context"],
                     position_bias=settings.get("position_bias"))
    teacher.load_state_dict(weights)
    teacher = teacher.to(device)
    distiller = Distiller(model, teacher, alpha=settings["alpha"], temperature=settings["temperature"])
    object.__setattr__(model, "distiller", distiller)
    return distiller


RDROP_KEYS = ("enabled", "alpha", "warmup_steps")


def rdrop_settings(cfg):
    """`runtime.rdrop` = {enabled: False, alpha: 1.0, warmup_steps: 0}: train() runs the R-Drop criterion inside the step
    (M2FNet.train_step(rdrop=)) - every batch twice in one plan under independent dropout masks, alpha times the symmetric KL divergence
    between the two predictions added to the cross entropy of both.  -> None when the block is absent or disabled, else {alpha,
    warmup_steps}.  Checked on the host before the GPU is touched: needs runtime.fused_step: True and solver.loss_fn: CE (the criterion
    has no focal or CRF form) and no runtime.distill."""
    from mer_amd.runtime import check_rdrop_alpha
    block = _runtime(cfg, "rdrop", None)
    if block is None:
        return None
    if not hasattr(block, "keys"):
        raise ValueError(f"runtime.rdrop must be a mapping {{{', '.join(RDROP_KEYS)}}} (got {block!r})")
    unknown = sorted(set(block.keys()) - set(RDROP_KEYS))
    if unknown:
        raise ValueError(f"runtime.rdrop: unknown key(s) {unknown} ({', '.join(RDROP_KEYS)})")
    enabled = block.get("enabled", False)
    if not isinstance(enabled, bool):
        raise ValueError(f"runtime.rdrop.enabled must be true or false (got {enabled!r})")
    alpha = check_rdrop_alpha(block.get("alpha", 1.0), "alpha", "runtime.rdrop")
    warm = block.get("warmup_steps", 0)
    if isinstance(warm, bool) or not isinstance(warm, int) or warm < 0:
        raise ValueError(f"runtime.rdrop.warmup_steps must be an integer >= 0 (got {warm!r})")
    if not enabled:
        return None
    if not bool(_runtime(cfg, "fused_step", True)):
        raise ValueError("runtime.rdrop.enabled needs runtime.fused_step: True (the R-Drop criterion lives in the train step)")
    solver = cfg.get("solver", None) if isinstance(cfg, dict) else getattr(cfg, "solver", None)
    loss_fn = None if solver is None else (solver.get("loss_fn", "CE") if hasattr(solver, "get") else getattr(solver, "loss_fn", "CE"))
    if loss_fn not in (None, "CE"):
        raise ValueError(f"runtime.rdrop.enabled needs solver.loss_fn: CE (got {loss_fn!r}: the R-Drop criterion has no focal or CRF form)")
    if resolve_distill(cfg) is not None:
        raise ValueError("runtime.rdrop.enabled does not combine with runtime.distill.enabled (the R-Drop criterion has no distillation form)")
    return {"alpha": alpha, "warmup_steps": warm}


def _warmed(value: float, warmup_steps: int, global_step: int) -> float:
    """A criterion weight at optimizer step `global_step` under a linear warm-up: value * (step + 1) / warmup_steps until warmup_steps
    (0: the value from the first step)."""
    return value * min(1.0, (global_step + 1) / warmup_steps) if warmup_steps > 0 else value


def _rdrop_kw(model, global_step: int):
    """{rdrop: alpha} of optimizer step `global_step` for train_step / DataParallelStep when main() hung the runtime.rdrop settings on the
    model (`model.rdrop`), else nothing - the calls of a run without it are today's.  alpha is `_warmed`."""
    r = getattr(model, "rdrop", None)
    return {} if r is None else {"rdrop": _warmed(r["alpha"], r["warmup_steps"], global_step)}


class _SharesLog:
    """Running means of the two shares of the loss for wandb, for whichever weighted term main() hung on the model: {"Train/CE"} and
    {"Train/RDrop_KL"} (`model.rdrop`), {"Train/SupCon"} (`model.supcon`) or {"Train/Aux"} (`model.aux_head`), beside Train/Running_loss
    (CE + weight * share at a constant weight).  Reads `model.*_terms()` only when something is logged: two more scalars on a path that
    has just waited for loss.item()."""
    TERMS = (("rdrop", "rdrop_terms", "Train/RDrop_KL"), ("supcon", "supcon_terms", "Train/SupCon"), ("aux_head", "aux_terms", "Train/Aux"))

    def __init__(self, model, on: bool):
        self.model = model
        self.terms = [(fn, key, [0.0, 0.0]) for attr, fn, key in self.TERMS if on and getattr(model, attr, None) is not None]

    def __call__(self, step: int):
        out = {}
        for fn, key, sums in self.terms:
            for i, share in enumerate(getattr(self.model, fn)()):
                sums[i] += share.item()
            out.update({"Train/CE": sums[0] / (step + 1), key: sums[1] / (step + 1)})
        return out


SUPCON_KEYS = ("enabled", "weight", "temperature", "warmup_steps")


def supcon_settings(cfg):
    """`runtime.supcon` = {enabled: False, weight: 0.1, temperature: 0.1, warmup_steps: 0}: train() adds the supervised contrastive term
    on the classifier's hidden features inside the step (M2FNet.train_step(supcon=)).  -> None when the block is absent or disabled,
    else {weight, temperature, warmup_steps}.  Checked on the host before the GPU is touched: needs runtime.fused_step: True and
    solver.loss_fn: CE (the term rides on the plain cross entropy), no runtime.distill, no runtime.rdrop and one process (a shard's
    contrast set is a different objective)."""
    from mer_amd.runtime import check_supcon_pair
    block = _runtime(cfg, "supcon", None)
    if block is None:
        return None
    if not hasattr(block, "keys"):
        raise ValueError(f"runtime.supcon must be a mapping {{{', '.join(SUPCON_KEYS)}}} (got {block!r})")
    unknown = sorted(set(block.keys()) - set(SUPCON_KEYS))
    if unknown:
        raise ValueError(f"runtime.supcon: unknown key(s) {unknown} ({', '.join(SUPCON_KEYS)})")
    enabled = block.get("enabled", False)
    if not isinstance(enabled, bool):
        raise ValueError(f"runtime.supcon.enabled must be true or false (got {enabled!r})")
    weight, temperature = check_supcon_pair((block.get("weight", 0.1), block.get("temperature", 0.1)), "(weight, temperature)", "runtime.supcon")
    warm = block.get("warmup_steps", 0)
    if isinstance(warm, bool) or not isinstance(warm, int) or warm < 0:
        raise ValueError(f"runtime.supcon.warmup_steps must be an integer >= 0 (got {warm!r})")
    if not enabled:
        return None
    if not bool(_runtime(cfg, "fused_step", True)):
        raise ValueError("runtime.supcon.enabled needs runtime.fused_step: True (the supervised contrastive criterion lives in the train step)")
    solver = cfg.get("solver", None) if isinstance(cfg, dict) else getattr(cfg, "solver", None)
    loss_fn = None if solver is None else (solver.get("loss_fn", "CE") if hasattr(solver, "get") else getattr(solver, "loss_fn", "CE"))
    if loss_fn not in (None, "CE"):
        raise ValueError(f"runtime.supcon.enabled needs solver.loss_fn: CE (got {loss_fn!r}: the supervised contrastive criterion has no focal or CRF form)")
    if resolve_distill(cfg) is not None:
        raise ValueError("runtime.supcon.enabled does not combine with runtime.distill.enabled (the supervised contrastive criterion has no distillation form)")
    if rdrop_settings(cfg) is not None:
        raise ValueError("runtime.supcon.enabled does not combine with runtime.rdrop.enabled (the supervised contrastive criterion has no R-Drop form)")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("runtime.supcon.enabled runs in one process (the data-parallel step refuses supcon: a shard's contrast set is a different objective)")
    return {"weight": weight, "temperature": temperature, "warmup_steps": warm}


def _supcon_kw(model, global_step: int):
    """{supcon: (weight, temperature)} of optimizer step `global_step` for train_step when main() hung the runtime.supcon settings on
    the model (`model.supcon`), else nothing - the calls of a run without it are today's.  The weight is `_warmed`."""
    r = getattr(model, "supcon", None)
    return {} if r is None else {"supcon": (_warmed(r["weight"], r["warmup_steps"], global_step), r["temperature"])}


AUX_KEYS = ("enabled", "labels", "weight", "label_smoothing", "lr", "warmup_steps")
AUX_LABEL_COLUMNS = {"sentiment": 3}                    # batch key -> classes (dataset.SENTIMENTS)


def aux_head_settings(cfg):
    """`runtime.aux_head` = {enabled: False, labels: sentiment, weight: 0.5, label_smoothing: 0.0, lr: 1.0e-3, warmup_steps: 0}: train()
    trains a second linear head over the classifier's hidden features against the table's second label inside the step
    (M2FNet.train_step(aux=)).  -> None when the block is absent or disabled, else {labels, weight, label_smoothing, lr, warmup_steps}.
    Checked on the host before the GPU is touched: needs runtime.device_batcher: False (the DataLoader path carries the second label),
    runtime.fused_step: True, solver.loss_fn: CE or Focal, no runtime.distill / rdrop / supcon, runtime.grad_accumulation 1 and one
    process (the head trains: its gradient is normalised by one batch's den and is not all-reduced)."""
    from mer_amd.aux_head import check_pair
    block = _runtime(cfg, "aux_head", None)
    if block is None:
        return None
    if not hasattr(block, "keys"):
        raise ValueError(f"runtime.aux_head must be a mapping {{{', '.join(AUX_KEYS)}}} (got {block!r})")
    unknown = sorted(set(block.keys()) - set(AUX_KEYS))
    if unknown:
        raise ValueError(f"runtime.aux_head: unknown key(s) {unknown} ({', '.join(AUX_KEYS)})")
    enabled = block.get("enabled", False)
    if not isinstance(enabled, bool):
        raise ValueError(f"runtime.aux_head.enabled must be true or false (got {enabled!r})")
    labels = block.get("labels", "sentiment")
    if labels not in AUX_LABEL_COLUMNS:
        raise ValueError(f"runtime.aux_head.labels must be one of {sorted(AUX_LABEL_COLUMNS)} (got {labels!r})")
    weight, smoothing = check_pair(block.get("weight", 0.5), block.get("label_smoothing", 0.0), "runtime.aux_head")
    lr = block.get("lr", 1.0e-3)
    if isinstance(lr, bool) or not isinstance(lr, (int, float)) or not (math.isfinite(lr) and lr > 0.0):
        raise ValueError(f"runtime.aux_head.lr must be a finite number > 0 (got {lr!r})")
    warm = block.get("warmup_steps", 0)
    if isinstance(warm, bool) or not isinstance(warm, int) or warm < 0:
        raise ValueError(f"runtime.aux_head.warmup_steps must be an integer >= 0 (got {warm!r})")
    if not enabled:
        return None
    if bool(_runtime(cfg, "device_batcher", False)):
        raise ValueError("runtime.aux_head.enabled needs runtime.device_batcher: False (the device batcher gathers the emotion label only; "
                         "the DataLoader path carries the second label)")
    if not bool(_runtime(cfg, "fused_step", True)):
        raise ValueError("runtime.aux_head.enabled needs runtime.fused_step: True (the auxiliary head lives in the train step)")
    solver = cfg.get("solver", None) if isinstance(cfg, dict) else getattr(cfg, "solver", None)
    loss_fn = None if solver is None else (solver.get("loss_fn", "CE") if hasattr(solver, "get") else getattr(solver, "loss_fn", "CE"))
    if loss_fn not in (None, "CE", "Focal"):
        raise ValueError(f"runtime.aux_head.enabled needs solver.loss_fn: CE or Focal (got {loss_fn!r}: the CRF criterion has no auxiliary form)")
    if resolve_distill(cfg) is not None:
        raise ValueError("runtime.aux_head.enabled does not combine with runtime.distill.enabled (the auxiliary head has no distillation form)")
    if rdrop_settings(cfg) is not None:
        raise ValueError("runtime.aux_head.enabled does not combine with runtime.rdrop.enabled (both write the criterion tail's fourth float)")
    if supcon_settings(cfg) is not None:
        raise ValueError("runtime.aux_head.enabled does not combine with runtime.supcon.enabled (both join the backward at the hidden activation's gradient)")
    if int(_runtime(cfg, "grad_accumulation", 1) or 1) > 1:
        raise ValueError("runtime.aux_head.enabled does not combine with runtime.grad_accumulation > 1 (the head trains: its gradient would need the group's den)")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("runtime.aux_head.enabled runs in one process (the head trains: the data-parallel step does not all-reduce its gradient)")
    return {"labels": labels, "weight": weight, "label_smoothing": smoothing, "lr": float(lr), "warmup_steps": warm}


def attach_aux_head(model, settings, hidden_size: int, device, with_optimizer: bool = True) -> None:
    """Under runtime.aux_head the head travels on the model as `model.aux_head` (object.__setattr__: not a sub-module - its block is neither
    in M2FNet's state_dict nor in the model's optimizer), with its settings and the torch Adam that steps its block behind the model's
    optimizer, as the CRF's (with_optimizer False - test.py: `head.optimizer` is None); checkpoints then carry it as
    'aux_head_state_dict'.  settings None: `model.aux_head` is None."""
    head = None
    if settings is not None:
        from mer_amd.aux_head import AuxiliaryHead
        head = AuxiliaryHead(int(hidden_size), AUX_LABEL_COLUMNS[settings["labels"]]).to(device)
        head.settings = dict(settings)
        head.optimizer = torch.optim.Adam(head.parameters(), lr=settings["lr"]) if with_optimizer else None
    object.__setattr__(model, "aux_head", head)


def _aux_zero_grad(aux) -> None:
    """`aux`: what `_aux_kw` returned.  The head's own optimizer, in front of the step (nothing without a head)."""
    if aux and getattr(aux["aux"][0], "optimizer", None) is not None:
        aux["aux"][0].optimizer.zero_grad()


def _aux_step(aux) -> None:
    """The head's own optimizer, behind the model's (its gradient is the step's own buffer); nothing without a head."""
    if aux and getattr(aux["aux"][0], "optimizer", None) is not None:
        aux["aux"][0].optimizer.step()


def _aux_kw(model, batch, device, global_step: int):
    """{aux: (head, labels, weight), aux_label_smoothing} of optimizer step `global_step` for train_step when main() hung an auxiliary
    head on the model (`model.aux_head`), else nothing - the calls of a run without it are today's.  The weight is `_warmed`."""
    head = getattr(model, "aux_head", None)
    if head is None:
        return {}
    r = head.settings
    if r["labels"] not in batch:
        raise ValueError(f"runtime.aux_head: the batch carries no {r['labels']!r} (Dataset({r['labels']}=True) and runtime.device_batcher: False are needed)")
    weight = _warmed(r["weight"], r["warmup_steps"], global_step)
    return {"aux": (head, batch[r["labels"]].to(device, non_blocking=True), weight), "aux_label_smoothing": r["label_smoothing"]}


class AuxAccuracy:
    """The auxiliary head's accuracy over an evaluation pass, on the host: `update(model, batch, device)` behind a batch's forward counts
    `head(model.last_features()).argmax` against the batch's second label over the utterances that carry one.  Off (every call a
    no-op, `result()` None) when the model has no head or the batches no such label."""

    def __init__(self, model):
        self.head = getattr(model, "aux_head", None)
        self.hits = self.count = 0

    def update(self, model, batch, device) -> None:
        if self.head is None or self.head.settings["labels"] not in batch:
            return
        labels = batch[self.head.settings["labels"]].to(device)
        with torch.no_grad():
            pred = self.head(model.last_features()).argmax(-1)
        ok = labels >= 0
        self.hits += int(((pred == labels) & ok).sum())
        self.count += int(ok.sum())

    def result(self):
        return self.hits / self.count if self.count else None


def _distill_kw(model, text, audio, padding_mask):
    """{teacher_logits, distill} of this batch for train_step / DataParallelStep when the model carries a Distiller, else nothing."""
    d = getattr(model, "distiller", None)
    if d is None:
        return {}
    return {"teacher_logits": d.teacher_logits(text, audio, padding_mask), "distill": (d.alpha, d.temperature)}


def context_settings(cfg):
    """`runtime.context` = {past, future}: the context band of every attention site of the model (M2FNet(context=...)) - utterance i
    attends to utterances i - past .. i + future of its dialogue; null = unlimited on that side.  {past: null, future: 0} is the online
    setting (an utterance is labelled from the past only), {past: k, future: 0} its bounded form.  -> None when the block is absent,
    null or unlimited on both sides (the reference's offline attention), else (past, future).  Checked on the host before the GPU is
    touched."""
    block = _runtime(cfg, "context", None)
    if block is None:
        return None
    if not hasattr(block, "keys"):
        raise ValueError(f"runtime.context must be a mapping {{past, future}} (got {block!r})")
    unknown = sorted(set(block.keys()) - {"past", "future"})
    if unknown:
        raise ValueError(f"runtime.context: unknown key(s) {unknown} (past, future)")
    band = []
    for k in ("past", "future"):
        v = block.get(k, None)
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 0):
            raise ValueError(f"runtime.context.{k} must be null or an integer >= 0 (got {v!r})")
        band.append(v)
    return None if band == [None, None] else (band[0], band[1])


def _position_bias_value(v, where):
    """null -> None; a finite number >= 0 -> itself (0 -> None: off); anything else: ValueError naming `where`."""
    from mer_amd.runtime import position_bias
    try:
        return position_bias(v) and float(v) or None
    except ValueError:
        raise ValueError(f"{where} must be null or a finite number >= 0: the gain of the distance-decay attention bias, 1.0 is ALiBi "
                         f"(got {v!r})") from None


def position_bias_settings(cfg):
    """`runtime.position_bias`: null (default) or a finite number >= 0 - the gain of the distance-decay attention bias of every attention
    site of the model (M2FNet(position_bias=...): score(i, j) -= slope_h * gain * |i - j|; 1.0 is ALiBi, applied as rounded to bf16).
    -> None when absent, null or 0, else the number.  Checked on the host before the GPU is touched."""
    return _position_bias_value(_runtime(cfg, "position_bias", None), "runtime.position_bias")


def speaker_heads_settings(cfg, world: int = 1):
    """`runtime.speaker_heads` = {same, other}: speaker-aware heads of every attention site of the model (M2FNet(speaker_heads=(same,
    other)): the first `same` heads of a site see the utterances of the query's own speaker only, the next `other` heads those of the
    other speakers only).  -> None when the key is absent or null (the loop then behaves as it does without it), else (same, other).
    Checked on the host before the GPU is touched: integers >= 0, at least one positive (whether they fit the heads is the model's
    check); needs runtime.device_batcher: False (the device batcher gathers no speaker ids) and a single rank (the data-parallel
    step refuses a model with speaker heads)."""
    from mer_amd.runtime import speaker_heads
    block = _runtime(cfg, "speaker_heads", None)
    if block is None:
        return None
    if not hasattr(block, "keys"):
        raise ValueError(f"runtime.speaker_heads must be a mapping {{same, other}} (got {block!r})")
    unknown = sorted(set(block.keys()) - {"same", "other"})
    if unknown:
        raise ValueError(f"runtime.speaker_heads: unknown key(s) {unknown} (same, other)")
    try:
        heads = speaker_heads((block.get("same", 0), block.get("other", 0)))
    except ValueError as e:
        raise ValueError(f"runtime.speaker_heads: {e}") from None
    if _runtime(cfg, "device_batcher", False):
        raise ValueError("runtime.speaker_heads needs runtime.device_batcher: False (the device batcher gathers no speaker ids)")
    if world > 1:
        raise ValueError("runtime.speaker_heads does not combine with data-parallel training (DataParallelStep refuses a model with "
                         "speaker heads): launch a single process")
    return heads


def _speaker_kw(model, batch, device):
    """{speakers} of this batch when the model has speaker heads (runtime.speaker_heads), else nothing - the loop as it was."""
    if getattr(model, "speaker_heads", None) is None:
        return {}
    if "speaker" not in batch:
        raise ValueError("the model has speaker heads but the batch carries no \"speaker\" ids (Dataset(speakers=True))")
    from mer_amd.runtime import speaker_ids
    # range-checked and narrowed to one byte on the HOST, where the collated ids are: nothing waits for the device in front of the step
    return {"speakers": speaker_ids(batch["speaker"], "batch[\"speaker\"]").to(device, non_blocking=True)}


def build_model(config, device):
    """The M2FNet of `config` on `device` as train.py and test.py both build it: runtime.precision, runtime.context,
    runtime.position_bias and runtime.speaker_heads - so a model trained under a context band, a position bias or speaker heads is
    validated and tested, streamed or not, under the same."""
    return M2FNet(config.model, precision=_runtime(config, "precision", "fp32"), context=context_settings(config),
                  position_bias=position_bias_settings(config), speaker_heads=speaker_heads_settings(config)).to(device)


def watch_settings(cfg, world: int = 1):
    """`runtime.watch` = {enabled, log, log_freq, bins, file}: per-tensor statistics and histograms of the buffers the optimizer step
    uses, every log_freq optimizer steps (mer_amd.watch.ModelWatch) - what `wandb.watch_model` asks of wandb's hooks, which cannot see
    those buffers.  -> None when the block is absent or disabled, else {"log": kinds, "log_freq", "bins", "file"}.  Checked on the host
    before the GPU is touched: the optimizer must run outside the step (runtime.fused_optimizer: False) and, with several ranks and
    gradients or updates watched, behind the whole exchange (runtime.grad_overlap: False; one rank ignores that key)."""
    block = _runtime(cfg, "watch", None)
    if block is None:
        return None
    if not hasattr(block, "keys"):
        raise ValueError(f"runtime.watch must be a mapping {{enabled, log, log_freq, bins, file}} (got {block!r})")
    unknown = sorted(set(block.keys()) - {"enabled", "log", "log_freq", "bins", "file"})
    if unknown:
        raise ValueError(f"runtime.watch: unknown key(s) {unknown} (enabled, log, log_freq, bins, file)")
    enabled = block.get("enabled", False)
    if not isinstance(enabled, bool):
        raise ValueError(f"runtime.watch.enabled must be true or false (got {enabled!r})")
    try:
        kinds = check_kinds(block.get("log", "all"))
        log_freq = check_log_freq(block.get("log_freq", 100))
        bins = check_bins(block.get("bins", 64))
    except ValueError as e:
        raise ValueError(str(e).replace("ModelWatch: ", "runtime.watch.")) from None
    file = block.get("file", None)
    if file is not None and (not isinstance(file, str) or not file):
        raise ValueError(f"runtime.watch.file must be null or a path (got {file!r})")
    if not enabled:
        return None
    if bool(_runtime(cfg, "fused_optimizer", False)):
        raise ValueError("runtime.watch.enabled does not combine with runtime.fused_optimizer: True "
                         "(the optimizer inside the step never stores the matrices' gradients)")
    if world > 1 and bool(_runtime(cfg, "grad_overlap", False)) and ("gradients" in kinds or "updates" in kinds):
        raise ValueError("runtime.watch with gradients or updates does not combine with runtime.grad_overlap: True "
                         "(the collection needs every bucket's reduced gradients before the first update)")
    return {"log": kinds, "log_freq": log_freq, "bins": bins, "file": file}


def attach_watch(cfg, model, optimizer, rank: int = 0, world: int = 1):
    """Builds the ModelWatch `runtime.watch` asks for and attaches it to the optimizer - on rank 0 only: the replicas' reduced gradients
    are identical, and what a due step adds waits on collectives that are already issued, so no rank blocks another.  -> the watch, or
    None (block off, or another rank).  An optimizer that is not a FusedAdam is refused: only it knows the buffers a step reads."""
    settings = watch_settings(cfg, world)
    if settings is None:
        return None
    if not isinstance(optimizer, FusedAdam):
        raise ValueError(f"runtime.watch.enabled needs the FusedAdam / FusedAdamW optimizer (got {type(optimizer).__name__}): "
                         "it hands the watch the buffers each step reads")
    if rank != 0:
        return None
    w = ModelWatch(model, log=settings["log"], log_freq=settings["log_freq"], bins=settings["bins"])
    w.file = None if settings["file"] is None else os.path.abspath(settings["file"])
    if w.file is not None:
        os.makedirs(os.path.dirname(w.file), exist_ok=True)
    optimizer.watch = w
    return w


def _under(name: str, prefix: str) -> bool:
    return name == prefix or name.startswith(prefix + ".")


def optimizer_groups(cfg, named_shapes):
    """`runtime.optimizer` = {name: adam | adamw, no_decay_1d: bool, lr_scale: {state_dict prefix: multiplier of solver.lr},
    frozen: [state_dict prefixes]} cut into parameter groups, on the host, from the model's (name, shape) list - checked before the
    GPU is touched.  -> None when the block is absent or holds its defaults (the single coupled group of the reference, src/train.py:56),
    else (name, groups, frozen names): groups = [{"names", "lr", "weight_decay"}] in order of first appearance, one per
    (lr multiplier, decays or not) that occurs.  adamw = decoupled weight decay (torch.optim.AdamW); no_decay_1d: weight_decay 0 for every
    1-D parameter (biases, LayerNorm); frozen parameters are handed to no group (their gradients are still computed)."""
    block = _runtime(cfg, "optimizer", None)
    if not block:
        return None
    unknown = sorted(set(block) - {"name", "no_decay_1d", "lr_scale", "frozen"})
    if unknown:
        raise ValueError(f"runtime.optimizer: unknown key(s) {unknown} (name, no_decay_1d, lr_scale, frozen)")
    name = block.get("name", "adam")
    if name not in ("adam", "adamw"):
        raise ValueError(f"runtime.optimizer.name must be adam or adamw (got {name!r})")
    no_decay_1d = block.get("no_decay_1d", False)
    if not isinstance(no_decay_1d, bool):
        raise ValueError(f"runtime.optimizer.no_decay_1d must be true or false (got {no_decay_1d!r})")
    lr_scale = dict(block.get("lr_scale", None) or {})
    frozen = list(block.get("frozen", None) or [])
    for k, v in lr_scale.items():
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not v > 0 or v == float("inf"):
            raise ValueError(f"runtime.optimizer.lr_scale[{k!r}] must be a positive finite number (got {v!r})")
    if name == "adam" and not no_decay_1d and not lr_scale and not frozen:
        return None
    names = [n for n, _ in named_shapes]
    prefixes = [str(k) for k in lr_scale] + [str(k) for k in frozen]
    for pre in prefixes:
        if not any(_under(n, pre) for n in names):
            raise ValueError(f"runtime.optimizer: prefix {pre!r} matches no parameter of the model")
    for n in names:
        hit = [pre for pre in prefixes if _under(n, pre)]
        if len(hit) > 1:
            raise ValueError(f"runtime.optimizer: prefixes {hit} overlap (both match {n!r})")
    solver = cfg["solver"] if isinstance(cfg, dict) else cfg.solver
    lr0 = float(solver["lr"] if isinstance(solver, dict) else solver.lr)
    wd0 = float(solver["weight_decay"] if isinstance(solver, dict) else solver.weight_decay)
    groups, at, frozen_names = [], {}, []
    for n, shape in named_shapes:
        if any(_under(n, pre) for pre in frozen):
            frozen_names.append(n)
            continue
        scale = next((float(v) for k, v in lr_scale.items() if _under(n, str(k))), 1.0)
        decays = not (no_decay_1d and len(shape) == 1)
        if (scale, decays) not in at:
            at[(scale, decays)] = len(groups)
            groups.append({"names": [], "lr": lr0 * scale, "weight_decay": wd0 if decays else 0.0})
        groups[at[(scale, decays)]]["names"].append(n)
    if not groups:
        raise ValueError("runtime.optimizer.frozen leaves no parameter to train")
    if len(groups) > MAX_GROUPS:
        raise ValueError(f"runtime.optimizer cuts {len(groups)} parameter groups; the optimizer takes at most {MAX_GROUPS}")
    return name, groups, frozen_names


def model_named_shapes(model_cfg):
    """(state_dict name, shape) of every parameter of M2FNet(model_cfg), without building it."""
    from mer_amd.layout import M2FConfig, param_specs
    return [(sp.name, sp.shape) for sp in param_specs(M2FConfig.from_model_config(model_cfg))[0]]


def build_optimizer(config, model):
    """torch.optim.Adam(model.parameters(), lr, weight_decay) of the reference (src/train.py:56), or what `runtime.optimizer` asks for."""
    cut = optimizer_groups(config, [(n, tuple(p.shape)) for n, p in model.named_parameters(remove_duplicate=False)])
    ema = ema_settings(config)
    ema_kw = {} if ema is None else {"ema_decay": ema[0], "ema_warmup": ema[1]}
    rho = sam_settings(config)
    if rho is not None:
        ema_kw["sam_rho"] = rho
    if cut is None:
        return FusedAdam(model, lr=config.solver.lr, weight_decay=config.solver.weight_decay, **ema_kw)
    name, groups, _ = cut
    named = dict(model.named_parameters(remove_duplicate=False))
    params, seen = [], {}
    for gi, g in enumerate(groups):
        ps = []
        for n in g["names"]:
            p = named[n]
            if seen.setdefault(id(p), gi) != gi:          # (the final LayerNorm the encoders of a modality share has several names)
                raise ValueError(f"runtime.optimizer: {n!r} shares its tensor with a parameter of another group")
            if not any(p is q for q in ps):
                ps.append(p)
        params.append({"params": ps, "lr": g["lr"], "weight_decay": g["weight_decay"]})
    cls = FusedAdamW if name == "adamw" else FusedAdam
    return cls(model, lr=config.solver.lr, weight_decay=config.solver.weight_decay, params=params, **ema_kw)


def group_batches(batches, k: int):
    """k consecutive batches per group; the last group of an epoch may be shorter."""
    group = []
    for b in batches:
        group.append(b)
        if len(group) == k:
            yield group
            group = []
    if group:
        yield group


# ---- construction of the solver pieces from config.solver -----------------------------------------------------------
def focal_gamma_setting(cfg) -> float:
    """`runtime.focal_gamma`: gamma of the focal criterion `solver.loss_fn: Focal` builds (mer_amd.optim.M2FFocalLoss) - a finite number
    in [0, 8], default 2.0; checked on the host before the GPU is touched, ignored under `loss_fn: CE`."""
    from mer_amd.runtime import check_focal_gamma
    return check_focal_gamma(_runtime(cfg, "focal_gamma", 2.0), "focal_gamma", "runtime")


def crf_settings(cfg) -> dict:
    """`runtime.crf` = {init: zeros | bigram, smoothing: 1.0, trainable: True, lr: 1.0e-2}: the block `solver.loss_fn: CRF` builds
    (mer_amd.crf.LinearChainCRF).  init: bigram fills it with the log bigram, start and end frequencies of the training labels
    (`from_label_counts`, with `smoothing`); trainable: a second torch.optim.Adam with `lr` steps it beside the model's optimizer.
    Checked on the host before the GPU is touched; ignored under other criteria."""
    block = dict(_runtime(cfg, "crf", None) or {})
    unknown = sorted(set(block) - {"init", "smoothing", "trainable", "lr"})
    if unknown:
        raise ValueError(f"runtime.crf: unknown key(s) {unknown}; it takes init, smoothing, trainable, lr")
    out = {"init": block.get("init", "zeros"), "smoothing": block.get("smoothing", 1.0), "trainable": block.get("trainable", True),
           "lr": block.get("lr", 1.0e-2)}
    if out["init"] not in ("zeros", "bigram"):
        raise ValueError(f"runtime.crf.init must be zeros or bigram, got {out['init']!r}")
    if not isinstance(out["trainable"], bool):
        raise ValueError(f"runtime.crf.trainable must be true or false, got {out['trainable']!r}")
    for key, low_ok in (("smoothing", lambda v: v >= 0.0), ("lr", lambda v: v > 0.0)):
        v = out[key]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not low_ok(v):
            raise ValueError(f"runtime.crf.{key} must be a finite number " + (">= 0" if key == "smoothing" else "> 0") + f", got {v!r}")
        out[key] = float(v)
    return out


def build_crf(settings: dict, train_set, device):
    """The criterion of `solver.loss_fn: CRF`: a LinearChainCRF of N_CLASSES classes on `device`; `crf.optimizer` is the torch Adam that
    steps it when it is trainable (None: frozen - a pure input of the step)."""
    if settings["init"] == "bigram":
        labels, lengths = train_set.get_dialogue_labels()
        crf = LinearChainCRF.from_label_counts(labels, lengths, smoothing=settings["smoothing"], num_classes=N_CLASSES)
    else:
        crf = LinearChainCRF(N_CLASSES)
    crf = crf.to(device)
    crf.params.requires_grad_(settings["trainable"])
    crf.optimizer = torch.optim.Adam(crf.parameters(), lr=settings["lr"]) if settings["trainable"] else None
    return crf


def _crit_kw(criterion, data_parallel: bool = False):
    """The criterion's arguments of train_step / eval_step / DataParallelStep: label smoothing, class weights and gamma of the cross
    entropies; under the CRF criterion no smoothing, no weights and (the data-parallel step holds it itself) `crf=`."""
    if isinstance(criterion, LinearChainCRF):
        return {"label_smoothing": 0.0, "class_weights": None, **({} if data_parallel else {"crf": criterion})}
    return {"label_smoothing": criterion.label_smoothing, "class_weights": criterion.weight, **_focal_kw(criterion)}


def _crf_zero_grad(criterion) -> None:
    if getattr(criterion, "optimizer", None) is not None:
        criterion.optimizer.zero_grad()


def _crf_step(criterion) -> None:
    """The second optimizer of a trainable CRF criterion, behind the model's (its gradient is the step's own buffer, or autograd's)."""
    if getattr(criterion, "optimizer", None) is not None:
        criterion.optimizer.step()


def _focal_kw(criterion):
    """{focal_gamma} for train_step / DataParallelStep / eval_step when the criterion is the focal one (its gamma as it stands: a schedule
    may have changed it), else nothing - the calls of a CE run are today's."""
    return {"focal_gamma": criterion.gamma} if isinstance(criterion, M2FFocalLoss) else {}


def build_criterion(solver, train_set, device, focal_gamma: float = 2.0, crf: dict = None):
    """CE(ignore_index=-1, label_smoothing=0.1), optionally with sklearn's balanced class weights of the train labels; `loss_fn: Focal`:
    the same with every utterance's term scaled by (1 - p_y)^focal_gamma (M2FFocalLoss, an M2FCrossEntropyLoss: the fused step, the
    device metrics and every training mode take it)."""
    if solver.loss_fn == "CRF":
        if solver.balance_classes:
            raise ValueError("solver.loss_fn: CRF does not combine with solver.balance_classes (the CRF criterion has no class-weighted form)")
        return build_crf(crf if crf is not None else crf_settings({}), train_set, device)
    if solver.loss_fn not in ("CE", "Focal"):
        raise ValueError("Criterion not supported")
    class_weights = None
    if solver.balance_classes:
        import numpy as np                                 # (current sklearn takes `classes` as an ndarray only)
        balanced = class_weight.compute_class_weight(class_weight="balanced", classes=np.arange(N_CLASSES),
                                                     y=np.asarray(train_set.get_labels()))
        class_weights = torch.as_tensor(balanced, dtype=torch.float, device=device)
    if solver.loss_fn == "Focal":
        return M2FFocalLoss(weight=class_weights, ignore_index=-1, label_smoothing=0.1, gamma=focal_gamma)
    return M2FCrossEntropyLoss(weight=class_weights, ignore_index=-1, label_smoothing=0.1)


def build_scheduler(solver, optimizer):
    if not solver.scheduler.enabled:
        return None
    if solver.scheduler.scheduler_fn != "ExponentialLR":
        raise ValueError("Scheduler not supported")
    return torch.optim.lr_scheduler.ExponentialLR(optimizer=optimizer, gamma=solver.scheduler.gamma)


TEXT_ENCODER_GEOMETRY = {"base": dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072),
                         "large": dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096)}


def build_text_encoder(te_cfg, d_text, device):
    """`runtime.text_encoder`: {enabled, precision: fp32 | bf16 | fp8, geometry: base | large | a dict of RobertaConfig fields,
    checkpoint: path of a state_dict in transformers.RobertaModel(add_pooling_layer=False) key layout (the encoder of the reference's
    TextERC, src/feature_extractors/text/model.py:16) or null = random weights}."""
    from mer_amd.roberta import RobertaEncoder
    geo = te_cfg.get("geometry", "base")
    cfg = dict(TEXT_ENCODER_GEOMETRY[geo]) if isinstance(geo, str) else dict(geo)
    for k, v in dict(vocab_size=50265, max_position_embeddings=514, type_vocab_size=1, pad_token_id=1, layer_norm_eps=1e-5, hidden_act="gelu").items():
        cfg.setdefault(k, v)
    if cfg["hidden_size"] != d_text:
        raise ValueError(f"runtime.text_encoder produces {cfg['hidden_size']}-wide rows but model.TEXT.embedding_size is {d_text}")
    enc = RobertaEncoder(cfg, precision=te_cfg.get("precision", "bf16"))
    ck = te_cfg.get("checkpoint", None)
    if ck:
        enc.load_state_dict(torch.load(os.path.abspath(ck), map_location="cpu"))
    return enc.to(device).eval()


def build_audio_encoder(ae_cfg, d_audio, device, n_head=None):
    """`runtime.audio_encoder`: {enabled, model: wav2vec2 (default) | mel_resnet18, precision: fp32 | bf16, wav_dir, checkpoint}.
    wav2vec2: geometry: base | a dict of Wav2Vec2Config fields; checkpoint: path of a state_dict in transformers.Wav2Vec2Model or
    torchaudio wav2vec2 key layout (the encoder of the reference's AudioERC) or null = random weights.
    mel_resnet18: the reference's audio_mel extractor (300-wide rows, so model.AUDIO.embedding_size must be 300 and n_head must
    divide it); checkpoint: the reference's checkpoints/audio_mel/checkpoint.pth or a bare state_dict in its key layout; png_levels:
    True (default: the 8-bit levels of the reference's spectrogram cache) | False."""
    kind = ae_cfg.get("model", "wav2vec2")
    if kind == "mel_resnet18":
        from mer_amd.mel_resnet import EMBED, MelResNetEncoder
        if d_audio != EMBED:
            raise ValueError(f"runtime.audio_encoder.model mel_resnet18 produces {EMBED}-wide rows but model.AUDIO.embedding_size is "
                             f"{d_audio}: set it to {EMBED}")
        if n_head is not None and EMBED % int(n_head):
            raise ValueError(f"runtime.audio_encoder.model mel_resnet18: model.AUDIO.n_head {n_head} does not divide {EMBED}")
        enc = MelResNetEncoder(precision=ae_cfg.get("precision", "bf16"), png_levels=bool(ae_cfg.get("png_levels", True)))
        ck = ae_cfg.get("checkpoint", None)
        if ck:
            enc.load_state_dict(torch.load(os.path.abspath(ck), map_location="cpu"))
        return enc.to(device).eval()
    if kind != "wav2vec2":
        raise ValueError(f"runtime.audio_encoder.model {kind!r}: wav2vec2 or mel_resnet18")
    from mer_amd.wav2vec2 import Wav2Vec2Encoder, base_config
    geo = ae_cfg.get("geometry", "base")
    cfg = base_config()
    if not isinstance(geo, str):
        cfg.update(dict(geo))
    elif geo != "base":
        raise ValueError(f"runtime.audio_encoder.geometry {geo!r}: base or a dict of Wav2Vec2Config fields")
    if cfg["hidden_size"] != d_audio:
        raise ValueError(f"runtime.audio_encoder produces {cfg['hidden_size']}-wide rows but model.AUDIO.embedding_size is {d_audio}")
    enc = Wav2Vec2Encoder(cfg, precision=ae_cfg.get("precision", "bf16"))
    ck = ae_cfg.get("checkpoint", None)
    if ck:
        enc.load_state_dict(torch.load(os.path.abspath(ck), map_location="cpu"))
    return enc.to(device).eval()


def start_wandb(config):
    if wandb is None:
        raise RuntimeError("wandb.enabled is set but the wandb package is not installed")
    run_name = datetime.now().isoformat().split(".")[0]
    wandb.init(project=config.wandb.project_name, name=run_name, config=dict(config), entity=config.wandb.entity,
               settings=wandb.Settings(start_method="spawn" if os.name == "nt" else "fork"),
               resume="must" if config.wandb.resume_run else False, id=config.wandb.resume_run_id)


def resume_if_requested(config, model, optimizer, device):
    """-> first epoch to run (0, or the checkpoint's epoch + 1)."""
    path = os.path.abspath(config.checkpoint.load_path)
    if not (config.checkpoint.load_checkpoint and os.path.exists(path)):
        return 0
    state = torch.load(path, map_location=device)
    model.load_state_dict(state["model_state_dict"])
    optimizer.load_state_dict(state["optimizer_state_dict"])
    crf = getattr(model, "crf", None)
    if crf is not None:
        if CRF_KEY in state:
            crf.load_state_dict(state[CRF_KEY])
        elif _rank() == 0:
            print(f"Checkpoint {path} holds no {CRF_KEY}: the CRF block starts from its initialisation")
    head = getattr(model, "aux_head", None)
    if head is not None:
        if AUX_KEY in state:
            head.load_state_dict(state[AUX_KEY])
        elif _rank() == 0:
            print(f"Checkpoint {path} holds no {AUX_KEY}: the auxiliary head starts from its initialisation")
    if ema_settings(config) is not None:
        if EMA_KEY in state:
            optimizer.load_ema_state_dict(state[EMA_KEY])
        elif _rank() == 0:
            print(f"Checkpoint {path} holds no {EMA_KEY}: the weight average starts afresh")
    return state["epoch"] + 1


def _has_average(optimizer) -> bool:
    return getattr(optimizer, "n_averaged", 0) > 0


def attach_crf(model, criterion) -> None:
    """Under `solver.loss_fn: CRF` the criterion travels on the model as `model.crf` (object.__setattr__: not a sub-module - its block is
    neither in M2FNet's state_dict nor in the model's optimizer); checkpoints then carry it as 'crf_state_dict'."""
    object.__setattr__(model, "crf", criterion if isinstance(criterion, LinearChainCRF) else None)


def write_checkpoint(path, epoch, model, optimizer):
    """The reference's three entries - the LIVE weights, so a resume is exact - and, when the optimizer keeps a weight average
    (runtime.ema), FusedAdam.ema_state_dict() beside them."""
    state = dict(zip(CHECKPOINT_KEYS, (epoch, model.state_dict(), optimizer.state_dict())))
    if _has_average(optimizer):
        state[EMA_KEY] = optimizer.ema_state_dict()
    if getattr(model, "crf", None) is not None:           # (solver.loss_fn: CRF - the block is not in the model's state_dict)
        state[CRF_KEY] = model.crf.state_dict()
    if getattr(model, "aux_head", None) is not None:      # (runtime.aux_head - likewise outside the model's state_dict)
        state[AUX_KEY] = model.aux_head.state_dict()
    torch.save(state, path)


def main(config=None):
    config = get_config()
    # One process per GPU when launched under torchrun (WORLD_SIZE > 1) or with runtime.data_parallel: True - dialogues of every
    # global batch are sharded over the ranks, gradients are summed over RCCL with the GLOBAL valid-utterance denominator
    # (mer_amd/dp.py).  The reference is single-process (src/train.py:20); a single rank behaves exactly like it.
    want_dp = _runtime(config, "data_parallel", "auto")
    grad_accumulation_steps(config, int(os.environ.get("WORLD_SIZE", "1")))      # (refusals before the GPU is touched)
    clip_grad_norm(config, int(os.environ.get("WORLD_SIZE", "1")))
    ema_settings(config)
    sam_settings(config, int(os.environ.get("WORLD_SIZE", "1")))
    adversarial_settings(config, int(os.environ.get("WORLD_SIZE", "1")))
    context_settings(config)
    position_bias_settings(config)
    spk_on = speaker_heads_settings(config, int(os.environ.get("WORLD_SIZE", "1"))) is not None
    resolve_distill(config)
    rdrop_settings(config)
    supcon_settings(config)
    aux_on = aux_head_settings(config)
    focal_gamma_setting(config)
    crf_settings(config)
    watch_settings(config, int(os.environ.get("WORLD_SIZE", "1")))
    optimizer_groups(config, model_named_shapes(config.model))
    if want_dp not in (True, "auto") and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        # W independent trainings on one device, all writing the same checkpoint, is never what a launcher was asked for
        raise RuntimeError(f"runtime.data_parallel is {want_dp!r} but this process was launched as one of "
                           f"{os.environ['WORLD_SIZE']} ranks (WORLD_SIZE): set runtime.data_parallel to True / 'auto' or "
                           "launch a single process")
    rank, world, local = dp.init_distributed() if want_dp in (True, "auto") else (0, 1, 0)
    device = torch.device(f"cuda:{local}" if torch.cuda.is_available() else "cpu")
    if rank == 0:
        print(f"Using device {device}..." + (f" ({world} ranks)" if world > 1 else ""))
    torch.manual_seed(int(_runtime(config, "seed", 0)))       # identical replicas and identical shuffles on every rank

    ae_cfg = _runtime(config, "audio_encoder", None) or {}
    ae_on = bool(ae_cfg.get("enabled", False))
    ds_kw = {"train": {}, "val": {}}
    if spk_on:
        for mode in ds_kw:
            ds_kw[mode]["speakers"] = True                 # (batches then carry "speaker")
    if aux_on is not None:
        for mode in ds_kw:
            ds_kw[mode][aux_on["labels"]] = True           # (batches then carry the second label)
    if ae_on:
        # waveforms of every table row, read once (dia{D}_utt{U}.wav); the audio pickle is not read
        if not ae_cfg.get("wav_dir", None):
            raise RuntimeError("runtime.audio_encoder.enabled needs runtime.audio_encoder.wav_dir: the directory with dia{D}_utt{U}.wav")
        if _runtime(config, "device_batcher", False):
            raise RuntimeError("runtime.audio_encoder needs the DataLoader path (runtime.device_batcher: False): batches carry waveforms")
        from dataset import load_waveforms
        from utils import get_text
        for mode in ds_kw:
            table = get_text(mode)
            ds_kw[mode] = dict(ds_kw[mode], table=table, waveforms=load_waveforms(table, os.path.abspath(ae_cfg["wav_dir"])))
    te_on = bool((_runtime(config, "text_encoder", None) or {}).get("enabled", False))
    if te_on:
        # the tokenizer is the caller's: a LOCAL directory with the files of the reference's RobertaTokenizer (text/dataset.py:9,42 fetch
        # 'roberta-base' by name - there is no network here)
        tok_dir = _runtime(config, "text_encoder").get("tokenizer", None)
        if not tok_dir:
            raise RuntimeError("runtime.text_encoder.enabled needs runtime.text_encoder.tokenizer: a local directory with the tokenizer files")
        from transformers import AutoTokenizer
        from dataset import tokenised_contexts
        tok = AutoTokenizer.from_pretrained(os.path.abspath(tok_dir))
        max_tokens = int(_runtime(config, "text_encoder").get("max_tokens", 64))
        train_set, val_set = Dataset(mode="train", **ds_kw["train"]), Dataset(mode="val", **ds_kw["val"])
        for ds_ in (train_set, val_set):
            ds_.token_ids, ds_.token_mask = tokenised_contexts(ds_.text, tok, max_tokens)
    else:
        train_set, val_set = Dataset(mode="train", **ds_kw["train"]), Dataset(mode="val", **ds_kw["val"])
    if _runtime(config, "device_batcher", False):          # embedding tables in HBM, one gather kernel per batch
        dl_train = DeviceLoader(train_set, device=device, seed=_runtime(config, "seed", 0), **config.train.data_loader)
        dl_val = DeviceLoader(val_set, device=device, **config.val.data_loader)
    else:
        gen = torch.Generator().manual_seed(int(_runtime(config, "seed", 0)))
        dl_train = torch.utils.data.DataLoader(train_set, collate_fn=collate_fn, generator=gen, **config.train.data_loader)
        dl_val = torch.utils.data.DataLoader(val_set, collate_fn=collate_fn, **config.val.data_loader)
    if world > 1:
        dl_train = dp.ShardedLoader(dl_train, rank, world)

    model = build_model(config, device)
    # how train() runs the loop body: (fused m2f_step instead of forward / criterion / backward, as one hipGraph)
    model.step_mode = (bool(_runtime(config, "fused_step", True)), bool(_runtime(config, "use_graph", True)))
    model.fused_optimizer = bool(_runtime(config, "fused_optimizer", False))
    model.grad_accumulation_k = grad_accumulation_steps(config, world)
    model.device_metrics = bool(_runtime(config, "device_metrics", False))      # validate(): score on the device (M2FNet.eval_step)
    if bool(_runtime(config, "grad_bf16", False)) and world == 1:
        model.set_grad_bf16(True)
    te_cfg = _runtime(config, "text_encoder", None)
    if te_cfg and te_cfg.get("enabled", False):
        # BASELINE config C5: the text rows are computed in the loop from token ids (Dataset(token_ids=...)) instead of read from
        # embeddings/<text>/<mode>.pkl.  Built OUTSIDE the fusion model (object.__setattr__: not a sub-module - its weights are
        # neither in M2FNet's state_dict / checkpoint format nor in the optimizer, as in the reference, which trains it in its own stage).
        object.__setattr__(model, "text_encoder", build_text_encoder(te_cfg, config.model.TEXT.embedding_size, device))
    if ae_on:
        # the audio rows are computed in the loop from waveforms; built outside the fusion model, like the text encoder
        object.__setattr__(model, "audio_encoder", build_audio_encoder(ae_cfg, config.model.AUDIO.embedding_size, device,
                                                                             n_head=config.model.AUDIO.n_head))
    attach_distiller(config, model, device)
    object.__setattr__(model, "rdrop", rdrop_settings(config))       # (None: off; train() passes rdrop= on in every branch)
    object.__setattr__(model, "supcon", supcon_settings(config))     # (None: off; train() passes supcon= on to train_step)
    object.__setattr__(model, "adversarial", adversarial_settings(config, world))    # (None: off; train() then calls adversarial_step)
    attach_aux_head(model, aux_on, config.model.CLASSIFIER.hidden_size, device)      # (None: off; train() passes aux= on to train_step)
    criterion = build_criterion(config.solver, train_set, device, focal_gamma=focal_gamma_setting(config), crf=crf_settings(config))
    attach_crf(model, criterion)
    optimizer = build_optimizer(config, model)
    optimizer.max_grad_norm = clip_grad_norm(config, world)
    attach_watch(config, model, optimizer, rank, world)
    if world > 1:
        model.dp_step = dp.DataParallelStep(model, optimizer, n_buckets=int(_runtime(config, "grad_buckets", 4)),
                                            exchange=_runtime(config, "grad_exchange", "fp32"),
                                            overlap=bool(_runtime(config, "grad_overlap", False)),
                                            algorithm=_runtime(config, "grad_algorithm", "all_reduce"),
                                            crf=getattr(model, "crf", None))
    if config.wandb.enabled and rank == 0:
        start_wandb(config)
    lr_scheduler = build_scheduler(config.solver, optimizer)
    first_epoch = resume_if_requested(config, model, optimizer, device)

    if rank == 0:
        print("Training...")
    training_loop(model, dl_train, dl_val, criterion, optimizer, lr_scheduler, first_epoch, config, device)
    if rank == 0:
        print("Training complete")
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def _rank():
    return torch.distributed.get_rank() if torch.distributed.is_initialized() else 0


# ---- early stopping on the validation LOSS with the reference's best-weights file protocol --------------------------
class EarlyStopper:
    def __init__(self, settings, save_path):
        self.enabled = bool(settings.enabled)
        self.patience = settings.patience
        self.restore = bool(settings.restore_best_weights)
        self.save_path = save_path
        self.best_path = os.path.join(os.path.dirname(save_path), "best_weights.pth")
        self.best_loss = float("inf")
        self.epochs_without_improvement = 0

    def should_stop(self, val_loss, epoch, model, optimizer) -> bool:
        if not self.enabled:
            return False
        if val_loss < self.best_loss:
            self.best_loss, self.epochs_without_improvement = val_loss, 0
            if self.restore and _rank() == 0:
                write_checkpoint(self.best_path, epoch, model, optimizer)
            return False
        self.epochs_without_improvement += 1
        if self.epochs_without_improvement < self.patience:
            return False
        if _rank() != 0:
            return True
        print(f"Early stopping: patience {self.patience} reached")
        if self.restore:                                 # the final checkpoint becomes the best one; the side file goes away
            best = torch.load(self.best_path)
            torch.save({k: best[k] for k in CHECKPOINT_KEYS + (EMA_KEY, CRF_KEY) if k in best}, self.save_path)
            os.remove(self.best_path)
            print(f"Best model at epoch {best['epoch']} restored")
        return True


def training_loop(model, dl_train, dl_val, criterion, optimizer, lr_scheduler, start_epoch, config, device):
    solver = config.solver
    rank0 = _rank() == 0
    log_to_wandb = config.wandb.enabled and rank0
    save_path = os.path.abspath(config.checkpoint.save_path)
    os.makedirs(os.path.dirname(save_path), exist_ok=True)
    if log_to_wandb and config.wandb.watch_model:
        wandb.watch(model, criterion=criterion, log="all", log_freq=100, log_graph=False)
        if getattr(optimizer, "watch", None) is None:
            print("wandb.watch_model: wandb's parameter hooks do not see the gradients the kernels write (INTEGRATION.md section B); "
                  "runtime.watch: {enabled: True} logs them from the buffers the optimizer reads")

    stopper = EarlyStopper(solver.early_stopping, save_path)
    history = {"loss_values": [], "val_loss_values": []}
    ema = ema_settings(config)
    for epoch in range(start_epoch, solver.epochs):
        train_loss = train(model, dl_train, criterion, optimizer, epoch, log_to_wandb, device)
        if ema is not None and ema[2] and _has_average(optimizer):
            # runtime.ema.evaluate: the printed and early-stopping numbers are those of the averaged weights (host path and
            # device_metrics alike); the checkpoints below are written outside the context, with the live weights
            with optimizer.averaged_parameters():
                val_loss, accuracy, weighted_f1 = validate(model, dl_val, criterion, device)
        else:
            val_loss, accuracy, weighted_f1 = validate(model, dl_val, criterion, device)
        history["loss_values"].append(train_loss)
        history["val_loss_values"].append(val_loss)

        if config.checkpoint.save_checkpoint and rank0:
            write_checkpoint(save_path, epoch, model, optimizer)
        lr_now = optimizer.param_groups[0]["lr"]
        if lr_scheduler is not None and solver.scheduler.enabled:
            lr_scheduler.step()
        if rank0:
            print(f"Epoch: {epoch} lr: {lr_now:.3E} Train=[{train_loss:.3E}] Val=[{val_loss:.3E}] "
                  f"Accuracy=[{accuracy * 100:.3f}%] Weighted_F1=[{weighted_f1 * 100:.3f}%]")
        aux_accuracy = getattr(model, "aux_val_accuracy", None)          # (runtime.aux_head: the head's accuracy of this validation pass)
        if rank0 and aux_accuracy is not None:
            print(f"Epoch: {epoch} Aux_accuracy=[{aux_accuracy * 100:.3f}%]")
        if log_to_wandb:
            wandb.log({"Params/Epoch": epoch, "Params/Learning_Rate": lr_now, "Train/Loss": train_loss,
                       "Validation/Loss": val_loss, "Validation/Accuracy": accuracy, "Validation/Weighted_F1": weighted_f1,
                       **({} if aux_accuracy is None else {"Validation/Aux_accuracy": aux_accuracy})})
        if stopper.should_stop(val_loss, epoch, model, optimizer):
            break
    if log_to_wandb:
        wandb.finish()
    if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        torch.distributed.barrier()                      # rank 0 may still be moving checkpoint files
    return history


def _step_mode(model, criterion):
    """(fused, use_graph): the whole loop body as one m2f_step launch when the model / criterion are the HIP-backed ones.
    The two switches are read from the `runtime:` block ONCE, in main(), and travel on the model (`model.step_mode`)."""
    fused, use_graph = getattr(model, "step_mode", (True, True))
    return fused and isinstance(criterion, (M2FCrossEntropyLoss, LinearChainCRF)) and hasattr(model, "train_step"), use_graph


def _grad_norm_log(optimizer):
    """{"Train/Grad_norm": ...} of the step just taken when the optimizer clips (runtime.clip_grad_norm), else nothing.  One more
    scalar read on a path that already waits for loss.item() every step."""
    if getattr(optimizer, "max_grad_norm", None) is None:
        return {}
    return {"Train/Grad_norm": float(optimizer.grad_norm())}


def _sam_log(optimizer):
    """{"Train/SAM_grad_norm": ...} of the step just taken when the optimizer runs sharpness-aware minimisation (runtime.sam): the norm
    of the first pass's gradient, else nothing.  One more scalar read on a path that already waits for loss.item() every step."""
    if getattr(optimizer, "sam_rho", None) is None:
        return {}
    return {"Train/SAM_grad_norm": float(optimizer.sam_norm())}


def _watch_log(optimizer, wandb_log):
    """After a due step of the optimizer's watch (runtime.watch): reads its record - one copy, on a path that has just waited for
    loss.item() - appends the JSON line to runtime.watch.file and returns {"gradients/<name>": wandb.Histogram, ...} for the step's
    wandb.log call; otherwise nothing."""
    w = getattr(optimizer, "watch", None)
    if w is None or not w.pending:
        return {}
    rec = w.read()
    if w.file is not None:
        with open(w.file, "a") as f:
            f.write(w.json_line(rec) + "\n")
    if not wandb_log:
        return {}
    return {k: wandb.Histogram(np_histogram=v) for k, v in w.wandb_payload(rec).items()}


def train(model, dl_train, criterion, optimizer, epoch, wandb_log, device):
    """One epoch; returns the mean of the per-batch losses (reference src/train.py:217-243)."""
    model.train()
    fused, use_graph = _step_mode(model, criterion)
    dp_step = getattr(model, "dp_step", None)             # set by main() when there is more than one rank
    k = int(getattr(model, "grad_accumulation_k", 1))
    if k > 1:
        return _train_accumulating(model, dl_train, criterion, optimizer, epoch, wandb_log, device, k, fused, use_graph, dp_step)
    running = 0.0
    shares_log = _SharesLog(model, bool(wandb_log))
    progress = tqdm(enumerate(dl_train), total=len(dl_train), desc=f"Epoch {epoch}", disable=_rank() != 0)
    for step, batch in progress:
        text, audio, emotion, padding_mask = move_batch(batch, device, non_blocking=True, text_encoder=getattr(model, "text_encoder", None),
                                                           audio_encoder=getattr(model, "audio_encoder", None))
        rdrop = _rdrop_kw(model, epoch * len(dl_train) + step)
        if rdrop and not fused:
            raise ValueError("runtime.rdrop needs runtime.fused_step: True and the M2FCrossEntropyLoss criterion")
        supcon = _supcon_kw(model, epoch * len(dl_train) + step)
        if supcon and (not fused or dp_step is not None):
            raise ValueError("runtime.supcon needs runtime.fused_step: True, the M2FCrossEntropyLoss criterion and one process")
        aux = _aux_kw(model, batch, device, epoch * len(dl_train) + step)
        if aux and (not fused or dp_step is not None):
            raise ValueError("runtime.aux_head needs runtime.fused_step: True, the M2FCrossEntropyLoss criterion and one process")
        if dp_step is not None:
            # sharded step: local sum-gradient -> RCCL all-reduce with the global denominator -> fused Adam, all inside
            loss = dp_step(text, audio, padding_mask, emotion, use_graph=use_graph, **_distill_kw(model, text, audio, padding_mask),
                           **_crit_kw(criterion, data_parallel=True), **rdrop)
        else:
            optimizer.zero_grad()
            _crf_zero_grad(criterion)
            _aux_zero_grad(aux)
            if fused and getattr(model, "fused_optimizer", False) and isinstance(optimizer, FusedAdam):
                # forward, criterion, backward AND optimizer.step() as one launch list (src/train.py:227-231 of the reference)
                loss = model.train_step(text, audio, padding_mask, emotion, use_graph=use_graph, optimizer=optimizer,
                                        **_distill_kw(model, text, audio, padding_mask), **_speaker_kw(model, batch, device),
                                        **_crit_kw(criterion), **rdrop, **supcon, **aux)
                _crf_step(criterion)
                _aux_step(aux)
                running += loss.item()
                if wandb_log:
                    wandb.log({"Train/Running_loss": running / (step + 1), "Params/Global_step": epoch * len(dl_train) + step,
                               **_grad_norm_log(optimizer), **shares_log(step)})
                continue
            sam = getattr(optimizer, "sam_rho", None) is not None
            if sam and not fused:
                raise ValueError("runtime.sam needs runtime.fused_step: True and the M2FCrossEntropyLoss criterion")
            if sam:
                # sharpness-aware minimisation: the step at w, the perturbation, the step at w + e, the restore and the update
                loss = model.sam_step(text, audio, padding_mask, emotion, optimizer, use_graph=use_graph,
                                      **_distill_kw(model, text, audio, padding_mask), **_speaker_kw(model, batch, device),
                                      **_crit_kw(criterion), **rdrop, **supcon, **aux)
                _crf_step(criterion)
                _aux_step(aux)
                running += loss.item()
                watched = _watch_log(optimizer, wandb_log)
                if wandb_log:
                    wandb.log({"Train/Running_loss": running / (step + 1), "Params/Global_step": epoch * len(dl_train) + step,
                               **_grad_norm_log(optimizer), **_sam_log(optimizer), **watched, **shares_log(step)})
                continue
            adv = getattr(model, "adversarial", None)
            if adv and not fused:
                raise ValueError("runtime.adversarial needs runtime.fused_step: True and the M2FCrossEntropyLoss criterion")
            if adv:
                # adversarial training on the input embeddings: K passes on text + delta / audio + delta, the summed gradient applied
                loss = model.adversarial_step(text, audio, padding_mask, emotion, optimizer, use_graph=use_graph, **adv,
                                              **_distill_kw(model, text, audio, padding_mask), **_speaker_kw(model, batch, device),
                                              **_crit_kw(criterion), **supcon, **aux)
                _crf_step(criterion)
                _aux_step(aux)
                delta_norm = _adv_delta_norm(model, padding_mask) if wandb_log else None
                running += loss.item()
                watched = _watch_log(optimizer, wandb_log)
                if wandb_log:
                    wandb.log({"Train/Running_loss": running / (step + 1), "Params/Global_step": epoch * len(dl_train) + step,
                               "Train/Adv_delta_norm": float(delta_norm), **_grad_norm_log(optimizer), **watched, **shares_log(step)})
                continue
            if fused:
                loss = model.train_step(text, audio, padding_mask, emotion, use_graph=use_graph, **_distill_kw(model, text, audio, padding_mask),
                                        **_speaker_kw(model, batch, device), **_crit_kw(criterion), **rdrop, **supcon, **aux)
            else:
                if getattr(model, "distiller", None) is not None:
                    raise ValueError("runtime.distill needs runtime.fused_step: True and the M2FCrossEntropyLoss criterion")
                loss = criterion(model(text, audio, padding_mask, **_speaker_kw(model, batch, device)).permute(0, 2, 1), emotion)
                loss.backward()
            optimizer.step()
            _crf_step(criterion)
            _aux_step(aux)
        running += loss.item()
        watched = _watch_log(optimizer, wandb_log)
        if wandb_log:
            wandb.log({"Train/Running_loss": running / (step + 1), "Params/Global_step": epoch * len(dl_train) + step,
                       **_grad_norm_log(optimizer), **watched, **shares_log(step)})
    return running / len(dl_train)


def _train_accumulating(model, dl_train, criterion, optimizer, epoch, wandb_log, device, k, fused, use_graph, dp_step):
    """One epoch with runtime.grad_accumulation = k > 1: k consecutive batches per optimizer step, each a train_step(normalise=False)
    that adds its gradients and its criterion den / num into the model's buffers (M2FNet.set_grad_accumulation); the optimizer then
    divides by the group's den - the reference criterion on the concatenated batch.  The last, shorter group steps as well.  Under
    data parallelism micro-batches 1 .. k-1 run with sync=False and the last one exchanges once.  Returns the mean over the
    optimizer steps of the group losses num / den."""
    if not fused:
        raise ValueError("runtime.grad_accumulation > 1 needs runtime.fused_step: True and the M2FCrossEntropyLoss criterion")
    if getattr(optimizer, "sam_rho", None) is not None:
        raise ValueError("runtime.sam does not combine with runtime.grad_accumulation > 1 in this loop (FusedAdam's docstring has the two-sweep form)")
    if getattr(model, "aux_head", None) is not None:
        raise ValueError("runtime.aux_head does not combine with runtime.grad_accumulation > 1 (the head trains: its gradient would need the group's den)")
    if dp_step is None:
        model.set_grad_accumulation(True)
    n_groups = (len(dl_train) + k - 1) // k
    running = 0.0
    shares_log = _SharesLog(model, bool(wandb_log))          # (no auxiliary head here: refused above)
    progress = tqdm(enumerate(group_batches(dl_train, k)), total=n_groups, desc=f"Epoch {epoch}", disable=_rank() != 0)
    for step, group in progress:
        rdrop = _rdrop_kw(model, epoch * n_groups + step)     # (one alpha per optimizer step: the group's shares add up)
        supcon = _supcon_kw(model, epoch * n_groups + step)   # (likewise one weight; each micro-batch contrasts within itself)
        if supcon and dp_step is not None:
            raise ValueError("runtime.supcon needs one process (the data-parallel step refuses supcon)")
        if dp_step is None:
            optimizer.zero_grad()                        # (every .grad None: the first micro-batch overwrites, den / num too)
        for j, batch in enumerate(group):
            text, audio, emotion, padding_mask = move_batch(batch, device, non_blocking=True, text_encoder=getattr(model, "text_encoder", None),
                                                               audio_encoder=getattr(model, "audio_encoder", None))
            if dp_step is not None:
                loss = dp_step(text, audio, padding_mask, emotion, use_graph=use_graph, sync=j == len(group) - 1,
                               **_distill_kw(model, text, audio, padding_mask), **_crit_kw(criterion, data_parallel=True), **rdrop)
            else:
                model.train_step(text, audio, padding_mask, emotion, normalise=False, use_graph=use_graph,
                                 **_distill_kw(model, text, audio, padding_mask), **_speaker_kw(model, batch, device),
                                 **_crit_kw(criterion), **rdrop, **supcon)
        if dp_step is None:
            terms = model.loss_terms()
            optimizer.grad_scale = terms[1:2]            # the group's den: gradients / den = the mean over every valid utterance
            optimizer.step()
            loss = terms[2] / terms[1]
        running += loss.item()
        watched = _watch_log(optimizer, wandb_log)
        if wandb_log:
            wandb.log({"Train/Running_loss": running / (step + 1), "Params/Global_step": epoch * n_groups + step,
                       **_grad_norm_log(optimizer), **watched, **shares_log(step)})
    if dp_step is None:
        optimizer.grad_scale = None
    return running / max(n_groups, 1)


def _rank_share(dl_val, rank, world):
    """Batches r, r + W, ... of the validation loader.  A torch DataLoader is re-built over exactly those index batches, so a rank
    neither collates nor uploads the batches it would discard; that needs the batches to be the same on every rank, i.e. no
    shuffling (the reference validates with shuffle: False, src/config.yaml:66).  Other loaders (DeviceLoader) are iterated and
    the foreign batches skipped."""
    if world == 1:
        return dl_val
    if isinstance(dl_val, torch.utils.data.DataLoader) and dl_val.batch_sampler is not None:
        if not isinstance(dl_val.sampler, torch.utils.data.SequentialSampler):
            raise ValueError("validation over several ranks deals whole batches to the ranks: val.data_loader.shuffle must be False")
        mine = list(dl_val.batch_sampler)[rank::world]
        return torch.utils.data.DataLoader(dl_val.dataset, batch_sampler=mine, collate_fn=dl_val.collate_fn,
                                           num_workers=dl_val.num_workers, pin_memory=dl_val.pin_memory)
    return (b for i, b in enumerate(dl_val) if i % world == rank)


def decoded(crf, logits, padding_mask):
    """What the scores' per-row argmax reads: the logits - or, under a CRF (a LinearChainCRF; anything else: the logits), the one-hot
    rows of its Viterbi path over each dialogue's utterances, so that the argmax IS the path."""
    if not isinstance(crf, LinearChainCRF):
        return logits
    path = crf.decode(logits, padding_mask.bool())
    return torch.nn.functional.one_hot(path.clamp(min=0), logits.shape[-1]).to(logits.dtype)


def _note_aux_accuracy(model, aux_acc) -> None:
    """The auxiliary head's accuracy of a validation pass (runtime.aux_head) travels on the model as `model.aux_val_accuracy` for the
    epoch's print and wandb line.  Nothing without a head: the pass of a run without it is today's."""
    if aux_acc.head is not None:
        model.aux_val_accuracy = aux_acc.result()


def validate(model, dl_val, criterion, device):
    """-> (mean batch loss, accuracy, weighted_f1); scores by the per-batch rule of ``metrics.BatchScores``.
    With several ranks the replicas are identical and the rule is a plain mean over the reference's batches
    (src/train.py:245-272), so rank r evaluates batches r, r + W, ... WHOLE and the per-batch sums are added over the ranks:
    the same three numbers as the single-process loop, on every rank (early stopping decides alike everywhere).
    With ``model.device_metrics`` (runtime.device_metrics, read once in main()) the loop body is ``model.eval_step``: loss, argmax,
    accuracy and weighted F1 of every batch are formed on the device and the host reads one record after the last batch."""
    rank = _rank()
    world = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
    model.eval()
    if getattr(model, "device_metrics", False):
        return _validate_on_device(model, dl_val, criterion, device, rank, world)
    scores, loss_total = BatchScores(), 0.0
    aux_acc = AuxAccuracy(model)
    with torch.inference_mode():
        for batch in tqdm(_rank_share(dl_val, rank, world), total=(len(dl_val) - rank + world - 1) // world, desc="Validation", disable=rank != 0):
            text, audio, emotion, padding_mask = move_batch(batch, device, text_encoder=getattr(model, "text_encoder", None),
                                                           audio_encoder=getattr(model, "audio_encoder", None))
            logits = model(text, audio, padding_mask, **_speaker_kw(model, batch, device))
            loss_total += criterion(logits.permute(0, 2, 1), emotion).item()
            scores.update(decoded(criterion, logits, padding_mask), emotion)
            aux_acc.update(model, batch, device)
    _note_aux_accuracy(model, aux_acc)
    acc_sum, f1_sum = scores.sums()
    loss_total, acc_sum, f1_sum, n = dp.sum_over_ranks([loss_total, acc_sum, f1_sum, float(scores.n_batches)], device=device)
    n = max(n, 1.0)
    return loss_total / n, acc_sum / n, f1_sum / n


def _validate_on_device(model, dl_val, criterion, device, rank, world):
    from mer_amd.metrics import DeviceScores
    if not isinstance(criterion, (M2FCrossEntropyLoss, LinearChainCRF)):
        raise ValueError("runtime.device_metrics: True scores with the M2FCrossEntropyLoss criterion's kernel; another criterion needs the host loop")
    scores = DeviceScores(model.m2f_config.cls_out, device)
    _, use_graph = _step_mode(model, criterion)
    aux_acc = AuxAccuracy(model)
    with torch.inference_mode():
        for batch in tqdm(_rank_share(dl_val, rank, world), total=(len(dl_val) - rank + world - 1) // world, desc="Validation", disable=rank != 0):
            text, audio, emotion, padding_mask = move_batch(batch, device, text_encoder=getattr(model, "text_encoder", None),
                                                           audio_encoder=getattr(model, "audio_encoder", None))
            model.eval_step(text, audio, padding_mask, emotion, scores, use_graph=use_graph, **_speaker_kw(model, batch, device),
                            **_crit_kw(criterion))
            aux_acc.update(model, batch, device)
    _note_aux_accuracy(model, aux_acc)
    loss_total, acc_sum, f1_sum, n = dp.sum_over_ranks(list(scores.totals()), device=device)      # (the one read of the pass)
    n = max(n, 1.0)
    return loss_total / n, acc_sum / n, f1_sum / n


if __name__ == "__main__":
    main()
