"""``M2FNet`` / ``FusionAttentionModule``: host-side mirrors of the reference's ``src/model.py``.

Same constructor arguments, ``forward`` signature, ``state_dict`` keys and default initialisation as
/root/reference/src/model.py:5-145, but the modules here only HOLD parameters (as views into one flat
fp32 buffer in HBM); every forward/backward FLOP runs in the gfx950 kernels behind ``runtime.Plan``.
No ``nn.Transformer*`` / ``nn.MultiheadAttention`` / ``nn.Linear`` forward is ever called.
"""
from __future__ import annotations

import collections
import copy
import math
import os
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import runtime
from .criterion import PLAIN, resolve
from .layout import M2FConfig, param_specs


# ------------------------------------------------------------------------------------------------------
# parameter holders (names chosen so the state_dict keys equal the reference's)
# ------------------------------------------------------------------------------------------------------
class _LinearParams(nn.Module):
    """weight [out, in], bias [out]; default init of nn.Linear (kaiming_uniform(a=sqrt(5)) + fan-in bias)."""

    def __init__(self, in_features: int, out_features: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(in_features) if in_features > 0 else 0.0
        nn.init.uniform_(self.bias, -bound, bound)


class _NormParams(nn.Module):
    def __init__(self, d: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.bias = nn.Parameter(torch.zeros(d))


class _MHAParams(nn.Module):
    """in_proj_weight [3E, E] (xavier-uniform), in_proj_bias = 0, out_proj.{weight, bias = 0}:
    the parameter set and init order of nn.MultiheadAttention (out_proj is created before the
    xavier init of in_proj_weight, so the RNG is consumed in the same order as the reference)."""

    def __init__(self, embed_dim: int, num_heads: int):
        super().__init__()
        if embed_dim % num_heads != 0:
            raise AssertionError("embed_dim must be divisible by num_heads")
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * embed_dim))
        self.out_proj = _LinearParams(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.in_proj_bias, 0.0)
        nn.init.constant_(self.out_proj.bias, 0.0)


class _EncoderLayerParams(nn.Module):
    def __init__(self, d: int, n_head: int, dim_ff: int):
        super().__init__()
        self.self_attn = _MHAParams(d, n_head)
        self.linear1 = _LinearParams(d, dim_ff)
        self.linear2 = _LinearParams(dim_ff, d)
        self.norm1 = _NormParams(d)
        self.norm2 = _NormParams(d)


class _EncoderStack(nn.Module):
    """nn.TransformerEncoder(encoder_layer, num_layers, norm): the layers are deep copies of ONE template
    (identical initial weights), the final norm object is shared, not cloned (model.py:61-65)."""

    def __init__(self, template: _EncoderLayerParams, d: int, n_head: int, dim_ff: int, num_layers: int,
                 norm: _NormParams):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(template) for _ in range(num_layers)])
        self.norm = norm


class FusionAttentionModule(nn.Module):
    """Mirror of reference src/model.py:5-20.  Inside ``M2FNet`` it is a parameter holder (the fusion stack
    runs in the plan); called on its own it executes the same gfx950 kernels layer-wise (inference only)."""

    def __init__(self, embedding_size: int, n_head: int, dropout: float, position_bias: Optional[float] = None,
                 speaker_heads: Optional[Tuple[int, int]] = None):
        super().__init__()
        # speaker heads of a standalone call (runtime.speaker_heads: None = off); inside M2FNet the model's own setting rules
        self.speaker_heads = runtime.speaker_heads(speaker_heads, {"this module": n_head})
        # gain of the distance-decay attention bias of a standalone call (runtime.position_bias: None = off; stored as applied);
        # inside M2FNet the model's own setting rules (M2FNet.set_position_bias), this attribute is not read
        self.position_bias = runtime.position_bias(position_bias) or None
        self.multihead_attention = _MHAParams(embedding_size, n_head)
        self.linear = _LinearParams(2 * embedding_size, embedding_size)
        self.relu = nn.ReLU()
        self.embedding_size, self.n_head, self.dropout_p = embedding_size, n_head, dropout

    def forward(self, text: torch.Tensor, audio: torch.Tensor, key_padding_mask: torch.Tensor,
                past: Optional[int] = None, future: Optional[int] = None, need_weights: bool = False,
                speakers: Optional[torch.Tensor] = None):
        """past / future: context band of the attention (``functional.attention_fwd``): text utterance i attends to the audio of
        utterances i - past .. i + future only, None = unlimited.  The reference's module has no such argument.
        need_weights: return ``(y, weights [B, L, L])`` - the head-averaged attention map that the reference's own
        ``nn.MultiheadAttention`` call computes and drops (src/model.py:14); default: ``y`` alone, as ever.
        The module's ``position_bias`` (constructor; None = off) adds the distance-decay bias of ``functional.attention_fwd``.
        speakers ([B, L] ids, ``runtime.speaker_ids``): required by a module built with ``speaker_heads=(n_same, n_other)`` - text
        utterance i then sees, on its same-speaker heads, the audio of its own speaker's utterances only, on its other-speaker heads
        that of the others only; a module without the setting refuses the argument."""
        from . import functional as F
        _check_speakers("FusionAttentionModule.forward", self.speaker_heads, speakers, key_padding_mask.shape)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("standalone FusionAttentionModule.forward is inference-only; train it inside M2FNet "
                               "(wrap the call in torch.no_grad())")
        return F.fam_layer_forward(text, audio, key_padding_mask, self.multihead_attention.in_proj_weight,
                                   self.multihead_attention.in_proj_bias, self.multihead_attention.out_proj.weight,
                                   self.multihead_attention.out_proj.bias, self.linear.weight, self.linear.bias,
                                   self.n_head, past=past, future=future, need_weights=need_weights, bias=self.position_bias,
                                   speakers=speakers, speaker_heads=self.speaker_heads)


def _check_speakers(who: str, heads, speakers, shape) -> Optional[torch.Tensor]:
    """The batch's speaker ids as uint8 [B, L] for a model / module with speaker heads; None for one without.  A model with the setting
    called without ids, and a model without it called WITH ids (it would ignore them), both raise ValueError."""
    if heads is None:
        if speakers is not None:
            raise ValueError(f"{who}: speakers were given, but this model has no speaker heads (speaker_heads=(n_same, n_other)); "
                             "it would ignore them")
        return None
    if speakers is None:
        raise ValueError(f"{who}: this model has speaker_heads={heads}; pass speakers= (one id per utterance, [B, L])")
    ids = runtime.speaker_ids(speakers, f"{who}: speakers")
    if tuple(ids.shape) != tuple(shape):
        raise ValueError(f"{who}: speakers must be [B, L] = {tuple(shape)} like the mask, got {tuple(ids.shape)}")
    return ids


class _Anchor(torch.autograd.Function):
    """Connects the plan's forward/backward to autograd: ``text`` and ``audio`` are real inputs (as in the reference, where they are
    ordinary autograd leaves or outputs of whatever made them), the dummy leaf ``anchor`` stands for the parameters.
    ``loss.backward()`` (reference src/train.py:230) reaches ``backward`` below, which runs the HIP backward launch list, publishes
    the flat gradient buffer as the parameters' ``.grad`` views (when the plan computes them) and returns fresh copies of the
    input gradients the plan computed."""

    @staticmethod
    def forward(ctx, anchor, text, audio, model, plan):
        eng = model._engine
        if plan.cfg.dropout > 0.0 and plan.train:
            runtime.check(runtime.lib().m2f_rng_advance(eng.rng.data_ptr(), runtime.stream_ptr()), "m2f_rng_advance")
        logits = plan.forward()
        ctx.model, ctx.plan, ctx.version = model, plan, plan.version
        # the token-row map of THIS batch (a later forward on another instance cannot touch it, a packed plan re-makes it per batch)
        ctx.rows = (plan._dst, plan._valid, (plan.in_B, plan.in_L))
        ctx.in_shapes = tuple((x.shape, x.dtype) if isinstance(x, torch.Tensor) else None for x in (text, audio))
        return logits.clone()

    @staticmethod
    def backward(ctx, dlogits):
        plan = ctx.plan
        if not plan.handle:
            raise RuntimeError("M2FNet: the plan holding the activations of this forward was destroyed")
        if plan.version != ctx.version:
            raise RuntimeError("M2FNet: the activations of this forward were overwritten by a later forward of the "
                               "same plan shape (more graphs were kept alive than the plan cache may hold - raise "
                               "M2F_MAX_PLANS / M2F_MAX_PLAN_BYTES, or call backward() before further forwards)")
        plan.set_dlogits(dlogits)
        if plan.param_grads:
            ctx.model._engine.begin_backward(plan)
        plan.backward()
        plan.release()                                    # (a second backward through the same graph re-runs on the same buffers)
        if plan.param_grads:
            ctx.model._engine.publish_grads()
        dst, valid, shape = ctx.rows
        grads = []
        for i, bit in ((1, runtime.IN_TEXT), (2, runtime.IN_AUDIO)):
            if not (ctx.needs_input_grad[i] and plan.input_mask & bit):
                grads.append(None)
                continue
            g = plan.input_grad(bit, dst, valid, shape)
            xshape, xdtype = ctx.in_shapes[i - 1]
            grads.append(g.to(xdtype).reshape(xshape))
        return None, grads[0], grads[1], None, None


class _Engine:
    """Device state of one M2FNet: flat parameter / gradient buffers, dropout RNG state, plan cache."""

    def __init__(self, model: "M2FNet", device: torch.device):
        runtime.require_gpu()
        self.model, self.device, self.cfg = model, device, model.m2f_config
        total = runtime.verify_layout(self.cfg)
        specs, _ = param_specs(self.cfg)
        named = dict(model.named_parameters(remove_duplicate=False))
        self.flat = torch.zeros(total, dtype=torch.float32, device=device)
        self.flat_grad: Optional[torch.Tensor] = None
        self.flat_grad_ext: Optional[torch.Tensor] = None
        self.items = []                       # (param, offset, numel, shape)
        seen = set()
        with torch.no_grad():
            for sp in specs:
                p = named[sp.name]
                if sp.alias_of or id(p) in seen:
                    continue
                seen.add(id(p))
                view = self.flat[sp.offset: sp.offset + sp.numel].view(sp.shape)
                view.copy_(p.detach().to(device=device, dtype=torch.float32))
                p.data = view
                self.items.append((p, sp.offset, sp.numel, sp.shape))
        from .dp import dropout_seed
        rank = torch.distributed.get_rank() if torch.distributed.is_available() and torch.distributed.is_initialized() else 0
        lo, hi = dropout_seed(torch.initial_seed(), rank)     # replicas share weights (same seed) but not dropout masks
        to_i32 = lambda u: u - (1 << 32) if u >= (1 << 31) else u
        self.rng = torch.tensor([to_i32(lo), to_i32(hi), 0, 0], dtype=torch.int32, device=device)
        # plan cache: least-recently-used first; at most `max_plans` plans / `max_plan_bytes` of workspaces (+ captured graphs)
        # stay alive.  Keys are (shape bucket, mode, instance): a shape whose plan still holds the activations of a forward
        # that has not run its backward yet (`Plan.busy`) gets a second instance instead of overwriting them, so
        # `forward(A); forward(B); loss_A.backward()` works as it does in the reference when A and B share a bucket.
        # Shape buckets make the working set of a training run 3 L-buckets x {full, last partial batch} x {train, eval}.
        self.plans: "collections.OrderedDict[Tuple, runtime.Plan]" = collections.OrderedDict()
        self.max_plans = int(os.environ.get("M2F_MAX_PLANS", "16"))
        self.max_plan_bytes = int(float(os.environ.get("M2F_MAX_PLAN_BYTES", str(96 * 2 ** 30))))
        self.shape_buckets = model.shape_buckets
        self.grad_views = None
        self.anchor = torch.zeros(1, device=device, requires_grad=True)
        self.stream = torch.cuda.Stream(device=device)    # hipGraph capture is illegal on the default stream
        self.precision = runtime.PRECISIONS[model.precision]
        # bf16 mode: ONE buffer of bf16 parameter shadows (W and W^T of every 2-D parameter) for all plans, kept current by
        # FusedAdam.step itself (m2f_adam_step_shadowed).  `_fresh_token` = the parameters' version counters at the moment the
        # optimizer last wrote the shadows: any later in-place change through torch (load_state_dict, a foreign optimizer,
        # p.mul_(), writes through the flat buffer or its views) moves the counters, the plans then re-cast the shadows at the head of
        # their forward as before.  Writes that bypass the counters (p.data...) need `invalidate_shadows()`; `flat_parameters()` calls it.  M2F_SHARED_SHADOWS=0: off.
        self.wshadow: Optional[torch.Tensor] = None
        self.last = None                                      # (plan, version, dst, valid, (b, l)) of the most recent forward (note_forward)
        self.last_inputs = None                               # ... of the most recent train_step(input_grads=) + its input mask (last_input_grads)
        self.last_adv = None                                  # ... of the most recent adversarial_step + its modality mask (last_perturbation)
        self.grad_bf16_buf: Optional[torch.Tensor] = None     # bf16 [n_params]: train plans leave their gradients here (set_grad_bf16)
        self.accumulate = False                               # torch's .grad rule at every backward (M2FNet.set_grad_accumulation)
        self._fresh_token = None
        if self.precision == runtime.BF16 and os.environ.get("M2F_SHARED_SHADOWS", "1") != "0":
            self.wshadow = runtime.param_shadow_buffer(self.cfg, device)

    def note_forward(self, plan) -> None:
        """`plan` has just run a forward for this model: `M2FNet.last_attention` reads its saved probabilities (and the row map of
        THIS batch - a packed plan re-makes it per batch)."""
        self.last = (plan, plan.version, plan._dst, plan._valid, (plan.in_B, plan.in_L))

    def _version_token(self):
        # the parameters' own counters + the flat buffer's (shared by every view of it: a write through `flat_parameters()` or a
        # slice of it moves that one; the fused Adam kernels write through raw pointers and move neither)
        # (an engine first built under torch.inference_mode() holds an inference tensor: no counter, and no in-place writes outside
        # inference mode either)
        return (sum(p._version for (p, _, _, _) in self.items), 0 if self.flat.is_inference() else self.flat._version)

    def mark_shadows_fresh(self) -> None:
        self._fresh_token = self._version_token()

    def invalidate_shadows(self) -> None:
        self._fresh_token = None

    def shadows_fresh(self) -> bool:
        return self.wshadow is not None and self._fresh_token is not None and self._fresh_token == self._version_token()

    def ensure_grad(self) -> torch.Tensor:
        if self.flat_grad is None:
            from .dp import TAIL
            # [gradients | den, num, 0...]: the tail rides along in the data-parallel all-reduce (dp.py)
            self.flat_grad_ext = torch.zeros(self.flat.numel() + TAIL, dtype=torch.float32, device=self.device)
            self.flat_grad = self.flat_grad_ext[: self.flat.numel()]
            self.grad_views = [self.flat_grad[o: o + n].view(s) for (_, o, n, s) in self.items]
        return self.flat_grad

    @staticmethod
    def bucket(B: int, L: int) -> Tuple[int, int]:
        """Plan shape for a batch of B dialogues x L utterances: L rounded up to a multiple of 16 (the attention kernels'
        tile; MELD batches have L anywhere in 1..33 -> three shapes) - above 64, to a multiple of 64 (the long-dialogue
        kernels' block) -, B to a power of two below 8 and a multiple of 8 above (only the last, partial batch of an epoch
        differs from batch_size)."""
        Lb = (L + 15) // 16 * 16 if L <= 64 else (L + 63) // 64 * 64
        Bb = 1 << max(B - 1, 0).bit_length() if B <= 8 else (B + 7) // 8 * 8
        return Bb, Lb

    @staticmethod
    def plan_key(B, L, T, want_backward, dropout_active, precision, outputs=(0, True), band=(None, None), bias=None, speakers=None) -> Tuple:
        """A plan's key without its instance number.  Only a non-default `outputs` / context band / position bias (the applied gain;
        None or 0 = off) extends the tuple: the keys of a model that uses none of them are what they were before any existed."""
        key = (B, L, T, want_backward, dropout_active, precision) + (() if outputs == (0, True) else (outputs,))
        key = key if band == (None, None) else key + (("context",) + tuple(band),)
        key = key if not bias else key + (("position_bias", float(bias)),)
        return key if not speakers else key + (("speaker_heads",) + tuple(speakers),)      # (a speaker setting: its own plans again)

    def plan(self, B: int, L: int, want_backward: bool, dropout_active: bool, valid: Optional[int] = None,
             outputs: Tuple[int, bool] = (0, True)) -> runtime.Plan:
        """valid: number of valid utterances of the batch (packed mode) - the plan then holds that many token rows (rounded up to
        a multiple of 64, plus one row per filler dialogue and one spare) instead of B x L slots; batches that are at least
        85 % full keep the padded plan.  Batches with L > 64 always get a packed plan (padded plans hold L <= 64).
        outputs: what a backward computes - (input_mask, parameter gradients) of m2f_plan_backward_outputs; part of the key, so a
        plan of one setting never flips to another (train_step uses the default (0, True) unless it is asked for input_grads=).
        The model's context band (M2FNet.context) is part of the key in the same way: every band has its own plans; so is its
        position bias (M2FNet.position_bias)."""
        b_in, l_in = B, L
        if self.shape_buckets:
            B, L = self.bucket(B, L)
        long = L > 64
        if long and valid is None:
            valid = b_in * l_in
        T = None
        if valid is not None:
            need = int(valid) + (B - b_in) + 1
            Tb = (need + 63) // 64 * 64
            if long or Tb <= 0.85 * B * L:
                T = min(max(Tb, B), B * L)            # (every dialogue full: no spare row - runtime.Plan handles that)
        outputs = (int(outputs[0]), bool(outputs[1]))
        band = self.model.context                         # (read per call: M2FNet.set_context only changes which plans are handed out)
        bias = self.model.position_bias                   # (read per call, as the band)
        spk = self.model.speaker_heads                    # (likewise)
        base = self.plan_key(B, L, T, want_backward, dropout_active, self.precision, outputs, band, bias, spk)
        inst, key, pl, oldest = 0, None, None, None
        while True:                                       # first instance of this shape that no live autograd graph owns
            key = base + (inst,)
            pl = self.plans.get(key)
            if pl is None or not pl.busy():
                break
            oldest = oldest or key
            inst += 1
        if pl is None:
            if inst > 0 and not self._room_for(self.plans[oldest].nbytes()):
                # no room for another instance: hand out the least recently used one (its pending backward will raise)
                key = next(k for k in self.plans if k[:-1] == base)
                pl = self.plans[key]
        if pl is None:
            cfg = self.cfg
            if not dropout_active and cfg.dropout != 0.0:
                cfg = M2FConfig(**{**cfg.__dict__, "dropout": 0.0})
            # the C side couples "keeps a backward list" and "dropout active" in its train flag
            train = want_backward or dropout_active
            pgrads = train and outputs[1]                 # (input gradients only: the plan gets no gradient buffer at all)
            if pgrads:
                self.ensure_grad()
            self._evict(max(self.max_plans, 1) - 1, self.max_plan_bytes)
            # (outside inference mode even when the caller is inside it: the workspace and its views stay ordinary tensors, so a plan
            # first used under torch.inference_mode() - a Distiller's teacher - still serves torch.no_grad() and autograd callers)
            with torch.inference_mode(False):
                pl = runtime.Plan(cfg, B, L, self.precision, train, self.flat, self.flat_grad_ext if pgrads else None, self.rng, T=T,
                                  param_shadow=self.wshadow)
            pl._on_cast = self.mark_shadows_fresh
            if train and outputs != (0, True):
                pl.backward_outputs(*outputs)
            if band != (None, None):
                pl.attention_band(*band)                  # (once, before its first launch: a plan keeps the band of its key)
            if bias:
                pl.attention_bias(bias)                   # (likewise: a plan keeps the gain of its key)
            if spk:
                pl.attention_speakers(spk)                # (likewise)
            self.plans[key] = pl
            self._evict(max(self.max_plans, 1), self.max_plan_bytes, protect=key)
        else:
            self.plans.move_to_end(key)
            self._evict(max(self.max_plans, 1), self.max_plan_bytes, protect=key)      # (the caps may have been lowered since)
        pl.params_fresh(self.shadows_fresh())
        if pl.train and pl.param_grads:
            self._arm_grad_bf16(pl)
        return pl

    # -- gradients left as bf16 by the step (M2FNet.set_grad_bf16) -------------------------------------------------------------
    def _arm_grad_bf16(self, pl) -> None:
        want = self.grad_bf16_buf
        if pl._g16_ref is want or pl._g16_bad:
            return
        try:
            pl.grad_bf16(want)
        except runtime.HipError:
            if want is None:
                raise
            pl._g16_bad = True                               # (fp32 mode, another table form): this plan keeps fp32 gradients ...
            self.grad_bf16_buf = None                        # ... and then so does every plan: the optimizer reads ONE buffer
            for other in self.plans.values():
                if other._g16_ref is not None:
                    other.grad_bf16(None)

    def _room_for(self, nbytes: int) -> bool:
        """Could one more plan of `nbytes` be cached after evicting every idle plan?"""
        busy = [p for p in self.plans.values() if p.busy()]
        return len(busy) + 1 <= max(self.max_plans, 1) and sum(p.nbytes() for p in busy) + nbytes <= self.max_plan_bytes

    def _evict(self, keep: int, keep_bytes: Optional[int] = None, protect=None) -> None:
        """Drop least-recently-used IDLE plans until at most `keep` plans / `keep_bytes` of workspaces are left: frees their
        workspaces and captured graphs.  A plan whose activations a live autograd graph still needs is never closed."""
        def over():
            return len(self.plans) > keep or (keep_bytes is not None and self.plan_bytes() > keep_bytes and len(self.plans) > 1)
        for k in list(self.plans):
            if not over():
                break
            if k == protect or self.plans[k].busy():
                continue
            old = self.plans.pop(k)
            torch.cuda.synchronize(self.device)                        # nothing queued may still use it
            old.close()

    def plan_bytes(self) -> int:
        """HBM held by the cached plans' workspaces."""
        return sum(p.nbytes() for p in self.plans.values())

    def begin_backward(self, plan) -> None:
        """Chooses the form of the next backward of `plan`, which writes parameter gradients.  Accumulation off: the overwrite form,
        as ever.  On (M2FNet.set_grad_accumulation), torch's rule per parameter: ``.grad`` None (or a foreign tensor, which
        `publish_grads` adds to) takes this backward's gradient, the engine's view adds it.  Every ``.grad`` None: the overwrite form
        (the criterion tail's den / num start afresh too); otherwise the views of the parameters that take a fresh gradient are zeroed
        in one launch and the plan runs its accumulate form."""
        if not self.accumulate:
            if plan._acc:
                plan.accumulate_grads(False)
            return
        fresh = []
        for i, ((p, _, _, _), v) in enumerate(zip(self.items, self.grad_views)):
            g = p.grad
            if g is None or (g is not v and g.data_ptr() != v.data_ptr()):
                fresh.append(i)
        if len(fresh) == len(self.items):
            plan.accumulate_grads(False)
            return
        if fresh:
            idx = torch.cat([torch.arange(self.items[i][1], self.items[i][1] + self.items[i][2]) for i in fresh])
            self.flat_grad.index_fill_(0, idx.to(self.device), 0.0)
        plan.accumulate_grads(True)

    def publish_grads(self) -> None:
        """Expose the flat gradient buffer as ``p.grad`` views.  Gradients are OVERWRITTEN each backward
        (the reference zeroes them every step, src/train.py:227) unless accumulation is on (`begin_backward`); a foreign ``.grad``
        tensor is added to."""
        for (p, _, _, _), v in zip(self.items, self.grad_views):
            g = p.grad
            if g is None:
                p.grad = v
            elif g is not v and g.data_ptr() != v.data_ptr():
                g.add_(v)

    def owns(self) -> bool:
        base = self.flat.data_ptr()
        return all(p.data_ptr() == base + 4 * o for (p, o, _, _) in self.items)


class M2FNet(nn.Module):
    """Drop-in for reference ``src/model.py:23-145``: ``M2FNet(config.model)``; ``forward(text, audio, mask)``
    with text [B,L,d_t], audio [B,L,d_a] fp32 and mask bool [B,L] (True = pad) -> logits [B,L,output_size].

    Limits the reference does not have: at most 512 utterances per dialogue - longer inputs raise from ``m2f_plan_create``.
    Batches whose longest dialogue has more than 64 utterances always run on a packed plan (long-dialogue attention
    kernels), whatever ``packed`` says: their logits at pad slots are zero, where the reference computes numbers that its
    loss and metrics mask out (valid slots agree).  By default each backward OVERWRITES the gradients (the reference zeroes them
    every step, ``src/train.py:227``); after ``set_grad_accumulation(True)`` every backward follows torch's ``.grad`` rule and adds
    into the gradients, inside the kernels (micro-batches; ``loss_terms()`` holds the group's criterion denominator).

    ``text`` and ``audio`` are autograd inputs as in the reference: when they require grad, ``backward`` gives them (fresh tensors of
    their shape and dtype) d loss / d input computed by the gfx950 backward, so an adapter or encoder in front of the model trains.
    Padded plans match the reference at every slot, pad slots included; packed and long-dialogue plans at valid slots, with exact
    zeros at pad slots (their logits are zero there, see above).  When NO parameter requires grad (``requires_grad_(False)``:
    saliency, attribution, adversarial inputs) the backward computes the input gradients only and every ``p.grad`` is left as it
    was; a partly frozen model computes and publishes all parameter gradients as before."""

    def __init__(self, config, precision: Optional[str] = None, shape_buckets: Optional[bool] = None,
                 packed: Optional[bool] = None, context: Optional[Tuple[Optional[int], Optional[int]]] = None,
                 position_bias: Optional[float] = None, speaker_heads: Optional[Tuple[int, int]] = None):
        super().__init__()
        self.config = config
        self._context: Tuple[Optional[int], Optional[int]] = (None, None)
        self.set_context(*(context if context is not None else (None, None)))
        self._position_bias: Optional[float] = None
        self.set_position_bias(position_bias)
        # packed ("varlen") token layout for `train_step` and no-grad `forward` (runtime.Plan, m2f_plan_create_packed): a ragged
        # batch costs its valid utterances, not B x L slots; needs the batch's valid count on the host (one sync per call).
        # Off by default (M2F_PACKED=1 or packed=True): the reference's batches reach the model as padded tensors either way
        self.packed = (os.environ.get("M2F_PACKED", "0") == "1") if packed is None else bool(packed)
        # round batch shapes up to a few plan shapes (see _Engine.bucket); M2F_SHAPE_BUCKETS=0 plans every shape exactly
        self.shape_buckets = (os.environ.get("M2F_SHAPE_BUCKETS", "1") != "0") if shape_buckets is None else bool(shape_buckets)
        c = M2FConfig.from_model_config(config)           # raises the reference's two ValueErrors
        self.m2f_config = c
        self.audio_enabled, self.text_enabled, self.fam_enabled = c.audio_enabled, c.text_enabled, c.fam_enabled
        self.n_head_audio, self.n_head_text, self.n_head_fam = c.nhead_audio, c.nhead_text, c.nhead_fam
        self.dropout = nn.Dropout(c.dropout)               # kept for attribute parity; never called
        # GEMM operand precision: "fp32" (exact-fp32 MFMA, the 1e-3 parity mode) or "bf16" (bf16 MFMA, fp32 accumulate)
        self.precision = precision or os.environ.get("M2F_PRECISION", "fp32")
        if self.precision not in runtime.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(runtime.PRECISIONS)}")

        # construction order == reference (model.py:59-100) so that a given torch seed yields the same weights
        if c.audio_enabled:
            tmpl = _EncoderLayerParams(c.d_audio, c.nhead_audio, c.dim_ff)
            norm = _NormParams(c.d_audio)
            self.audio_encoders = nn.ModuleList([
                _EncoderStack(tmpl, c.d_audio, c.nhead_audio, c.dim_ff, c.nlayers_audio, norm)
                for _ in range(c.ntrans_audio)])
            self.audio_proj = _LinearParams(c.d_audio, c.d_fam)
        if c.text_enabled:
            tmpl = _EncoderLayerParams(c.d_text, c.nhead_text, c.dim_ff)
            norm = _NormParams(c.d_text)
            self.text_encoders = nn.ModuleList([
                _EncoderStack(tmpl, c.d_text, c.nhead_text, c.dim_ff, c.nlayers_text, norm)
                for _ in range(c.ntrans_text)])
            self.text_proj = _LinearParams(c.d_text, c.d_fam)
        if c.fam_enabled:
            self.fusion_layers = nn.ModuleList([
                FusionAttentionModule(embedding_size=c.d_fam, n_head=c.nhead_fam, dropout=c.dropout)
                for _ in range(c.nlayers_fam)])
        head = [_LinearParams(c.cls_in, c.cls_hidden)]
        for _ in range(max(c.cls_layers - 2, 0)):
            head.append(nn.ReLU())
            head.append(_LinearParams(c.cls_hidden, c.cls_hidden))
        head.append(nn.ReLU())
        head.append(self.dropout)
        head.append(_LinearParams(c.cls_hidden, c.cls_out))
        self.output_layer = nn.Sequential(*head)
        self._speaker_heads: Optional[Tuple[int, int]] = None
        self.set_speaker_heads(*(speaker_heads if speaker_heads is not None else (None,)))
        self._engine: Optional[_Engine] = None
        self._grad_accumulation = False
        self._last_criterion = PLAIN                       # the criterion.Criterion of the last train step (M2FNet's or a DataParallelStep's)

    # -- device plumbing -------------------------------------------------------------------------------
    def _apply(self, fn, *args, **kwargs):
        self._engine = None                                # .to()/.cuda()/.cpu() re-home the parameters
        return super()._apply(fn, *args, **kwargs)

    def engine(self, device: Optional[torch.device] = None) -> _Engine:
        if device is None:
            device = next(self.parameters()).device
        if device.type != "cuda":
            raise runtime.HipError("M2FNet runs only on an MI355X (gfx950): move the model and the batch to 'cuda' "
                                   "(there is no CPU fallback; the CPU oracle lives in oracle/ for tests only)")
        if self._engine is None or self._engine.device != device or not self._engine.owns():
            self._engine = _Engine(self, device)
            self._engine.accumulate = self._grad_accumulation
        return self._engine

    # -- context band ----------------------------------------------------------------------------------
    @property
    def context(self) -> Tuple[Optional[int], Optional[int]]:
        """(past, future): how many utterances before / after its own an utterance attends to; None = unlimited."""
        return self._context

    def set_context(self, past: Optional[int] = None, future: Optional[int] = None) -> None:
        """Context band of EVERY attention site - both modality encoders and every fusion layer - in ``forward``, ``train_step``
        and ``eval_step``, padded, packed, bucketed and long-dialogue plans alike: utterance i attends to utterances i - past ..
        i + future of its dialogue.  ``(None, 0)``: causal, the online setting (an utterance is labelled from the past only);
        ``(k, 0)``: the last k utterances and this one; ``(None, None)``, the default: the reference's offline attention, bit for bit
        what the model computed without a band.  The reference has no such setting (its modules are given no ``attn_mask``).
        Valid utterances always see themselves; pad slots under a band are not the reference's numbers (a pad slot whose band holds
        no valid utterance gets zero attention output where torch's masked softmax gives NaN) - loss and metrics mask them out, as
        they do the pad slots of packed plans.  Takes effect at the next call; each band keeps its own plans, none is rewritten."""
        runtime.context_band(past, future)                 # (raises ValueError)
        self._context = (past, future)

    # -- position bias ---------------------------------------------------------------------------------
    @property
    def position_bias(self) -> Optional[float]:
        """The APPLIED gain of the distance-decay attention bias (the requested one rounded to bf16), or None when it is off."""
        return self._position_bias

    def set_position_bias(self, gain: Optional[float] = None) -> None:
        """Distance-decay bias (ALiBi) of EVERY attention site - both modality encoders and every fusion layer: the score of query
        utterance i and visible key utterance j of head h gets ``-slope(h, H, gain) * |i - j|`` (``functional.position_bias_slopes``
        has the fixed geometric slopes), so near utterances weigh more than far ones where the reference's attention cannot tell
        them apart.  ``gain``: a finite number >= 0 - 1.0 is ALiBi - applied as rounded to bf16 (``position_bias`` reports the applied
        value); None or 0, the default: off, bit for bit what the model computed before.  One gain for the whole model, as the
        band: one unbiased site in the stack would see another geometry.  No parameters: ``state_dict``, checkpoints and optimizers
        are untouched.  Reaches ``forward``, autograd, ``train_step``, ``eval_step``, attention maps, ``Distiller`` and data-parallel
        steps through the plans; takes effect at the next call, and every gain keeps its own plans.  A ``DialogueStream`` keeps
        the gain it was created under (``DialogueStream.position_bias``) and refuses to run after a change."""
        self._position_bias = runtime.position_bias(gain) or None

    # -- speaker heads ---------------------------------------------------------------------------------
    @property
    def speaker_heads(self) -> Optional[Tuple[int, int]]:
        """(n_same, n_other), or None when the model has no speaker heads."""
        return self._speaker_heads

    def _site_heads(self) -> Dict[str, int]:
        c = self.m2f_config
        sites = {}
        if c.audio_enabled and c.ntrans_audio * c.nlayers_audio > 0:
            sites["the audio encoder (n_head_audio)"] = c.nhead_audio
        if c.text_enabled and c.ntrans_text * c.nlayers_text > 0:
            sites["the text encoder (n_head_text)"] = c.nhead_text
        if c.fam_enabled and c.nlayers_fam > 0:
            sites["the fusion layers (n_head_fam)"] = c.nhead_fam
        return sites

    def set_speaker_heads(self, n_same: Optional[int] = None, n_other: Optional[int] = None) -> None:
        """Speaker-aware heads of EVERY attention site - both modality encoders and every fusion layer: at a site with H heads, heads
        ``0 .. n_same - 1`` let query utterance i see key utterance j only if ``speakers[b, j] == speakers[b, i]`` (a speaker's own
        earlier turns: inertia; the utterance itself always qualifies), heads ``n_same .. n_same + n_other - 1`` only if the speakers
        differ (other people's turns: influence), the remaining heads are untouched.  The condition is ANDed with key padding and
        the context band, the position bias applies to what stays visible; a hidden key has probability exactly 0, a query that
        sees no key (an other-speaker head in a monologue, a first utterance under a causal band) gets a zero row where torch gives
        NaN.  At a fusion site utterance i has one speaker as text query and as audio key.  ``set_speaker_heads(None)`` (or no
        argument), the default: off, bit for bit what the model computed before.  ``n_same + n_other`` must fit the heads of every
        enabled site (ValueError naming the site).  No parameters: ``state_dict``, checkpoints and optimizers are untouched.
        With the setting on, ``forward`` / ``train_step`` / ``eval_step`` / ``attention_maps`` REQUIRE ``speakers=`` ([B, L] ids laid
        out like ``mask``: uint8 / int32 / int64, values 0 .. 255, only equality is used, pad slots ignored) and a model without it
        refuses the argument; ``Distiller`` hands the batch's speakers to whichever of student and teacher has the setting;
        ``DataParallelStep`` refuses such a model.  Takes effect at the next call, every setting keeps its own plans.  A
        ``DialogueStream`` keeps the setting it was created under and refuses to run after a change until ``reset()``."""
        if n_same is None and n_other is None:
            self._speaker_heads = None
            return
        self._speaker_heads = runtime.speaker_heads((n_same, 0 if n_other is None else n_other), self._site_heads())

    # -- reference surface -----------------------------------------------------------------------------
    def forward(self, text, audio, mask, speakers=None):
        ids = _check_speakers("M2FNet.forward", self._speaker_heads, speakers, mask.shape)
        eng = self.engine(mask.device)
        B, L = mask.shape
        grad_on = torch.is_grad_enabled()
        want_params = grad_on and any(p.requires_grad for p, *_ in eng.items)
        in_mask = 0
        if grad_on:
            if self.text_enabled and isinstance(text, torch.Tensor) and text.requires_grad:
                in_mask |= runtime.IN_TEXT
            if self.audio_enabled and isinstance(audio, torch.Tensor) and audio.requires_grad:
                in_mask |= runtime.IN_AUDIO
        want_bwd = want_params or in_mask != 0
        valid = int((~mask.bool()).sum()) if (self.packed or L > 64) else None
        outputs = (in_mask, want_params) if in_mask else (0, True)          # (no input gradient wanted: today's plans, keys and all)
        plan = eng.plan(B, L, want_bwd, self.training and self.m2f_config.dropout > 0.0, valid, outputs)
        # (detached: the staging copies are plumbing, autograd reaches the inputs through _Anchor)
        det = lambda x: x.detach() if isinstance(x, torch.Tensor) else x          # noqa: E731
        plan.set_inputs(det(text) if self.text_enabled else None, det(audio) if self.audio_enabled else None, mask, speakers=ids)
        if plan.train:
            plan.supcon(False)                     # (the criterion is the caller's here: nothing joins the backward at the hidden features)
            plan.set_aux(None)
        if want_bwd:
            out = _Anchor.apply(eng.anchor, text, audio, self, plan)
            plan.hold(out.grad_fn)
            eng.note_forward(plan)
            return out
        if plan.train and plan.cfg.dropout > 0.0:
            runtime.check(runtime.lib().m2f_rng_advance(eng.rng.data_ptr(), runtime.stream_ptr()), "m2f_rng_advance")
        out = plan.forward().clone()
        eng.note_forward(plan)
        return out

    # -- attention maps (what need_weights=True returns; csrc/attention_weights.hip) ---------------------------------------------------
    def last_attention(self, average_heads: bool = True, sites=None) -> Dict[str, torch.Tensor]:
        """The attention maps of the most recent ``forward`` / ``train_step`` / ``eval_step`` of this model: ``{site: tensor}``, the
        sites named by the ``state_dict`` prefixes of their parameters (``layout.attention_sites``: ``audio_encoders.{e}.layers.{l}.
        self_attn``, ``text_encoders.{e}.layers.{l}.self_attn``, ``fusion_layers.{i}.multihead_attention``), each ``[B, L, L]`` -
        ``weights[b, i, j]`` = how much utterance i of dialogue b attends to utterance j, the heads averaged as torch's
        ``need_weights=True`` does (fp32 sum over the heads in order, times fp32(1 / H)) - or ``[B, H, L, L]`` with
        ``average_heads=False``.  After ``train_step(rdrop=)``, which runs every dialogue twice, B is twice the batch: the maps of view 0,
        then those of view 1.  These are the weights that the reference's fusion module computes at every layer and throws away
        (src/model.py:14).  sites: names to return (default: all).

        No second forward: every attention site saves its probabilities at every forward, and one eager gather launch turns them
        into fresh tensors in the caller's dialogue order and ``L``, whatever bucket or packed layout ran; no logit changes by a bit.
        Padded keys, pairs a context band hides and (packed and long-dialogue plans) the rows and columns of pad slots are exactly 0;
        a row that sees no key is zeros where torch gives NaN.  In train mode with dropout > 0 the maps are the PRE-dropout
        probabilities (rows sum to 1); torch returns post-dropout weights there.
        Raises RuntimeError when no forward has run, or the plan that ran it was destroyed or has run again since (another model
        instance cannot, a plan driven by hand can)."""
        eng = self._engine
        if eng is None or eng.last is None:
            raise RuntimeError("M2FNet.last_attention: no forward has run on this model (or it was moved since)")
        plan, version, dst, valid, shape = eng.last
        if not plan.handle:
            raise RuntimeError("M2FNet.last_attention: the plan holding the probabilities of the last forward was destroyed "
                               "(evicted from the plan cache)")
        if plan.version != version:
            raise RuntimeError("M2FNet.last_attention: the probabilities of the last forward were overwritten by a later forward "
                               "of the same plan")
        names = [n for (n, _, _) in plan.attention_sites()]
        want = names if sites is None else list(sites)
        unknown = [n for n in want if n not in names]
        if unknown:
            raise ValueError(f"M2FNet.last_attention: unknown attention site(s) {unknown}; this model has {names}")
        maps = plan.attention_maps([names.index(n) for n in want], not average_heads, dst, valid, shape)
        return dict(zip(want, maps))

    def attention_maps(self, text, audio, mask, average_heads: bool = True, sites=None, speakers=None):
        """``(logits, maps)``: a no-grad ``forward`` in the model's current mode, then ``last_attention(average_heads, sites)``.
        speakers: as ``forward`` (a model with speaker heads; pairs its heads hide are exactly 0 in the maps)."""
        with torch.no_grad():
            logits = self(text, audio, mask, speakers=speakers) if speakers is not None else self(text, audio, mask)
        return logits, self.last_attention(average_heads, sites)

    # -- fused fast path (forward + criterion + backward as one launch list / hipGraph) ---------------
    def train_step(self, text, audio, mask, emotion, label_smoothing: float = 0.1,
                   class_weights: Optional[torch.Tensor] = None, normalise: bool = True,
                   use_graph: bool = True, optimizer=None, teacher_logits: Optional[torch.Tensor] = None,
                   distill: Optional[Tuple[float, float]] = None, speakers: Optional[torch.Tensor] = None,
                   focal_gamma: Optional[float] = None, crf=None, rdrop: Optional[float] = None,
                   supcon: Optional[Tuple[float, float]] = None, aux=None, aux_label_smoothing: float = 0.0,
                   input_grads=None) -> torch.Tensor:
        """Body of reference src/train.py:227-230 in one call: returns the (device) loss scalar and leaves
        the gradients in ``p.grad`` (views of the flat buffer).
        teacher_logits (fp32 [B, L, cls_out] on the model's device) with distill=(alpha, temperature): the step's criterion is the
        distillation criterion (distill.py) - ``(1 - alpha) * cross entropy + alpha * temperature^2 * KL(softmax(teacher / temperature) ||
        softmax(logits / temperature))`` over the labelled utterances, one kernel in the criterion's place, the same ``loss_terms()``
        tail; both or neither, anything invalid is a ValueError before any launch.  The pair lives on the device (uploaded only when it
        changed): a schedule of alpha replays the captured step.  Distilled and plain calls mix freely on one model.
        optimizer (a ``FusedAdam`` of this model): the call is ALSO ``optimizer.step()`` (src/train.py:231) - in bf16 mode the
        weight-gradient launch applies the update itself (``FusedAdam.prepare_fused``; the matrices' ``.grad`` is then not written),
        otherwise the optimizer's own kernel runs behind the step.
        speakers ([B, L] ids): required by a model with speaker heads (``set_speaker_heads``), refused by one without; an input like
        the mask - a captured step replays while the ids change.
        focal_gamma (a finite number in [0, 8]): the step's criterion is the focal form (Lin et al. 2017) - every labelled utterance's
        hard-label term scaled by ``(1 - p_y)^gamma``, one kernel in the criterion's place, the same ``loss_terms()`` tail; with
        ``teacher_logits`` / ``distill`` the factor scales the hard-label term only.  gamma lives on the device (uploaded only when it
        changed): a schedule of gamma replays the captured step.  None (default): the criterion without it, bit for bit; focal and plain
        calls mix freely on one model.  Anything else is a ValueError before any launch.
        crf (a ``crf.LinearChainCRF`` of cls_out classes on the model's device): the step's criterion is the linear-chain CRF over each
        dialogue's labelled utterances (token_mean), one kernel in the criterion's place and the same tail - the step stays one
        replayed graph.  Its parameter block is an input of the step, never part of this model's parameters; trainable,
        ``crf.params.grad`` is a view of a gradient buffer this step overwrites, and any torch optimizer over ``crf.parameters()``
        trains it beside ``FusedAdam`` (the values are read on the device: the captured step replays while they change).  Refused
        (ValueError naming the pair) with class_weights, teacher_logits / distill, focal_gamma, label_smoothing != 0.0, and - trainable
        only - under gradient accumulation; a frozen block (``crf.params.requires_grad_(False)``) works under every training mode.
        rdrop (alpha, a finite number >= 0): the R-Drop criterion (Liang et al. 2021).  The B dialogues run TWICE in one ordinary plan of
        2B dialogues - view 0 and behind it view 1, the same inputs, mask, labels and speaker ids (copied device to device; buckets,
        packed plans and long dialogues as ever) -, the hashed dropout streams give the two views independent masks at every site, and
        one kernel in the criterion's place adds ``alpha * w_y * 0.5 * (KL(p || q) + KL(q || p))`` between each labelled utterance's two
        predictions to the cross entropy of both views, over the one denominator (the labelled weight of both views) and the same
        ``loss_terms()`` tail: ``0.5 * (CE(view 0) + CE(view 1)) + alpha * 0.5 * (kl_div(v0, v1) + kl_div(v1, v0))``, batchmean over the
        labelled utterances.  ``rdrop_terms()`` gives the two shares.  alpha lives on the device (uploaded only when it changed): a
        warm-up replays the captured step.  With dropout 0 or in eval mode the call is allowed: the twins then agree, the term and its
        gradient are exactly zero.  None (default): today's launches, bit for bit; R-Drop and plain calls mix freely on one model.
        Refused (ValueError naming the pair, before any launch) beside teacher_logits / distill, focal_gamma or crf.  After such a
        step ``last_attention()`` returns the 2B dialogues' maps, view 0 first.
        supcon (weight, temperature; weight finite and >= 0, temperature finite and > 0): the supervised contrastive criterion (Khosla et
        al. 2020) on the classifier's last hidden activation ``h`` - post-ReLU, and post-dropout in train mode: what the final Linear
        reads, ``last_features()``.  Over V = the labelled utterances of ALL dialogues of the batch with ``||h|| > 0``, ``z = h / ||h||``:
        ``l_i = logsumexp_{a in V, a != i} (z_i . z_a / temperature) - mean_{p: y_p = y_i, p != i} (z_i . z_p / temperature)`` (0 for an
        utterance without a positive), and ``weight * w_y * l_i`` joins the utterance's numerator over the one denominator:
        ``loss = CE + weight * sum(w l) / sum(w)``.  Exact-fp32 kernels in both precision modes; the gradient enters the backward at the
        hidden activation's gradient.  ``supcon_terms()`` gives the two shares.  The pair lives on the device (uploaded only when it
        changed): a weight schedule replays the captured step; weight 0 gives the plain step's loss and gradients.  None (default):
        today's launches, bit for bit; contrastive and plain calls mix freely on one model.  Under gradient accumulation each
        micro-batch contrasts within itself.  Refused (ValueError naming the pair, before any launch) beside teacher_logits / distill,
        focal_gamma, crf or rdrop.
        aux (head, aux_labels, weight): an ``aux_head.AuxiliaryHead`` over ``cls_hidden``, a second label per utterance (int64
        ``[B, L]``, laid out like ``emotion``; a value outside the head's classes = ignored) and a weight (finite, >= 0).  For every
        utterance with an emotion label AND an auxiliary label, ``weight * w_y * a`` joins the numerator over the one denominator, ``a``
        the cross entropy (``aux_label_smoothing``, no class weights of its own) of ``head(h)`` against the auxiliary label, ``h`` =
        ``last_features()``: with no class weights and every row labelled twice the loss is ``CE(z, y) + weight * CE(head(h), s)``.
        Exact-fp32 kernels in both precision modes inside the one step graph; the gradient enters the backward at the hidden
        activation's gradient, and a trainable head's own gradient lands in ``head.params.grad`` (overwritten by every step; step it with
        an optimizer of your own, as a CRF's block).  ``aux_terms()`` gives the two shares, ``last_aux_logits()`` the head's logits.
        The weight and the smoothing live on the device (uploaded only when changed): a weight schedule replays the captured step;
        weight 0 gives the plain step's loss and gradients.  None (default): today's launches, bit for bit; auxiliary and plain calls
        mix freely on one model.  Combines with focal_gamma (the focal factor scales the emotion term only); refused (ValueError naming
        the pair, before any launch) beside teacher_logits / distill, crf, rdrop or supcon, and - a trainable head - under gradient
        accumulation.
        input_grads ("text", "audio" or both, enabled modalities only): the step ALSO leaves d loss / d text and / or d loss / d audio
        - one more dgrad launch inside the same replayed graph, on a plan of its own (key ``outputs=(mask, True)``; the parameter
        gradients keep their bits) - and ``last_input_grads()`` returns them as fresh ``[B, L, d]`` tensors.  With ``normalise=False``
        they are the gradients of the un-normalised numerator, as the parameter gradients are.  None (default): today's plan key,
        launches and bits.  Refused by name beside optimizer= (the in-launch optimizer), bf16 gradients (``set_grad_bf16``) and rdrop."""
        in_mask = 0
        if input_grads is not None:
            in_mask = runtime.input_modalities(input_grads, self.text_enabled, self.audio_enabled, "M2FNet.train_step")
            if optimizer is not None:
                raise RuntimeError("M2FNet.train_step: input_grads= does not combine with optimizer= (the optimizer step inside the train "
                                   "step: its fused setup belongs to the plan without input gradients); call optimizer.step() yourself")
            if rdrop is not None:
                raise ValueError("M2FNet.train_step: input_grads= does not combine with rdrop (the step runs every dialogue twice: "
                                 "there is no one gradient per input row)")
            if self._engine is not None and self._engine.grad_bf16_buf is not None:
                raise RuntimeError("M2FNet.train_step: input_grads= does not combine with bf16 gradients (set_grad_bf16(True)): the "
                                   "plan that also computes input gradients keeps fp32 gradients; call set_grad_bf16(False) first")
        spec = self._resolve("M2FNet.train_step", mask, label_smoothing, class_weights, teacher_logits=teacher_logits, distill=distill,
                             focal_gamma=focal_gamma, crf=crf, rdrop=rdrop, supcon=supcon, aux=aux, aux_label_smoothing=aux_label_smoothing)
        ids = _check_speakers("M2FNet.train_step", self._speaker_heads, speakers, mask.shape)
        if optimizer is not None and getattr(optimizer, "sam_rho", None) is not None:
            raise RuntimeError("M2FNet.train_step: optimizer= (the optimizer step inside the train step) does not combine with "
                               "sharpness-aware minimisation (optimizer.sam_rho): the in-launch optimizer cannot wait for the second "
                               "pass; call M2FNet.sam_step(..., optimizer), or set sam_rho = None")
        eng = self.engine(mask.device)
        if optimizer is not None and eng.accumulate:
            raise RuntimeError("M2FNet.train_step: optimizer= (the optimizer step inside the train step) does not combine with "
                               "gradient accumulation (set_grad_accumulation(True)); call optimizer.step() after the group's micro-batches")
        if spec.rdrop is not None:                       # view 0, then view 1: the ordinary plan of 2B dialogues
            text, audio, mask, emotion, ids = (None if x is None else torch.cat([x, x], 0) for x in (text, audio, mask, emotion, ids))
        B, L = mask.shape
        valid = int((~mask.bool()).sum()) if (self.packed or L > 64) else None
        if in_mask and eng.grad_bf16_buf is not None:
            raise RuntimeError("M2FNet.train_step: input_grads= does not combine with bf16 gradients (set_grad_bf16(True)): the plan "
                               "that also computes input gradients keeps fp32 gradients; call set_grad_bf16(False) first")
        plan = (eng.plan(B, L, True, self.training and self.m2f_config.dropout > 0.0, valid, (in_mask, True)) if in_mask
                else eng.plan(B, L, True, self.training and self.m2f_config.dropout > 0.0, valid))
        self._last_criterion = spec

        def body():
            plan.set_inputs(text if self.text_enabled else None, audio if self.audio_enabled else None, mask, emotion, speakers=ids)
            if class_weights is not None:
                plan.class_w[: class_weights.numel()].copy_(class_weights)
            plan.set_criterion(spec)
            if optimizer is None:
                eng.begin_backward(plan)
                return plan.step(label_smoothing, class_weights is not None, normalise, use_graph)
            eng.begin_backward(plan)                     # (accumulation is refused above: the overwrite form)
            plan.params_fresh(eng.shadows_fresh())
            if optimizer.prepare_fused(plan):
                out = plan.step(label_smoothing, class_weights is not None, normalise, use_graph)
                optimizer.finish_fused(plan)
                return out
            out = plan.step(label_smoothing, class_weights is not None, normalise, use_graph)
            eng.publish_grads()
            optimizer.step()
            return out

        if use_graph:                                    # capture / replay on the engine's own stream
            cur = torch.cuda.current_stream(eng.device)
            eng.stream.wait_stream(cur)
            with torch.cuda.stream(eng.stream):
                loss = body()
            cur.wait_stream(eng.stream)
        else:
            loss = body()
        eng.publish_grads()
        for block in (spec.crf, spec.aux and spec.aux[0]):
            if block is not None:
                block.publish_grad()
        eng.note_forward(plan)
        if in_mask:
            eng.last_inputs = eng.last + (in_mask,)
        return loss[0].clone()          # (the buffer is overwritten by the next step)

    def _last_rows(self, who: str, what: str, record):
        """(plan, dst, valid, shape, mask) of `record` (an engine's last_inputs / last_adv), or the RuntimeError that says why not."""
        if record is None:
            raise RuntimeError(f"M2FNet.{who}: no {what} has run on this model (or it was moved since)")
        plan, version, dst, valid, shape, mask = record
        if not plan.handle:
            raise RuntimeError(f"M2FNet.{who}: the plan of the last {what} was destroyed (evicted from the plan cache)")
        if plan.version != version:
            raise RuntimeError(f"M2FNet.{who}: the buffers of the last {what} were overwritten by a later step of the same plan")
        return plan, dst, valid, shape, mask

    def last_input_grads(self) -> Dict[str, torch.Tensor]:
        """``{"text": d loss / d text, "audio": d loss / d audio}`` (the modalities asked for) of the most recent
        ``train_step(input_grads=)`` of this model: fresh ``[B, L, d]`` tensors in the caller's dialogue order, whatever bucket, packed or
        long-dialogue plan ran; pad slots are exact zeros.  Raises RuntimeError when no such step has run, or the plan that ran it was
        destroyed or has run again since."""
        eng = self._engine
        plan, dst, valid, shape, mask = self._last_rows("last_input_grads", "train_step(input_grads=)", eng.last_inputs if eng else None)
        out = {}
        for name, bit in (("text", runtime.IN_TEXT), ("audio", runtime.IN_AUDIO)):
            if mask & bit:
                g = plan.input_grad(bit, dst, valid, shape)
                if not plan.packed:                          # (a padded plan computes numbers at pad slots, as the reference does)
                    g = g.masked_fill(plan.keypad_in.view(plan.B, plan.L)[: shape[0], : shape[1]].bool()[..., None], 0.0)
                out[name] = g
        return out

    def last_perturbation(self) -> Dict[str, torch.Tensor]:
        """``{modality: delta}`` of the most recent ``adversarial_step`` of this model: the final perturbation of every perturbed
        modality as a fresh ``[B, L, d]`` tensor in the caller's dialogue order; pad slots are exact zeros.  Raises as
        ``last_input_grads``."""
        eng = self._engine
        plan, dst, valid, shape, mask = self._last_rows("last_perturbation", "adversarial_step", eng.last_adv if eng else None)
        return {name: plan.perturbation(bit, dst, valid, shape)
                for name, bit in (("text", runtime.IN_TEXT), ("audio", runtime.IN_AUDIO)) if mask & bit}

    def adversarial_step(self, text, audio, mask, emotion, optimizer=None, *, epsilon, steps: int = 2, step_size: Optional[float] = None,
                         norm: str = "utterance", modalities=None, init_mag: float = 0.0, same_dropout: bool = True,
                         **train_step_arguments) -> torch.Tensor:
        """Embedding-space adversarial training in one call (FGM, Miyato et al. 2017; PGD, Madry et al. 2018; FreeLB, Zhu et al. 2020):
        ``steps`` = K >= 1 passes of the train step on ONE plan, each on ``x_clean + delta`` of the perturbed modalities, nothing
        waiting for the host.  The batch is staged once; pass 0 overwrites the gradients; before every later pass one row-wise launch
        per modality (csrc/adversarial.hip) takes the input gradients the pass before left - ``delta <- project(delta + step_size * g /
        ||g||)`` onto the ``epsilon`` ball, ``||.||`` per utterance row (``norm="utterance"``) or over all valid rows of the modality
        (``"batch"``), rows that are padding untouched - and the pass ADDS its gradients (the accumulate form): the call leaves exactly
        what this loop over the public pieces leaves::

            model.set_grad_accumulation(True); optimizer.zero_grad()
            for k in range(K):                      # delta_0 = 0; delta_k from last_input_grads() through functional.adversarial_ascend
                model.train_step(text + delta_t, audio + delta_a, mask, emotion, normalise=False, input_grads=...)

        ``.grad`` is the fp32 sum of the K un-normalised gradients and ``loss_terms()[1:]`` the summed den / num.  Returns the loss of
        pass 0 (the clean loss when ``init_mag = 0``).  ``steps=2, step_size=epsilon`` (the default) is FGM with the clean loss kept,
        ``steps=K`` PGD / FreeLB (K passes, averaged gradient).  step_size None = epsilon.
        optimizer (a ``FusedAdam`` of this model without sam_rho): the call also sets ``optimizer.grad_scale`` to the group's den, runs
        ``optimizer.step()`` - clipping, EMA, the watch, parameter groups and AdamW see the summed gradient, as after any accumulation
        group - and puts the previous ``grad_scale`` back.
        modalities: a subset of ("text", "audio") to perturb (None: every enabled one).  init_mag > 0: delta starts uniform in
        ``+- init_mag / sqrt(d)`` per element (the device's hash under a site of its own; tests/golden/adversarial_ref.py is the host
        replica), projected, instead of at zero.  same_dropout (FreeLB's rule): every pass draws the masks of pass 0; False: fresh masks
        per pass.  Either way the dropout state afterwards is the one a single step leaves.
        ``train_step_arguments``: label_smoothing, class_weights, use_graph, speakers and the criterion arguments of ``train_step``;
        a frozen CRF or auxiliary head works, a trainable one is refused as under accumulation.  (epsilon, step_size) live on the device
        (uploaded only when changed): a schedule replays the captured graphs - after the second call on a shape every pass does.
        Refused by name, before any launch: bf16 gradients (``set_grad_bf16``), the caller's own ``set_grad_accumulation(True)``, a SAM
        optimizer, rdrop, ``DataParallelStep`` / more than one process, ``steps < 1``, a non-finite or negative epsilon / step_size /
        init_mag, an unknown norm, a disabled modality.  ``last_perturbation()`` returns the final delta."""
        who = "M2FNet.adversarial_step"
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
            raise ValueError(f"{who}: steps must be an integer >= 1, got {steps!r}")
        eps, step, mag = runtime.check_adv_hyper(epsilon, step_size, init_mag, who)
        kind = runtime.adv_norm_kind(norm, who)
        adv_mask = runtime.input_modalities(modalities, self.text_enabled, self.audio_enabled, who, "modalities")
        for name in ("normalise", "input_grads"):
            if name in train_step_arguments:
                raise TypeError(f"{who}: {name}= is not an argument of the passes (the call normalises nothing and asks for the input "
                                "gradients itself)")
        if train_step_arguments.get("rdrop") is not None:
            raise ValueError(f"{who}: rdrop does not combine with adversarial_step (the R-Drop step runs every dialogue twice: there is "
                             "no one perturbation per input row)")
        if type(optimizer).__name__ == "DataParallelStep" or (torch.distributed.is_available() and torch.distributed.is_initialized()
                                                              and torch.distributed.get_world_size() > 1):
            raise RuntimeError(f"{who}: DataParallelStep / more than one process is not supported (the passes accumulate on one device "
                               "and the perturbation's norm is this rank's)")
        if optimizer is not None and getattr(optimizer, "sam_rho", None) is not None:
            raise RuntimeError(f"{who}: a SAM optimizer (optimizer.sam_rho) does not combine with adversarial_step: both re-run the "
                               "batch, one moving the weights, one the inputs; set sam_rho = None")
        if self._grad_accumulation:
            raise RuntimeError(f"{who}: gradient accumulation is on (set_grad_accumulation(True)): the K passes are an accumulation group "
                               "of their own; call set_grad_accumulation(False) first")
        if self._engine is not None and self._engine.grad_bf16_buf is not None:
            raise RuntimeError(f"{who}: bf16 gradients are on (set_grad_bf16(True)); the passes accumulate fp32 gradients - call "
                               "set_grad_bf16(False) first")
        label_smoothing = train_step_arguments.pop("label_smoothing", 0.1)
        class_weights = train_step_arguments.pop("class_weights", None)
        use_graph = train_step_arguments.pop("use_graph", True)
        speakers = train_step_arguments.pop("speakers", None)
        spec = self._resolve(who, mask, label_smoothing, class_weights, accumulating=steps > 1, **train_step_arguments)
        ids = _check_speakers(who, self._speaker_heads, speakers, mask.shape)
        eng = self.engine(mask.device)
        if eng.grad_bf16_buf is not None:
            raise RuntimeError(f"{who}: bf16 gradients are on (set_grad_bf16(True)); the passes accumulate fp32 gradients - call "
                               "set_grad_bf16(False) first")
        B, L = mask.shape
        valid = int((~mask.bool()).sum()) if (self.packed or L > 64) else None
        dropout_on = self.training and self.m2f_config.dropout > 0.0
        plan = eng.plan(B, L, True, dropout_on, valid, (adv_mask, True))
        self._last_criterion = spec
        cw = class_weights is not None

        def body():
            plan.set_inputs(text if self.text_enabled else None, audio if self.audio_enabled else None, mask, emotion, speakers=ids)
            if cw:
                plan.class_w[: class_weights.numel()].copy_(class_weights)
            plan.set_criterion(spec)
            plan.adversarial(adv_mask)                        # (the mask is part of the plan's key: allocated once per plan)
            plan.adv_begin(eps, step, mag, kind)
            saved = eng.rng.clone() if dropout_on else None   # (16 bytes, device to device)
            after0 = None
            first = None
            for k in range(steps):
                if k:
                    plan.adv_ascend(kind)
                    if dropout_on and same_dropout:
                        eng.rng.copy_(saved)                  # the masks of pass 0 again
                plan.accumulate_grads(k > 0)
                out = plan.step(label_smoothing, cw, False, use_graph)
                if k == 0:
                    first = out[0].clone()
                    after0 = eng.rng.clone() if dropout_on else None
            plan.accumulate_grads(False)
            if dropout_on:
                eng.rng.copy_(after0)                         # the state a single step leaves
            return first

        if use_graph:                                    # capture / replay on the engine's own stream
            cur = torch.cuda.current_stream(eng.device)
            eng.stream.wait_stream(cur)
            with torch.cuda.stream(eng.stream):
                loss = body()
            cur.wait_stream(eng.stream)
        else:
            loss = body()
        eng.publish_grads()
        for block in (spec.crf, spec.aux and spec.aux[0]):
            if block is not None:
                block.publish_grad()
        eng.note_forward(plan)
        eng.last_adv = eng.last + (adv_mask,)
        eng.last_inputs = eng.last + (adv_mask,)
        if optimizer is not None:
            held = optimizer.grad_scale
            optimizer.grad_scale = self.loss_terms()[1:2]
            try:
                optimizer.step()
            finally:
                optimizer.grad_scale = held
        return loss

    def sam_step(self, text, audio, mask, emotion, optimizer, **train_step_arguments) -> torch.Tensor:
        """One optimizer step of sharpness-aware minimisation (Foret et al., ICLR 2021; ``FusedAdam(sam_rho=...)``): ``train_step``
        at ``w``, ``optimizer.first_step()`` (``w <- w + e``), ``train_step`` on the same batch at ``w + e``, ``optimizer.step()``
        (``w`` restored to its bits, then the update with the second gradient).  Returns the FIRST pass's loss, the loss at ``w``.
        ``train_step_arguments``: every keyword of ``train_step`` but ``optimizer`` - criterion arguments, ``speakers=``,
        ``class_weights``, ``use_graph`` - handed to both passes unchanged.  Both passes run the one plan of the batch's shape and
        replay its one captured graph; with dropout on, the second pass draws fresh masks, as every torch implementation of SAM does.
        Nothing waits for the host.  Under gradient accumulation the two passes are two sweeps over the group's micro-batches: make
        the calls by hand (``FusedAdam``'s docstring has the loop)."""
        if getattr(optimizer, "sam_rho", None) is None:
            raise RuntimeError("M2FNet.sam_step: optimizer.sam_rho is None; construct the optimizer with sam_rho= (or set the attribute)")
        if getattr(optimizer, "sam_pending", False):
            raise RuntimeError("M2FNet.sam_step: a perturbation is already pending on the optimizer; call step() or restore() first")
        if self._grad_accumulation:
            raise RuntimeError("M2FNet.sam_step: under gradient accumulation (set_grad_accumulation(True)) the two passes are two sweeps "
                               "over the group's micro-batches; make the calls by hand (see FusedAdam's docstring)")
        loss = self.train_step(text, audio, mask, emotion, **train_step_arguments)
        optimizer.first_step()
        self.train_step(text, audio, mask, emotion, **train_step_arguments)
        optimizer.step()
        return loss

    def _resolve(self, who: str, mask, label_smoothing, class_weights, accumulating: Optional[bool] = None, **criterion_args):
        """``criterion.resolve`` for a step of this model on `mask`'s batch (`who` names the entry point in the refusals).
        accumulating: None = whether gradient accumulation is on; True: the step accumulates by itself (adversarial_step)."""
        c = self.m2f_config
        if accumulating is None:
            accumulating = self._engine is not None and self._engine.accumulate
        return resolve(who, num_classes=c.cls_out, cls_hidden=c.cls_hidden, mask_shape=mask.shape, device=mask.device,
                       label_smoothing=label_smoothing, class_weights=class_weights, accumulating=bool(accumulating), **criterion_args)

    # -- evaluation fast path (forward + scoring as one launch list / hipGraph) -----------------------
    def eval_step(self, text, audio, mask, emotion, scores, class_weights: Optional[torch.Tensor] = None,
                  label_smoothing: float = 0.1, use_graph: bool = True, speakers: Optional[torch.Tensor] = None,
                  focal_gamma: Optional[float] = None, crf=None) -> None:
        """Loop body of the reference's ``validate`` / ``test`` (src/train.py:252-272, src/test.py:55-74) in one call: the forward of
        a no-grad ``forward`` (same plan: buckets, packed plans, long dialogues), then the batch's criterion loss, accuracy, weighted
        F1 and confusion matrix ADDED to ``scores`` (a ``metrics.DeviceScores``), all on the device.  Returns nothing and waits for
        nothing: ``scores.last()`` is a device view of the batch's three numbers, ``scores.result()`` / ``mean_loss()`` read the pass.
        The plan's own token rows are scored - pad and filler rows carry label -1.  speakers: as ``train_step``.
        focal_gamma: as ``train_step`` - the loss is the focal criterion's (the bits its train kernel gives for the same rows), so
        validation and early stopping see the criterion that trains; accuracy, F1 and the confusion matrix do not depend on it.
        crf (a ``crf.LinearChainCRF``): the loss is the CRF loss over the labelled rows (the train kernel's bits), and predictions,
        accuracy, F1 and the confusion matrix come from the Viterbi path over each dialogue's utterances instead of the per-row argmax.
        The same refusals as ``train_step``."""
        spec = self._resolve("M2FNet.eval_step", mask, label_smoothing, class_weights, evaluating=True, focal_gamma=focal_gamma, crf=crf)
        ids = _check_speakers("M2FNet.eval_step", self._speaker_heads, speakers, mask.shape)
        if self.training and self.m2f_config.dropout > 0.0:
            raise RuntimeError("M2FNet.eval_step: the model is in training mode with dropout > 0; evaluation scores the model "
                               "without dropout - call model.eval() first")
        eng = self.engine(mask.device)
        if scores.n_classes != self.m2f_config.cls_out or scores.record.device != eng.device:
            raise ValueError(f"M2FNet.eval_step: scores must be a DeviceScores({self.m2f_config.cls_out}, {eng.device})")
        B, L = mask.shape
        valid = int((~mask.bool()).sum()) if (self.packed or L > 64) else None
        plan = eng.plan(B, L, False, False, valid)

        def body():
            plan.set_inputs(text if self.text_enabled else None, audio if self.audio_enabled else None, mask, emotion, speakers=ids)
            if class_weights is not None:
                plan.class_w[: class_weights.numel()].copy_(class_weights)
            plan.set_criterion(spec)
            plan.eval_step(scores.record, label_smoothing, class_weights is not None, use_graph)

        if use_graph:                                    # capture / replay on the engine's own stream
            cur = torch.cuda.current_stream(eng.device)
            eng.stream.wait_stream(cur)
            with torch.cuda.stream(eng.stream):
                body()
            cur.wait_stream(eng.stream)
        else:
            body()
        eng.note_forward(plan)

    # -- streaming inference (one new utterance per live dialogue; streaming.DialogueStream) -----------------------------------------
    def stream(self, max_streams: int, capacity: Optional[int] = None, use_graph: bool = True, max_chunk: int = 1,
               pages: Optional[int] = None, page_rows: int = 16, attention: bool = False, crf=None):
        """A ``DialogueStream`` of ``max_streams`` slots over this model's weights: ``stream.step(text [S, d_t], audio [S, d_a],
        active)`` labels the utterance that has just arrived in each active slot from per-site K / V caches on the device, at the
        cost of one row per dialogue - where ``forward`` would re-run the whole prefix.  Needs a causal context band
        (``context=(past, 0)``: a band that looks ahead cannot stream) and eval mode (or dropout = 0).
        capacity: cache rows per slot and site, 1 .. 512; default ``past + 1`` for a window (a ring: no length limit; a smaller value is
        raised to it) and 512 for ``past=None`` (the most utterances a slot can then hold).  The caches cost
        ``2 * sum_sites pad(d_site) * max_streams * capacity * 4 B`` (bf16 mode: 2 B per element): 3.8 GB at C3, 64 streams, capacity 512.
        They belong to the weights that wrote them - after ``load_state_dict``, an optimizer step or ``averaged_parameters()`` call
        ``stream.reset()``.
        max_chunk: 1 (default: nothing beyond the step plan is created), or T in 2 .. 64 - the stream also gets a chunk plan and
        ``stream.prefill(text [S, n, d_t], audio [S, n, d_a], counts)`` loads a history T utterances per slot and call (one forward over
        S * T rows each) instead of one launch-bound step per utterance; ``stream.run`` then feeds collate-layout batches T columns at a
        time.
        pages: None (default: the dense caches above), or N >= 1 - PAGED caches: every site holds pools of N pages of ``page_rows`` (16,
        32 or 64) rows, ``2 * sum_sites pad(d_site) * N * page_rows`` elements, and a slot takes pages as its dialogue grows and
        returns them at ``reset`` (``streaming.PageAllocator``).  Memory follows the utterances cached, not ``max_streams * capacity``:
        the 3.8 GB above hold 2,048 pages of 16 rows, about 2,000 live MELD-length dialogues.  Same logits, bit for bit; a call that
        would need more pages than are free raises RuntimeError and changes nothing.
        crf (a ``crf.LinearChainCRF`` of cls_out classes on the model's device): the stream also runs the CRF's forward filter inside
        every step / prefill graph, behind the classifier - ``stream.crf_posterior()`` returns log P(label of each slot's last utterance
        | its dialogue so far); the logits are unchanged; C floats per slot, so it works under any window; snapshots carry the state.
        attention: True - every step also keeps, per attention site, slot and head, the row of attention probabilities of the new
        utterance over the cached ones, and ``stream.attention(average_heads=True, sites=None)`` returns them after a ``step`` (which
        cached utterances did this prediction use); ``sum_sites H * max_streams * capacity * 4 B`` more memory (17.8 MB at C3, 64
        streams, capacity 512), the same logits bit for bit, the step still one replayed graph.
        Every refusal is raised before the GPU is touched."""
        from .streaming import DialogueStream, resolve_capacity, resolve_max_chunk, resolve_pages
        past, future = self._context
        if future != 0:
            raise ValueError(f"M2FNet.stream: streaming needs a causal context band (past, 0), this model has context={self._context}; "
                             "a band that looks ahead cannot label an utterance when it arrives (M2FNet(config, context=(past, 0)))")
        if self.training and self.m2f_config.dropout > 0.0:
            raise RuntimeError("M2FNet.stream: the model is in training mode with dropout > 0; a stream scores the model "
                               "without dropout - call model.eval() first")
        if isinstance(max_streams, bool) or not isinstance(max_streams, int) or max_streams < 1:
            raise ValueError(f"M2FNet.stream: max_streams must be an integer >= 1, got {max_streams!r}")
        pages, page_rows = resolve_pages(pages, page_rows)
        return DialogueStream(self, max_streams, resolve_capacity(past, capacity), use_graph, resolve_max_chunk(max_chunk), pages, page_rows,
                              attention=bool(attention), crf=crf)

    def set_grad_bf16(self, on: bool = True) -> bool:
        """bf16 mode: every following training step leaves its gradients ROUNDED ONCE TO BF16 in one flat bf16 buffer - the weight-gradient
        launch writes bf16 dW directly, one cast launch rounds the rest - and ``FusedAdam`` reads that buffer (fp32 moments and parameters as
        ever).  It is the precision every rank's gradient has under the data-parallel bf16 exchange (dp.py), so a one-GPU run and an
        eight-GPU run then train with the same gradient precision; it saves the fp32 dW round trip (8 bytes per parameter and step: 2.66 ->
        2.59 ms per C3 step).  The matrices' fp32 ``.grad`` is NOT written in this mode.  Returns whether the mode is on (fp32 models: no)."""
        eng = self.engine()
        if on and eng.accumulate:
            raise RuntimeError("M2FNet.set_grad_bf16: bf16 gradients do not combine with gradient accumulation "
                               "(set_grad_accumulation(True)): accumulated gradients stay fp32")
        if not on:
            eng.grad_bf16_buf = None
        else:
            for pl in list(eng.plans.values()):             # (plans left in the accumulate form by a data-parallel micro-batch group)
                if pl._acc:
                    pl.accumulate_grads(False)
        if on and eng.grad_bf16_buf is None and eng.precision == runtime.BF16:
            eng.grad_bf16_buf = torch.zeros(eng.flat.numel(), dtype=torch.bfloat16, device=eng.flat.device)
        for pl in list(eng.plans.values()):
            if pl.train and pl.param_grads:
                eng._arm_grad_bf16(pl)
        return eng.grad_bf16_buf is not None

    def set_grad_accumulation(self, on: bool = True) -> None:
        """Every following backward - ``loss.backward()`` or ``train_step`` - follows torch's ``.grad`` rule per parameter: a ``.grad``
        of None takes the gradient of this backward (a view of the flat buffer, as ever), the engine's view ADDS it (inside the kernels:
        one rounded fp32 add per element, so the sum of k backwards is the fp32 sum of their gradients bit for bit), a foreign tensor is
        added to.  ``train_step``'s criterion tail follows suit: ``loss_terms()[1:]`` (den, num) sum over the micro-batches since the
        gradients were last None (``optimizer.zero_grad()`` starts a group; ``zero_grad(set_to_none=False)`` restarts the gradients but
        not den / num).  Exact big-batch training on one GPU::

            optimizer.zero_grad()
            for mb in group:
                model.train_step(*mb, normalise=False)
            optimizer.grad_scale = model.loss_terms()[1:2]
            optimizer.step()

        Off (the default): every backward overwrites, with today's kernels, launch lists and graphs.  Refused together with bf16
        gradients (``set_grad_bf16``), ``train_step(optimizer=...)`` and the data-parallel split step (``overlap=True``)."""
        on = bool(on)
        if on and self._engine is not None and self._engine.grad_bf16_buf is not None:
            raise RuntimeError("M2FNet.set_grad_accumulation: bf16 gradients are on (set_grad_bf16(True)); accumulated gradients "
                               "stay fp32 - call set_grad_bf16(False) first")
        self._grad_accumulation = on
        if self._engine is not None:
            self._engine.accumulate = on
            if not on:                                      # every plan back in the overwrite form now, whatever runs next
                for pl in list(self._engine.plans.values()):
                    if pl._acc:
                        pl.accumulate_grads(False)

    def grad_accumulation(self) -> bool:
        return self._grad_accumulation

    def loss_terms(self) -> torch.Tensor:
        """Device view ``(loss, den, num)`` of the criterion tail of the gradient buffer that ``train_step`` writes: ``loss`` of the last
        micro-batch, and - with accumulation on - ``den`` / ``num`` summed over the micro-batches of the group (valid utterances,
        weighted by the class weights; label-smoothed numerators)."""
        eng = self.engine()
        eng.ensure_grad()
        n = eng.flat.numel()
        return eng.flat_grad_ext[n: n + 3]

    def _term_shares(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(ce, term) from the criterion tail: den, num and, in its fourth float, the sum of the weighted term's rows; the weight is the
        last step's (``_last_criterion``)."""
        eng = self.engine()
        eng.ensure_grad()
        n = eng.flat.numel()
        t = eng.flat_grad_ext[n: n + 4]
        term = t[3] / t[1]
        return t[2] / t[1] - self._last_criterion.term_weight * term, term

    def rdrop_terms(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(ce, kl)`` of the last ``train_step(rdrop=alpha)`` as device scalars: the cross-entropy share of its loss (both views,
        over the one denominator) and the symmetric KL divergence per unit of labelled weight WITHOUT alpha - ``ce + alpha * kl`` is the
        loss.  Read from the criterion tail (den, num and, in its fourth float, the sum of ``w_y * s``, reduced in a fixed order): with
        accumulation on they cover the group's micro-batches, and behind a data-parallel step's all-reduce of the tail they are the
        global values.  alpha is the last step's."""
        return self._term_shares()

    def supcon_terms(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(ce, con)`` of the last ``train_step(supcon=(weight, temperature))`` as device scalars: the cross-entropy share of its
        loss and the contrastive term per unit of labelled weight WITHOUT the weight - ``ce + weight * con`` is the loss.  Read from the
        criterion tail (den, num and, in its fourth float, the sum of ``w_y * l``, reduced in a fixed order): with accumulation on they
        cover the group's micro-batches.  The weight is the last step's."""
        return self._term_shares()

    def aux_terms(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(ce, aux)`` of the last ``train_step(aux=(head, aux_labels, weight))`` as device scalars: the emotion criterion's share of
        its loss and the auxiliary term per unit of labelled weight WITHOUT the weight - ``ce + weight * aux`` is the loss.  Read from
        the criterion tail (den, num and, in its fourth float, the sum of ``w_y * a``, reduced in a fixed order): with accumulation on
        they cover the group's micro-batches.  The weight is the last step's."""
        return self._term_shares()

    def last_aux_logits(self) -> torch.Tensor:
        """The auxiliary head's logits of the most recent ``train_step(aux=)`` of this model as a fresh ``[B, L, A]`` tensor in the
        caller's dialogue order, whatever bucket, packed or long-dialogue plan ran: ``head(last_features())``.  Pad slots are 0.
        Raises RuntimeError when no such step has run, or the plan that ran it was destroyed or has run again since."""
        eng = self._engine
        if eng is None or eng.last is None:
            raise RuntimeError("M2FNet.last_aux_logits: no train_step(aux=) has run on this model (or it was moved since)")
        plan, version, dst, valid, shape = eng.last
        if not plan.handle:
            raise RuntimeError("M2FNet.last_aux_logits: the plan holding the activations of the last step was destroyed "
                               "(evicted from the plan cache)")
        if plan.version != version:
            raise RuntimeError("M2FNet.last_aux_logits: the activations of the last step were overwritten by a later forward "
                               "of the same plan")
        if not plan.train or "aux" not in plan.held or self._last_criterion.aux is None:
            raise RuntimeError("M2FNet.last_aux_logits: the last forward of this model was not a train_step(aux=)")
        return plan.aux_logits(self._last_criterion.aux[0].num_classes, dst, valid, shape).detach()

    def last_features(self) -> torch.Tensor:
        """The classifier's last hidden activation of the most recent ``forward`` / ``train_step`` / ``eval_step`` of this model as a
        fresh, detached ``[B, L, cls_hidden]`` tensor in the caller's dialogue order, whatever bucket, packed or long-dialogue plan ran:
        post-ReLU and - in train mode with dropout > 0 - post-dropout, the operand the final Linear reads and what ``train_step(supcon=)``
        contrasts.  Pad slots are 0.  No second forward.  Raises RuntimeError when no forward has run, or the plan that ran it was
        destroyed or has run again since."""
        eng = self._engine
        if eng is None or eng.last is None:
            raise RuntimeError("M2FNet.last_features: no forward has run on this model (or it was moved since)")
        plan, version, dst, valid, shape = eng.last
        if not plan.handle:
            raise RuntimeError("M2FNet.last_features: the plan holding the activations of the last forward was destroyed "
                               "(evicted from the plan cache)")
        if plan.version != version:
            raise RuntimeError("M2FNet.last_features: the activations of the last forward were overwritten by a later forward "
                               "of the same plan")
        return plan.features(dst, valid, shape).detach()

    def invalidate_shadows(self) -> None:
        """Call after writing parameters in a way torch's version counters do not see (``p.data`` edits, writes through
        ``flat_parameters()``): the next forward re-casts the bf16 parameter shadows."""
        if self._engine is not None:
            self._engine.invalidate_shadows()

    def flat_parameters(self) -> torch.Tensor:
        """The flat fp32 parameter buffer (reference state_dict order).  Handing it out invalidates the bf16 parameter shadows:
        the caller may write through it (in-place writes also move its version counter, which the freshness token includes;
        writes that bypass the counters - ``.data`` - are caught by this call having invalidated)."""
        eng = self.engine()
        eng.invalidate_shadows()
        return eng.flat

    def flat_gradients(self) -> torch.Tensor:
        return self.engine().ensure_grad()
