"""CPU oracle for the M2FNet dialogue-level training step.

TEST INFRASTRUCTURE ONLY.  Nothing under ``oracle/`` is part of the product path:
only ``tests/``, ``__graft_entry__.smoke()`` and the ``cpu_baseline`` leg of
``bench.py`` may import it, and there only as the checker / CPU baseline.  The
product path (``multimodal-emotion-recognition_amd``) never falls back to it.

What it is: an explicit, op-by-op restatement (plain ``torch`` CPU fp32 tensor
arithmetic: matmul, exp, sum, sqrt) of the arithmetic the reference obtains from
``torch.nn`` modules.  No ``nn.Transformer*``, ``nn.MultiheadAttention``,
``nn.LayerNorm``, ``nn.Linear``, ``nn.CrossEntropyLoss`` or ``torch.optim`` object is
used here; the backward pass is ``torch.autograd`` applied to these explicit ops.

Parity pin: the reference ships no tests or golden vectors, so this
oracle is pinned by running the REAL reference (``/root/reference/src/model.py``
imported on CPU in the build container) on seeded inputs:
``tests/golden/make_golden.py`` writes the fixtures, ``tests/test_oracle.py`` checks
this file against them (and against the live reference when it is present).

Reference sites restated (paths relative to /root/reference):
  src/model.py:5-20     FusionAttentionModule           -> fam_layer
  src/model.py:102-145  M2FNet.forward                  -> forward
  src/model.py:61-65    nn.TransformerEncoder stack     -> encoder_stack / encoder_layer
  src/train.py:41-52    CrossEntropyLoss(ls=0.1, ignore=-1[, weight]) -> cross_entropy
  src/train.py:56       torch.optim.Adam (coupled L2)   -> adam_step
  src/train.py:260-272  per-batch accuracy / weighted-F1, mean over batches -> batch_metrics
  src/dataset.py:71-89  collate_fn padding contract     -> collate
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

Tensor = torch.Tensor
LN_EPS = 1e-5          # torch default layer_norm_eps, inherited at src/model.py:61-62
DIM_FF = 2048          # torch default dim_feedforward, inherited at src/model.py:61


def _get(cfg, name):
    """Attribute-or-key access so both Munch-like objects and dicts work."""
    if isinstance(cfg, dict):
        return cfg[name]
    return getattr(cfg, name)


# --------------------------------------------------------------------------------------
# primitive ops
# --------------------------------------------------------------------------------------
def linear(x: Tensor, w: Tensor, b: Optional[Tensor]) -> Tensor:
    """y = x W^T + b with W stored [out, in] (nn.Linear convention)."""
    y = x @ w.t()
    return y if b is None else y + b


def layer_norm(x: Tensor, g: Tensor, b: Tensor, eps: float = LN_EPS) -> Tensor:
    """Biased-variance LayerNorm over the last dim (nn.LayerNorm semantics)."""
    mu = x.mean(dim=-1, keepdim=True)
    xc = x - mu
    var = (xc * xc).mean(dim=-1, keepdim=True)
    return xc / torch.sqrt(var + eps) * g + b


def attention(q: Tensor, k: Tensor, v: Tensor, key_pad: Tensor, n_head: int,
              return_probs: bool = False, drop=None, name: str = ""):
    """Multi-head scaled-dot-product attention on [B, L, E] tensors.

    key_pad: bool [B, L], True = padded key (gets -inf before softmax), the
    key_padding_mask / src_key_padding_mask convention of src/model.py:14,107.
    drop (see `forward`): applied to the softmax probabilities [B, H, L, L] under `name`, where nn.MultiheadAttention applies its
    dropout; the returned probabilities are the ones before it.
    """
    B, L, E = q.shape
    hd = E // n_head
    qh = q.reshape(B, L, n_head, hd).permute(0, 2, 1, 3)
    kh = k.reshape(B, L, n_head, hd).permute(0, 2, 1, 3)
    vh = v.reshape(B, L, n_head, hd).permute(0, 2, 1, 3)
    s = (qh @ kh.transpose(-1, -2)) * (1.0 / math.sqrt(hd))
    s = s.masked_fill(key_pad[:, None, None, :], float("-inf"))
    s = s - s.max(dim=-1, keepdim=True).values
    p = torch.exp(s)
    p = p / p.sum(dim=-1, keepdim=True)
    o = ((p if drop is None else drop(name, p)) @ vh).permute(0, 2, 1, 3).reshape(B, L, E)
    return (o, p) if return_probs else o


# --------------------------------------------------------------------------------------
# bf16-mode emulation (opt-in: loss_and_grads(..., rounding=Bf16Rounding()))
# --------------------------------------------------------------------------------------
class Bf16Rounding:
    """Where bf16 mode rounds to bf16.  The emulation computes in float64 and rounds, round to nearest even on the fp32 value
    (m2f_bf16_bits, csrc/common.h:72-75: a plain (__bf16) cast), exactly the operands the kernels round; everything else -
    bias, ReLU, residual, gate, LayerNorm, softmax, criterion, the sums - is unrounded.  One attribute per rule, all on by
    default; switching one off is what tests/test_bf16_emulation_cpu.py does to show the GPU bound would see it.
    Paths below are relative to multimodal-emotion-recognition_amd/csrc.

    GEMMs (every nn.Linear / in-projection / out-projection, the FAM's two-segment cat(relu(x), text) operand, the classifier):
      fwd_x     forward A operand (activation) rounded: the producer writes a bf16 shadow at the same element index
                (gemm.hip:353,360, rowops / attention epilogues), GEMMs stage from it ("bf16 operand
                shadows"); a launch staged from fp32 rounds on the way into LDS (gemm.hip:208,215): the same value.
      fwd_w     forward B operand (weight) rounded: parameter shadow W [rows][pad8(cols)] (m2f_cast_t_kernel, or
                m2f_adam_shadow_kernel after a FusedAdam step).  Bias, ReLU, residual, gate: fp32 after the product
                (gemm.hip:229).
      dgrad_dy  dX = bf16(dY) . bf16(W): dY from the shadow its producer wrote (LayerNorm backward, attention backward, the
                gated dgrad epilogue), ...
      dgrad_w   ... and W from the transposed parameter shadow W^T [cols][pad8(rows)] (the NN dgrad rerouted through it).
      wgrad_dy  dW = bf16(dY)^T . bf16(X): the weight-gradient table launch reads the row-major shadows (gemm_p8.h,
      wgrad_x   gemm_ring.h TABLE form); the [T, C] criterion gradient is cast to 8-column bf16 rows in front of it (plan_build.hip, build_wgrad_table).
      bias_dy   bias gradient = column sum of bf16(dY): the table forms sum the bf16 fragments they stage (gemm_p8.h:395,
                gemm_ring.h:663), the bf16-source grouped form its staged bf16 tile (gemm.hip:829,914).  Finding: the
                fp32-SOURCE grouped form sums the fp32 values before it rounds them (gemm.hip:185-191, a contract
                tests/test_kernels_gpu.py::test_gemm_layouts pins); with M2F_WGRAD_TABLE=0 it takes the one weight-gradient
                problem whose dY has no shadow, the classifier's last Linear (the [T, C] criterion gradient), so
                wgrad_table=False (that variant) sums that bias gradient from the fp32 dY.
      skinny    the classifier's last Linear ([T, C] problems, C <= 8) runs on the skinny kernels, which round both operands
                as the MFMA kernels do (skinny.hip:16-18,192: shadows when every operand has one, else r16): off = its
                forward and its input gradient are not rounded (its weight gradient stays in the table launch).
      The criterion gradient itself is fp32 (m2f_ce_kernel) and is rounded only where it enters these products.

    Dialogue attention, L <= 64 (attention.hip, AttnBatch::bf16_math = 63 in bf16 mode, plan_build.hip, to_launches):
      bit 1 (attention.hip:129,337,388): Q K^T and dO V^T on the bf16 MFMA - both operands rounded on the way in
                (slab8_bf16, attention.hip:42-50), whatever the slabs hold; the scale 1/sqrt(hd) is applied to the fp32
                product afterwards (attention.hip:113,151: s * scale; backward: p * (dp - delta) * scale).
      bits 2/4/8 (Q/K/V, forward and backward) and 16/32 (dO/O, backward) (attention.hip:35,662): the slabs are staged
                from the operands' bf16 shadows, so EVERY use of the operand sees it rounded: P V (forward), dQ = dS K,
                dK = dS^T Q, dV = P^T dO and delta = sum(dO * O) (attention.hip:264-275).  Only on the fast staging path
                (slab_fast_ok, attn_slab.h:68-71, with slab_shadow: hd % 4 == 0 and head dim padded to 16 <= 128; backward
                also attn_bwd_fast, attention.hip:601-603: 5 Lp (W + 2) + Lp floats <= 160 KiB).  Otherwise the slabs are
                fp32 and only the bit-1 contractions round (finding: e.g. head dim 75 of c2_slice's audio encoder, 15 of
                tiny_odd_heads: there V, and in the backward K, Q, dO (for dQ/dK/dV) and O stay fp32).
      P, dS, the softmax and the row sums are fp32.  attn_q / attn_k / attn_v / attn_do / attn_o switch one operand's
      rounding (everywhere it is rounded); attn = False switches all of them (M2F_ATTN_BF16=0).  The mode is decided per
      attention problem from its own head dim (a merged launch takes the widest head dim for attn_bwd_fast: it only
      matters at Lp = 64 with head dims 113..128 in one launch and others narrower, which no test case has).
    Plans with L > 64 (attention_dlong.hip; picked by the plan's L, plan.hip, run_launches, packed or not): no attention
    rounding, those kernels read fp32 operands.  The L here is the batch's L (the shape bucket rounds up to a multiple of 16,
    which does not cross 64).
    LayerNorm, the residual stream, the criterion and Adam: fp32, no rounding.
    """
    GEMM_RULES = ("fwd_x", "fwd_w", "dgrad_dy", "dgrad_w", "wgrad_dy", "wgrad_x", "bias_dy", "skinny")
    ATTN_RULES = ("attn_q", "attn_k", "attn_v", "attn_do", "attn_o")
    RULES = GEMM_RULES + ATTN_RULES

    def __init__(self, attn: bool = True, wgrad_table: bool = True, jitter: float = 0.0, seed: int = 0, **off):
        for r in self.RULES:
            setattr(self, r, True)
        self.attn, self.wgrad_table = bool(attn), bool(wgrad_table)
        # jitter > 0: every value is multiplied by (1 + jitter * N(0, 1)) just before it is rounded - a stand-in for the fp32
        # summation noise of the kernels, to measure how stable a case's rounding decisions are (the emulation against itself)
        self.jitter = float(jitter)
        self._gen = torch.Generator().manual_seed(seed)
        for r, v in off.items():
            if r not in self.RULES:
                raise ValueError(f"unknown rounding rule {r!r}")
            setattr(self, r, bool(v))

    def r(self, x: Tensor, on: bool) -> Tensor:
        if on and self.jitter:
            x = x * (1.0 + self.jitter * torch.randn(x.shape, generator=self._gen, dtype=x.dtype))
        return _bf16(x, on)


def _bf16(x: Tensor, on: bool = True) -> Tensor:
    """Round to bf16 (nearest even, from the fp32 value as m2f_bf16_bits does) and back to x's dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype) if on else x


class _Linear16(torch.autograd.Function):
    """y = bf16(x) bf16(W)^T + b; backward dX = bf16(dY) bf16(W), dW = bf16(dY)^T bf16(X), db = sum bf16(dY)."""

    @staticmethod
    def forward(ctx, x, w, b, rnd, skinny):
        sk = rnd.skinny or not skinny
        ctx.rnd, ctx.sk, ctx.skinny = rnd, sk, skinny
        ctx.save_for_backward(x, w)
        y = rnd.r(x, rnd.fwd_x and sk) @ rnd.r(w, rnd.fwd_w and sk).t()
        return y if b is None else y + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        r, sk = ctx.rnd, ctx.sk
        dx = r.r(dy, r.dgrad_dy and sk) @ r.r(w, r.dgrad_w and sk)
        dy2 = dy.reshape(-1, dy.shape[-1])
        dw = r.r(dy2, r.wgrad_dy).t() @ r.r(x.reshape(-1, x.shape[-1]), r.wgrad_x)
        db = r.r(dy2, r.bias_dy and (r.wgrad_table or not ctx.skinny)).sum(dim=0)
        return dx, dw, db, None, None


class _Attn16(torch.autograd.Function):
    """Dialogue attention as attention.hip computes it in bf16 mode (see Bf16Rounding); [B, L, E] in and out."""

    @staticmethod
    def forward(ctx, q, k, v, key_pad, n_head, rnd, keep=None):
        B, L, E = q.shape
        hd = E // n_head
        W, Lp = (hd + 15) // 16 * 16, 16 * ((L + 15) // 16)
        fast = hd % 4 == 0 and W <= 128                                   # staged from the shadows (forward)
        ctx.bwd_fast = fast and (5 * Lp * (W + 2) + Lp) * 4 <= 160 * 1024
        heads = lambda t: t.reshape(B, L, n_head, hd).permute(0, 2, 1, 3)
        qh, kh, vh = heads(q), heads(k), heads(v)
        scale = 1.0 / math.sqrt(hd)
        s = (rnd.r(qh, rnd.attn_q) @ rnd.r(kh, rnd.attn_k).transpose(-1, -2)) * scale
        s = s.masked_fill(key_pad[:, None, None, :], float("-inf"))
        s = s - s.max(dim=-1, keepdim=True).values
        p = torch.exp(s)
        p = p / p.sum(dim=-1, keepdim=True)
        # keep (dropout on the probabilities: mask / (1 - p), [B, H, L, L]): P stays fp32 in the kernels, the dropped P feeds P V
        # (attention.hip:176), and in the backward dV = (P keep)^T dO, dP = (dO V^T) keep (attention.hip:355,407)
        o = (p if keep is None else p * keep) @ rnd.r(vh, rnd.attn_v and fast)
        ctx.save_for_backward(qh, kh, vh, p, o)
        ctx.keep = keep
        ctx.rnd, ctx.scale, ctx.shape = rnd, scale, (B, L, n_head, hd)
        return o.permute(0, 2, 1, 3).reshape(B, L, E)

    @staticmethod
    def backward(ctx, do):
        qh, kh, vh, p, o = ctx.saved_tensors
        r, f = ctx.rnd, ctx.bwd_fast
        B, L, H, hd = ctx.shape
        doh = do.reshape(B, L, H, hd).permute(0, 2, 1, 3)
        dp = r.r(doh, r.attn_do) @ r.r(vh, r.attn_v).transpose(-1, -2)           # bit 1: always rounded
        if ctx.keep is not None:
            dp = dp * ctx.keep
        dor = r.r(doh, r.attn_do and f)
        delta = (dor * r.r(o, r.attn_o and f)).sum(dim=-1, keepdim=True)
        ds = p * (dp - delta) * ctx.scale
        dq = ds @ r.r(kh, r.attn_k and f)
        dk = ds.transpose(-1, -2) @ r.r(qh, r.attn_q and f)
        dv = (p if ctx.keep is None else p * ctx.keep).transpose(-1, -2) @ dor
        back = lambda t: t.permute(0, 2, 1, 3).reshape(B, L, H * hd)
        return back(dq), back(dk), back(dv), None, None, None, None


def _lin(x: Tensor, w: Tensor, b: Optional[Tensor], rnd: Optional[Bf16Rounding], skinny: bool = False) -> Tensor:
    return linear(x, w, b) if rnd is None else _Linear16.apply(x, w, b, rnd, skinny)


def _attn(q, k, v, key_pad, n_head, rnd: Optional[Bf16Rounding], return_probs: bool = False, drop=None, name: str = ""):
    if rnd is None:
        return attention(q, k, v, key_pad, n_head, return_probs, drop, name)
    if not rnd.attn or q.shape[1] > 64:
        return attention(q, k, v, key_pad, n_head, return_probs, drop, name)
    keep = None
    if drop is not None:          # the hook is a mask times a scale: its image of ones is that factor
        B, L, _ = q.shape
        keep = drop(name, torch.ones(B, n_head, L, L, dtype=q.dtype))
    o = _Attn16.apply(q, k, v, key_pad, n_head, rnd, keep)
    return (o, None) if return_probs else o


def _drop(drop, name: str, x: Tensor) -> Tensor:
    return x if drop is None else drop(name, x)


# --------------------------------------------------------------------------------------
# blocks
# --------------------------------------------------------------------------------------
def encoder_layer(x: Tensor, sd: Dict[str, Tensor], pre: str, key_pad: Tensor, n_head: int,
                  rnd: "Optional[Bf16Rounding]" = None, drop=None) -> Tensor:
    """Post-LN TransformerEncoderLayer (norm_first=False, ReLU), dropout = identity unless `drop` is given.

    x <- LN1(x + SA(x)); x <- LN2(x + W2 relu(W1 x + b1) + b2)   
    drop (see `forward`), where nn.TransformerEncoderLayer applies its four dropouts: `<pre>attn` on the softmax probabilities,
    `<pre>dropout1` after out_proj before the residual, `<pre>ff` after relu(linear1), `<pre>dropout2` after linear2 before the
    residual.  In bf16 mode the masks act on the fp32 results of the GEMM epilogues (bias, ReLU, mask, residual in that order),
    i.e. before the value is rounded as the next GEMM's operand - which is where these lines put them.
    """
    E = x.shape[-1]
    qkv = _lin(x, sd[pre + "self_attn.in_proj_weight"], sd[pre + "self_attn.in_proj_bias"], rnd)
    q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
    a = _attn(q, k, v, key_pad, n_head, rnd, drop=drop, name=pre + "attn")
    a = _drop(drop, pre + "dropout1", _lin(a, sd[pre + "self_attn.out_proj.weight"], sd[pre + "self_attn.out_proj.bias"], rnd))
    x = layer_norm(x + a, sd[pre + "norm1.weight"], sd[pre + "norm1.bias"])
    h = _drop(drop, pre + "ff", torch.relu(_lin(x, sd[pre + "linear1.weight"], sd[pre + "linear1.bias"], rnd)))
    h = _drop(drop, pre + "dropout2", _lin(h, sd[pre + "linear2.weight"], sd[pre + "linear2.bias"], rnd))
    return layer_norm(x + h, sd[pre + "norm2.weight"], sd[pre + "norm2.bias"])


def encoder_stack(x: Tensor, sd: Dict[str, Tensor], pre: str, key_pad: Tensor, n_head: int,
                  n_layers: int, rnd: "Optional[Bf16Rounding]" = None, drop=None) -> Tensor:
    """nn.TransformerEncoder(layer, num_layers, norm): layers then the final LayerNorm."""
    for l in range(n_layers):
        x = encoder_layer(x, sd, f"{pre}layers.{l}.", key_pad, n_head, rnd, drop)
    return layer_norm(x, sd[pre + "norm.weight"], sd[pre + "norm.bias"])


def fam_layer(text: Tensor, audio: Tensor, sd: Dict[str, Tensor], pre: str, key_pad: Tensor,
              n_head: int, inter: Optional[dict] = None, rnd: "Optional[Bf16Rounding]" = None, drop=None) -> Tensor:
    """FusionAttentionModule.forward (src/model.py:13-20): Q = V = text, K = audio.
    drop (see `forward`): `<pre>attn` on the softmax probabilities (nn.MultiheadAttention's own dropout); the dropout BEHIND the
    layer (src/model.py:131) is applied by `forward` under `<pre>out`."""
    E = text.shape[-1]
    w = sd[pre + "multihead_attention.in_proj_weight"]
    b = sd[pre + "multihead_attention.in_proj_bias"]
    q = _lin(text, w[:E], b[:E], rnd)
    k = _lin(audio, w[E:2 * E], b[E:2 * E], rnd)
    v = _lin(text, w[2 * E:], b[2 * E:], rnd)
    a, p = _attn(q, k, v, key_pad, n_head, rnd, return_probs=True, drop=drop, name=pre + "attn")
    x = _lin(a, sd[pre + "multihead_attention.out_proj.weight"],
             sd[pre + "multihead_attention.out_proj.bias"], rnd)
    y = torch.relu(_lin(torch.relu(torch.cat((x, text), dim=2)),
                        sd[pre + "linear.weight"], sd[pre + "linear.bias"], rnd))
    if inter is not None:
        inter.update(q=q, k=k, v=v, p=p, attn=a, x=x, y=y)
    return y


def forward(sd: Dict[str, Tensor], cfg, text: Tensor, audio: Tensor, key_pad: Tensor,
            inter: Optional[dict] = None, rnd: "Optional[Bf16Rounding]" = None, drop=None) -> Tensor:
    """M2FNet.forward (src/model.py:102-145).  Without `drop` every dropout is the identity (eval mode, or train mode with
    model.dropout = 0.0); with it, train mode under the caller's masks.  rnd: see Bf16Rounding (None = no rounding).

    drop: None (the default), or a callable (name, tensor) -> tensor standing for train-mode dropout
    with masks the CALLER supplies - an element-wise factor keep / (1 - p); this file knows nothing about where masks come from.
    It is called wherever the reference applies a dropout, under these names: `<stack>.layers.<l>.{attn, dropout1, ff, dropout2}`
    (encoder_layer), `{audio, text}.pre_proj` / `.post_proj` before and after each projection (src/model.py:111-113,123-125),
    `fusion_layers.<i>.attn` and `fusion_layers.<i>.out` (after every fusion layer, :131), `classifier` after the head's last
    ReLU (:98).

    text [B,L,d_t], audio [B,L,d_a] fp32; key_pad bool [B,L] (True = pad) -> logits [B,L,C].
    """
    A, Tx, F, C = _get(cfg, "AUDIO"), _get(cfg, "TEXT"), _get(cfg, "FAM"), _get(cfg, "CLASSIFIER")
    a_on, t_on, f_on = bool(_get(A, "enabled")), bool(_get(Tx, "enabled")), bool(_get(F, "enabled"))
    if not a_on and not t_on:
        raise ValueError("At least one of audio and text must be enabled!")       # src/model.py:32-33
    if f_on and not (a_on and t_on):
        raise ValueError("Fusion Attention Module can only be used with both audio and text enabled!")

    if a_on:
        for e in range(_get(A, "n_transformers")):                                 # src/model.py:106-107
            audio = audio + encoder_stack(audio, sd, f"audio_encoders.{e}.", key_pad,
                                          _get(A, "n_head"), _get(A, "n_encoder_layers"), rnd, drop)
        audio = _drop(drop, "audio.post_proj",
                      _lin(_drop(drop, "audio.pre_proj", audio), sd["audio_proj.weight"], sd["audio_proj.bias"], rnd))      # :111-113
    if t_on:
        for e in range(_get(Tx, "n_transformers")):                                # :118-119
            text = text + encoder_stack(text, sd, f"text_encoders.{e}.", key_pad,
                                        _get(Tx, "n_head"), _get(Tx, "n_encoder_layers"), rnd, drop)
        text = _drop(drop, "text.post_proj",
                     _lin(_drop(drop, "text.pre_proj", text), sd["text_proj.weight"], sd["text_proj.bias"], rnd))          # :123-125
    if inter is not None:
        inter["audio_proj"] = audio if a_on else None
        inter["text_proj"] = text if t_on else None

    if f_on:
        for i in range(_get(F, "n_layers")):                                       # :129-131
            li = {} if inter is not None else None
            text = _drop(drop, f"fusion_layers.{i}.out",
                         fam_layer(text, audio, sd, f"fusion_layers.{i}.", key_pad, _get(F, "n_head"), li, rnd, drop))
            if inter is not None:
                inter[f"fam{i}"] = li
        x = torch.cat((audio, text), dim=2)                                        # :134  (audio, text)
    elif a_on and t_on:
        x = torch.cat((audio, text), dim=2)
    else:
        x = text if t_on else audio

    n_cls = _get(C, "n_layers")                                                    # :89-100
    x = _lin(x, sd["output_layer.0.weight"], sd["output_layer.0.bias"], rnd)
    idx = 0
    for _ in range(max(n_cls - 2, 0)):
        idx += 2
        x = _lin(torch.relu(x), sd[f"output_layer.{idx}.weight"], sd[f"output_layer.{idx}.bias"], rnd)
    idx += 3
    return _lin(_drop(drop, "classifier", torch.relu(x)), sd[f"output_layer.{idx}.weight"], sd[f"output_layer.{idx}.bias"], rnd,
                skinny=True)


# --------------------------------------------------------------------------------------
# criterion / optimizer / metrics
# --------------------------------------------------------------------------------------
def cross_entropy(logits: Tensor, target: Tensor, class_weight: Optional[Tensor] = None,
                  label_smoothing: float = 0.1, ignore_index: int = -1) -> Tensor:
    """CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1[, weight]) of src/train.py:48-50
    on logits [B,L,C] vs target int64 [B,L] (the reference permutes to [B,C,L], same thing).

    unweighted: mean_valid( (1-e)*(-logp_y) + e*mean_c(-logp_c) )
    weighted:   [ sum_valid (1-e)*w_y*(-logp_y) + e*sum_c w_c*(-logp_c)/C ] / sum_valid w_y
    (closed form verified against nn.CrossEntropyLoss).
    """
    C = logits.shape[-1]
    z = logits.reshape(-1, C)
    t = target.reshape(-1)
    valid = t != ignore_index
    zc = z - z.max(dim=-1, keepdim=True).values
    logp = zc - torch.log(torch.exp(zc).sum(dim=-1, keepdim=True))
    ts = torch.where(valid, t, torch.zeros_like(t))
    w = torch.ones(C, dtype=z.dtype) if class_weight is None else class_weight
    nll = -(logp.gather(1, ts[:, None])[:, 0]) * w[ts]
    smooth = -(logp * w[None, :]).sum(dim=-1) / C
    per = (1.0 - label_smoothing) * nll + label_smoothing * smooth
    vf = valid.to(z.dtype)
    return (per * vf).sum() / (w[ts] * vf).sum()


def adam_step(params: Sequence[Tensor], grads: Sequence[Tensor], exp_avg: List[Tensor],
              exp_avg_sq: List[Tensor], step: int, lr: float = 5e-5, weight_decay: float = 0.01,
              beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8) -> None:
    """torch.optim.Adam with COUPLED L2 (g += wd*p), bias-corrected (src/train.py:56).
    `step` is the 1-based step count AFTER this update.  In-place on params/state."""
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    with torch.no_grad():
        for p, g, m, v in zip(params, grads, exp_avg, exp_avg_sq):
            g = g + weight_decay * p
            m.mul_(beta1).add_(g, alpha=1.0 - beta1)
            v.mul_(beta2).add_(g * g, alpha=1.0 - beta2)
            denom = v.sqrt() / math.sqrt(bc2) + eps
            p.add_(-(lr / bc1) * (m / denom))


def weighted_f1(y_true: Tensor, y_pred: Tensor) -> float:
    """sklearn f1_score(average='weighted') restated: per-class F1 over the labels present
    in y_true or y_pred, weighted by true support (0/0 -> 0)."""
    labels = torch.unique(torch.cat((y_true, y_pred)))
    total, acc = 0, 0.0
    for c in labels.tolist():
        tp = int(((y_true == c) & (y_pred == c)).sum())
        fp = int(((y_true != c) & (y_pred == c)).sum())
        fn = int(((y_true == c) & (y_pred != c)).sum())
        sup = tp + fn
        f1 = 0.0 if (2 * tp + fp + fn) == 0 else 2.0 * tp / (2 * tp + fp + fn)
        acc += f1 * sup
        total += sup
    return acc / total if total else 0.0


def batch_metrics(logits: Tensor, target: Tensor, ignore_index: int = -1) -> Tuple[float, float]:
    """One batch's (accuracy, weighted-F1) as src/train.py:261-267 computes them."""
    pred = logits.argmax(dim=2)
    m = target != ignore_index
    yt, yp = target[m].flatten(), pred[m].flatten()
    return float((yt == yp).to(torch.float64).mean()), weighted_f1(yt, yp)


def epoch_metrics(batches: Sequence[Tuple[Tensor, Tensor]]) -> Tuple[float, float]:
    """UNWEIGHTED mean over batches of the per-batch scores (src/train.py:272, src/test.py:73)."""
    accs, f1s = zip(*(batch_metrics(lg, tg) for lg, tg in batches))
    return sum(accs) / len(accs), sum(f1s) / len(f1s)


def collate(dialogues: Sequence[Dict[str, Tensor]]) -> Dict[str, Tensor]:
    """collate_fn / apply_padding (src/dataset.py:71-89, src/utils.py:15-31): zero-pad features to
    the longest dialogue of the batch, pad labels with -1, padding_mask = (emotion == -1)."""
    L = max(d["text"].shape[0] for d in dialogues)
    B = len(dialogues)
    text = torch.zeros(B, L, dialogues[0]["text"].shape[1])
    audio = torch.zeros(B, L, dialogues[0]["audio"].shape[1])
    emo = torch.full((B, L), -1, dtype=torch.int64)
    for i, d in enumerate(dialogues):
        n = d["text"].shape[0]
        text[i, :n], audio[i, :n] = d["text"], d["audio"]
        emo[i, :n] = torch.as_tensor(d["emotion"], dtype=torch.int64).reshape(-1)
    return {"text": text, "audio": audio, "padding_mask": emo == -1, "emotion": emo}


def loss_and_grads(sd: Dict[str, Tensor], cfg, text, audio, key_pad, target,
                   class_weight: Optional[Tensor] = None, rounding: "Optional[Bf16Rounding]" = None, drop=None,
                   input_grads: bool = False):
    """forward + criterion + backward; returns (logits, loss, {name: grad}) for unique tensors.
    drop: the dropout hook of `forward`.  input_grads: the dict also holds d loss / d text and d loss / d audio under "text" / "audio".
    Without `rounding` the arithmetic runs in the dtype of `sd` and the inputs (float64 tensors give a float64 reference).

    rounding (a Bf16Rounding): emulate bf16 mode - everything in float64, rounded to bf16 where the kernels round; the
    results are float64.  None (the default): the plain oracle."""
    if rounding is not None:
        text, audio = text.double(), audio.double()
        class_weight = None if class_weight is None else class_weight.double()
    leaves: Dict[int, Tensor] = {}
    sd2 = {}
    for k, v in sd.items():
        if id(v) not in leaves:
            t = v.detach().clone() if rounding is None else v.detach().double()
            leaves[id(v)] = t.requires_grad_(True)
        sd2[k] = leaves[id(v)]
    if input_grads:
        text, audio = text.detach().clone().requires_grad_(True), audio.detach().clone().requires_grad_(True)
    logits = forward(sd2, cfg, text, audio, key_pad, rnd=rounding, drop=drop)
    loss = cross_entropy(logits, target, class_weight)
    loss.backward()
    grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in sd2.items()}
    if input_grads:
        grads["text"] = text.grad if text.grad is not None else torch.zeros_like(text)
        grads["audio"] = audio.grad if audio.grad is not None else torch.zeros_like(audio)
    return logits.detach(), loss.detach(), grads
