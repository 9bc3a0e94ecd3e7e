"""What M2FNet.adversarial_step computes, stated with the float64 oracle (oracle/m2fnet_oracle.py) and the float64 ascent of
tests/golden/adversarial_ref.py: the inputs are autograd leaves, every pass differentiates the UN-NORMALISED numerator (the criterion's
loss times its denominator) at text + delta / audio + delta, the ascent moves delta along the input gradients, the K parameter gradients
are summed.  For tests only (tests/golden/ already holds an adversarial_ref module: hence this file's name)."""
from __future__ import annotations

import torch

import adversarial_ref as ref
import synth
from oracle import m2fnet_oracle as O


def _pass(cfg, text, audio, key_pad, emotion, label_smoothing):
    """One float64 pass: -> (num, den, {name: d num / d parameter}, d num / d text, d num / d audio)."""
    leaves, sd = {}, {}
    for k, v in synth.make_state_dict(cfg).items():           # (one leaf per unique tensor, as oracle.loss_and_grads)
        if id(v) not in leaves:
            leaves[id(v)] = v.detach().double().requires_grad_(True)
        sd[k] = leaves[id(v)]
    t, a = text.clone().requires_grad_(True), audio.clone().requires_grad_(True)
    logits = O.forward(sd, cfg, t, a, key_pad)
    den = (emotion != -1).sum().double()
    num = O.cross_entropy(logits, emotion, None, label_smoothing) * den
    num.backward()
    zero = lambda x: torch.zeros_like(x) if x.grad is None else x.grad
    return num.detach(), den, {k: zero(v) for k, v in sd.items()}, zero(t), zero(a)


def adversarial_grads(cfg, text, audio, key_pad, emotion, epsilon, steps, step_size=None, norm="utterance", modalities=("text", "audio"),
                      label_smoothing=0.1):
    """-> {"grads": {name: sum over the K passes of d num / d parameter}, "clean": the first pass's, "num": [K], "den", "delta": {modality:
    [B, L, d] float64}}.  CPU tensors; delta starts at zero."""
    step_size = epsilon if step_size is None else step_size
    text, audio = text.double(), audio.double()
    B, L = key_pad.shape
    delta = {"text": torch.zeros_like(text), "audio": torch.zeros_like(audio)}
    total, clean, nums = None, None, []
    gin = {}
    for k in range(steps):
        if k:
            for name, x in (("text", text), ("audio", audio)):
                if name in modalities:
                    d = x.shape[-1]
                    new, _ = ref.ascend(x.reshape(B * L, d), gin[name].reshape(B * L, d), delta[name].reshape(B * L, d), key_pad.reshape(B * L),
                                        epsilon, step_size, norm, torch.float64)
                    delta[name] = new.reshape(B, L, d)
        num, den, g, gin["text"], gin["audio"] = _pass(cfg, text + delta["text"], audio + delta["audio"], key_pad, emotion, label_smoothing)
        nums.append(num)
        if k == 0:
            clean = {n: v.clone() for n, v in g.items()}
            total = g
        else:
            total = {n: total[n] + g[n] for n in g}
    return {"grads": total, "clean": clean, "num": nums, "den": den, "delta": {n: delta[n] for n in modalities}}
