"""The CPU oracle's input gradients (d loss / d text, d loss / d audio with text and audio as autograd leaves) against the
reference-written fixtures input_grads*.npz (make_golden_input_grads.py), for both losses of input_grad_cases.LOSSES and every
case.  Bound: the full-gradient bound of test_oracle.py, 3e-5 + 5e-4 x max|ref|.  CPU only."""
import os

import numpy as np
import pytest
import torch

import input_grad_cases as IG
import synth
from oracle import m2fnet_oracle as O

CASES = [(f, n) for f, names in IG.FILES.items() for n in names]


def oracle_input_grads(name, kind):
    cfg, text, audio, key_pad, emotion = IG.inputs(name)
    sd = synth.make_state_dict(cfg)
    t = text.clone().requires_grad_(True)
    a = audio.clone().requires_grad_(True)
    loss = IG.loss_fn(kind, O.forward(sd, cfg, t, a, key_pad), emotion, IG.loss_weights(name))
    gt, ga = torch.autograd.grad(loss, [t, a], allow_unused=True)
    return {"text": gt, "audio": ga}


@pytest.mark.parametrize("kind", IG.LOSSES)
@pytest.mark.parametrize("fname,name", CASES)
def test_oracle_input_grads_match_reference(golden_dir, fname, name, kind):
    fx = np.load(os.path.join(golden_dir, fname), allow_pickle=False)
    cfg = IG.CASES[name][0]
    got = oracle_input_grads(name, kind)
    for mod in ("text", "audio"):
        key = f"{name}|d{mod}_{kind}"
        if not cfg[mod.upper()]["enabled"]:
            assert key not in fx.files and got[mod] is None
            continue
        ref = torch.from_numpy(fx[key])
        assert got[mod].shape == ref.shape, key
        err = (got[mod] - ref).abs().max().item()
        assert err <= 3e-5 + 5e-4 * ref.abs().max().item(), (key, err)
