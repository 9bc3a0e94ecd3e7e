"""Generate tests/golden/input_grads.npz and input_grads_c1.npz by running the REAL reference on CPU (as make_golden.py does).

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_input_grads.py
Cases: input_grad_cases.py (every tiny_* case, c1, a config with n_transformers = 0 / n_encoder_layers = 0, an L = 80 long case).
The reference's src/model.py in eval mode with synth.py weights; `text` and `audio` are leaves that require grad, and their
gradients are recorded for the two losses of input_grad_cases.LOSSES.  Only tensors are written - never reference source or
bytecode.  Keys: "<case>|d<text|audio>_<loss>" (a disabled modality has none)."""
from __future__ import annotations

import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import input_grad_cases as IG  # noqa: E402
import synth  # noqa: E402

REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "src"))
sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")
import model as ref_model  # noqa: E402  (the reference's src/model.py)


def ns(d):
    return types.SimpleNamespace(**{k: (ns(v) if isinstance(v, dict) else v) for k, v in d.items()})


def run_case(name, rec):
    cfg, text, audio, key_pad, emotion = IG.inputs(name)
    sd = synth.make_state_dict(cfg)
    torch.manual_seed(0)
    m = ref_model.M2FNet(ns(cfg))
    m.load_state_dict(sd, strict=True)
    m.eval()
    R = IG.loss_weights(name)
    for kind in IG.LOSSES:
        t = text.clone().requires_grad_(True)
        a = audio.clone().requires_grad_(True)
        loss = IG.loss_fn(kind, m(t, a, key_pad), emotion, R)
        gt, ga = torch.autograd.grad(loss, [t, a], allow_unused=True)
        for mod, g in (("text", gt), ("audio", ga)):
            if g is not None:
                rec[f"{name}|d{mod}_{kind}"] = g.numpy().astype(np.float32)


def main():
    torch.set_num_threads(8)
    for fname, names in IG.FILES.items():
        rec = {}
        for name in names:
            run_case(name, rec)
            print(name, "done")
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **rec)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
