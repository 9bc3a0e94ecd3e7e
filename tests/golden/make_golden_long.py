"""Generate tests/golden/long_dialogues.npz by running the REAL reference on CPU (as make_golden.py does).

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_long.py
Cases: long_cases.py (dialogues of 110, 129, 128 and 512 utterances, seeded synth.py weights and inputs) and a standalone
FusionAttentionModule at L = 100 with a key-padding mask.  Records eval logits, the train-mode (dropout 0) loss, gradient
norms / digests (full gradients of the tiny cases' smaller tensors), three torch.optim.Adam steps, and the fusion module's output on every row.
Only tensors are written - never reference source or bytecode.  Keys: "<case>|<record>"."""
from __future__ import annotations

import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import long_cases  # noqa: E402
import synth  # noqa: E402

REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "src"))
sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")
import model as ref_model  # noqa: E402  (the reference's src/model.py)


def ns(d):
    return types.SimpleNamespace(**{k: (ns(v) if isinstance(v, dict) else v) for k, v in d.items()})


def run_case(name, rec):
    cfg, text, audio, key_pad, emotion = long_cases.inputs(name)
    sd = synth.make_state_dict(cfg)
    torch.manual_seed(0)
    m = ref_model.M2FNet(ns(cfg))
    m.load_state_dict(sd, strict=True)
    put = lambda k, v: rec.__setitem__(f"{name}|{k}", v)      # noqa: E731
    m.eval()
    with torch.inference_mode():
        put("logits_eval", m(text, audio, key_pad).numpy())
    m.train()                                                 # dropout = 0.0 -> deterministic
    crit = torch.nn.CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    out = m(text, audio, key_pad)
    loss = crit(out.permute(0, 2, 1), emotion)
    put("loss", np.float64(loss.item()))
    m.zero_grad()
    loss.backward()
    seen, names, norms, dots = set(), [], [], []
    for i, (k, p) in enumerate(m.state_dict(keep_vars=True).items()):
        if id(p) in seen:
            continue
        seen.add(id(p))
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        names.append(k)
        norms.append(float(g.double().norm()))
        dots.append(float((g.double() * synth.digest_vector(tuple(g.shape), 3, i).double()).sum()))
        if (name in long_cases.FULL_GRAD and g.numel() <= 32768) or g.dim() == 1:
            put("grad::" + k, g.numpy().copy())
    put("grad_names", np.array(names))
    put("grad_norms", np.array(norms))
    put("grad_dots", np.array(dots))
    if name not in long_cases.FULL_GRAD:
        return
    m.load_state_dict(sd, strict=True)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=0.01)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        lo = crit(m(text, audio, key_pad).permute(0, 2, 1), emotion)
        lo.backward()
        opt.step()
        losses.append(lo.item())
    put("adam_losses", np.array(losses, dtype=np.float64))
    seen, pn = set(), []
    for k, p in m.state_dict(keep_vars=True).items():
        if id(p) not in seen:
            seen.add(id(p))
            pn.append(float(p.detach().double().norm()))
    put("adam3_norms", np.array(pn))
    m.eval()
    with torch.inference_mode():
        put("adam3_logits_eval", m(text, audio, key_pad).numpy())


def run_fam(rec):
    E, H, w, text, audio, key_pad = long_cases.fam_case()
    f = ref_model.FusionAttentionModule(E, H, 0.0)
    f.load_state_dict(w, strict=True)
    f.eval()
    with torch.inference_mode():
        rec["fam_l100|out"] = f(text, audio, key_pad).numpy()


def main():
    rec = {}
    for name in long_cases.CASES:
        run_case(name, rec)
        print(name, "loss", float(rec[f"{name}|loss"]))
    run_fam(rec)
    path = os.path.join(HERE, "long_dialogues.npz")
    np.savez_compressed(path, **rec)
    print(f"{path}: {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
