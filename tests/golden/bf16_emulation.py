"""Shared by tests/test_bf16_emulation_gpu.py and tests/test_bf16_emulation_cpu.py: the bound a bf16-mode plan must meet against
the bf16-emulating oracle (oracle/m2fnet_oracle.py, Bf16Rounding), and the comparison itself."""
from __future__ import annotations

import torch

# max |plan - emulation| <= TOL x max |emulation| per tensor (logits: valid rows; loss: TOL x |loss|).  How it was chosen and what
# it measured: tests/test_bf16_emulation_gpu.py.
TOL = 1e-4

# gradients whose largest element is below this are structurally zero (e.g. the key biases: softmax shift invariance) and
# are not compared, as in the other parity tests
ZERO_GRAD = 1e-6


def errors(logits, loss, grads, ref, valid):
    """{name: max |d| / scale} of the logits (valid rows), the loss and every compared gradient against ref = (logits, loss,
    grads) of the emulating oracle.  grads: {name: tensor} for the names to compare (structurally zero ones are skipped)."""
    rl, rs, rg = ref
    out = {}
    r = rl[valid].double()
    out["logits"] = (logits[valid].double() - r).abs().max().item() / r.abs().max().item()
    out["loss"] = abs(float(loss) - float(rs)) / abs(float(rs))
    for k, g in grads.items():
        want = rg[k].double()
        scale = want.abs().max().item()
        if scale < ZERO_GRAD:
            continue
        out[k] = (g.double() - want).abs().max().item() / scale
    return out


def worst(errs):
    k = max(errs, key=errs.get)
    return errs[k], k
