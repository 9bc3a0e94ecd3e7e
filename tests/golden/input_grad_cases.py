"""Cases of the input-gradient fixtures (input_grads.npz, input_grads_c1.npz), shared by make_golden_input_grads.py and the tests:
seeded configs and inputs from synth.py / long_cases.py, and the seeded weights R of the second loss, (logits * R).sum()."""
from __future__ import annotations

import numpy as np
import torch

import long_cases
import synth

# name -> (config.model dict, B, L, dialogue lengths)
CASES = {name: (cfg, B, L, lengths) for name, (cfg, B, L, lengths, _) in synth.CASES.items()
         if name.startswith("tiny") or name == "c1"}
# text: no encoder stack at all (n_transformers = 0: the embedding goes straight to the projection)
CASES["no_text_stack"] = (synth._cfg(48, 64, 64, 4, 4, 4, 1, 2, 1, nt_a=1, nt_t=0), 3, 7, [7, 4, 1])
# L = 80 > 64: a packed plan on the long-dialogue kernels, built as long_cases.py builds its cases
CASES["long_l80"] = (long_cases.CASES["long_tiny"][0], 3, 80, [80, 33, 61])
LONG = {"long_l80"}
FILES = {"input_grads.npz": [n for n in CASES if n != "c1"], "input_grads_c1.npz": ["c1"]}
LOSSES = ("ce", "r")                 # the criterion of src/train.py:48-50 | (logits * R).sum(), R also weighting pad slots


def inputs(name):
    """(config, text, audio, key_pad, emotion) of a case."""
    cfg, B, L, lengths = CASES[name]
    return (cfg,) + synth.make_inputs(cfg, B, L, lengths, "randn")


def loss_weights(name) -> torch.Tensor:
    """R [B, L, n_classes]: seeded normal weights on every slot, pads included."""
    cfg, B, L, _ = CASES[name]
    g = np.random.Generator(np.random.Philox(key=[31, sum(map(ord, name))]))
    return torch.from_numpy(g.standard_normal((B, L, cfg["CLASSIFIER"]["output_size"]), dtype=np.float32))


def loss_fn(kind: str, logits: torch.Tensor, emotion: torch.Tensor, R: torch.Tensor) -> torch.Tensor:
    if kind == "ce":
        crit = torch.nn.CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
        return crit(logits.permute(0, 2, 1), emotion)
    return (logits * R).sum()
