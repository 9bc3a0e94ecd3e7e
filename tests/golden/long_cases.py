"""Long-dialogue cases (more than 64 utterances per dialogue) of long_dialogues.npz, shared by make_golden_long.py and the GPU
tests: seeded configs, inputs and the standalone FusionAttentionModule case, all built from synth.py."""
from __future__ import annotations

import numpy as np
import torch

import synth

# name -> (config.model dict, B, L, dialogue lengths)
CASES = {
    "long_tiny": (synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2), 4, 110, [110, 97, 64, 1]),
    # hd = 300 / 12 = 25 (audio, fusion) and 300 / 5 = 60 (text); one past a 64-row block boundary
    "long_odd_heads": (synth._cfg(300, 300, 300, 12, 5, 12, 1, 1, 1, hid=40), 3, 129, [129, 50, 2]),
    "long_512": (synth._cfg(32, 32, 32, 2, 2, 2, 1, 1, 1), 2, 512, [512, 300]),
    # every dialogue full-length: the packed plan has exactly B * L rows (no spare row)
    "long_full": (synth._cfg(32, 48, 32, 2, 4, 2, 1, 1, 1), 2, 128, [128, 128]),
}
FULL_GRAD = {"long_tiny", "long_full"}          # full gradients (tensors up to 32,768 elements) and the three-step Adam record

# standalone FusionAttentionModule: the weights of long_tiny's first fusion layer, padded keys, output on every row
FAM_B, FAM_L, FAM_LENGTHS = 3, 100, [100, 37, 80]


def inputs(name):
    cfg, B, L, lengths = CASES[name]
    return (cfg,) + synth.make_inputs(cfg, B, L, lengths, "randn")


def fam_case():
    """(E, n_head, fusion-layer state dict, text [B,L,E], audio [B,L,E], key_pad bool [B,L])."""
    cfg = CASES["long_tiny"][0]
    E, H = cfg["FAM"]["embedding_size"], cfg["FAM"]["n_head"]
    sd = synth.make_state_dict(cfg)
    pre = "fusion_layers.0."
    w = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
    g = np.random.Generator(np.random.Philox(key=[23, 0]))
    text = torch.from_numpy(g.standard_normal((FAM_B, FAM_L, E), dtype=np.float32))
    audio = torch.from_numpy(g.standard_normal((FAM_B, FAM_L, E), dtype=np.float32) * np.float32(0.5))
    key_pad = torch.zeros(FAM_B, FAM_L, dtype=torch.bool)
    for b, n in enumerate(FAM_LENGTHS):
        key_pad[b, n:] = True
    return E, H, w, text, audio, key_pad
