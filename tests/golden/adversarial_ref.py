"""Host replica of the adversarial ascent on the input embeddings (csrc/adversarial.hip), for tests only.

`ascend` states the definition in plain torch, in whatever dtype it is handed: float64 is the reference, float32 "the same statements
in plain fp32 torch" whose distance from float64 sets the tests' bound.  `uniform_start` is the device's uniform start of the
perturbation, bit for bit: the dropout hash (dropout_ref.mix32 / site_key - the hash behind m2f_keep's decision) of element row * d + col
under a site of its own, turned into a number in [-1, 1) and scaled once.  Nothing here is imported by the product."""
from __future__ import annotations

import numpy as np
import torch

from dropout_ref import U32, mix32, site_key

SITE_TEXT, SITE_AUDIO = 0xAD510001, 0xAD510002


def keep_hash(key, idx):
    """The 32-bit hash m2f_keep compares with its threshold: mix32(mix32(idx * 0x9E3779B1 + key) ^ (key >> 7) ^ 0x68E31DA4)."""
    key = U32(key)
    with np.errstate(over="ignore"):
        h = mix32(np.asarray(idx, dtype=np.uint64).astype(U32) * U32(0x9E3779B1) + key)
        return mix32(h ^ (key >> U32(7)) ^ U32(0x68E31DA4))


def uniform_unit(state4, site, rows, d):
    """float32 [len(rows), d]: 2 * (h >> 8) * 2^-24 - 1 for the token rows `rows` of a [T, d] matrix - exact in fp32."""
    r = np.asarray(rows, dtype=np.uint64)
    idx = ((r[:, None] * np.uint64(d) + np.arange(d, dtype=np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)).astype(U32)
    h = keep_hash(site_key(state4, site), idx)
    return ((h >> U32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)).astype(np.float32)


def uniform_start(state4, site, rows, d, init_mag):
    """delta_0 of the rows: fp32(init_mag / sqrt(d)), formed in float64 and rounded once, times `uniform_unit` - one fp32 multiply."""
    scale = np.float32(float(init_mag) / np.sqrt(float(d)))
    return (scale * uniform_unit(state4, site, rows, d)).astype(np.float32)


def ascend(x_clean, g, delta, key_pad, epsilon, step_size, norm, dtype=torch.float64):
    """(delta', x) of one ascent step in `dtype`: u = g / ||g||, cand = delta + step_size * u (a zero or non-finite norm: cand = delta),
    delta' = cand * min(1, epsilon / ||cand||) (a zero norm: cand), x = x_clean + delta'.  norm "utterance": the row's L2 norm; "batch":
    the L2 norm over all rows with key_pad False.  Rows with key_pad True keep their delta and x_clean.  [T, d] tensors on the CPU."""
    xc, dl = x_clean.to(dtype), delta.to(dtype)
    gg = torch.zeros_like(dl) if g is None else g.to(dtype)
    live = ~key_pad.bool()
    eps, step = torch.tensor(epsilon, dtype=dtype), torch.tensor(step_size, dtype=dtype)

    def l2(t):
        if norm == "batch":
            return (t[live] ** 2).sum().sqrt().expand(t.shape[0])[:, None]
        return (t ** 2).sum(-1, keepdim=True).sqrt()

    ng = l2(gg)
    move = torch.isfinite(ng) & (ng > 0)
    u = torch.where(move, gg / torch.where(move, ng, torch.ones_like(ng)), torch.zeros_like(gg))
    cand = torch.where(move, dl + step * u, dl)
    nc = l2(cand)
    clip = nc > eps
    new = torch.where(clip, cand * (eps / torch.where(clip, nc, torch.ones_like(nc))), cand)
    new = torch.where(live[:, None], new, dl)
    return new, torch.where(live[:, None], xc + new, xc)
