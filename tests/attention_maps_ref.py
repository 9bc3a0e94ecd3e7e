"""Reference side of the attention-map tests: a recorder that stores the probabilities of every attention site while the oracle's
`forward` runs, and torch-only restatements of the map rules (masked view of the saved P^T, the head average's fixed order, the
stream's causal rows).  No GPU and no kernel of the project is used here.

The oracle looks `attention` up at call time and passes `name=<state_dict prefix of the layer>attn` (oracle/m2fnet_oracle.py:273,300), so
the recorder swaps a wrapper in - the pattern of tests/golden/band_ref.py::swapped_in, which also supplies the banded form - and the
oracle file stays as it is.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

import band_ref

Band = Tuple[Optional[int], Optional[int]]


def site_name(oracle_name: str) -> str:
    """`audio_encoders.0.layers.1.attn` -> `audio_encoders.0.layers.1.self_attn`; `fusion_layers.2.attn` -> `fusion_layers.2.multihead_attention`"""
    assert oracle_name.endswith("attn"), oracle_name
    prefix = oracle_name[: -len("attn")]
    return prefix + ("self_attn" if ".layers." in prefix else "multihead_attention")


@contextlib.contextmanager
def recording(band: Band = (None, None)):
    """Inside the block oracle.m2fnet_oracle.attention stores `(site name, P [B, H, L, L])` per call into the yielded dict (and computes
    under `band`: band_ref.attention; no band: the oracle's own statements)."""
    from oracle import m2fnet_oracle as O
    plain = O.attention
    rec: Dict[str, Tensor] = {}

    def wrapper(q, k, v, key_pad, n_head, return_probs=False, drop=None, name=""):
        if band == (None, None):
            o, p = plain(q, k, v, key_pad, n_head, True, drop, name)
        else:
            o, p = band_ref.attention(q, k, v, key_pad, n_head, True, drop, name, band)
        rec[site_name(name)] = p.detach()
        return (o, p) if return_probs else o

    O.attention = wrapper
    try:
        yield rec
    finally:
        O.attention = plain


def hidden(key_pad: Tensor, L: int, band: Band) -> Tensor:
    """bool [B, 1, i, j]: key j is hidden from query i (a padded key, or outside the band)"""
    return key_pad[:, None, None, :] | band_ref.band_mask(L, *band).to(key_pad.device)[None, None]


def masked_view(probs: Tensor, B: int, H: int, L: int, hide: Tensor) -> Tensor:
    """The saved P^T [B*H, Lp, Lp] as [B, H, i, j], zero where `hide` ([B, 1 or H, i, j])."""
    Lp = probs.shape[-1]
    P = probs.view(B, H, Lp, Lp)[:, :, :L, :L].transpose(-1, -2)
    return torch.where(hide.expand(B, H, L, L), torch.zeros_like(P), P).contiguous()


def head_average(P: Tensor) -> Tensor:
    """[B, H, L, L] -> [B, L, L] by the project's rule: a sequential sum over h = 0 .. H - 1, times fp(1 / H) in P's own precision -
    elementwise torch ops only, one rounding each."""
    acc = P[:, 0]
    for h in range(1, P.shape[1]):
        acc = acc + P[:, h]
    return acc * torch.tensor(1.0, dtype=P.dtype, device=P.device).div(P.shape[1])
