"""Reference for the distance-decay attention bias (ALiBi: M2FNet(position_bias=gain), functional.attention_fwd(bias=gain)).

`slopes(H, gain)` is the recipe in float64: head h of H (0-based) has slope gain * base(h, H); with n = 2^floor(log2 H),
base = 2^(-8 (h + 1) / n) for h < n and 2^(-4 (2 (h - n) + 1) / n) for h >= n.  `attention` is band_ref.attention's statements plus one
term: a key's score gets -slope_h * |i - j| (i, j: positions inside the dialogue) before the keys are hidden, so a hidden key stays
-inf.  `applied_gain` rounds a requested gain to bf16 the way the launch descriptors hold it - the gain every comparison against the
kernels uses.  `swapped_in(band, gain)` puts `attention` in oracle.m2fnet_oracle.attention's place while a test runs the oracle (the
oracle looks it up at call time; its file stays as it is).  tests/test_position_bias_cpu.py pins `attention` against
torch.nn.MultiheadAttention / nn.TransformerEncoderLayer with a float attn_mask on the rows that see a key.
"""
from __future__ import annotations

import contextlib
import math
from typing import Optional

import torch
from torch import Tensor

from band_ref import Band, band_mask


def applied_gain(gain: Optional[float]) -> float:
    """The gain as the kernels apply it: None -> 0, otherwise rounded to bf16 (round to nearest even), as a Python float."""
    if gain is None:
        return 0.0
    return float(torch.tensor(float(gain), dtype=torch.float32).to(torch.bfloat16).to(torch.float64))


def slopes(H: int, gain: float = 1.0) -> Tensor:
    """float64 [H]: gain * base(h, H).  `gain` is used as given (pass `applied_gain(g)` to compare with the kernels)."""
    n = 1 << (int(H).bit_length() - 1)
    base = [2.0 ** (-8.0 * (h + 1) / n) if h < n else 2.0 ** (-4.0 * (2 * (h - n) + 1) / n) for h in range(H)]
    return torch.tensor(base, dtype=torch.float64) * float(gain)


def bias_term(L: int, H: int, gain: float, dtype=torch.float64) -> Tensor:
    """[H, L, L]: -slope_h * |i - j| - the float attn_mask torch's modules would be given."""
    i = torch.arange(L)[:, None]
    j = torch.arange(L)[None, :]
    return (-(slopes(H, gain)[:, None, None]) * (i - j).abs().to(torch.float64)[None]).to(dtype)


def attention(q: Tensor, k: Tensor, v: Tensor, key_pad: Tensor, n_head: int, return_probs: bool = False, drop=None, name: str = "",
              band: Band = (None, None), gain: float = 0.0):
    """band_ref.attention with the distance term on every visible key.  A query with no visible key: P = 0, output row 0."""
    B, L, E = q.shape
    hd = E // n_head
    qh = q.reshape(B, L, n_head, hd).permute(0, 2, 1, 3)
    kh = k.reshape(B, L, n_head, hd).permute(0, 2, 1, 3)
    vh = v.reshape(B, L, n_head, hd).permute(0, 2, 1, 3)
    s = (qh @ kh.transpose(-1, -2)) * (1.0 / math.sqrt(hd))
    if gain:
        s = s + bias_term(L, n_head, gain, s.dtype).to(s.device)[None]
    hidden = key_pad[:, None, None, :] | band_mask(L, *band).to(key_pad.device)[None, None]          # [B, 1, L, L]
    s = s.masked_fill(hidden, float("-inf"))
    empty = hidden.all(dim=-1, keepdim=True)                                                          # [B, 1, L, 1]
    m = s.max(dim=-1, keepdim=True).values
    s = s - torch.where(empty, torch.zeros_like(m), m)          # (an empty row stays -inf: exp gives 0, not exp(-inf + inf))
    p = torch.exp(s)
    den = p.sum(dim=-1, keepdim=True)
    p = p / torch.where(empty, torch.ones_like(den), den)
    o = ((p if drop is None else drop(name, p)) @ vh).permute(0, 2, 1, 3).reshape(B, L, E)
    return (o, p) if return_probs else o


@contextlib.contextmanager
def swapped_in(band: Band, gain: Optional[float]):
    """Inside the block oracle.m2fnet_oracle.attention is `attention` with this band and the APPLIED gain."""
    from oracle import m2fnet_oracle as O
    plain = O.attention
    g = applied_gain(gain)

    def biased(q, k, v, key_pad, n_head, return_probs=False, drop=None, name=""):
        return attention(q, k, v, key_pad, n_head, return_probs, drop, name, band, g)

    O.attention = biased
    try:
        yield
    finally:
        O.attention = plain
