"""Reference for the context band of the dialogue attention (M2FNet(context=(past, future)), functional.attention_fwd(past=, future=)).

`attention` is oracle.m2fnet_oracle.attention's statements plus two things: the band - query position i sees key position j only if
j >= i - past and j <= i + future, each side None = unlimited - and the rule for a query that sees no key at all (a pad slot whose
band holds pad keys only): its probabilities are zero and so is its output row, where a plain masked softmax gives NaN.  `swapped_in`
puts it in the oracle's place while a test runs the oracle's `forward` / `loss_and_grads` (the oracle looks `attention` up at call
time), so every attention site of the oracle's model - both encoders, every fusion layer - gets the band, and the oracle file stays
as it is.  tests/test_context_window_cpu.py pins `attention` against torch.nn.MultiheadAttention / nn.TransformerEncoderLayer with
attn_mask= on the rows that see a key.
"""
from __future__ import annotations

import contextlib
import math
from typing import Optional, Tuple

import torch
from torch import Tensor

Band = Tuple[Optional[int], Optional[int]]


def band_mask(L: int, past: Optional[int], future: Optional[int]) -> Tensor:
    """bool [L, L], [i, j] True = key j is HIDDEN from query i (torch's attn_mask convention)."""
    i = torch.arange(L)[:, None]
    j = torch.arange(L)[None, :]
    hidden = torch.zeros(L, L, dtype=torch.bool)
    if past is not None:
        hidden |= j < i - past
    if future is not None:
        hidden |= j > i + future
    return hidden


def attention(q: Tensor, k: Tensor, v: Tensor, key_pad: Tensor, n_head: int, return_probs: bool = False, drop=None, name: str = "",
              band: Band = (None, None)):
    """oracle.m2fnet_oracle.attention under a band.  A query with no visible key: P = 0, output row 0, no gradient."""
    B, L, E = q.shape
    hd = E // n_head
    qh = q.reshape(B, L, n_head, hd).permute(0, 2, 1, 3)
    kh = k.reshape(B, L, n_head, hd).permute(0, 2, 1, 3)
    vh = v.reshape(B, L, n_head, hd).permute(0, 2, 1, 3)
    s = (qh @ kh.transpose(-1, -2)) * (1.0 / math.sqrt(hd))
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


def visible_rows(key_pad: Tensor, band: Band) -> Tensor:
    """bool [B, L]: the query slots that see at least one key (every valid slot; pad slots depend on the band)."""
    L = key_pad.shape[1]
    hidden = key_pad[:, None, :] | band_mask(L, *band).to(key_pad.device)[None]
    return ~hidden.all(dim=-1)


@contextlib.contextmanager
def swapped_in(band: Band):
    """Inside the block oracle.m2fnet_oracle.attention is `attention` with this band."""
    from oracle import m2fnet_oracle as O
    plain = O.attention

    def banded(q, k, v, key_pad, n_head, return_probs=False, drop=None, name=""):
        return attention(q, k, v, key_pad, n_head, return_probs, drop, name, band)

    O.attention = banded
    try:
        yield
    finally:
        O.attention = plain
