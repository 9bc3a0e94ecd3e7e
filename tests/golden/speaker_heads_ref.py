"""Reference for speaker-aware attention heads (M2FNet(speaker_heads=(n_same, n_other)), functional.attention_fwd(speakers=,
speaker_heads=)).

`head_class(h, heads)` is the rule: head h < n_same is a SAME-speaker head (query utterance i sees key j only if speakers[b, j] ==
speakers[b, i]; the utterance itself always qualifies), n_same <= h < n_same + n_other an OTHER-speaker head (only if they differ), the
rest are untouched.  `speaker_hidden` is that rule as a boolean [B, H, L, L] (True = hidden) - the per-head `attn_mask` torch's modules
would be given.  `attention` is position_bias_ref.attention's statements with that condition ORed into `hidden`, per head, so the
probabilities are [B, H, L, L]; the distance term applies to whatever stays visible; a query that sees no key has P = 0 and a zero
output row.  `swapped_in(band, gain, speakers, heads)` puts it in oracle.m2fnet_oracle.attention's place while a test runs the oracle
(the oracle looks it up at call time and hands no speakers on, so the context manager closes over the batch's [B, L] tensor; its file
stays as it is).  tests/test_speaker_heads_cpu.py pins `attention` against torch.nn.MultiheadAttention / nn.TransformerEncoderLayer
with a boolean attn_mask [B*H, L, L] on the rows that see a key.
"""
from __future__ import annotations

import contextlib
import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from band_ref import Band, band_mask
from position_bias_ref import applied_gain, bias_term

NONE, SAME, OTHER = 0, 1, 2
Heads = Optional[Tuple[int, int]]


def head_class(h: int, heads: Heads) -> int:
    if heads is None:
        return NONE
    n_same, n_other = heads
    return SAME if h < n_same else (OTHER if h < n_same + n_other else NONE)


def speaker_hidden(speakers: Tensor, n_head: int, heads: Heads) -> Tensor:
    """bool [B, H, L, L]: True where head h hides key j from query i on account of the speakers alone."""
    B, L = speakers.shape
    same = speakers[:, :, None] == speakers[:, None, :]                                               # [B, i, j]
    out = torch.zeros(B, n_head, L, L, dtype=torch.bool, device=speakers.device)
    for h in range(n_head):
        c = head_class(h, heads)
        if c == SAME:
            out[:, h] = ~same
        elif c == OTHER:
            out[:, h] = same
    return out


def attention(q: Tensor, k: Tensor, v: Tensor, key_pad: Tensor, n_head: int, return_probs: bool = False, drop=None, name: str = "",
              band: Band = (None, None), gain: float = 0.0, speakers: Optional[Tensor] = None, heads: Heads = None):
    """position_bias_ref.attention with the speaker condition in `hidden`, per head.  A query with no visible key: P = 0, output row 0."""
    B, L, E = q.shape
    hd = E // n_head
    qh = q.reshape(B, L, n_head, hd).permute(0, 2, 1, 3)
    kh = k.reshape(B, L, n_head, hd).permute(0, 2, 1, 3)
    vh = v.reshape(B, L, n_head, hd).permute(0, 2, 1, 3)
    s = (qh @ kh.transpose(-1, -2)) * (1.0 / math.sqrt(hd))
    if gain:
        s = s + bias_term(L, n_head, gain, s.dtype).to(s.device)[None]
    hidden = (key_pad[:, None, None, :] | band_mask(L, *band).to(key_pad.device)[None, None]).expand(B, n_head, L, L)   # [B, H, L, L]
    if heads is not None:
        hidden = hidden | speaker_hidden(speakers.to(key_pad.device), n_head, heads)
    s = s.masked_fill(hidden, float("-inf"))
    empty = hidden.all(dim=-1, keepdim=True)                                                          # [B, H, L, 1]
    m = s.max(dim=-1, keepdim=True).values
    s = s - torch.where(empty, torch.zeros_like(m), m)          # (an empty row stays -inf: exp gives 0, not exp(-inf + inf))
    p = torch.exp(s)
    den = p.sum(dim=-1, keepdim=True)
    p = p / torch.where(empty, torch.ones_like(den), den)
    o = ((p if drop is None else drop(name, p)) @ vh).permute(0, 2, 1, 3).reshape(B, L, E)
    return (o, p) if return_probs else o


@contextlib.contextmanager
def swapped_in(band: Band, gain: Optional[float], speakers: Optional[Tensor], heads: Heads):
    """Inside the block oracle.m2fnet_oracle.attention is `attention` with this band, the APPLIED gain and these speakers / heads."""
    from oracle import m2fnet_oracle as O
    plain = O.attention
    g = applied_gain(gain)

    def aware(q, k, v, key_pad, n_head, return_probs=False, drop=None, name=""):
        return attention(q, k, v, key_pad, n_head, return_probs, drop, name, band, g, speakers, heads)

    O.attention = aware
    try:
        yield
    finally:
        O.attention = plain
