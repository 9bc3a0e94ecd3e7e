"""Float64 references of the two fp32 kernels the in-loop encoders' token path starts with (TEST INFRASTRUCTURE ONLY): the token-level
attention of csrc/attention.hip (m2f_attention_long_fwd) and the embedding LayerNorm of csrc/rowops.hip (m2f_embed_layernorm).  Plain
tensor ops, no nn.*; pinned on the CPU by tests/test_token_attention_ref_cpu.py.  `dtype=torch.float32` evaluates the same formulas
in fp32 - the yardstick for inputs whose fp32 error no project bound covers."""
import math

import torch


def scores(q, k, H, dtype=torch.float64):
    """q / k [B, S, H*hd] -> q k^T / sqrt(hd) as [B, H, S(query), S(key)]"""
    B, S, E = q.shape
    hd = E // H
    qh = q.to(dtype).view(B, S, H, hd).permute(0, 2, 1, 3)
    kh = k.to(dtype).view(B, S, H, hd).permute(0, 2, 1, 3)
    return qh @ kh.transpose(-1, -2) / math.sqrt(hd)


def token_attention(q, k, v, key_pad, H, dtype=torch.float64):
    """q / k / v [B, S, H*hd], key_pad [B, S] (nonzero = padded key) or None -> (softmax(q k^T / sqrt(hd) + mask) v as [B, S, H*hd],
    largest |score| between a query at an unpadded position and an unpadded key).  A row whose keys are all padded is 0: the kernel's
    documented behaviour (torch's masked softmax gives NaN there)."""
    B, S, E = q.shape
    hd = E // H
    pad = torch.zeros(B, S, dtype=torch.bool) if key_pad is None else key_pad.bool()
    sc = scores(q, k, H, dtype)
    masked = sc.masked_fill(pad[:, None, None, :], float("-inf"))
    m = masked.max(-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(masked - m)                                         # exp(-inf) = 0 at the padded keys
    den = e.sum(-1, keepdim=True)
    p = torch.where(den > 0, e / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(e))
    vh = v.to(dtype).view(B, S, H, hd).permute(0, 2, 1, 3)
    out = (p @ vh).permute(0, 2, 1, 3).reshape(B, S, E)
    live = ~pad
    pair = (live[:, None, :, None] & live[:, None, None, :]).expand_as(sc)
    top = sc[pair].abs().max().item() if pair.any() else 0.0
    return out, top


def embed_layernorm(ids, pos_ids, word, pos, type_row0, gamma, beta, eps, dtype=torch.float64):
    """LayerNorm(word[ids] + pos[pos_ids] + type_row0) * gamma + beta with the two-pass (centred) variance; ids / pos_ids int64 [T]"""
    x = word.to(dtype)[ids] + pos.to(dtype)[pos_ids] + type_row0.to(dtype)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma.to(dtype) + beta.to(dtype)
