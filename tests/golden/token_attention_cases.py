"""The case grid and the deterministic inputs of tests/test_text_encoder_kernels_gpu.py (TEST INFRASTRUCTURE ONLY).  They live here, apart
from the GPU test, so that tests/test_token_attention_ref_cpu.py can check without a GPU that every constructed input is what it claims
to be (the score cap of the sharp inputs, the block order of the ordered ones, the saturated rows of the padded queries)."""
from collections import namedtuple

import torch

import token_attention_ref as TR

SCORE_CAP = 60.0          # the float64 reference's largest |score| of a sharp / ordered input stays at or below this ...
SHARP_TARGET = 50.0       # ... the generators aim here ("in the tens")
PAD_VALUE = 1.0e4         # magnitude of what sits in padded token rows of q / k / v
PAD_GAP = 30.0            # a padded query's best score leads its second best by at least this (see _fill_pads)

# layout: how q | k | v sit in memory.  "packed" [T, 3d], "pad8" [T, pad8(3d) + 8 * (3d % 8 == 0)] (a pitch wider than the rows), both on the
# float4 staging path when hd % 4 == 0; "ld+1" [T, 3d + 1] and "offset1" (packed, the buffer starting one float behind a 16-byte
# boundary): the generic staging path whatever the head dim
# mask: "none" (key_pad = None), "ragged", "holes", "lead64" (sequence 0: keys 0..63 padded), "dead" (sequence 1: every key padded),
# "lead64+dead"
# family: "randn", "sharp" (q scaled until the largest |score| is SHARP_TARGET), "rising" (block maxima grow block after block for every
# query), "first" (the global maximum of every query sits in key block 0)
AttnCase = namedtuple("AttnCase", "B S H hd layout mask family")

ATTN_CASES = [
    # ---- the float4 staging path, every head-dim class ----
    AttnCase(2, 1, 3, 8, "packed", "none", "randn"),             # CT = 1, 2 k-steps, a single key
    AttnCase(2, 65, 2, 8, "pad8", "ragged", "randn"),
    AttnCase(2, 63, 3, 12, "pad8", "holes", "randn"),            # 3 k-steps (odd tail), W = 16 > hd
    AttnCase(3, 130, 3, 12, "packed", "lead64+dead", "randn"),
    AttnCase(2, 64, 3, 20, "pad8", "ragged", "randn"),           # 5 k-steps, W = 32 > hd
    AttnCase(2, 200, 1, 20, "packed", "none", "randn"),
    AttnCase(3, 130, 2, 64, "packed", "lead64+dead", "randn"),   # the encoders' head dim
    AttnCase(2, 1, 2, 64, "packed", "none", "randn"),
    AttnCase(2, 200, 1, 64, "pad8", "holes", "randn"),
    AttnCase(2, 65, 2, 80, "packed", "ragged", "randn"),         # the largest default-LDS size
    AttnCase(2, 63, 1, 80, "pad8", "none", "randn"),
    AttnCase(2, 130, 2, 96, "packed", "lead64", "randn"),        # the first opt-in LDS size
    AttnCase(3, 64, 1, 96, "pad8", "dead", "randn"),
    AttnCase(2, 200, 2, 128, "packed", "ragged", "randn"),       # CT = 8, the stated limit
    AttnCase(3, 64, 1, 128, "packed", "dead", "randn"),
    AttnCase(1, 1, 2, 128, "packed", "none", "randn"),
    AttnCase(2, 65, 1, 128, "pad8", "holes", "randn"),
    # ---- the generic staging path ----
    AttnCase(2, 130, 3, 25, "packed", "holes", "randn"),         # hd % 4 != 0
    AttnCase(3, 1, 2, 25, "packed", "none", "randn"),
    AttnCase(3, 64, 2, 25, "packed", "dead", "randn"),
    AttnCase(2, 65, 2, 75, "packed", "ragged", "randn"),
    AttnCase(1, 200, 1, 75, "packed", "lead64", "randn"),
    AttnCase(2, 130, 2, 64, "ld+1", "ragged", "randn"),          # a leading dimension of 3d + 1
    AttnCase(2, 63, 2, 64, "offset1", "none", "randn"),          # one float behind a 16-byte boundary
    # ---- large scores ----
    AttnCase(2, 200, 2, 64, "packed", "ragged", "sharp"),
    AttnCase(2, 200, 2, 128, "packed", "none", "sharp"),
    AttnCase(2, 130, 3, 12, "pad8", "lead64", "sharp"),
    AttnCase(2, 65, 2, 25, "packed", "ragged", "sharp"),
    AttnCase(1, 200, 2, 128, "packed", "none", "rising"),
    AttnCase(1, 200, 2, 25, "packed", "none", "rising"),
    AttnCase(1, 200, 2, 128, "packed", "none", "first"),
    AttnCase(1, 200, 2, 20, "pad8", "none", "first"),
]


def case_id(c):
    return f"B{c.B}-S{c.S}-H{c.H}-hd{c.hd}-{c.layout}-{c.mask}-{c.family}"


def fast_path(c):
    """the kernel's slab_fast_ok for this case's operands"""
    return c.hd % 4 == 0 and c.layout in ("packed", "pad8")


def leading_dim(c):
    d3 = 3 * c.H * c.hd
    if c.layout == "pad8":
        return (d3 + 7) // 8 * 8 + (8 if d3 % 8 == 0 else 0)
    return d3 + 1 if c.layout == "ld+1" else d3


def key_pad(c):
    """uint8 [B, S] (1 = padded) or None"""
    B, S = c.B, c.S
    if c.mask == "none":
        return None
    kp = torch.zeros(B, S, dtype=torch.uint8)

    def ragged(b, n):
        kp[b, max(1, min(n, S)):] = 1

    def holes(b):
        for i in range(1, S - 1):
            if i % 5 == 2 or i % 7 == b + 3:
                kp[b, i] = 1
    tails = [S - 1, S // 2 + 1, S // 3]
    if c.mask == "ragged":
        for b in range(B):
            ragged(b, tails[b])
    elif c.mask == "holes":
        for b in range(B):
            holes(b)
    else:
        assert c.mask in ("lead64", "dead", "lead64+dead") and ("lead64" not in c.mask or S > 64) and ("dead" not in c.mask or B >= 2)
        for b in range(B):
            if b == 0 and "lead64" in c.mask:
                kp[0, :64] = 1
            elif b == 1 and "dead" in c.mask:
                kp[1, :] = 1
            elif b == 0:
                ragged(0, tails[0])
            elif b == 1:
                ragged(1, tails[1])
            else:
                holes(b)
    return kp


def _fill_pads(q, k, v, kp, H, g):
    """Padded token rows hold finite values around PAD_VALUE: a padded key that leaks into a sum shows as an O(1) error or worse.
    The QUERIES at padded positions then have scores of the order of PAD_VALUE against the live keys, where an fp32 product carries an
    absolute error around PAD_VALUE * 2^-24 * sqrt(hd) ~ 1e-2 whatever the summation order - their softmax is a contract only where
    it is saturated.  So a padded query row is drawn again until its best live key leads the second best by PAD_GAP in every head
    (p_second <= e^-30: the row's output is its best key's value row to the last bit, in fp32 as in float64)."""
    pad = kp.bool()
    n = int(pad.sum())
    if n == 0:
        return
    E = q.shape[-1]
    for t in (q, k, v):
        t[pad] = PAD_VALUE * torch.randn(n, E, generator=g)
    for _ in range(64):
        sc = TR.scores(q, k, H).masked_fill(pad[:, None, None, :], float("-inf"))
        if sc.shape[-1] < 2:
            return
        top2 = sc.topk(2, dim=-1).values
        gap = top2[..., 0] - top2[..., 1]                                  # inf with one live key, nan with none
        close = (gap < PAD_GAP).any(1) & pad                               # [B, S]: padded queries with a near tie in some head
        if not close.any():
            return
        q[close] = PAD_VALUE * torch.randn(int(close.sum()), E, generator=g)
    raise AssertionError("padded query rows keep a near tie")


def attn_inputs(c):
    """-> (q, k, v) float32 [B, S, H*hd] on the CPU, key_pad uint8 [B, S] or None"""
    B, S, H, hd = c.B, c.S, c.H, c.hd
    E = H * hd
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(case_id(c))))
    kp = key_pad(c)
    if c.family in ("rising", "first"):
        # one direction u per head: keys a_j u + noise, queries sqrt(hd) u + noise -> score(i, j) = a_j + O(0.1 (1 + |a_j| / sqrt(hd)))
        u = torch.randn(H, hd, generator=g)
        u = u / u.norm(dim=-1, keepdim=True)
        a = torch.linspace(-28.0, 28.0, S)
        if c.family == "first":
            a = a.flip(0)
        k = (a[None, :, None, None] * u + 0.1 * torch.randn(B, S, H, hd, generator=g)).reshape(B, S, E)
        q = (hd ** 0.5 * u + 0.1 * torch.randn(B, S, H, hd, generator=g)).reshape(B, S, E)
    else:
        q, k = torch.randn(B, S, E, generator=g), torch.randn(B, S, E, generator=g)
    v = torch.randn(B, S, E, generator=g)
    q, k, v = q.float().contiguous(), k.float().contiguous(), v.float().contiguous()
    if c.family == "sharp":
        _, top = TR.token_attention(q, k, v, kp, H)
        q = (q * (SHARP_TARGET / top)).float()
    if kp is not None:
        _fill_pads(q, k, v, kp, H, g)
    return (q, k, v), kp


# ---- embedding LayerNorm ---------------------------------------------------------------------------------------------------------------
EMBED_WIDTHS = [4, 64, 252, 256, 260, 768, 1024, 2048]
EMBED_ROWS = [1, 5, 8]
EMBED_VOCAB, EMBED_MAX_POS, EMBED_PAD_ID = 11, 9, 1
# (d, T, data): "ordinary" tables as synth_roberta scales them, everywhere; "offset" (every table = 50 + values of spread 0.1: a row's
# mean of 150 against a spread of 0.17, where a one-pass variance E[x^2] - mean^2 has lost every digit) at T = 5
EMBED_CASES = [(d, T, "ordinary") for d in EMBED_WIDTHS for T in EMBED_ROWS] + [(d, 5, "offset") for d in EMBED_WIDTHS]


def embed_inputs(d, T, data):
    """-> ids, pos_ids int64 [T]; word [vocab, d], pos [max_pos, d], type_row0 / gamma / beta [d] float32 (CPU)"""
    g = torch.Generator().manual_seed(7919 * d + 31 * T + (data == "offset"))
    ids = torch.tensor([EMBED_VOCAB - 1, 0, 3, 3, 0, EMBED_VOCAB - 1, 2, 5][:T], dtype=torch.int64)
    pos_ids = torch.tensor([EMBED_MAX_POS - 1, EMBED_PAD_ID, 2, 3, EMBED_PAD_ID, EMBED_MAX_POS - 1, 4, 5][:T], dtype=torch.int64)
    shapes = [(EMBED_VOCAB, d), (EMBED_MAX_POS, d), (d,)]
    if data == "offset":
        word, pos, type_row0 = (50.0 + 0.1 * torch.randn(*s, generator=g) for s in shapes)
    else:
        word, pos, type_row0 = (0.5 * torch.randn(*s, generator=g) for s in shapes)
    gamma, beta = 1.0 + 0.1 * torch.randn(d, generator=g), 0.05 * torch.randn(d, generator=g)
    return ids, pos_ids, word, pos, type_row0, gamma, beta
