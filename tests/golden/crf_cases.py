"""Inputs shared by tests/test_crf_cpu.py and tests/test_crf_kernels_gpu.py (CPU tensors from fixed seeds; the GPU tests move them)."""
import torch

VITERBI_L = [1, 2, 3, 16, 17, 64, 65, 200, 512]
VITERBI_C, VITERBI_B = 7, 2
GAP = 1e-3                    # positions whose float64 max-marginal gap is below this are decided by rounding: not compared
MAX_EXCLUDED = 0.01           # ... and at most this share of the positions may be such


def params_block(C, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C * C + 2 * C, generator=g) * scale


def viterbi_case(L):
    """logits [B, L, C] ~ 2 N(0, 1), mask [B, L] (20 % True, never the first row of dialogue 0), params ~ N(0, 1)."""
    g = torch.Generator().manual_seed(7000 + L)
    logits = torch.randn(VITERBI_B, L, VITERBI_C, generator=g) * 2.0
    mask = torch.rand(VITERBI_B, L, generator=g) < 0.2
    mask[0, 0] = False
    return logits, mask, params_block(VITERBI_C, 7100 + L)


def nll_case(C, B, L, packed, seed, logit_scale=2.0, param_scale=1.0):
    """One batch of the loss tests -> dict(logits [T, C], labels [T], params, spans [(r0, r1)], cu (int32 [B+1] or None), B, L, T).
    padded: rows b*L + i.  packed: dialogue lengths in 1..L (the first one L), rows by cu_seqlens, and 3 rows behind the last
    dialogue that belong to nobody.  30 % of the labels are -1; dialogue 1 (B > 1) is unlabelled as a whole, and dialogue 0 (L >= 3)
    has a -1 in its middle."""
    g = torch.Generator().manual_seed(seed)
    if packed:
        lens = torch.randint(1, L + 1, (B,), generator=g)
        lens[0] = L
        cu = torch.zeros(B + 1, dtype=torch.int32)
        cu[1:] = torch.cumsum(lens, 0).to(torch.int32)
        T = int(cu[-1]) + 3
        spans = [(int(cu[b]), int(cu[b + 1])) for b in range(B)]
    else:
        cu, T = None, B * L
        spans = [(b * L, b * L + L) for b in range(B)]
    logits = torch.randn(T, C, generator=g) * logit_scale
    labels = torch.randint(0, C, (T,), generator=g)
    labels[torch.rand(T, generator=g) < 0.3] = -1
    if packed:
        labels[int(cu[-1]):] = -1
    if B > 1:
        labels[spans[1][0]: spans[1][1]] = -1
    if L >= 3:
        r0 = spans[0][0]
        labels[r0] = 0
        labels[r0 + 1] = -1
        labels[r0 + 2] = C - 1
    if B == 1 and L == 1:
        labels[0] = 1
    return {"logits": logits, "labels": labels, "params": params_block(C, seed + 1, param_scale), "spans": spans, "cu": cu,
            "B": B, "L": L, "T": T, "C": C}
