"""Operands for the exact GEMM suite (tests/test_gemm_exact_cpu.py checks the premises, tests/test_gemm_exact_gpu.py uses them).

* Small integers in [-4, 4] are exact in fp32, bf16 and e4m3; every partial sum of a product of K <= 2^19 / 16 of them stays
  below 2^24, so ANY fp32 summation order gives the float64 result exactly and a correct kernel matches it bit for bit.
* Power-of-two row / column scales keep that property: each output is an integer multiple of the smallest scale product.
* Epilogue terms (bias, residual, accumulated C) are integers up to 2^12: exact in fp32 but NOT in bf16 (8 significant bits), so a
  term added after a rounding to bf16 moves the result.
* Rounding probes: fp32 values at, just below and just above bf16 / e4m3 rounding ties.  A one-hot operand turns a GEMM into a
  copy of the rounded other operand.
"""
import numpy as np
import torch

MAX_K = 2048                 # the largest reduction the GPU suite runs (keeps |partial sums| <= 16 * MAX_K < 2^24)
TERM = 4096                  # epilogue terms: integers in [-TERM, TERM]


def ints(shape, seed, lo=-4, hi=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def pow2(n, seed, lo=-3, hi=3):
    """n power-of-two scales 2^e, e in [lo, hi]."""
    g = torch.Generator().manual_seed(seed)
    return torch.pow(2.0, torch.randint(lo, hi + 1, (n,), generator=g).float())


def terms(shape, seed):
    return ints(shape, seed, -TERM, TERM)


def one_hot(n, k, seed):
    """[n, k] with exactly one 1 per row, at perm[i] (distinct positions while n <= k): B of a GEMM that copies A's columns."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(k, generator=g)[:n] if n <= k else torch.randint(0, k, (n,), generator=g)
    b = torch.zeros(n, k)
    b[torch.arange(n), perm] = 1.0
    return b, perm


def _f32(bits):
    return torch.tensor(np.array(bits, dtype=np.uint32).view(np.float32))


# upper halves (sign, exponent, 7 stored mantissa bits) of the bf16 probes: both parities of the kept last bit, both signs,
# exponents from the smallest normal up to 2^100 (nothing that rounds to inf)
BF16_HI = [0x3F80, 0x3F81, 0xBF80, 0xBF81, 0x4110, 0x4111, 0xC4FE, 0xC4FF, 0x0080, 0x0081, 0x8080, 0x8081, 0x7176, 0x7177,
           0x2A55, 0x2A56]
BF16_LO = [0x7FFF, 0x8000, 0x8001, 0x0001, 0x0000, 0xFFFF, 0x4000, 0xC000]


def bf16_probes():
    """-> (fp32 values, kind) where kind: 0 below a tie, 1 at a tie, 2 above a tie, 3 other."""
    bits, kind = [], []
    for hi in BF16_HI:
        for lo in BF16_LO:
            bits.append((hi << 16) | lo)
            kind.append({0x7FFF: 0, 0x8000: 1, 0x8001: 2}.get(lo, 3))
    for b in (0x3FFFFFFF, 0xBFFFFFFF, 0x3F7FFFFF, 0x3F7F8000, 0x407F8000, 0x00FF8000, 0x00800000, 0x00808000):
        bits.append(b)                                          # carries into the exponent; the smallest normal bf16
        kind.append(1 if (b & 0xFFFF) == 0x8000 else 3)
    return _f32(bits), torch.tensor(kind)


def bf16_subnormal_probes():
    """fp32 subnormals at, below and above bf16 ties, and the bf16 subnormals themselves."""
    bits = [0x00008000, 0x00018000, 0x00017FFF, 0x00018001, 0x007F8000, 0x007FFFFF, 0x00010000, 0x80018000, 0x807F7FFF, 0x00000001]
    return _f32(bits)


def bf16_overflow_probes():
    """values whose bf16 rounding is or is next to the largest finite bf16 / inf (converters only: 0 x inf poisons a GEMM row)."""
    return _f32([0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7EFFFF, 0xFF7F8000, 0xFF7FFFFF, 0x7F800000, 0xFF800000])


def fp24_probes(n, seed):
    """fp32 values with full 24-bit mantissas (low 16 bits nonzero), exponents within +-20: what fp32 mode must pass through unchanged."""
    g = torch.Generator().manual_seed(seed)
    mant = torch.randint(1 << 23, 1 << 24, (n,), generator=g).double() / (1 << 23)
    e = torch.randint(-20, 21, (n,), generator=g).double()
    s = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    return (s * mant * torch.pow(2.0, e)).float()


E4M3_MAX = 448.0


def e4m3_grid():
    """every finite non-negative e4m3 value, ascending"""
    v = torch.arange(0, 256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    v = v[torch.isfinite(v) & (v >= 0)]
    return torch.unique(v)


def e4m3_probes():
    """midpoints between neighbouring e4m3 values (ties), their fp32 neighbours, both signs, the subnormal range, and the
    values beyond +-448 that saturate."""
    g = e4m3_grid().double()
    mid = ((g[1:] + g[:-1]) / 2).float()
    below = torch.nextafter(mid, torch.zeros_like(mid))
    above = torch.nextafter(mid, torch.full_like(mid, 1e9))
    v = torch.cat([mid, below, above, torch.tensor([448.0, 449.0, 464.0, 480.0, 1000.0, 1e30])])
    return torch.cat([v, -v])


def round_bf16_trunc(x):
    """fp32 -> bf16 by truncation (a wrong staging rule the suite must catch)"""
    b = x.contiguous().view(torch.int32) & ~0xFFFF
    return b.view(torch.float32)


def round_bf16_half_away(x):
    """fp32 -> bf16 rounding half away from zero (another wrong rule)"""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    b = (b + 0x8000) & 0xFFFF0000
    b = torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32)
    return b.view(torch.float32)
