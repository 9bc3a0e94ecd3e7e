"""Premises of tests/test_gemm_exact_gpu.py, checked without a GPU.

* Exactness: integer operands (and power-of-two scaled ones) give products that fp32 sums exactly in ANY order, so a kernel's result
  may be compared with the float64 reference bit for bit.
* The rounding probes are what they claim to be: at a bf16 / e4m3 tie torch's rounding (nearest even) differs from truncation and
  from rounding half away from zero.
* Sensitivity: emulated kernel faults fail the exact comparison; the ones the old bf16 bound (1.5e-2 of the output scale, against the
  unrounded fp32 product, tests/test_kernels_gpu.py) lets through are named in the output.
"""
import numpy as np
import pytest
import torch

import exact_gemm as X

OLD_TOL = 1.5e-2


def _sum_orders(a, b):
    """[M, N] products of float32 a [M, K], b [N, K] summed in float32: k ascending, k descending, and 8 interleaved chunks."""
    p = a[:, None, :].astype(np.float32) * b[None, :, :].astype(np.float32)     # exact: |a b| <= 16 (times a power of two)
    up = np.zeros(p.shape[:2], np.float32)
    for k in range(p.shape[2]):
        up = (up + p[:, :, k]).astype(np.float32)
    down = np.zeros(p.shape[:2], np.float32)
    for k in reversed(range(p.shape[2])):
        down = (down + p[:, :, k]).astype(np.float32)
    parts = [np.cumsum(p[:, :, j::8], axis=2, dtype=np.float32)[:, :, -1] for j in range(8)]
    chunked = np.zeros(p.shape[:2], np.float32)
    for q in parts[::-1]:
        chunked = (chunked + q).astype(np.float32)
    return up, down, chunked


@pytest.mark.parametrize("scaled", [False, True])
def test_integer_operands_are_summed_exactly_in_any_order(scaled):
    K = X.MAX_K
    a, b = X.ints((6, K), 1).numpy(), X.ints((5, K), 2).numpy()
    a[0] = 4.0; b[0] = 4.0; b[1] = -4.0                       # the largest partial sums the generator allows
    sa, sb = (X.pow2(6, 3).numpy(), X.pow2(5, 4).numpy()) if scaled else (np.ones(6, np.float32), np.ones(5, np.float32))
    a, b = a * sa[:, None], b * sb[:, None]
    ref = a.astype(np.float64) @ b.astype(np.float64).T
    for got in _sum_orders(a, b):
        assert np.array_equal(got.astype(np.float64), ref)
    # every output: an integer multiple of ONE power of two (its row scale x its column scale), under 2^24 of them
    q = ref / (sa[:, None].astype(np.float64) * sb[None, :])
    assert np.array_equal(q, np.round(q)) and np.abs(q).max() <= 16 * K < 2 ** 24
    if scaled:
        assert len(np.unique(sa)) > 1 and len(np.unique(sb)) > 1


def test_epilogue_terms_are_exact_in_fp32_and_not_in_bf16():
    t = X.terms((4096,), 5)
    assert torch.equal(t.double(), t.double().round()) and t.abs().max() <= X.TERM
    assert (t.to(torch.bfloat16).float() != t).float().mean() > 0.5


def test_bf16_probes_are_ties_and_their_neighbours():
    v, kind = X.bf16_probes()
    bits = v.view(torch.int32) & 0xFFFF
    assert torch.equal(bits[kind == 0], torch.full_like(bits[kind == 0], 0x7FFF))
    assert torch.equal(bits[kind == 1], torch.full_like(bits[kind == 1], 0x8000))
    assert torch.equal(bits[kind == 2], torch.full_like(bits[kind == 2], 0x8001))
    assert torch.isfinite(v.to(torch.bfloat16).float()).all()                       # nothing here rounds to inf
    assert (v.abs() >= 2.0 ** -126).all()                                          # ... or below the normal range
    rne, tr, away = v.to(torch.bfloat16).float(), X.round_bf16_trunc(v), X.round_bf16_half_away(v)
    tie = kind == 1
    even = ((v.view(torch.int32) >> 16) & 1) == 0
    assert (rne[tie & even] != away[tie & even]).all()      # a tie with an even kept bit: nearest even keeps it, half-away rounds up
    assert (rne[tie & ~even] == away[tie & ~even]).all()
    assert (rne[kind == 2] != tr[kind == 2]).all()          # above a tie: truncation is one bf16 step short
    assert (rne[kind == 0] == tr[kind == 0]).all()
    carry = v.view(torch.int32) == 0x3FFFFFFF
    assert rne[carry].item() == 2.0                          # a carry into the exponent
    assert v.view(torch.int32).eq(0x00808000).any()          # a tie at the smallest normal bf16
    sub = X.bf16_subnormal_probes()
    assert (sub.abs() < 2.0 ** -126).all() and (sub != 0).all()
    ovf = X.bf16_overflow_probes().to(torch.bfloat16).float()
    assert torch.isinf(ovf).sum() >= 4 and torch.isfinite(ovf).sum() >= 2


def test_fp24_probes_do_not_survive_bf16():
    v = X.fp24_probes(4096, 7)
    assert ((v.view(torch.int32) & 0xFFFF) != 0).float().mean() > 0.99
    assert (v.to(torch.bfloat16).float() != v).float().mean() > 0.99


def test_e4m3_probes_are_ties_and_their_neighbours():
    v = X.e4m3_probes()
    grid = X.e4m3_grid()
    assert grid.max().item() == X.E4M3_MAX and len(grid) == 127
    mids = v[:len(grid) - 1]
    r = mids.to(torch.float8_e4m3fn).float()
    lo_hi = torch.stack([grid[:-1], grid[1:]], 1)
    assert ((r == lo_hi[:, 0]) | (r == lo_hi[:, 1])).all()
    # nearest even: the result's last mantissa bit is 0 at every tie
    code = mids.to(torch.float8_e4m3fn).view(torch.uint8)
    assert ((code & 1) == 0).all()
    trunc = lo_hi[:, 0]
    assert (r != trunc).any() and (r == trunc).any()         # ties that round up and ties that round down
    clamped = v.clamp(-X.E4M3_MAX, X.E4M3_MAX).to(torch.float8_e4m3fn).float()
    assert torch.isfinite(clamped).all() and clamped.abs().max().item() == X.E4M3_MAX


# ---- sensitivity: emulated faults against the exact check and against the old bound ----------------------------------------

def _old_bound_ok(got, ref):
    return (got - ref).abs().max().item() <= OLD_TOL * max(ref.abs().max().item(), 1e-6) + 1e-7


def _fault_truncating_staging():
    """bf16 staging that truncates: caught by the one-hot probe GEMM; on random data (test_gemm_layouts' (512, 768, 768)) the
    error stays inside the old bound."""
    v, _ = X.bf16_probes()
    b, perm = X.one_hot(v.numel(), v.numel(), 3)
    exact_new = torch.equal(X.round_bf16_trunc(v)[perm], v.to(torch.bfloat16).float()[perm])
    g = torch.Generator().manual_seed(1)
    a, w = torch.randn(512, 768, generator=g), torch.randn(768, 768, generator=g)
    ref = a.double() @ w.double().t()
    got = X.round_bf16_trunc(a).double() @ X.round_bf16_trunc(w).double().t()
    return exact_new, _old_bound_ok(got, ref)


def _fault_term_rounded(term):
    def f():
        g = torch.Generator().manual_seed(2)
        M, N, K = 256, 192, 300
        a, w = X.ints((M, K), 11), X.ints((N, K), 12)
        t = X.terms((M, N) if term != "bias" else (N,), 13)
        acc = a.double() @ w.double().t()
        exact = acc + t.double()
        faulty = acc + t.to(torch.bfloat16).double()
        a2, w2 = torch.randn(512, 768, generator=g), torch.randn(768, 768, generator=g)
        t2 = torch.randn((512, 768) if term != "bias" else (768,), generator=g)
        ref = a2.double() @ w2.double().t() + t2.double()
        got = a2.to(torch.bfloat16).double() @ w2.to(torch.bfloat16).double().t() + t2.to(torch.bfloat16).double()
        return torch.equal(exact, faulty), _old_bound_ok(got, ref)
    return f


def _fault_dropped_k_tail():
    """the last element of a ragged k tail is never multiplied (K = 3 * 64 + 5)"""
    M, N, K = 128, 96, 197
    a, w = X.ints((M, K), 21), X.ints((N, K), 22)
    exact = a.double() @ w.double().t()
    faulty = a[:, :-1].double() @ w[:, :-1].double().t()
    g = torch.Generator().manual_seed(3)
    a2, w2 = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    ref = a2.double() @ w2.double().t()
    got = a2[:, :-1].double() @ w2[:, :-1].double().t()
    return torch.equal(exact, faulty), _old_bound_ok(got, ref)


def _fault_write_past_n():
    """an edge tile stores one column past N: the result itself is right; only the guard band shows it"""
    M, N, ld = 70, 50, 53
    buf = torch.full((M + 2, ld), float("nan"))
    out = buf[1:M + 1, :N]
    ref = X.ints((M, N), 31)
    out.copy_(ref)
    buf[1:M + 1, N] = 1.0                                    # the stray store
    guard = torch.ones_like(buf, dtype=torch.bool)
    guard[1:M + 1, :N] = False
    guard_ok = bool(torch.isnan(buf[guard]).all())
    return torch.equal(out, ref) and guard_ok, _old_bound_ok(out.double(), ref.double())


FAULTS = {"truncating_staging": _fault_truncating_staging, "bias_added_as_bf16": _fault_term_rounded("bias"),
          "residual_added_as_bf16": _fault_term_rounded("res"), "accumulate_added_as_bf16": _fault_term_rounded("acc"),
          "dropped_k_tail_element": _fault_dropped_k_tail, "store_past_n": _fault_write_past_n}
# faults the 1.5e-2 bound of tests/test_kernels_gpu.py does not see (measured here; asserted so that the record stays true)
MISSED_BY_OLD_BOUND = {"truncating_staging", "bias_added_as_bf16", "residual_added_as_bf16", "accumulate_added_as_bf16",
                       "store_past_n"}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_emulated_fault_is_caught_by_the_exact_check(fault):
    new_passes, old_passes = FAULTS[fault]()
    print(f"\n{fault}: exact check {'MISSES' if new_passes else 'catches'} it; old 1.5e-2 bound "
          f"{'misses' if old_passes else 'catches'} it")
    assert not new_passes
    assert old_passes == (fault in MISSED_BY_OLD_BOUND)
