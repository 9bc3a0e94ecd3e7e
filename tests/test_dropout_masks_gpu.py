"""Every kernel that applies a dropout mask, against float64 torch math under the mask the HOST says the kernel must draw
(tests/golden/dropout_ref.py, the integer replica of csrc/common.h's hash).

The other dropout tests take the mask from the code under test (statistics, replay, a mask read back from the output).  Here the
mask comes from outside, so an index built from the leading dimension instead of the logical width, a wrong 1 / (1 - p), a site
or a step counter that does not enter the key as documented, or a mask applied on the wrong side of bias / ReLU / residual all
fail.  Two assertions everywhere a kernel writes the masked value itself:
  (a) out is within the tolerance of ref64 * keep * scale, the rest of the epilogue in its documented order
      (+bias -> relu -> dropout -> +res);
  (b) wherever |ref64| > tol (with ReLU: ref64 > tol), out == 0 exactly iff the replica drops the element (with a residual:
      out == res exactly - the residual is added behind the mask).  The elements (b) skips are under 0.1 % of the output, with
      ReLU the checked set covers at least 40 % of it; both shares are asserted from the reference alone.
Tolerances: the one of the same kernel's no-dropout test in tests/test_kernels_gpu.py / test_attention_long_gpu.py, times the
dropout scale 1 / (1 - p) (the mask multiplies value and error alike).  bf16 GEMMs: the float64 reference rounds the operands to
bf16 as the kernel does and the bound is the 2e-5 that test_skinny_classifier_gemms holds the bf16 kernels to against such a
reference - tighter than the 1.5e-2 of test_gemm_layouts (whose reference is unrounded), and the only way (b)'s 0.1 % share can
be met: 1.5e-2 of the output scale would skip about 8 % of a Gaussian output.
The attention kernels apply the mask to the probabilities, not to what they write: their outputs and dq / dk / dv are checked by
(a) against float64 autograd of softmax * keep * scale @ V (oracle attention with its `drop` hook).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dropout_ref as R  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402
from mer_amd import runtime  # noqa: E402
from oracle import m2fnet_oracle as O  # noqa: E402

DEV = "cuda"
STATE = [123, 456, 7, 0]
P_DROP = 0.4


def _rng(state=STATE):
    return torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in state], dtype=torch.int32, device=DEV)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _bf16(t):
    return t.to(torch.bfloat16).float()


def _tol_abs(ref, tol, p=P_DROP):
    """the no-dropout test's bound (tol x the reference's largest magnitude + 1e-7), times the dropout scale"""
    return (tol * max(ref.abs().max().item(), 1e-6) + 1e-7) * R.thresh_scale(p)[1]


def _check_masked(out, pre64, keep, res64, tol, relu, what, p=P_DROP, check_a=True):
    """(a) and (b) for a kernel that writes dropout(pre) (+ res).  out: the kernel's fp32 result (CPU); pre64: float64 value in
    front of the mask (after bias / ReLU); keep: the replica's bool mask; res64: float64 residual or None."""
    scale = R.thresh_scale(p)[1]
    keep = torch.from_numpy(np.ascontiguousarray(keep))
    want = pre64 * keep.double() * scale + (0.0 if res64 is None else res64)
    tol_abs = _tol_abs(want, tol, p)
    if check_a:
        err = (out.double() - want).abs().max().item()
        assert err <= tol_abs, f"{what}: max err {err:.3e} > {tol_abs:.3e}"
    sure = pre64 > tol_abs if relu else pre64.abs() > tol_abs
    share = sure.double().mean().item()
    if relu:
        assert share >= 0.40, f"{what}: only {share:.3f} of the output is checked by (b)"
    else:
        assert 1.0 - share < 1e-3, f"{what}: (b) skips {1 - share:.5f} of the output"
    zero = (out == 0) if res64 is None else (out == res64.float())
    wrong = (zero != ~keep) & sure
    assert not wrong.any(), (f"{what}: {int(wrong.sum())} of {int(sure.sum())} elements are dropped / kept against the replica's mask "
                            f"(first at {tuple(wrong.nonzero()[0].tolist())})")
    assert 0.5 < keep.double().mean().item() / (1 - p) < 1.5            # (the mask is not degenerate)


# ---------------------------------------------------------------------------------------------------------------------------------
# GEMM epilogue
# ---------------------------------------------------------------------------------------------------------------------------------
FORMS = {
    "fp32_tile64": dict(precision=runtime.F32, tile=64),
    "fp32_tile128": dict(precision=runtime.F32, tile=128),
    "bf16_src16_tile64": dict(precision=runtime.BF16, tile=64, src16=True),
    "fp32_split_k": dict(precision=runtime.F32, tile=64, split_k=True),
}
GEMM_TOL = 2e-5          # test_gemm_layouts (fp32); test_skinny_classifier_gemms (bf16 against the operand-rounding reference)


def _gemm_reference(M, N, K, terms, bf16, seed, layout_nn=False):
    a, b = _rand(M, K, seed=seed), _rand(N, K, seed=seed + 1)
    bias, res = (_rand(N, seed=seed + 2), _rand(M, N, seed=seed + 3)) if terms == "all" else (None, None)
    r = _bf16 if bf16 else (lambda t: t)
    pre = r(a).double() @ r(b).double().t()
    if bias is not None:
        pre = torch.relu(pre + bias.double())
    return a, (b.t().contiguous() if layout_nn else b), bias, res, pre


@pytest.mark.parametrize("terms", ["all", "alone"])
@pytest.mark.parametrize("shape", [(70, 50, 45), (129, 300, 64), "column_block"])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_gemm_epilogue_mask_is_the_replicas(form, shape, terms):
    """bias, ReLU and residual together, and dropout alone; C as a column block of a wider matrix (ldc = 64, N = 50): the keep index
    is row * N + col, not row * ldc + col.
    The split-K form runs the same M x N at K = 512: launch_tile (csrc/gemm.hip) gives a slice at least two k-tiles of 64, so the
    K = 45 / 64 of the other forms would not split at all; at 512 these launches (2 and 15 tiles) split four ways, and the mask is
    applied once, by the last-arriving slice, behind the reduce.  That the split ran shows in the bits: the result differs from
    the unsplit kernel's in summation order only (1e-5 of the scale, as test_gemm_split_k_matches_unsplit_and_is_reproducible)."""
    kw = FORMS[form]
    M, N, K = (70, 50, 45) if shape == "column_block" else shape
    if kw.get("split_k"):
        K = 512
    a, b, bias, res, pre = _gemm_reference(M, N, K, terms, kw["precision"] == runtime.BF16, seed=100 + M)
    dev = lambda t: None if t is None else t.to(DEV)          # noqa: E731
    out = None
    if shape == "column_block":
        wide = torch.full((M, 64), 7.0, device=DEV)
        out = wide[:, 8:8 + N]
    c = F.gemm(dev(a), dev(b), F.NT, bias=dev(bias), res=dev(res), relu_out=bias is not None, out=out, drop_site=5, drop_p=P_DROP,
               rng=_rng(), **kw)
    torch.cuda.synchronize()
    if shape == "column_block":
        assert (wide[:, :8] == 7.0).all() and (wide[:, 8 + N:] == 7.0).all(), "columns outside the block were written"
    keep = R.rows_mask(STATE, 5, P_DROP, M, N)
    _check_masked(c.cpu(), pre, keep, None if res is None else res.double(), GEMM_TOL, bias is not None, f"{form} {shape} {terms}")
    if kw.get("split_k"):
        plain = F.gemm(dev(a), dev(b), F.NT, bias=dev(bias), res=dev(res), relu_out=bias is not None, drop_site=5, drop_p=P_DROP,
                       rng=_rng(), **dict(kw, split_k=False))
        assert not torch.equal(plain, c), "the launch did not split along K (same bits as the unsplit kernel)"
        _close(c, plain.double().cpu(), 1e-5, "split against unsplit", p=0.0)


@pytest.mark.parametrize("form", ["fp32_tile64", "bf16_src16_tile64"])
def test_gemm_nn_layout_mask_is_the_replicas(form):
    """layout NN with a site: the backward through the pre-projection dropout (d x = dropout(d xp W))."""
    kw = FORMS[form]
    M, N, K = 70, 50, 45
    a, b_kn, _, _, pre = _gemm_reference(M, N, K, "alone", kw["precision"] == runtime.BF16, seed=300, layout_nn=True)
    c = F.gemm(a.to(DEV), b_kn.to(DEV), F.NN, drop_site=9, drop_p=P_DROP, rng=_rng(), **kw)
    _check_masked(c.cpu(), pre, R.rows_mask(STATE, 9, P_DROP, M, N), None, GEMM_TOL, False, f"NN {form}")


@pytest.mark.parametrize("prec,src16", [(runtime.F32, False), (runtime.BF16, False), (runtime.BF16, True)])
@pytest.mark.parametrize("T,K,ncls", [(300, 768, 7), (37, 50, 3), (1024, 1024, 8)])
def test_skinny_shapes_with_a_site(T, K, ncls, prec, src16):
    """The shapes of test_skinny_classifier_gemms with a dropout site: csrc/skinny.hip has no dropout epilogue and hands such a
    launch on to the MFMA kernels (one column of tiles, N <= 8) - the mask must come out whichever kernel takes it."""
    h, w, bias = _rand(T, K, seed=61), _rand(ncls, K, seed=62) * 0.1, _rand(ncls, seed=63)
    r = _bf16 if prec == runtime.BF16 else (lambda t: t)
    pre = r(h).double() @ r(w).double().t() + bias.double()
    got = F.gemm(h.to(DEV), w.to(DEV), F.NT, prec, bias=bias.to(DEV), src16=src16, drop_site=2, drop_p=P_DROP, rng=_rng())
    _check_masked(got.cpu(), pre, R.rows_mask(STATE, 2, P_DROP, T, ncls), None, GEMM_TOL, False, f"skinny-shaped NT {T}x{ncls}x{K}")


RING_WIDTH = {"128x128": 3328, "128x64": 1344, "64x64": 512}          # tests/test_gemm_ring_gpu.py: WIDTH without 256x128


@pytest.mark.skipif(os.environ.get("M2F_RING", "1") == "0", reason="ring form switched off in the environment")
@pytest.mark.parametrize("form", sorted(RING_WIDTH))
def test_ring_form_mask_is_the_replicas(form):
    """The ring forms that take dropout, at test_gemm_ring_gpu.py's short_k shape (K = 40) with its residual + dropout terms:
    assertion (b).  That file proves the ring forms equal the 64x64 build bit for bit; this pins the chain to the replica."""
    M, N, K = 1024, RING_WIDTH[form], 40
    a, b, res = _rand(M, K, seed=11), _rand(N, K, seed=12), _rand(M, N, seed=13)
    pre = _bf16(a).double() @ _bf16(b).double().t()
    before = runtime.lib().m2f_gemm_ring_launches()
    c = F.gemm(a.to(DEV), b.to(DEV), F.NT, runtime.BF16, src16=True, tile=0, res=res.to(DEV), drop_site=7, drop_p=P_DROP, rng=_rng([11, 22, 3, 0]))
    torch.cuda.synchronize()
    assert runtime.lib().m2f_gemm_ring_launches() == before + 1, "the ring form did not run"
    _check_masked(c.cpu(), pre, R.rows_mask([11, 22, 3, 0], 7, P_DROP, M, N), res.double(), GEMM_TOL, False, f"ring {form}", check_a=False)


def test_rng_advance_carries_into_the_high_word():
    """From step_lo = 0xFFFFFFFF one m2f_rng_advance gives (step_lo, step_hi) = (0, 1), and the mask is the replica's for that
    state (both words enter the key)."""
    rng = _rng([5, 6, 0xFFFFFFFF, 0])
    runtime.check(runtime.lib().m2f_rng_advance(rng.data_ptr(), runtime.stream_ptr()), "m2f_rng_advance")
    assert R.state_of(rng) == [5, 6, 0, 1]
    M, N, K = 70, 50, 45
    a, b, _, _, pre = _gemm_reference(M, N, K, "alone", False, seed=400)
    c = F.gemm(a.to(DEV), b.to(DEV), F.NT, drop_site=3, drop_p=P_DROP, rng=rng, tile=64)
    _check_masked(c.cpu(), pre, R.rows_mask([5, 6, 0, 1], 3, P_DROP, M, N), None, GEMM_TOL, False, "after the carry")
    stale = R.rows_mask([5, 6, 0, 0], 3, P_DROP, M, N)
    assert ((c.cpu() == 0) != ~torch.from_numpy(stale)).float().mean().item() > 0.3, "the high word must change the mask"


# ---------------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------------
def _attn_inputs(B, L, H, hd, lengths, seed, wscale=1.0):
    E = H * hd
    q, k, v, dout = (_rand(B * L, E, seed=seed + i, scale=wscale) for i in range(4))
    key_pad = torch.zeros(B, L, dtype=torch.bool)
    for b, n in enumerate(lengths):
        key_pad[b, n:] = True
    return q, k, v, dout, key_pad


def _attn_reference(q, k, v, dout, key_pad, H, keep, p):
    """float64 autograd of softmax * keep * scale @ V on padded [B, L, E] tensors -> (out, dq, dk, dv) as [B * L, E]."""
    B, L = key_pad.shape
    E = q.shape[1]
    factor = torch.from_numpy(np.ascontiguousarray(keep)).double() * R.thresh_scale(p)[1]
    leaves = [t.double().view(B, L, E).clone().requires_grad_(True) for t in (q, k, v)]
    out = O.attention(*leaves, key_pad, H, drop=lambda name, pr: pr * factor, name="site")
    out.backward(dout.double().view(B, L, E))
    return [out.detach().reshape(B * L, E)] + [t.grad.reshape(B * L, E) for t in leaves]


def _close(got, ref, tol, what, p=P_DROP, floor=1e-6):
    bound = (tol * max(ref.abs().max().item(), floor) + 1e-7) * R.thresh_scale(p)[1]
    err = (got.double().cpu() - ref).abs().max().item()
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


ATTN_SHAPES = [(2, 7, 3, 75, [7, 1]), (3, 33, 4, 15, [33, 17, 1]), (2, 64, 2, 128, [64, 40]), (2, 16, 2, 32, [16, 1])]


@pytest.mark.parametrize("B,L,H,hd,lengths", ATTN_SHAPES)
def test_attention_dropout_forward_backward(B, L, H, hd, lengths):
    """attention.hip (L <= 64): no V = [I | 0] trick, so any head dim; bounds of test_attention_forward_backward (2e-5 / 3e-5)."""
    q, k, v, dout, key_pad = _attn_inputs(B, L, H, hd, lengths, seed=20)
    keep = R.attn_mask(STATE, 3, P_DROP, B, H, L)
    ro, rdq, rdk, rdv = _attn_reference(q, k, v, dout, key_pad, H, keep, P_DROP)
    qd, kd, vd, dd, kp = (t.to(DEV) for t in (q, k, v, dout, key_pad))
    out, probs = F.attention_fwd(qd, kd, vd, kp, B, L, H, drop_site=3, drop_p=P_DROP, rng=_rng())
    _close(out, ro, 2e-5, "out")
    dq, dk, dv = F.attention_bwd(qd, kd, vd, kp, out, probs, dd, B, L, H, drop_site=3, drop_p=P_DROP, rng=_rng())
    for name, g, r in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
        _close(g, r, 3e-5, name)


@pytest.mark.parametrize("form", [1, 63])
@pytest.mark.parametrize("B,L,H,hd,lengths", ATTN_SHAPES)
def test_attention_dropout_bf16_forms(B, L, H, hd, lengths, form, monkeypatch):
    """The bf16-mode forms of the same kernels (M2F_ATTN_BF16_KERNEL: 1 = the head-dim contractions on the bf16 MFMA, 63 = also
    the slabs staged from the operands' bf16 shadows), laid out as test_attention_bf16_mode_forms does (q | k | v and dO | O in one
    workspace that has a shadow), at its bound against the exact result: 3e-2 of the scale."""
    E, T = H * hd, B * L
    ld = (3 * E + 7) // 8 * 8
    q, k, v, dout, key_pad = _attn_inputs(B, L, H, hd, lengths, seed=40, wscale=0.5)
    keep = R.attn_mask(STATE, 4, P_DROP, B, H, L)
    ro, rdq, rdk, rdv = _attn_reference(q, k, v, dout, key_pad, H, keep, P_DROP)
    ws = torch.zeros(2 * T, ld)
    ws[:T, :E], ws[:T, E:2 * E], ws[:T, 2 * E:3 * E], ws[T:, :E] = q, k, v, dout
    ws = ws.to(DEV)
    sh = ws.to(torch.bfloat16).contiguous()
    kp = key_pad.to(DEV)
    valid = ~key_pad.reshape(-1)
    lib = runtime.lib()
    monkeypatch.setenv("M2F_ATTN_BF16_KERNEL", str(form))
    runtime.check(lib.m2f_set_shadow_map(ws.data_ptr(), sh.data_ptr(), ws.numel()), "m2f_set_shadow_map")
    try:
        qd, kd, vd, dd = ws[:T, :E], ws[:T, E:2 * E], ws[:T, 2 * E:3 * E], ws[T:, :E]
        out, probs = F.attention_fwd(qd, kd, vd, kp, B, L, H, drop_site=4, drop_p=P_DROP, rng=_rng())
        o_in = ws[T:, E:2 * E]
        o_in.copy_(out)
        sh[T:, E:2 * E].copy_(out.to(torch.bfloat16))
        dq, dk, dv = F.attention_bwd(qd, kd, vd, kp, o_in, probs, dd, B, L, H, drop_site=4, drop_p=P_DROP, rng=_rng())
        torch.cuda.synchronize()
    finally:
        runtime.check(lib.m2f_set_shadow_map(None, None, 0), "m2f_set_shadow_map")
        monkeypatch.setenv("M2F_ATTN_BF16_KERNEL", "0")
    for name, g, r in (("out", out, ro), ("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
        _close(g.cpu()[valid], r[valid], 3e-2, f"{name} (form {form})")


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "padded"])
@pytest.mark.parametrize("hd", [25, 64])
@pytest.mark.parametrize("L", [65, 129])
def test_long_attention_dropout_forward_backward(L, hd, packed):
    """attention_dlong.hip (L > 64), packed (cu) and padded (key_pad) rows; bounds of test_attention_long_gpu.py (2e-5 / 5e-5 of
    max(scale, 1))."""
    B, H = 3, 3
    lengths = [L, 1, L // 2 + 3]
    q, k, v, dout, key_pad = _attn_inputs(B, L, H, hd, lengths, seed=L + hd, wscale=0.7)
    keep = R.attn_mask(STATE, 6, P_DROP, B, H, L)
    valid = ~key_pad.reshape(-1)
    if packed:
        dout[~valid] = 0            # a packed batch has no pad query rows: nothing flows back from them into dK / dV
    ref = _attn_reference(q, k, v, dout, key_pad, H, keep, P_DROP)
    if packed:
        rows = valid.nonzero()[:, 0]                                # dialogue b's valid slots in order = rows cu[b] ..
        cu = torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32, device=DEV)
        qd, kd, vd, dd = (t[rows].contiguous().to(DEV) for t in (q, k, v, dout))
        kw = dict(cu=cu)
        ref = [r[rows] for r in ref]
    else:
        qd, kd, vd, dd = (t.to(DEV) for t in (q, k, v, dout))
        kw = dict(key_pad=key_pad.to(DEV))
    kw.update(drop_site=6, drop_p=P_DROP, rng=_rng())
    out, probs = F.attention_varlen_fwd(qd, kd, vd, B, L, H, **kw)
    dq, dk, dv = F.attention_varlen_bwd(qd, kd, vd, out, probs, dd, B, L, H, **kw)
    _close(out, ref[0], 2e-5, "out", floor=1.0)
    for name, g, r in (("dq", dq, ref[1]), ("dk", dk, ref[2]), ("dv", dv, ref[3])):
        _close(g, r, 5e-5, name, floor=1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# row-wise kernels
# ---------------------------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(33, 50, 50), (17, 300, 304), (5, 2048, 2048)]          # d % 4 != 0; ld != d; the widest row; partial last row blocks


def _ln_case(T, d, ld, with_res):
    x, g, b = _rand(T, d, seed=60, scale=3.0), 1 + 0.1 * _rand(d, seed=61), 0.1 * _rand(d, seed=62)
    res = _rand(T, d, seed=63) if with_res else None
    dy, extra = _rand(T, d, seed=64), _rand(T, d, seed=65)

    def dev(t):             # rows of stride ld; the pad columns hold a sentinel
        if t is None or t.dim() == 1:
            return None if t is None else t.to(DEV)
        w = torch.full((T, ld), 9.0)
        w[:, :d] = t
        return w.to(DEV)[:, :d]
    return (x, g, b, res, dy, extra), [dev(t) for t in (x, g, b, res, dy, extra)]


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("T,d,ld", LN_SHAPES)
def test_layernorm_forward_site(T, d, ld, with_res):
    """LnProblem::drop_site (the pre-projection dropout on the last stack's final norm): out = dropout(res + LN(x)), keep index
    row * d + col; bound of test_layernorm_forward_backward (1e-5)."""
    (x, g, b, res, _, _), (xd, gd, bd, rd, _, _) = _ln_case(T, d, ld, with_res)
    pre = O.layer_norm(x.double(), g.double(), b.double()) + (0.0 if res is None else res.double())
    out, stats = F.layernorm_fwd_drop(xd, gd, bd, rd, drop_site=4, drop_p=P_DROP, rng=_rng())
    _check_masked(out.cpu(), pre, R.rows_mask(STATE, 4, P_DROP, T, d), None, 1e-5, False, f"ln fwd {T}x{d} ld {ld}")
    plain, stats0 = F.layernorm_fwd_drop(xd, gd, bd, rd)
    assert torch.equal(stats, stats0), "the statistics do not depend on the site"
    if ld == d:
        assert torch.equal(plain, F.layernorm_fwd(xd.contiguous(), gd, bd, None if rd is None else rd.contiguous())[0])


@pytest.mark.parametrize("T,d,ld", LN_SHAPES)
def test_layernorm_backward_masked_output(T, d, ld):
    """LnProblem::drop_site2: dx_masked = LNbwd(dy) * keep * scale next to dx = LNbwd(dy) + extra; dgamma / dbeta must not see the
    site.  Bounds of test_layernorm_forward_backward (2e-5)."""
    (x, g, b, _, dy, extra), (xd, gd, bd, _, dyd, exd) = _ln_case(T, d, ld, False)
    xr, gr, br = (t.double().clone().requires_grad_(True) for t in (x, g, b))
    O.layer_norm(xr, gr, br).backward(dy.double())
    _, stats = F.layernorm_fwd_drop(xd, gd, bd)
    dx, dxm, dg, db = F.layernorm_bwd_masked(xd, gd, stats, dyd, exd, drop_site2=8, drop_p=P_DROP, rng=_rng())
    _check_masked(dxm.cpu(), xr.grad, R.rows_mask(STATE, 8, P_DROP, T, d), None, 2e-5, False, f"ln bwd dx_masked {T}x{d} ld {ld}")
    _close(dx, xr.grad + extra.double(), 2e-5, "dx", p=0.0)
    _close(dg, gr.grad, 2e-5, "dgamma", p=0.0)
    _close(db, br.grad, 2e-5, "dbeta", p=0.0)
    dx0, dxm0, dg0, db0 = F.layernorm_bwd_masked(xd, gd, stats, dyd, exd)
    assert torch.equal(dx, dx0) and torch.equal(dg, dg0) and torch.equal(db, db0), "only dx_masked depends on the site"
    assert torch.equal(dxm0, F.layernorm_bwd_masked(xd, gd, stats, dyd)[0]), "without a site the second output is LNbwd(dy) itself"


def test_dropout_rows_two_buffers_two_sites():
    """m2f_launch_dropout_inplace2 (the two modalities' post-projection gradients in one launch): each buffer under its own site,
    index row * d + col, one fp32 multiplication by the scale (exact), the pad columns d .. ld-1 untouched."""
    T, d, ld = 9, 48, 56
    x0, x1 = _rand(T, ld, seed=70), _rand(T, ld, seed=71)
    b0, b1 = x0.to(DEV), x1.to(DEV)
    F.dropout_rows(b0[:, :d], 11, P_DROP, _rng(), x2=b1[:, :d], site2=12)
    scale = torch.tensor(R.thresh_scale(P_DROP)[1], dtype=torch.float32)
    for x, got, site in ((x0, b0.cpu(), 11), (x1, b1.cpu(), 12)):
        keep = torch.from_numpy(R.rows_mask(STATE, site, P_DROP, T, d))
        want = torch.where(keep, x[:, :d] * scale, torch.zeros(()))
        assert torch.equal(got[:, :d], want), f"site {site}"
        assert torch.equal(got[:, d:], x[:, d:]), "pad columns were written"
    one = x0.to(DEV)
    F.dropout_rows(one[:, :d], 11, P_DROP, _rng())
    assert torch.equal(one, b0), "one buffer alone draws the same mask"
