"""The two fp32 kernels at the head of the in-loop encoders' token path, each against its float64 reference (tests/golden/token_attention_ref.py)
at the kernel level: functional.attention_long_fwd (csrc/attention.hip m2f_attn_long_fwd_kernel, the m2f_attention_long_fwd C entry) and
functional.embed_layernorm (csrc/rowops.hip m2f_embed_ln_kernel, m2f_embed_layernorm).

Attention (grid: tests/golden/token_attention_cases.py): head dims 8 / 12 / 20 / 64 / 80 / 96 / 128 on the float4 staging path (packed and
wider pitches; 96 and 128 take the opt-in LDS launch, 128 all eight output tiles), 25 / 75, a leading dimension of 3d + 1 and operands one
float off a 16-byte boundary on the generic one; S = 1 / 63 / 64 / 65 / 130 / 200; no mask, ragged tails, holes, a fully padded first key
block, a fully padded sequence; padded rows of q / k / v around 1e4; randn scores, scores up to +-50, key orders whose block maxima rise
in every block or never.  Every case: the result against float64, finite everywhere, a NaN-filled output pitch left alone, a second launch
and every sequence launched alone bit-identical, and (float4 path) the same values through an unaligned copy bit-identical.
Embedding LayerNorm: d = 4 / 64 / 252 / 256 / 260 / 768 / 1024 / 2048, T = 1 / 5 / 8, output pitches d and d + 4, the first and last rows of
both tables, ordinary tables and tables offset by +50 (mean 150 against a spread of 0.17), the bf16 shadow of every result.

Bounds, none taken from the kernels: randn / ordinary data - the project's bounds for the same arithmetic, 2e-5 of max |ref| (attention,
tests/test_kernels_gpu.py::test_attention_forward_backward) and 1e-5 (LayerNorm forward, test_layernorm_forward_backward); large-score and
offset data - max(that, 4 * e32), e32 = the distance of the same formula evaluated by torch in fp32 on the CPU to the float64 result.

Measured on MI355X, distances relative to max |ref| (each test prints e32 and the kernel's): attention, randn: kernel 0 (S = 1) - 8.9e-7, e32
0 - 6.3e-7; sharp: kernel 8.2e-7 - 2.3e-6 against e32 1.6e-6 - 5.2e-6 (bounds 2.0e-5 - 2.1e-5); rising / first: kernel 2.3e-6 - 6.5e-6 against
e32 3.3e-6 - 8.5e-6 (bounds 2.0e-5 - 3.4e-5).  Embedding LayerNorm, ordinary: kernel 7e-8 - 1.9e-7, e32 5e-8 - 1.8e-7; offset: kernel 3.2e-5 -
5.0e-5 (d >= 64) and 2.1e-4 (d = 4) against e32 3.8e-5 - 5.4e-5 and 2.1e-4 (bounds 1.5e-4 - 2.2e-4 and 8.3e-4).  The whole file: 70 tests, 2.6 s.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import token_attention_cases as TC  # noqa: E402
import token_attention_ref as TR  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402
from mer_amd import runtime  # noqa: E402

DEV = "cuda"
TOL_ATTN, TOL_EMBED = 2e-5, 1e-5
PITCH_ATTN, PITCH_EMBED = 8, 4          # NaN columns behind the result's own
SENTINEL = 777.0                        # what a bf16 shadow holds before a launch (exact in bf16)
EPS = 1e-5

_REF = {}


def _ref(c):
    """one float64 reference per case, shared by every test that needs it: (q, k, v), key_pad, ref [T, d], bound, e32"""
    if c not in _REF:
        (q, k, v), kp = TC.attn_inputs(c)
        ref, _ = TR.token_attention(q, k, v, kp, c.H)
        r32, _ = TR.token_attention(q, k, v, kp, c.H, dtype=torch.float32)
        e32 = (r32.double() - ref).abs().max().item() / ref.abs().max().item()
        tol = TOL_ATTN if c.family == "randn" else max(TOL_ATTN, 4.0 * e32)
        _REF[c] = ((q, k, v), kp, ref.reshape(c.B * c.S, -1), tol, e32)
    return _REF[c]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _place(c, qkv, unaligned=False):
    """q | k | v column slices of one device buffer in the case's layout; the pitch columns hold NaN (nothing may read them)"""
    T, d = c.B * c.S, c.H * c.hd
    ld = TC.leading_dim(c)
    off = 1 if unaligned or c.layout == "offset1" else 0
    flat = torch.full((T * ld + 4,), float("nan"), device=DEV)
    assert flat.data_ptr() % 16 == 0
    buf = flat[off: off + T * ld].view(T, ld)
    for i, t in enumerate(qkv):
        buf[:, i * d: (i + 1) * d] = t.reshape(T, d).to(DEV)
    q, k, v = (buf[:, i * d: (i + 1) * d] for i in range(3))
    assert (q.data_ptr() % 16 == 0) == (off == 0) and q.stride(0) == ld
    return q, k, v


def _launch(c, q, k, v, kp, B=None):
    """-> (the NaN-prefilled [T, d + PITCH] buffer, the [T, d] view the wrapper returns)"""
    B = c.B if B is None else B
    full = torch.full((B * c.S, c.H * c.hd + PITCH_ATTN), float("nan"), device=DEV)
    out = F.attention_long_fwd(q, k, v, kp, B, c.S, c.H, out=full)
    assert out.data_ptr() == full.data_ptr() and out.shape == (B * c.S, c.H * c.hd) and out.stride(0) == full.stride(0)
    return full, out


def _pitch_untouched(full, d):
    return torch.equal(_bits(full[:, d:]), _bits(torch.full_like(full[:, d:], float("nan"))))


@pytest.mark.parametrize("c", TC.ATTN_CASES, ids=TC.case_id)
def test_fp32_token_attention_against_float64(c):
    qkv, kp, ref, tol, e32 = _ref(c)
    B, S, d = c.B, c.S, c.H * c.hd
    q, k, v = _place(c, qkv)
    kpd = None if kp is None else kp.to(DEV)
    full, out = _launch(c, q, k, v, kpd)
    assert torch.isfinite(out).all(), "a padded key, a pitch column or an unwritten element reached the result"
    assert _pitch_untouched(full, d), "the store guard let a column behind H * hd through"
    scale = ref.abs().max().item()
    err = (out.double().cpu() - ref).abs().max().item()
    print(f"attention {TC.case_id(c)}: e32 {e32:.2e}, kernel {err / scale:.2e}, bound {tol:.2e} (of max |ref| = {scale:.3f})")
    assert err <= tol * scale + 1e-7, (err / scale, tol)
    if kp is not None:
        for b in range(B):
            if kp[b].all():
                assert torch.all(out[b * S: (b + 1) * S] == 0), "a fully padded sequence must give zero rows"

    again, out2 = _launch(c, q, k, v, kpd)
    assert torch.equal(_bits(again), _bits(full)), "a second launch gave other bits"
    for b in range(B if B > 1 else 0):
        rows = slice(b * S, (b + 1) * S)
        alone, _ = _launch(c, q[rows], k[rows], v[rows], None if kpd is None else kpd[b: b + 1], B=1)
        assert torch.equal(_bits(alone), _bits(full[rows])), f"sequence {b} alone differs from its rows in the batch"
    if TC.fast_path(c):
        qu, ku, vu = _place(c, qkv, unaligned=True)
        other, _ = _launch(c, qu, ku, vu, kpd)
        assert torch.equal(_bits(other), _bits(full)), "the generic staging path built another LDS image than the float4 path"


def _shadow_map(ws, sh, on):
    runtime.check(runtime.lib().m2f_set_shadow_map(ws.data_ptr() if on else None, sh.data_ptr() if on else None, ws.numel() if on else 0),
                  "m2f_set_shadow_map")


SHADOW_CASES = [next(c for c in TC.ATTN_CASES if c.hd == hd and TC.fast_path(c) and c.S >= 130 and c.mask != "none") for hd in (12, 64, 128)]


@pytest.mark.parametrize("c", SHADOW_CASES, ids=TC.case_id)
def test_attention_shadow_is_the_rounded_fp32_result(c):
    qkv, kp, ref, tol, _ = _ref(c)
    T, d = c.B * c.S, c.H * c.hd
    q, k, v = _place(c, qkv)
    kpd = kp.to(DEV)
    plain, _ = _launch(c, q, k, v, kpd)
    ws = torch.full((T, d + PITCH_ATTN), float("nan"), device=DEV)
    sh = torch.full((T, d + PITCH_ATTN), SENTINEL, dtype=torch.bfloat16, device=DEV)
    _shadow_map(ws, sh, True)
    try:
        out = F.attention_long_fwd(q, k, v, kpd, c.B, c.S, c.H, out=ws)
    finally:
        _shadow_map(ws, sh, False)
    assert torch.equal(_bits(ws), _bits(plain)), "the fp32 result changed under a shadow map"
    assert torch.equal(_bits(sh[:, :d]), _bits(out.to(torch.bfloat16))), "the shadow is not the bf16 rounding of the fp32 result"
    assert torch.all(sh[:, d:] == SENTINEL), "shadow pitch columns were written"
    assert (out.double().cpu() - ref).abs().max().item() <= tol * ref.abs().max().item() + 1e-7
    sh.fill_(SENTINEL)
    F.attention_long_fwd(q, k, v, kpd, c.B, c.S, c.H, out=ws)                  # the map is off again: nothing reaches the shadow
    torch.cuda.synchronize()
    assert torch.all(sh == SENTINEL)


def test_attention_refusals_leave_the_output_alone():
    out = torch.full((8, 2 * 129 + PITCH_ATTN), float("nan"), device=DEV)
    before = _bits(out).clone()
    x = torch.randn(8, 2 * 129, device=DEV)
    with pytest.raises(runtime.HipError):
        F.attention_long_fwd(x, x, x, None, 2, 4, 2, out=out)                   # hd = 129
    e = x[:0, :32]
    with pytest.raises(runtime.HipError):
        F.attention_long_fwd(e, e, e, None, 2, 0, 2, out=out)                   # S = 0
    with pytest.raises(runtime.HipError):
        F.attention_long_fwd(e, e, e, None, 0, 4, 2, out=out)                   # B = 0
    y = x[:, :32]
    with pytest.raises(ValueError):
        F.attention_long_fwd(y, y[:4], y, None, 2, 4, 2, out=out)               # k holds other rows than q
    with pytest.raises(ValueError):
        F.attention_long_fwd(y, y, y, None, 2, 3, 2, out=out)                   # B * S is not the row count
    with pytest.raises(ValueError):
        F.attention_long_fwd(y, y, y, torch.zeros(2, 3, dtype=torch.uint8, device=DEV), 2, 4, 2, out=out)
    with pytest.raises(ValueError):
        F.attention_long_fwd(y, y, y, None, 2, 4, 2, out=out[:, :16])           # narrower than H * hd
    with pytest.raises(ValueError):
        F.attention_long_fwd(y, y, y, None, 2, 4, 3, out=out)                   # 32 columns, 3 heads
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), before)
    got = F.attention_long_fwd(y, y, y, None, 2, 4, 2, out=out)                 # (the same operands are accepted once the sizes agree)
    assert torch.isfinite(got).all() and _pitch_untouched(out, 32)


# ---- embedding LayerNorm ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,T,data", TC.EMBED_CASES)
def test_embed_layernorm_against_float64(d, T, data):
    cpu = TC.embed_inputs(d, T, data)
    ref = TR.embed_layernorm(*cpu, EPS)
    e32 = (TR.embed_layernorm(*cpu, EPS, dtype=torch.float32).double() - ref).abs().max().item() / ref.abs().max().item()
    tol = TOL_EMBED if data == "ordinary" else max(TOL_EMBED, 4.0 * e32)
    dev = [t.to(DEV) for t in cpu]
    scale = ref.abs().max().item()
    first = None
    for pitch in (0, PITCH_EMBED):
        ws = torch.full((T, d + pitch), float("nan"), device=DEV)
        sh = torch.full((T, d + pitch), SENTINEL, dtype=torch.bfloat16, device=DEV)
        _shadow_map(ws, sh, True)
        try:
            out = F.embed_layernorm(*dev, EPS, out=ws)
        finally:
            _shadow_map(ws, sh, False)
        assert out.data_ptr() == ws.data_ptr() and out.shape == (T, d) and out.stride(0) == d + pitch
        assert torch.isfinite(out).all() and _pitch_untouched(ws, d)
        err = (out.double().cpu() - ref).abs().max().item()
        print(f"embed LayerNorm d={d} T={T} {data} pitch {d + pitch}: e32 {e32:.2e}, kernel {err / scale:.2e}, bound {tol:.2e} (of max |ref| = {scale:.3f})")
        assert err <= tol * scale + 1e-7, (err / scale, tol)
        assert torch.equal(_bits(sh[:, :d]), _bits(out.to(torch.bfloat16))), "the shadow is not the bf16 rounding of the fp32 result"
        assert torch.all(sh[:, d:] == SENTINEL)
        first = out.clone() if first is None else first
        assert torch.equal(_bits(out), _bits(first)), "the output pitch changed the result"
        sh.fill_(SENTINEL)
        fresh = F.embed_layernorm(*dev, EPS)                                   # map off, the wrapper's own buffer: same bits, no shadow
        assert torch.equal(_bits(fresh), _bits(first))
        again = F.embed_layernorm(*dev, EPS, out=ws)
        assert torch.equal(_bits(again), _bits(first)) and torch.all(sh == SENTINEL)


def test_embed_layernorm_refusals_leave_the_output_alone():
    def args(d, T=5):
        return [t.to(DEV) for t in TC.embed_inputs(d, T, "ordinary")]
    for d, cols, T in ((6, 8, 5), (2052, 2052, 5), (64, 65, 5), (64, 64, 0)):       # d % 4, d > 2048, ld_out = d + 1, T = 0
        out = torch.full((5, cols), float("nan"), device=DEV)
        a = args(d)
        if T == 0:
            a[0], a[1] = a[0][:0], a[1][:0]
        with pytest.raises(runtime.HipError):
            F.embed_layernorm(*a, EPS, out=out)
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), (d, cols, T)
    a = args(64)
    out = torch.full((5, 64), float("nan"), device=DEV)
    for bad in (0, 1):
        b = list(a)
        b[bad] = b[bad].clone()
        b[bad][2] = (TC.EMBED_VOCAB, TC.EMBED_MAX_POS)[bad]                        # one past the table
        with pytest.raises(ValueError):
            F.embed_layernorm(*b, EPS, out=out)
    with pytest.raises(ValueError):
        F.embed_layernorm(a[0], a[1][:4], *a[2:], EPS, out=out)
    with pytest.raises(ValueError):
        F.embed_layernorm(*a, EPS, out=out[:, :32])
    with pytest.raises(ValueError):
        F.embed_layernorm(*a, EPS, out=out[:4])
    assert torch.isnan(out).all()


def test_the_grid_holds_the_cases_it_must():
    A = TC.ATTN_CASES
    lds = {hd: 3 * 64 * ((hd + 15) // 16 * 16 + 2) * 4 for hd in (80, 96, 128)}
    assert lds[80] <= 64 * 1024 < lds[96] < lds[128] <= 160 * 1024
    for hd in (8, 12, 20, 64, 80, 96, 128):                                       # float4 path: each is also run through an unaligned copy
        assert any(c.hd == hd and TC.fast_path(c) for c in A), hd
    assert any(c.hd == 128 and c.S == 200 for c in A)
    for hd in (25, 75):
        assert any(c.hd == hd and not TC.fast_path(c) for c in A), hd
    assert any(c.hd == 64 and c.layout == "ld+1" for c in A) and any(c.hd == 64 and c.layout == "offset1" for c in A)
    assert {1, 63, 64, 65, 130, 200} <= {c.S for c in A}
    assert {"none", "ragged", "holes", "lead64", "dead", "lead64+dead"} <= {c.mask for c in A}
    assert any("lead64" in c.mask and c.S == 130 for c in A)                        # a fully padded leading block, live blocks behind it
    assert any("dead" in c.mask and TC.key_pad(c)[1].all() and not TC.key_pad(c)[0].all() for c in A)     # a fully padded sequence among live ones
    assert {"randn", "sharp", "rising", "first"} <= {c.family for c in A}
    assert all(c.S == 200 for c in A if c.family in ("rising", "first"))
    assert all(c.B <= 3 and c.H <= 3 and c.B * c.S <= 600 for c in A)
    assert any(TC.leading_dim(c) > 3 * c.H * c.hd and c.layout == "pad8" for c in A)
    assert {c.hd for c in SHADOW_CASES} == {12, 64, 128}
    E = TC.EMBED_CASES
    assert {4, 252, 2048} <= {d for d, _, _ in E} and {1, 5, 8} <= {T for _, T, _ in E}
    assert all((d, T, "ordinary") in E for d in TC.EMBED_WIDTHS for T in TC.EMBED_ROWS) and any(data == "offset" for _, _, data in E)
