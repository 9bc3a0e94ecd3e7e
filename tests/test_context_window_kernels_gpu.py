"""Context band of the dialogue attention kernels (attention.hip for L <= 64, attention_dlong.hip above; past / future of the C entries) against
tests/golden/band_ref.py under autograd: out / probs / dq / dk / dv, exact zeros at hidden keys, the rows that see no key, the
bf16-mode forms, block skipping over a probabilities buffer that holds another launch's values, blindness to the future bit for bit,
and the unbanded entries unchanged."""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

import band_ref as R  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402
from mer_amd import runtime  # noqa: E402
from mer_amd.runtime import lib, check, ptr, stream_ptr  # noqa: E402

DEV = "cuda"


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _close(a, b, tol, what=""):
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item()
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, bound {tol * scale + 1e-7:.3e}")
    assert err <= tol * scale + 1e-7, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def _key_pad(B, L, lengths):
    kp = torch.zeros(B, L, dtype=torch.bool)
    if lengths:
        for b, n in enumerate(lengths):
            kp[b, n:] = True
    return kp.to(DEV)


def _band(past, future):
    """the issue's integers (negative = unlimited) -> the Python surface's (None = unlimited)"""
    return (None if past < 0 else past, None if future < 0 else future)


def _reference(q, k, v, key_pad, H, band, dout, dtype=torch.float32):
    """band_ref under autograd on [B, L, E] images: (out, P [B, H, i, j], dq, dk, dv)"""
    qr, kr, vr = (t.detach().to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    out, p = R.attention(qr, kr, vr, key_pad, H, return_probs=True, band=band)
    out.backward(dout.to(dtype))
    return out.detach(), p.detach(), qr.grad, kr.grad, vr.grad


def _hidden(key_pad, L, band):
    return key_pad[:, None, None, :] | R.band_mask(L, *band).to(DEV)[None, None]          # [B, 1, i, j]


def _probs_view(probs, B, H, L):
    Lp = probs.shape[-1]
    return probs.view(B, H, Lp, Lp)[:, :, :L, :L].transpose(-1, -2)                        # [B, H, i, j]


# ---- short kernels -----------------------------------------------------------------------------------------------------------------
SHORT = [(3, 16, 2, 32, [16, 5, 1], -1, 0),          # NT = 1, causal
         (2, 33, 4, 15, [33, 17], 2, 0),             # NT = 3, odd head dim, the window crosses 16-column tiles, empty-band pad queries
         (2, 64, 2, 128, [64, 40], 5, 3)]            # NT = 4, two-sided


def _check_short(q, k, v, key_pad, B, L, H, band, seed):
    E = q.shape[1]
    out, probs = F.attention_fwd(q, k, v, key_pad, B, L, H, past=band[0], future=band[1])
    dout = _rand(B * L, E, seed=seed)
    dq, dk, dv = F.attention_bwd(q, k, v, key_pad, out, probs, dout, B, L, H, past=band[0], future=band[1])
    img = lambda t: t.reshape(B, L, E)          # noqa: E731
    ro, rp, rdq, rdk, rdv = _reference(img(q), img(k), img(v), key_pad, H, band, img(dout))
    P = _probs_view(probs, B, H, L)
    _close(img(out), ro, 2e-5, "out")
    _close(P, rp, 2e-5, "probs")
    _close(img(dq), rdq, 3e-5, "dq")
    _close(img(dk), rdk, 3e-5, "dk")
    _close(img(dv), rdv, 3e-5, "dv")
    hidden = _hidden(key_pad, L, band).expand_as(P)
    assert torch.all(P[hidden] == 0), "a hidden key must have probability exactly 0"
    for t in (out, probs, dq, dk, dv):
        assert torch.isfinite(t).all()
    empty = ~R.visible_rows(key_pad, band)                       # [B, L]: queries with no visible key
    assert torch.all(img(out)[empty] == 0) and torch.all(img(dq)[empty] == 0)
    assert torch.all(P.permute(0, 2, 1, 3)[empty] == 0)
    assert torch.all(img(dk)[key_pad] == 0) and torch.all(img(dv)[key_pad] == 0)      # (a pad key is hidden from every query)
    return empty


@pytest.mark.parametrize("B,L,H,hd,lengths,past,future", SHORT)
def test_short_kernels_under_a_band(B, L, H, hd, lengths, past, future):
    E = H * hd
    q, k, v = _rand(B * L, E, seed=20), _rand(B * L, E, seed=21), _rand(B * L, E, seed=22)
    empty = _check_short(q, k, v, _key_pad(B, L, lengths), B, L, H, _band(past, future), 30)
    if (L, past) == (33, 2):
        assert empty.any(), "this case is here for its pad queries with an empty band"


def test_fusion_form_strided_operands_causal():
    """FusionAttentionModule form: q and v live in one [T, 2E] buffer, k in another (src/model.py:14)."""
    B, L, H, hd = 3, 12, 4, 32
    E = H * hd
    qv = _rand(B * L, 2 * E, seed=40)
    k = _rand(B * L, E, seed=41)
    key_pad = torch.zeros(B, L, dtype=torch.bool, device=DEV)
    key_pad[1, 5:] = True
    _check_short(qv[:, :E], k, qv[:, E:], key_pad, B, L, H, (None, 0), 42)


def test_diagonal_only_returns_v_bit_for_bit():
    B, L, H, hd = 2, 9, 2, 24
    E = H * hd
    q, k, v = _rand(B * L, E, seed=20), _rand(B * L, E, seed=21), _rand(B * L, E, seed=22)
    out, probs = F.attention_fwd(q, k, v, _key_pad(B, L, None), B, L, H, past=0, future=0)
    assert torch.equal(out, v)
    P = _probs_view(probs, B, H, L)
    assert torch.equal(P, torch.eye(L, device=DEV).expand(B, H, L, L))


def test_bf16_mode_forms_under_a_band(monkeypatch):
    """The first short case in the forms of test_kernels_gpu.py::test_attention_bf16_mode_forms (M2F_ATTN_BF16_KERNEL = 0, 62 with
    shadows, 63 with shadows), at that test's tolerances, with the band's own properties on top."""
    B, L, H, hd, lengths, past, future = SHORT[0]
    band = _band(past, future)
    ld = 200
    torch.manual_seed(B + hd)
    d, T = H * hd, B * L
    ws = torch.randn(2 * T, ld, device=DEV) * 0.5                     # rows [0, T): packed q | k | v, rows [T, 2T): dO | O
    sh = ws.to(torch.bfloat16).contiguous()
    wr = sh.float()
    kp = _key_pad(B, L, lengths)
    valid = ~kp.reshape(-1)
    hidden = _hidden(kp, L, band).expand(B, H, L, L)

    def shadows(on):
        check(lib().m2f_set_shadow_map(ws.data_ptr() if on else None, sh.data_ptr() if on else None, ws.numel() if on else 0), "m2f_set_shadow_map")

    def run(src, mask, with_shadows):
        q, k, v, do = src[:T, :d], src[:T, d:2 * d], src[:T, 2 * d:3 * d], src[T:, :d]
        monkeypatch.setenv("M2F_ATTN_BF16_KERNEL", str(mask))
        shadows(with_shadows)
        try:
            out, probs = F.attention_fwd(q, k, v, kp, B, L, H, past=band[0], future=band[1])
            o_in = src[T:, d:2 * d]
            o_in.copy_(out)
            if with_shadows:
                sh[T:, d:2 * d].copy_(out.to(torch.bfloat16))
            dq, dk, dv = F.attention_bwd(q, k, v, kp, o_in, probs, do, B, L, H, past=band[0], future=band[1])
        finally:
            shadows(False)
            monkeypatch.setenv("M2F_ATTN_BF16_KERNEL", "0")
        assert torch.all(_probs_view(probs, B, H, L)[hidden] == 0)
        for t in (out, probs, dq, dk, dv):
            assert torch.isfinite(t).all()
        return out, dq, dk, dv

    src0 = ws.clone()
    exact = run(src0, 0, False)
    img = lambda t: t.reshape(B, L, d)          # noqa: E731
    ref = _reference(img(ws[:T, :d]), img(ws[:T, d:2 * d]), img(ws[:T, 2 * d:3 * d]), kp, H, band, img(ws[T:, :d]))
    _close(img(exact[0]), ref[0], 2e-5, "fp32 form, out")
    for a, b, what in zip(exact[1:], ref[2:], ("dq", "dk", "dv")):
        _close(img(a), b, 3e-5, "fp32 form, " + what)
    want = run(wr.clone(), 0, False)                                   # fp32 kernel on bf16-rounded inputs
    got = run(ws, 62, True)                                            # staged from the shadows, exact contractions
    assert torch.equal(got[0][valid], want[0][valid])
    for a, b in zip(got[1:], want[1:]):
        assert (a - b)[valid].abs().max().item() <= 2e-2 * b[valid].abs().max().item()
    both = run(ws, 63, True)                                           # + bf16 contractions
    for a, b, e in zip(both, got, exact):
        scale = e[valid].abs().max().item()
        assert (a - b)[valid].abs().max().item() <= 2e-2 * scale
        assert (a - e)[valid].abs().max().item() <= 3e-2 * scale


# ---- long kernels ------------------------------------------------------------------------------------------------------------------
LONG = [(2, 130, 2, 32, [130, 70], -1, 0),
        (2, 200, 2, 16, [200, 65], 10, 0),           # whole key blocks skippable; padded form: empty-band pad queries
        (1, 512, 1, 16, [512], 3, 70)]               # the future side crosses a block edge


def _long_case(B, L, H, hd, lengths, packed, seed):
    """rows of the launch (packed: the dialogues back to back + 3 rows behind the last; padded: B * L), and how they sit in [B, L]"""
    E = H * hd
    key_pad = _key_pad(B, L, lengths)
    if packed:
        cu = torch.tensor([0] + list(itertools.accumulate(lengths)), dtype=torch.int32)
        T = int(cu[-1]) + 3
        row = torch.full((B, L), T - 1, dtype=torch.long)
        for b, n in enumerate(lengths):
            row[b, :n] = torch.arange(int(cu[b]), int(cu[b]) + n)
        kw = dict(cu=cu.to(DEV))
    else:
        T = B * L
        row = torch.arange(T).view(B, L)
        kw = dict(key_pad=key_pad)
    own = (~key_pad) if packed else torch.ones(B, L, dtype=torch.bool, device=DEV)      # slots whose rows the launch owns
    q, k, v, dout = (_rand(T, E, seed=seed + i) for i in range(4))
    return dict(B=B, L=L, H=H, E=E, T=T, key_pad=key_pad, row=row.to(DEV), own=own, kw=kw, packed=packed, q=q, k=k, v=v, dout=dout)


def _img(c, t):
    """[T, E] rows -> the [B, L, E] image (slots the launch does not own: zeros)"""
    return t[c["row"]] * c["own"][..., None].to(t.dtype)


def _check_long(c, band, out, probs, dq, dk, dv):
    B, L, H = c["B"], c["L"], c["H"]
    ro, rp, rdq, rdk, rdv = _reference(_img(c, c["q"]), _img(c, c["k"]), _img(c, c["v"]), c["key_pad"], H, band, _img(c, c["dout"]))
    own = c["own"]
    _close(_img(c, out)[own], ro[own], 2e-5, "out")
    P = _probs_view(probs, B, H, L).permute(0, 2, 1, 3)          # [B, i, H, j]
    seen = ~_hidden(c["key_pad"], L, band).expand(B, H, L, L).permute(0, 2, 1, 3)
    sel = own[:, :, None, None] & seen                           # (hidden entries of skipped blocks are not written: not compared)
    _close(P[sel], rp.permute(0, 2, 1, 3)[sel], 2e-5, "probs")
    _close(_img(c, dq)[own], rdq[own], 3e-5, "dq")
    _close(_img(c, dk)[own], rdk[own], 3e-5, "dk")
    _close(_img(c, dv)[own], rdv[own], 3e-5, "dv")
    for t in (out, dq, dk, dv):
        assert torch.isfinite(t).all()
    empty = ~R.visible_rows(c["key_pad"], band) & own
    assert torch.all(_img(c, out)[empty] == 0) and torch.all(_img(c, dq)[empty] == 0)
    if c["packed"]:                                              # rows behind the last dialogue: zeros, as ever
        for t in (out, dq, dk, dv):
            assert torch.all(t[c["T"] - 3:] == 0)
    return empty


def _run_long(c, band, probs=None):
    kw = dict(c["kw"], past=band[0], future=band[1])
    out, probs = F.attention_varlen_fwd(c["q"], c["k"], c["v"], c["B"], c["L"], c["H"], probs=probs, **kw)
    dq, dk, dv = F.attention_varlen_bwd(c["q"], c["k"], c["v"], out, probs, c["dout"], c["B"], c["L"], c["H"], **kw)
    return out, probs, dq, dk, dv


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "padded"])
@pytest.mark.parametrize("B,L,H,hd,lengths,past,future", LONG)
def test_long_kernels_under_a_band(B, L, H, hd, lengths, past, future, packed):
    c = _long_case(B, L, H, hd, lengths, packed, seed=60)
    band = _band(past, future)
    got = _run_long(c, band)
    empty = _check_long(c, band, *got)
    # a fresh probabilities buffer is zero where no block was written: every hidden entry is exactly 0 here too
    P = _probs_view(got[1], B, H, L)
    assert torch.all(P[_hidden(c["key_pad"], L, band).expand_as(P)] == 0)
    if (L, past) == (200, 10) and not packed:
        assert empty.any(), "this case is here for its pad queries with an empty band"


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "padded"])
def test_skipped_blocks_of_a_used_probabilities_buffer_are_not_read(packed):
    """A plan's probabilities buffer holds the previous launch's values.  The banded forward skips whole blocks of it; the backward
    must skip the same ones."""
    B, L, H, hd, lengths, past, future = LONG[1]
    band = _band(past, future)
    other = _long_case(B, L, H, hd, lengths, packed, seed=90)
    _, probs = F.attention_varlen_fwd(other["q"], other["k"], other["v"], B, L, H, **other["kw"])      # unbanded, other data
    far = _probs_view(probs, B, H, L)[0, :, 199, 0].clone()
    assert torch.all(far > 0), "the buffer must hold something where the band will skip"
    c = _long_case(B, L, H, hd, lengths, packed, seed=60)
    got = _run_long(c, band, probs=probs)
    assert got[1] is probs and torch.equal(_probs_view(probs, B, H, L)[0, :, 199, 0], far)      # (skipped, not zeroed: no bytes spent)
    _check_long(c, band, *got)
    fresh = _run_long(c, band)
    for a, b in zip((got[0],) + got[2:], (fresh[0],) + fresh[2:]):
        assert torch.equal(a, b)


# ---- blind to the future, bit for bit ------------------------------------------------------------------------------------------------
def test_short_kernel_does_not_see_the_future():
    B, L, H, hd, n = 3, 16, 2, 32, 3
    E = H * hd
    key_pad = _key_pad(B, L, [16, 9, 12])
    q, k, v = _rand(B * L, E, seed=70), _rand(B * L, E, seed=71), _rand(B * L, E, seed=72)
    first, _ = F.attention_fwd(q, k, v, key_pad, B, L, H, past=None, future=0)
    q2, k2, v2 = (t.clone().view(B, L, E) for t in (q, k, v))
    for t, s in zip((q2, k2, v2), (73, 74, 75)):
        t[:, n + 1:] = _rand(B, L - n - 1, E, seed=s, scale=50.0)
    second, _ = F.attention_fwd(q2.view(B * L, E), k2.view(B * L, E), v2.view(B * L, E), key_pad, B, L, H, past=None, future=0)
    assert torch.equal(first.view(B, L, E)[:, :n + 1], second.view(B, L, E)[:, :n + 1])
    assert not torch.equal(first.view(B, L, E)[:, n + 1:], second.view(B, L, E)[:, n + 1:])


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "padded"])
def test_long_kernel_does_not_see_the_future(packed):
    B, L, H, hd, lengths, n = 2, 200, 2, 16, [200, 130], 70
    c = _long_case(B, L, H, hd, lengths, packed, seed=80)
    first, _ = F.attention_varlen_fwd(c["q"], c["k"], c["v"], B, L, H, past=None, future=0, **c["kw"])
    later = torch.zeros(c["T"], dtype=torch.bool, device=DEV)
    later[c["row"][:, n + 1:][c["own"][:, n + 1:]]] = True
    q2, k2, v2 = (t.clone() for t in (c["q"], c["k"], c["v"]))
    for t, s in zip((q2, k2, v2), (83, 84, 85)):
        t[later] = _rand(int(later.sum()), c["E"], seed=s, scale=50.0)
    second, _ = F.attention_varlen_fwd(q2, k2, v2, B, L, H, past=None, future=0, **c["kw"])
    keep = c["own"].clone()
    keep[:, n + 1:] = False
    assert torch.equal(_img(c, first)[keep], _img(c, second)[keep])
    assert not torch.equal(first[later], second[later])


# ---- the entries without a band are what they were -------------------------------------------------------------------------------------
def _ld(t):
    return t.stride(0)


def _no_option():
    """An m2f_attn_opts that states "no option" field by field (the header's M2F_ATTN_OPTS_NONE), where the plain launch passes NULL."""
    return ctypes.byref(runtime.AttnOptsC(past=-1, future=-1, bias_gain=0.0, n_same=0, n_other=0, speakers=None))


def _raw_short(q, k, v, kp, B, L, H, dout, stated):
    E = q.shape[1]
    hd = E // H
    Lp = 16 * ((L + 15) // 16)
    out = torch.empty(B * L, E, device=DEV)
    probs = torch.zeros(B * H, Lp, Lp, device=DEV)
    dq, dk, dv = (torch.zeros(B * L, E, device=DEV) for _ in range(3))
    kp8 = kp.reshape(-1).to(torch.uint8).contiguous()
    check(lib().m2f_attention_fwd(B, L, H, hd, ptr(q), _ld(q), ptr(k), _ld(k), ptr(v), _ld(v), ptr(kp8), ptr(out), _ld(out), ptr(probs), 0,
                                  0.0, None, stream_ptr(), _no_option() if stated else None), "forward")
    check(lib().m2f_attention_bwd(B, L, H, hd, ptr(q), _ld(q), ptr(k), _ld(k), ptr(v), _ld(v), ptr(kp8), ptr(out), _ld(out), ptr(probs),
                                  ptr(dout), _ld(dout), ptr(dq), _ld(dq), ptr(dk), _ld(dk), ptr(dv), _ld(dv), 0, 0.0, None, stream_ptr(),
                                  -1, -1), "backward")
    return out, probs, dq, dk, dv


def _raw_long(c, stated):
    B, L, H, E, T = c["B"], c["L"], c["H"], c["E"], c["T"]
    hd = E // H
    Lp = 16 * ((L + 15) // 16)
    q, k, v, dout = c["q"], c["k"], c["v"], c["dout"]
    out = torch.empty(T, E, device=DEV)
    probs = torch.zeros(B * H, Lp, Lp, device=DEV)
    dq, dk, dv = (torch.zeros(T, E, device=DEV) for _ in range(3))
    cu = c["kw"].get("cu")
    kp8 = None if cu is not None else c["key_pad"].reshape(-1).to(torch.uint8).contiguous()
    check(lib().m2f_attention_varlen_fwd(B, L, H, hd, ptr(q), _ld(q), ptr(k), _ld(k), ptr(v), _ld(v), ptr(cu), T, ptr(kp8), ptr(out), _ld(out),
                                         ptr(probs), 0, 0.0, None, stream_ptr(), _no_option() if stated else None), "forward")
    check(lib().m2f_attention_varlen_bwd(B, L, H, hd, ptr(q), _ld(q), ptr(k), _ld(k), ptr(v), _ld(v), ptr(cu), T, ptr(kp8), ptr(out), _ld(out),
                                         ptr(probs), ptr(dout), _ld(dout), ptr(dq), _ld(dq), ptr(dk), _ld(dk), ptr(dv), _ld(dv), 0, 0.0, None,
                                         stream_ptr(), -1, -1), "backward")
    return out, probs, dq, dk, dv


def test_band_entries_without_a_band_equal_the_plain_entries():
    """opts = NULL and an opts that states no option give equal bits: forward and, from each forward's probabilities, backward (which
    takes the band as two plain arguments, (-1, -1) here); short and long, packed and padded."""
    B, L, H, hd = 2, 33, 4, 15
    E = H * hd
    q, k, v, dout = (_rand(B * L, E, seed=100 + i) for i in range(4))
    kp = _key_pad(B, L, [33, 17])
    for a, b in zip(_raw_short(q, k, v, kp, B, L, H, dout, False), _raw_short(q, k, v, kp, B, L, H, dout, True)):
        assert torch.equal(a, b)
    for packed in (True, False):
        c = _long_case(2, 130, 2, 32, [130, 70], packed, seed=110)
        for a, b in zip(_raw_long(c, False), _raw_long(c, True)):
            assert torch.equal(a, b)
    assert runtime.context_band(None, None) == (-1, -1)
