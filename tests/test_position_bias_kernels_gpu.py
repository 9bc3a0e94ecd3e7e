"""Distance-decay attention bias (ALiBi) at kernel level: functional.attention_fwd / attention_varlen_fwd / attention_stream[_paged] /
attention_stream_chunk[_paged] with bias=gain (bias_gain of the C entries' options; csrc/attention.hip, attention_dlong.hip, attention_stream.hip,
attention_stream_chunk.hip) against tests/golden/position_bias_ref.py in float64 - outputs AND probabilities, the backward kernels fed
the biased forward's probabilities against autograd of the reference, the bf16 contraction form, bias=None / 0 against the calls without
the argument bit for bit, streams driven across the 64-row pass boundary and twice round a ring, the weights-emitting form, chunks on
empty, long and ring caches, and the paged forms against the dense ones bit for bit."""
import ctypes
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import band_ref as BR  # noqa: E402
import position_bias_ref as R  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402
from mer_amd import runtime  # noqa: E402
from test_context_window_kernels_gpu import _close, _hidden, _img, _key_pad, _long_case, _probs_view, _rand  # noqa: E402

DEV = "cuda"
GAIN = 1.0
TOL_OUT, TOL_GRAD = 2e-5, 3e-5          # fp32 outputs / probabilities; dq, dk, dv (tests/test_context_window_kernels_gpu.py)
TOL_BF16 = 3e-2                         # bf16 forms (the same file's bound of the bf16 contractions against the exact form)
BANDS = [(None, None), (None, 0), (8, 0)]
# B, L, H, hd, lengths
SHAPES = [(3, 9, 4, 16, [9, 4, 1]),            # ragged, a dialogue of 1
          (2, 33, 3, 24, [33, 17]),            # three 16-row tiles, slopes of a head count that is no power of two
          (2, 110, 5, 60, [110, 70]),          # two 64-row blocks: the distance across a block edge
          (3, 129, 5, 60, [129, 65, 1])]       # three blocks, one row in the last
IDS = ["L9", "L33", "L110", "L129"]


def _reference(q, k, v, key_pad, H, band, gain, dout):
    """position_bias_ref under autograd, float64, on [B, L, E] images: (out, P [B, H, i, j], dq, dk, dv)"""
    qr, kr, vr = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    out, p = R.attention(qr, kr, vr, key_pad, H, return_probs=True, band=band, gain=R.applied_gain(gain))
    out.backward(dout.double())
    return out.detach(), p.detach(), qr.grad, kr.grad, vr.grad


@functools.lru_cache(maxsize=None)
def _short_case(si):
    B, L, H, hd, lengths = SHAPES[si]
    E = H * hd
    q, k, v, dout = (_rand(B * L, E, seed=200 + 10 * si + i) for i in range(4))
    return q, k, v, dout, _key_pad(B, L, lengths)


@functools.lru_cache(maxsize=None)
def _short_reference(si, band):
    B, L, H, hd, _ = SHAPES[si]
    q, k, v, dout, kp = _short_case(si)
    img = lambda t: t.reshape(B, L, H * hd)          # noqa: E731
    return _reference(img(q), img(k), img(v), kp, H, band, GAIN, img(dout))


# ---- the dialogue kernels, L <= 64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", BANDS, ids=str)
@pytest.mark.parametrize("si", [0, 1], ids=IDS[:2])
def test_short_kernel_against_the_reference(si, band):
    B, L, H, hd, _ = SHAPES[si]
    E = H * hd
    q, k, v, dout, kp = _short_case(si)
    out, probs = F.attention_fwd(q, k, v, kp, B, L, H, past=band[0], future=band[1], bias=GAIN)
    dq, dk, dv = F.attention_bwd(q, k, v, kp, out, probs, dout, B, L, H, past=band[0], future=band[1])
    ro, rp, rdq, rdk, rdv = _short_reference(si, band)
    img = lambda t: t.reshape(B, L, E)          # noqa: E731
    P = _probs_view(probs, B, H, L)
    _close(img(out).double(), ro, TOL_OUT, "out")
    _close(P.double(), rp, TOL_OUT, "probs")
    _close(img(dq).double(), rdq, TOL_GRAD, "dq")
    _close(img(dk).double(), rdk, TOL_GRAD, "dk")
    _close(img(dv).double(), rdv, TOL_GRAD, "dv")
    assert torch.all(P[_hidden(kp, L, band).expand_as(P)] == 0), "a hidden key must keep probability exactly 0"
    # the term moves the probabilities by far more than the bound (the comparison can fail)
    _, plain = F.attention_fwd(q, k, v, kp, B, L, H, past=band[0], future=band[1])
    moved = (_probs_view(plain, B, H, L) - P).abs().max().item()
    print(f"probabilities moved by {moved:.3e}")
    assert moved > 100 * TOL_OUT


@pytest.mark.parametrize("si", [0, 1], ids=IDS[:2])
def test_short_kernel_bf16_contractions(si, monkeypatch):
    """AttnBatch::bf16_math bit 1 (the Q K^T contraction on the bf16 MFMA): the term is added in fp32 behind it.  The probabilities
    are the check that discriminates: with and without the term they differ by far more than the bf16 bound."""
    B, L, H, hd, _ = SHAPES[si]
    band = (None, 0)
    q, k, v, dout, kp = _short_case(si)
    monkeypatch.setenv("M2F_ATTN_BF16_KERNEL", "1")
    try:
        out, probs = F.attention_fwd(q, k, v, kp, B, L, H, past=band[0], future=band[1], bias=GAIN)
        _, plain = F.attention_fwd(q, k, v, kp, B, L, H, past=band[0], future=band[1])
    finally:
        monkeypatch.setenv("M2F_ATTN_BF16_KERNEL", "0")
    ro, rp, *_ = _short_reference(si, band)
    P = _probs_view(probs, B, H, L)
    _close(out.reshape(B, L, -1).double(), ro, TOL_BF16, "bf16 out")
    _close(P.double(), rp, TOL_BF16, "bf16 probs")
    moved = (_probs_view(plain, B, H, L).double() - rp).abs().max().item()
    print(f"without the term the probabilities are {moved:.3e} away")
    assert moved > 3 * TOL_BF16


def test_no_gain_is_the_call_without_the_argument():
    B, L, H, hd, _ = SHAPES[1]
    q, k, v, _, kp = _short_case(1)
    for band in BANDS:
        want = F.attention_fwd(q, k, v, kp, B, L, H, past=band[0], future=band[1])
        for gain in (None, 0.0, 0):
            got = F.attention_fwd(q, k, v, kp, B, L, H, past=band[0], future=band[1], bias=gain)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    c = _long_case(2, 110, 5, 60, [110, 70], True, seed=300)
    for band in BANDS:
        kw = dict(c["kw"], past=band[0], future=band[1])
        want = F.attention_varlen_fwd(c["q"], c["k"], c["v"], 2, 110, 5, **kw)
        for gain in (None, 0.0):
            got = F.attention_varlen_fwd(c["q"], c["k"], c["v"], 2, 110, 5, bias=gain, **kw)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError, match="position bias"):
        F.attention_fwd(q, k, v, kp, B, L, H, bias=-1.0)
    with pytest.raises(runtime.HipError):
        nan_gain = runtime.AttnOptsC(past=-1, future=-1, bias_gain=float("nan"))
        runtime.check(runtime.lib().m2f_attention_fwd(B, L, H, hd, q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(),
                                                       v.stride(0), kp.to(torch.uint8).data_ptr(), q.data_ptr(), q.stride(0), None, 0, 0.0,
                                                       None, None, ctypes.byref(nan_gain)), "m2f_attention_fwd")


def test_a_rounded_gain_is_what_is_applied():
    """gain 0.3 is applied as bf16(0.3): the result equals the call with the rounded value, bit for bit, and matches the reference at it"""
    B, L, H, hd, _ = SHAPES[0]
    q, k, v, dout, kp = _short_case(0)
    a = F.attention_fwd(q, k, v, kp, B, L, H, bias=0.3)
    b = F.attention_fwd(q, k, v, kp, B, L, H, bias=runtime.position_bias(0.3))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    img = lambda t: t.reshape(B, L, H * hd)          # noqa: E731
    ro, rp, *_ = _reference(img(q), img(k), img(v), kp, H, (None, None), 0.3, img(dout))
    _close(_probs_view(a[1], B, H, L).double(), rp, TOL_OUT, "probs at the applied gain")


# ---- the long-dialogue kernels (every shape; packed and padded rows) ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _varlen_case(si, packed):
    B, L, H, hd, lengths = SHAPES[si]
    return _long_case(B, L, H, hd, lengths, packed, seed=400 + 10 * si)


@functools.lru_cache(maxsize=None)
def _varlen_reference(si, packed, band):
    c = _varlen_case(si, packed)
    return _reference(_img(c, c["q"]), _img(c, c["k"]), _img(c, c["v"]), c["key_pad"], c["H"], band, GAIN, _img(c, c["dout"]))


@pytest.mark.parametrize("band", BANDS, ids=str)
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "padded"])
@pytest.mark.parametrize("si", range(4), ids=IDS)
def test_long_kernel_against_the_reference(si, packed, band):
    c = _varlen_case(si, packed)
    B, L, H = c["B"], c["L"], c["H"]
    kw = dict(c["kw"], past=band[0], future=band[1])
    out, probs = F.attention_varlen_fwd(c["q"], c["k"], c["v"], B, L, H, bias=GAIN, **kw)
    dq, dk, dv = F.attention_varlen_bwd(c["q"], c["k"], c["v"], out, probs, c["dout"], B, L, H, **kw)
    ro, rp, rdq, rdk, rdv = _varlen_reference(si, packed, band)
    own = c["own"]
    _close(_img(c, out)[own].double(), ro[own], TOL_OUT, "out")
    P = _probs_view(probs, B, H, L).permute(0, 2, 1, 3)          # [B, i, H, j]
    seen = ~_hidden(c["key_pad"], L, band).expand(B, H, L, L).permute(0, 2, 1, 3)
    sel = own[:, :, None, None] & seen                           # (hidden entries of skipped blocks are not written: not compared)
    _close(P[sel].double(), rp.permute(0, 2, 1, 3)[sel], TOL_OUT, "probs")
    _close(_img(c, dq)[own].double(), rdq[own], TOL_GRAD, "dq")
    _close(_img(c, dk)[own].double(), rdk[own], TOL_GRAD, "dk")
    _close(_img(c, dv)[own].double(), rdv[own], TOL_GRAD, "dv")
    Pf = _probs_view(probs, B, H, L)
    assert torch.all(Pf[_hidden(c["key_pad"], L, band).expand_as(Pf)] == 0)
    for t in (out, dq, dk, dv):
        assert torch.isfinite(t).all()


def test_short_and_long_kernels_agree_on_a_short_dialogue():
    """L = 33 fits both kernels: the same rule, so the same probabilities within two fp32 bounds"""
    B, L, H, hd, _ = SHAPES[1]
    q, k, v, _, kp = _short_case(1)
    a = F.attention_fwd(q, k, v, kp, B, L, H, past=None, future=0, bias=GAIN)
    b = F.attention_varlen_fwd(q, k, v, B, L, H, key_pad=kp, past=None, future=0, bias=GAIN)
    valid = ~kp.reshape(-1)
    _close(a[0][valid], b[0][valid], 2 * TOL_OUT, "short vs long kernel")


# ---- the stream step ---------------------------------------------------------------------------------------------------------------------
S_, H_, HD_ = 2, 4, 16
E_ = H_ * HD_


@functools.lru_cache(maxsize=None)
def _dialogue(n, bf16):
    """n utterances of S_ dialogues: q, k, v [n, S_, E_] (bf16: exact bf16 values - what the kernels round to once)"""
    q, k, v = (_rand(n, S_, E_, seed=500 + i) for i in range(3))
    if bf16:
        q, k, v = (t.to(torch.bfloat16).float() for t in (q, k, v))
    return q, k, v


@functools.lru_cache(maxsize=None)
def _dialogue_reference(n, bf16, past):
    """(out [S_, n, E_], P [S_, H_, n, n]) of the whole dialogues under the band (past, 0) and the gain, float64"""
    q, k, v = (t.permute(1, 0, 2).double() for t in _dialogue(n, bf16))
    kp = torch.zeros(S_, n, dtype=torch.bool, device=DEV)
    return R.attention(q, k, v, kp, H_, return_probs=True, band=(past, 0), gain=R.applied_gain(GAIN))


def _paged_setup(C, bf16, page_rows=16):
    tw = -(-C // page_rows)
    table = torch.tensor([[e * S_ + (S_ - 1 - s) for e in range(tw)] for s in range(S_)], dtype=torch.int32, device=DEV)
    kp, vp = F.attention_stream_pools(S_ * tw, H_, HD_, page_rows, bf16=bf16, device=DEV)
    return table, kp, vp


def _drive(n, C, ring, bf16, paged=False, weights=False, gain=GAIN):
    """n steps from empty caches -> (outs [n, S_, E_], weight rows [n, S_, H_, C] or None, caches)"""
    q, k, v = _dialogue(n, bf16)
    act = torch.ones(S_, device=DEV)
    if paged:
        table, kc, vc = _paged_setup(C, bf16)
    else:
        kc, vc = F.attention_stream_caches(S_, H_, HD_, C, bf16=bf16, device=DEV)
    outs, rows = [], []
    for i in range(n):
        lengths = torch.full((S_,), i, dtype=torch.int32, device=DEV)
        w = torch.full((S_, H_, C), float("nan"), device=DEV) if weights else None
        if paged:
            o = F.attention_stream_paged(q[i], k[i], v[i], kc, vc, table, lengths, act, H_, C, ring=ring, bf16=bf16, weights=w, bias=gain)
        else:
            o = F.attention_stream(q[i], k[i], v[i], kc, vc, lengths, act, H_, ring=ring, bf16=bf16, weights=w, bias=gain)
        outs.append(o)
        rows.append(w)
    return torch.stack(outs), (torch.stack(rows) if weights else None), (kc, vc)


STREAMS = [(70, 128, False), (10, 4, True)]          # (steps, capacity, ring): across the 64-rows-per-iteration boundary of pass 1; twice round a ring


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,C,ring", STREAMS, ids=["plain70", "ring4"])
def test_stream_steps_against_the_reference(n, C, ring, bf16):
    """Every step against the reference's last row over the live history.  bf16 caches: the inputs are exact bf16 values, so the kernel
    rounds nothing and the fp32 bound holds; the kernel's own rounding of arbitrary inputs is tests/test_streaming_kernels_gpu.py's."""
    past = C - 1 if ring else None
    outs, rows, _ = _drive(n, C, ring, bf16, weights=True)
    ro, rp = _dialogue_reference(n, bf16, past)
    _close(outs.permute(1, 0, 2).double(), ro, TOL_OUT, "step outputs")
    for i in range(n):                                        # the WEIGHTS form: column t = the t-th oldest live utterance
        lo = max(0, i - (C - 1)) if ring else 0
        live = i + 1 - lo
        _close(rows[i][:, :, :live].double(), rp[:, :, i, lo:i + 1], TOL_OUT, f"weights of step {i}")
        assert torch.all(rows[i][:, :, live:] == 0)
    plain, _, _ = _drive(n, C, ring, bf16, gain=None)
    moved = (plain - outs).abs().max().item()
    print(f"outputs moved by {moved:.3e}")
    assert moved > 100 * TOL_OUT * ro.abs().max().item()
    # the weights-emitting form and the plain form of the biased step: the same output bits
    again, _, _ = _drive(n, C, ring, bf16)
    assert torch.equal(again, outs)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,C,ring", STREAMS, ids=["plain70", "ring4"])
def test_paged_stream_steps_equal_the_dense_ones(n, C, ring, bf16):
    dense, drows, _ = _drive(n, C, ring, bf16, weights=True)
    paged, prows, _ = _drive(n, C, ring, bf16, paged=True, weights=True)
    assert torch.equal(dense, paged) and torch.equal(drows, prows)
    paged_plain, _, _ = _drive(n, C, ring, bf16, paged=True)
    assert torch.equal(dense, paged_plain)


# ---- the chunk ---------------------------------------------------------------------------------------------------------------------------
CHUNKS = [(0, 128, False), (70, 128, False), (20, 12, True)]          # (cached utterances, capacity, ring), then T = 8 more
T_ = 8


def _chunk(n_old, C, ring, bf16, paged):
    """n_old steps, then one chunk of T_ -> (chunk out [S_, T_, E_], caches behind it, caches of n_old + T_ steps)"""
    n = n_old + T_
    q, k, v = _dialogue(n, bf16)
    if paged:
        table, kc, vc = _paged_setup(C, bf16)
    else:
        kc, vc = F.attention_stream_caches(S_, H_, HD_, C, bf16=bf16, device=DEV)
    act = torch.ones(S_, device=DEV)
    for i in range(n_old):
        lengths = torch.full((S_,), i, dtype=torch.int32, device=DEV)
        if paged:
            F.attention_stream_paged(q[i], k[i], v[i], kc, vc, table, lengths, act, H_, C, ring=ring, bf16=bf16, bias=GAIN)
        else:
            F.attention_stream(q[i], k[i], v[i], kc, vc, lengths, act, H_, ring=ring, bf16=bf16, bias=GAIN)
    rows = lambda t: t[n_old:].permute(1, 0, 2).reshape(S_ * T_, E_).contiguous()          # noqa: E731  (row s*T + t)
    lengths = torch.full((S_,), n_old, dtype=torch.int32, device=DEV)
    new = torch.full((S_,), T_, dtype=torch.int32, device=DEV)
    if paged:
        out = F.attention_stream_chunk_paged(rows(q), rows(k), rows(v), kc, vc, table, lengths, new, H_, T_, C, ring=ring, bf16=bf16, bias=GAIN)
    else:
        out = F.attention_stream_chunk(rows(q), rows(k), rows(v), kc, vc, lengths, new, H_, T_, ring=ring, bf16=bf16, bias=GAIN)
    return out.view(S_, T_, E_), (kc, vc)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n_old,C,ring", CHUNKS, ids=["empty", "behind70", "ring12"])
def test_chunk_against_the_reference_and_the_steps(n_old, C, ring, bf16):
    n = n_old + T_
    past = C - 1 if ring else None
    out, (kc, vc) = _chunk(n_old, C, ring, bf16, paged=False)
    ro, _ = _dialogue_reference(n, bf16, past)
    _close(out.double(), ro[:, n_old:], TOL_OUT, "chunk outputs")
    steps, _, (kc_s, vc_s) = _drive(n, C, ring, bf16)
    _close(out, steps[n_old:].permute(1, 0, 2), 2 * TOL_OUT, "chunk vs steps")
    bits = lambda t: t.view(torch.int16 if bf16 else torch.int32)          # noqa: E731
    assert torch.equal(bits(kc), bits(kc_s)) and torch.equal(bits(vc), bits(vc_s)), "K and V rows do not depend on the bias or the path"
    pout, (kp, vp) = _chunk(n_old, C, ring, bf16, paged=True)
    assert torch.equal(pout, out), "paged chunk must give the dense chunk's bits"
    # the biased chunk is not the unbiased one (the comparison can fail)
    q, k, v = _dialogue(n, bf16)
    rows = lambda t: t[n_old:].permute(1, 0, 2).reshape(S_ * T_, E_).contiguous()          # noqa: E731
    kc0, vc0 = kc_s.clone(), vc_s.clone()
    if not ring:                                              # (a plain cache: re-run the chunk over the first n_old rows, no bias)
        plain = F.attention_stream_chunk(rows(q), rows(k), rows(v), kc0, vc0, torch.full((S_,), n_old, dtype=torch.int32, device=DEV),
                                         torch.full((S_,), T_, dtype=torch.int32, device=DEV), H_, T_, ring=False, bf16=bf16)
        assert (plain.view(S_, T_, E_) - out).abs().max().item() > 100 * TOL_OUT * ro.abs().max().item()


def test_stream_entries_refuse_a_bad_gain():
    kc, vc = F.attention_stream_caches(S_, H_, HD_, 4, device=DEV)
    q = _rand(S_, E_, seed=1)
    lengths, act = torch.zeros(S_, dtype=torch.int32, device=DEV), torch.ones(S_, device=DEV)
    for bad in (-1.0, float("inf"), float("nan"), "1"):
        with pytest.raises(ValueError, match="position bias"):
            F.attention_stream(q, q, q, kc, vc, lengths, act, H_, bias=bad)
        with pytest.raises(ValueError, match="position bias"):
            F.attention_stream_chunk(q.repeat(2, 1), q.repeat(2, 1), q.repeat(2, 1), kc, vc, lengths, lengths, H_, 2, bias=bad)
    assert math.isclose(float(F.position_bias_slopes(H_, GAIN)[0]), 0.25)
