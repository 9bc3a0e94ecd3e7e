"""Speaker-aware attention heads at kernel level: functional.attention_fwd / attention_varlen_fwd / attention_stream[_paged] /
attention_stream_chunk[_paged] with speakers= / speaker_heads= (the speaker fields of the C entries' options; the SPK instantiations of csrc/attention.hip,
attention_dlong.hip, attention_stream.hip, attention_stream_chunk.hip) against tests/golden/speaker_heads_ref.py in float64 - outputs
AND probabilities, the UNCHANGED backward kernels fed the new forward's probabilities against autograd of the reference, exact zeros at
hidden pairs, the zero rows of an other-speaker head in a monologue, the bf16 contraction form, speaker_heads=None against the calls
without the argument bit for bit, streams across the 64-row pass boundary and twice round a ring, the weights-emitting form with a zero
row, chunks on empty, long and ring caches against the reference and against that many steps, the cached speaker bytes, the paged forms
against the dense ones bit for bit, and every refused launch."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import speaker_heads_ref as R  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402
from mer_amd import runtime  # noqa: E402
from test_context_window_kernels_gpu import _close, _hidden, _img, _key_pad, _long_case, _probs_view, _rand  # noqa: E402

DEV = "cuda"
TOL_OUT, TOL_GRAD = 2e-5, 3e-5          # fp32 outputs / probabilities; dq, dk, dv (tests/test_context_window_kernels_gpu.py)
TOL_BF16 = 3e-2                         # bf16 forms (the same file's bound of the bf16 contractions against the exact form)
BANDS = [(None, None), (None, 0), (8, 0)]
HEADS = [(1, 1), (2, 0)]
GAINS = [None, 1.0]
# B, L, H, hd, lengths
SHAPES = [(3, 9, 4, 16, [9, 4, 1]),            # ragged, a dialogue of 1
          (2, 33, 3, 24, [33, 17]),            # three 16-row tiles, a head count that is no power of two
          (2, 110, 5, 60, [110, 70]),          # two 64-row blocks
          (3, 129, 5, 60, [129, 65, 1])]       # three blocks, one row in the last
IDS = ["L9", "L33", "L110", "L129"]


def _speakers(B, L):
    """[B, L] int64: three speakers in runs of five - the pattern changes INSIDE a 64-row block and across its edge - with id 255 among
    them; the LAST dialogue is a monologue (an other-speaker head sees no key there: zero rows)."""
    i = torch.arange(L)
    spk = ((i // 5) % 3)[None, :].repeat(B, 1) + torch.arange(B)[:, None]
    spk = spk % 3
    spk[spk == 2] = 255
    spk[B - 1] = 7
    return spk.to(DEV)


def _hidden_all(key_pad, L, band, spk, H, heads):
    """bool [B, H, i, j]: pad key | outside the band | hidden by the head's speaker class"""
    return _hidden(key_pad, L, band).expand(-1, H, -1, -1) | R.speaker_hidden(spk, H, heads)


def _reference(q, k, v, key_pad, H, band, gain, spk, heads, dout):
    """speaker_heads_ref under autograd, float64, on [B, L, E] images: (out, P [B, H, i, j], dq, dk, dv)"""
    qr, kr, vr = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    out, p = R.attention(qr, kr, vr, key_pad, H, return_probs=True, band=band, gain=R.applied_gain(gain), speakers=spk, heads=heads)
    out.backward(dout.double())
    return out.detach(), p.detach(), qr.grad, kr.grad, vr.grad


@functools.lru_cache(maxsize=None)
def _short_case(si):
    B, L, H, hd, lengths = SHAPES[si]
    E = H * hd
    q, k, v, dout = (_rand(B * L, E, seed=600 + 10 * si + i) for i in range(4))
    return q, k, v, dout, _key_pad(B, L, lengths), _speakers(B, L)


@functools.lru_cache(maxsize=None)
def _short_reference(si, band, gain, heads):
    B, L, H, hd, _ = SHAPES[si]
    q, k, v, dout, kp, spk = _short_case(si)
    img = lambda t: t.reshape(B, L, H * hd)          # noqa: E731
    return _reference(img(q), img(k), img(v), kp, H, band, gain, spk, heads, img(dout))


# ---- the dialogue kernels, L <= 64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", GAINS, ids=["nobias", "bias"])
@pytest.mark.parametrize("band", BANDS, ids=str)
@pytest.mark.parametrize("heads", HEADS, ids=str)
@pytest.mark.parametrize("si", [0, 1], ids=IDS[:2])
def test_short_kernel_against_the_reference(si, heads, band, gain):
    B, L, H, hd, _ = SHAPES[si]
    E = H * hd
    q, k, v, dout, kp, spk = _short_case(si)
    kw = dict(past=band[0], future=band[1])
    out, probs = F.attention_fwd(q, k, v, kp, B, L, H, bias=gain, speakers=spk, speaker_heads=heads, **kw)
    dq, dk, dv = F.attention_bwd(q, k, v, kp, out, probs, dout, B, L, H, **kw)          # the unchanged backward, the new probabilities
    ro, rp, rdq, rdk, rdv = _short_reference(si, band, gain, heads)
    img = lambda t: t.reshape(B, L, E)          # noqa: E731
    P = _probs_view(probs, B, H, L)
    _close(img(out).double(), ro, TOL_OUT, "out")
    _close(P.double(), rp, TOL_OUT, "probs")
    _close(img(dq).double(), rdq, TOL_GRAD, "dq")
    _close(img(dk).double(), rdk, TOL_GRAD, "dk")
    _close(img(dv).double(), rdv, TOL_GRAD, "dv")
    hidden = _hidden_all(kp, L, band, spk, H, heads)
    assert torch.all(P[hidden] == 0), "a hidden pair must keep probability exactly 0"
    for t in (out, probs, dq, dk, dv):
        assert torch.isfinite(t).all()
    # rows that see no key: a zero row of P and a zero output slice of that head
    empty = hidden.all(-1)                                       # [B, H, i]
    valid = ~kp
    if heads[1]:
        assert (empty & valid[:, None, :]).any(), "the monologue's other-speaker head must be an empty row of a VALID query"
    assert torch.all(P[empty] == 0)
    oh = img(out).view(B, L, H, hd).permute(0, 2, 1, 3)          # [B, H, i, hd]
    assert torch.all(oh[empty] == 0)
    # the setting moves the probabilities by far more than the bound: the assertion that fails without the feature
    _, plain = F.attention_fwd(q, k, v, kp, B, L, H, bias=gain, **kw)
    moved = (_probs_view(plain, B, H, L) - P).abs().max().item()
    print(f"probabilities moved by {moved:.3e}")
    assert moved > 100 * TOL_OUT


def test_short_kernel_bf16_contractions(monkeypatch):
    """AttnBatch::bf16_math bit 1 (the Q K^T contraction on the bf16 MFMA): the speaker test sits behind it, on the fp32 scores."""
    si, band, heads = 1, (None, 0), (1, 1)
    B, L, H, hd, _ = SHAPES[si]
    q, k, v, dout, kp, spk = _short_case(si)
    monkeypatch.setenv("M2F_ATTN_BF16_KERNEL", "1")
    try:
        out, probs = F.attention_fwd(q, k, v, kp, B, L, H, past=band[0], future=band[1], speakers=spk, speaker_heads=heads)
    finally:
        monkeypatch.setenv("M2F_ATTN_BF16_KERNEL", "0")
    ro, rp, *_ = _short_reference(si, band, None, heads)
    P = _probs_view(probs, B, H, L)
    _close(out.reshape(B, L, -1).double(), ro, TOL_BF16, "bf16 out")
    _close(P.double(), rp, TOL_BF16, "bf16 probs")
    assert torch.all(P[_hidden_all(kp, L, band, spk, H, heads)] == 0)


def test_library_head_class_is_the_rule():
    for H in (3, 4, 5, 8):
        for a in range(H + 1):
            for b in range(H + 1 - a):
                for h in range(H):
                    want = R.head_class(h, (a, b))
                    assert F.speaker_head_class(h, a, b) == want == runtime.speaker_head_class(h, a, b)


# ---- the long-dialogue kernels (every shape; packed and padded rows) ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _varlen_case(si, packed):
    B, L, H, hd, lengths = SHAPES[si]
    c = _long_case(B, L, H, hd, lengths, packed, seed=700 + 10 * si)
    spk = _speakers(B, L)
    rows = torch.zeros(c["T"], dtype=torch.int64, device=DEV)          # one id per TOKEN ROW, in the rows' order
    valid = ~c["key_pad"] if packed else torch.ones_like(c["key_pad"])
    rows[c["row"][valid]] = spk[valid]
    return dict(c, spk=spk, spk_rows=rows)


@functools.lru_cache(maxsize=None)
def _varlen_reference(si, packed, band, heads):
    c = _varlen_case(si, packed)
    return _reference(_img(c, c["q"]), _img(c, c["k"]), _img(c, c["v"]), c["key_pad"], c["H"], band, None, c["spk"], heads, _img(c, c["dout"]))


@pytest.mark.parametrize("band", BANDS, ids=str)
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "padded"])
@pytest.mark.parametrize("si", [2, 3], ids=IDS[2:])
def test_long_kernel_against_the_reference(si, packed, band):
    heads = (2, 1)
    c = _varlen_case(si, packed)
    B, L, H = c["B"], c["L"], c["H"]
    kw = dict(c["kw"], past=band[0], future=band[1])
    out, probs = F.attention_varlen_fwd(c["q"], c["k"], c["v"], B, L, H, speakers=c["spk_rows"], speaker_heads=heads, **kw)
    dq, dk, dv = F.attention_varlen_bwd(c["q"], c["k"], c["v"], out, probs, c["dout"], B, L, H, **kw)
    ro, rp, rdq, rdk, rdv = _varlen_reference(si, packed, band, heads)
    own = c["own"]
    _close(_img(c, out)[own].double(), ro[own], TOL_OUT, "out")
    P = _probs_view(probs, B, H, L).permute(0, 2, 1, 3)          # [B, i, H, j]
    seen = ~_hidden(c["key_pad"], L, band).expand(B, H, L, L).permute(0, 2, 1, 3)
    sel = own[:, :, None, None] & seen                           # (band-hidden entries of skipped blocks are not written: not compared)
    _close(P[sel].double(), rp.permute(0, 2, 1, 3)[sel], TOL_OUT, "probs")
    _close(_img(c, dq)[own].double(), rdq[own], TOL_GRAD, "dq")
    _close(_img(c, dk)[own].double(), rdk[own], TOL_GRAD, "dk")
    _close(_img(c, dv)[own].double(), rdv[own], TOL_GRAD, "dv")
    Pf = _probs_view(probs, B, H, L)
    assert torch.all(Pf[_hidden_all(c["key_pad"], L, band, c["spk"], H, heads)] == 0), "fresh buffer: every hidden pair is exactly 0"
    for t in (out, dq, dk, dv):
        assert torch.isfinite(t).all()
    _, plain = F.attention_varlen_fwd(c["q"], c["k"], c["v"], B, L, H, **kw)
    moved = (_probs_view(plain, B, H, L) - Pf).abs().max().item()
    assert moved > 100 * TOL_OUT


def test_long_kernel_writes_every_element_of_a_visited_block():
    """No block is skipped for speakers: over a buffer full of another launch's values every pair the band admits is written, hidden
    ones as 0."""
    c = _varlen_case(2, True)
    B, L, H = c["B"], c["L"], c["H"]
    Lp = 16 * ((L + 15) // 16)
    dirty = torch.full((B * H, Lp, Lp), 0.5, device=DEV)
    _, probs = F.attention_varlen_fwd(c["q"], c["k"], c["v"], B, L, H, probs=dirty, speakers=c["spk_rows"], speaker_heads=(2, 1), **c["kw"])
    P = _probs_view(probs, B, H, L)
    hid = R.speaker_hidden(c["spk"], H, (2, 1)) & (~c["key_pad"])[:, None, :, None] & (~c["key_pad"])[:, None, None, :]
    assert hid.any() and torch.all(P[hid] == 0)


def test_short_and_long_kernels_agree_on_a_short_dialogue():
    """L = 33 fits both kernels: the same rule, so the same outputs within two fp32 bounds"""
    B, L, H, hd, _ = SHAPES[1]
    q, k, v, _, kp, spk = _short_case(1)
    a = F.attention_fwd(q, k, v, kp, B, L, H, past=None, future=0, bias=1.0, speakers=spk, speaker_heads=(1, 1))
    b = F.attention_varlen_fwd(q, k, v, B, L, H, key_pad=kp, past=None, future=0, bias=1.0, speakers=spk, speaker_heads=(1, 1))
    valid = ~kp.reshape(-1)
    _close(a[0][valid], b[0][valid], 2 * TOL_OUT, "short vs long kernel")


# ---- the stream step ---------------------------------------------------------------------------------------------------------------------
S_, H_, HD_ = 2, 4, 16
E_ = H_ * HD_
SH = (1, 2)                             # one same-speaker head, two other-speaker heads, one untouched


@functools.lru_cache(maxsize=None)
def _dialogue(n, bf16):
    """n utterances of S_ dialogues: q, k, v [n, S_, E_] (bf16: exact bf16 values - what the kernels round to once) and speakers [n, S_]:
    slot 0 alternates in runs of three with id 255 among them, slot 1 is a monologue until utterance 5 (zero rows before)"""
    q, k, v = (_rand(n, S_, E_, seed=800 + i) for i in range(3))
    if bf16:
        q, k, v = (t.to(torch.bfloat16).float() for t in (q, k, v))
    i = torch.arange(n)
    spk = torch.stack([torch.where((i // 3) % 2 == 0, 255, 3), torch.where(i < 5, 9, (i % 4) + 9)], 1).to(DEV)
    return q, k, v, spk


@functools.lru_cache(maxsize=None)
def _dialogue_reference(n, bf16, past, gain=None):
    """(out [S_, n, E_], P [S_, H_, n, n]) of the whole dialogues under the band (past, 0), float64"""
    q, k, v, spk = _dialogue(n, bf16)
    q, k, v = (t.permute(1, 0, 2).double() for t in (q, k, v))
    kp = torch.zeros(S_, n, dtype=torch.bool, device=DEV)
    return R.attention(q, k, v, kp, H_, return_probs=True, band=(past, 0), gain=R.applied_gain(gain), speakers=spk.t().contiguous(), heads=SH)


def _paged_setup(C, bf16, page_rows=16):
    tw = -(-C // page_rows)
    table = torch.tensor([[e * S_ + (S_ - 1 - s) for e in range(tw)] for s in range(S_)], dtype=torch.int32, device=DEV)
    kp, vp = F.attention_stream_pools(S_ * tw, H_, HD_, page_rows, bf16=bf16, device=DEV)
    return table, kp, vp


def _drive(n, C, ring, bf16, paged=False, weights=False, heads=SH, gain=None, first=0, state=None):
    """steps first .. n - 1 (from empty caches, or on `state`) -> (outs, weight rows or None, (kc, vc, spk_cache, lengths, table))"""
    q, k, v, spk = _dialogue(n, bf16)
    act = torch.ones(S_, device=DEV)
    if state is not None:
        kc, vc, sc, lengths, table = state
    else:
        table = None
        if paged:
            table, kc, vc = _paged_setup(C, bf16)
        else:
            kc, vc = F.attention_stream_caches(S_, H_, HD_, C, bf16=bf16, device=DEV)
        sc = torch.full((S_, C), 77, dtype=torch.uint8, device=DEV)          # (stale bytes: never read behind the live count)
        lengths = torch.zeros(S_, dtype=torch.int32, device=DEV)
    outs, rows = [], []
    for i in range(first, n):
        w = torch.full((S_, H_, C), float("nan"), device=DEV) if weights else None
        kw = dict(ring=ring, bf16=bf16, weights=w, bias=gain)
        if heads is not None:
            kw.update(speakers=spk[i], speaker_cache=sc, speaker_heads=heads)
        if paged:
            o = F.attention_stream_paged(q[i], k[i], v[i], kc, vc, table, lengths, act, H_, C, **kw)
        else:
            o = F.attention_stream(q[i], k[i], v[i], kc, vc, lengths, act, H_, **kw)
        F.stream_advance_speakers(lengths, act, sc, spk[i], ring=ring)       # behind the attention launch: the id, then the count
        outs.append(o)
        rows.append(w)
    return (torch.stack(outs) if outs else None), (torch.stack(rows) if weights and rows else None), (kc, vc, sc, lengths, table)


STREAMS = [(70, 128, False), (10, 4, True)]          # (steps, capacity, ring): across the 64-rows-per-iteration boundary of pass 1; twice round a ring


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,C,ring", STREAMS, ids=["plain70", "ring4"])
def test_stream_steps_against_the_reference(n, C, ring, bf16):
    past = C - 1 if ring else None
    outs, rows, (_, _, sc, lengths, _) = _drive(n, C, ring, bf16, weights=True)
    ro, rp = _dialogue_reference(n, bf16, past)
    _close(outs.permute(1, 0, 2).double(), ro, TOL_OUT, "step outputs")
    zero_rows = 0
    for i in range(n):                                        # the WEIGHTS form: column t = the t-th oldest live utterance
        lo = max(0, i - (C - 1)) if ring else 0
        live = i + 1 - lo
        _close(rows[i][:, :, :live].double(), rp[:, :, i, lo:i + 1], TOL_OUT, f"weights of step {i}")
        assert torch.all(rows[i][:, :, live:] == 0)
        assert torch.all(rows[i][:, :, :live][rp[:, :, i, lo:i + 1] == 0] == 0), "a hidden row has weight exactly 0"
        zero_rows += int((rows[i].abs().sum(-1) == 0).sum())
    assert zero_rows > 0, "the monologue's other-speaker heads must give zero weight rows"
    assert torch.isfinite(outs).all() and torch.isfinite(rows).all()
    # slot 1, steps 0 .. 4: a monologue - the other-speaker heads' output slices are zero rows
    oh = outs.view(n, S_, H_, HD_)
    assert torch.all(oh[:5, 1, SH[0]:SH[0] + SH[1]] == 0)
    assert int(lengths[0]) == n
    # the cached bytes: logical row u % C holds utterance u's id
    _, _, _, spk = _dialogue(n, bf16)
    for u in range(max(0, n - C), n):
        assert torch.equal(sc[:, u % C if ring else u].long(), spk[u])
    plain, _, _ = _drive(n, C, ring, bf16, heads=None)
    moved = (plain - outs).abs().max().item()
    print(f"outputs moved by {moved:.3e}")
    assert moved > 100 * TOL_OUT * ro.abs().max().item()
    again, _, _ = _drive(n, C, ring, bf16)                     # the weights-emitting form and the plain form: the same output bits
    assert torch.equal(again, outs)


def test_stream_steps_with_bias_against_the_reference():
    n, C = 10, 4
    outs, _, _ = _drive(n, C, True, False, gain=1.0)
    ro, _ = _dialogue_reference(n, False, C - 1, 1.0)
    _close(outs.permute(1, 0, 2).double(), ro, TOL_OUT, "biased step outputs")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,C,ring", STREAMS, ids=["plain70", "ring4"])
def test_paged_stream_steps_equal_the_dense_ones(n, C, ring, bf16):
    dense, drows, ds = _drive(n, C, ring, bf16, weights=True)
    paged, prows, ps = _drive(n, C, ring, bf16, paged=True, weights=True)
    assert torch.equal(dense, paged) and torch.equal(drows, prows) and torch.equal(ds[2], ps[2])


# ---- the chunk ---------------------------------------------------------------------------------------------------------------------------
CHUNKS = [(0, 128, False), (70, 128, False), (20, 12, True)]          # (cached utterances, capacity, ring), then T = 8 more
T_ = 8


def _chunk(n_old, C, ring, bf16, paged, heads=SH):
    """n_old steps, then one chunk of T_ -> (chunk out [S_, T_, E_], state behind it)"""
    n = n_old + T_
    q, k, v, spk = _dialogue(n, bf16)
    _, _, (kc, vc, sc, lengths, table) = _drive(n_old, C, ring, bf16, paged=paged, heads=heads)
    rows = lambda t: t[n_old:].permute(1, 0, 2).reshape(S_ * T_, E_).contiguous()          # noqa: E731  (row s*T + t)
    new_ids = spk[n_old:].t().contiguous()                                                  # [S_, T_]
    new = torch.full((S_,), T_, dtype=torch.int32, device=DEV)
    kw = dict(ring=ring, bf16=bf16)
    if heads is not None:
        kw.update(speakers=new_ids, speaker_cache=sc, speaker_heads=heads)
    if paged:
        out = F.attention_stream_chunk_paged(rows(q), rows(k), rows(v), kc, vc, table, lengths, new, H_, T_, C, **kw)
    else:
        out = F.attention_stream_chunk(rows(q), rows(k), rows(v), kc, vc, lengths, new, H_, T_, **kw)
    F.stream_advance_speakers_n(lengths, new, sc, new_ids, T_, ring=ring)
    return out.view(S_, T_, E_), (kc, vc, sc, lengths)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n_old,C,ring", CHUNKS, ids=["empty", "behind70", "ring12"])
def test_chunk_against_the_reference_and_the_steps(n_old, C, ring, bf16):
    n = n_old + T_
    past = C - 1 if ring else None
    out, (kc, vc, sc, lengths) = _chunk(n_old, C, ring, bf16, paged=False)
    ro, _ = _dialogue_reference(n, bf16, past)
    _close(out.double(), ro[:, n_old:], TOL_OUT, "chunk outputs")
    steps, _, (kc_s, vc_s, sc_s, len_s, _) = _drive(n, C, ring, bf16)
    _close(out, steps[n_old:].permute(1, 0, 2), 2 * TOL_OUT, "chunk vs steps")
    live = slice(0, min(n, C))
    assert torch.equal(sc[:, live], sc_s[:, live]), "the cached speaker bytes after a chunk are those after the steps"
    assert torch.equal(lengths, len_s)
    # K / V rows are bitwise what they are without the setting
    _, (kc0, vc0, _, _) = _chunk(n_old, C, ring, bf16, paged=False, heads=None)
    bits = lambda t: t.view(torch.int16 if bf16 else torch.int32)          # noqa: E731
    assert torch.equal(bits(kc), bits(kc0)) and torch.equal(bits(vc), bits(vc0)) and torch.equal(bits(kc), bits(kc_s))
    pout, pstate = _chunk(n_old, C, ring, bf16, paged=True)
    assert torch.equal(pout, out), "paged chunk must give the dense chunk's bits"
    assert torch.equal(pstate[2][:, live], sc[:, live])
    if n_old == 0:                                             # slot 1 opens as a monologue: zero rows on its other-speaker heads
        assert torch.all(out.view(S_, T_, H_, HD_)[1, :5, SH[0]:SH[0] + SH[1]] == 0)
    assert torch.isfinite(out).all()


# ---- the call without the argument, and the refusals -----------------------------------------------------------------------------------
def test_no_setting_is_the_call_without_the_argument():
    B, L, H, hd, _ = SHAPES[1]
    q, k, v, _, kp, _ = _short_case(1)
    for band in BANDS:
        want = F.attention_fwd(q, k, v, kp, B, L, H, past=band[0], future=band[1])
        got = F.attention_fwd(q, k, v, kp, B, L, H, past=band[0], future=band[1], speaker_heads=None)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    c = _long_case(2, 110, 5, 60, [110, 70], True, seed=300)
    want = F.attention_varlen_fwd(c["q"], c["k"], c["v"], 2, 110, 5, **c["kw"])
    got = F.attention_varlen_fwd(c["q"], c["k"], c["v"], 2, 110, 5, speaker_heads=None, **c["kw"])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # stream and chunk: heads=None drives the calls without the arguments; against an explicit speaker_heads=None
    kc, vc = F.attention_stream_caches(S_, H_, HD_, 8, device=DEV)
    kc2, vc2 = kc.clone(), vc.clone()
    x = _rand(S_, E_, seed=5)
    lengths, act = torch.zeros(S_, dtype=torch.int32, device=DEV), torch.ones(S_, device=DEV)
    a = F.attention_stream(x, x, x, kc, vc, lengths, act, H_)
    b = F.attention_stream(x, x, x, kc2, vc2, lengths, act, H_, speakers=None, speaker_cache=None, speaker_heads=None)
    assert torch.equal(a, b) and torch.equal(kc, kc2)
    y = _rand(S_ * 2, E_, seed=6)
    new = torch.full((S_,), 2, dtype=torch.int32, device=DEV)
    a = F.attention_stream_chunk(y, y, y, kc, vc, lengths, new, H_, 2)
    b = F.attention_stream_chunk(y, y, y, kc2, vc2, lengths, new, H_, 2, speaker_heads=None)
    assert torch.equal(a, b) and torch.equal(kc, kc2)


def test_refused_launches():
    B, L, H, hd, _ = SHAPES[0]
    q, k, v, _, kp, spk = _short_case(0)
    with pytest.raises(ValueError, match="exceeds"):
        F.attention_fwd(q, k, v, kp, B, L, H, speakers=spk, speaker_heads=(3, 2))
    with pytest.raises(ValueError, match="at least one"):
        F.attention_fwd(q, k, v, kp, B, L, H, speakers=spk, speaker_heads=(0, 0))
    with pytest.raises(ValueError, match="needs speakers"):
        F.attention_fwd(q, k, v, kp, B, L, H, speaker_heads=(1, 1))
    with pytest.raises(ValueError, match="without speaker_heads"):
        F.attention_fwd(q, k, v, kp, B, L, H, speakers=spk)
    for bad in (256, -1):
        ids = spk.clone()
        ids[0, 0] = bad
        with pytest.raises(ValueError, match="0 .. 255"):
            F.attention_fwd(q, k, v, kp, B, L, H, speakers=ids, speaker_heads=(1, 1))
    with pytest.raises(ValueError, match="one id per token row"):
        F.attention_varlen_fwd(q, k, v, B, L, H, key_pad=kp, speakers=spk[:, :-1], speaker_heads=(1, 1))
    # the C entries themselves: refused before any launch (`out` is never written)
    lib, u8 = runtime.lib(), kp.to(torch.uint8)
    ids = spk.to(torch.uint8)
    out = torch.full_like(q, 3.0)
    def heads(speakers, n_same, n_other):
        return ctypes.byref(runtime.AttnOptsC(past=-1, future=-1, bias_gain=0.0, n_same=n_same, n_other=n_other, speakers=speakers))

    def stream_heads(spk_cache, spk_new, n_same, n_other):
        return ctypes.byref(runtime.AttnStreamOptsC(n_same=n_same, n_other=n_other, spk_cache=spk_cache, spk_new=spk_new))

    args = (B, L, H, hd, q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), u8.data_ptr(), out.data_ptr(),
            out.stride(0), None, 0, 0.0, None, None)
    for tail in ((ids.data_ptr(), H, 1), (None, 1, 1), (ids.data_ptr(), -1, 1)):
        with pytest.raises(runtime.HipError):
            runtime.check(lib.m2f_attention_fwd(*args, heads(*tail)), "m2f_attention_fwd")
    vargs = (B, L, H, hd, q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), None, B * L, u8.data_ptr(),
             out.data_ptr(), out.stride(0), None, 0, 0.0, None, None)
    for tail in ((ids.data_ptr(), H, 1), (None, 1, 1)):
        with pytest.raises(runtime.HipError):
            runtime.check(lib.m2f_attention_varlen_fwd(*vargs, heads(*tail)), "m2f_attention_varlen_fwd")
    C = 4
    kc, vc = F.attention_stream_caches(S_, H_, HD_, C, device=DEV)
    x = _rand(S_, E_, seed=1)
    so = torch.full_like(x, 3.0)
    lengths, act = torch.zeros(S_, dtype=torch.int32, device=DEV), torch.ones(S_, dtype=torch.uint8, device=DEV)
    sc, new_ids = torch.zeros(S_, C, dtype=torch.uint8, device=DEV), torch.zeros(S_, dtype=torch.uint8, device=DEV)
    sargs = (S_, H_, HD_, x.data_ptr(), x.stride(0), x.data_ptr(), x.stride(0), x.data_ptr(), x.stride(0), kc.data_ptr(), vc.data_ptr(),
             C, 0, lengths.data_ptr(), act.data_ptr(), so.data_ptr(), so.stride(0), 0, None)
    for tail in ((sc.data_ptr(), new_ids.data_ptr(), H_, 1), (None, new_ids.data_ptr(), 1, 1), (sc.data_ptr(), None, 1, 1)):
        with pytest.raises(runtime.HipError):
            runtime.check(lib.m2f_attention_stream(*sargs, stream_heads(*tail)), "m2f_attention_stream")
    y = _rand(S_ * 2, E_, seed=2)
    yo = torch.full_like(y, 3.0)
    new = torch.full((S_,), 2, dtype=torch.int32, device=DEV)
    ids2 = torch.zeros(S_, 2, dtype=torch.uint8, device=DEV)
    cargs = (S_, 2, H_, HD_, y.data_ptr(), y.stride(0), y.data_ptr(), y.stride(0), y.data_ptr(), y.stride(0), kc.data_ptr(), vc.data_ptr(),
             C, 0, lengths.data_ptr(), new.data_ptr(), yo.data_ptr(), yo.stride(0), 0, None)
    for tail in ((sc.data_ptr(), ids2.data_ptr(), H_, 1), (None, ids2.data_ptr(), 1, 1), (sc.data_ptr(), None, 1, 1)):
        with pytest.raises(runtime.HipError):
            runtime.check(lib.m2f_attention_stream_chunk(*cargs, stream_heads(*tail)), "m2f_attention_stream_chunk")
    torch.cuda.synchronize()
    assert torch.all(out == 3.0) and torch.all(so == 3.0) and torch.all(yo == 3.0), "nothing was launched"
    with pytest.raises(ValueError, match="speaker_cache"):
        F.attention_stream(x, x, x, kc, vc, lengths, act, H_, speakers=new_ids, speaker_cache=sc[:, :2], speaker_heads=(1, 1))
