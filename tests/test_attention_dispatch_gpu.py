"""Every instantiation of the four attention launchers is reached by the runtime flags that name it.  The launchers pick among the full
products of their boolean template flags (csrc/common.h, m2f_pick_bools); here each family is swept over that product at the smallest
shapes that still tell the flags apart, and every launch is compared in float64 with tests/golden/speaker_heads_ref.py swapped into the
oracle (`swapped_in(band, gain, speakers, heads)`) at the tolerances of tests/test_speaker_heads_kernels_gpu.py:
  short  NT 1..4 (L = 5, 17, 33, 49) x BAND x BIAS x SPK            32 launches: output and probabilities
  long   CTM 8 / 16 (hd = 8, 136), packed rows, x BAND x BIAS x SPK  16 launches: output and probabilities
  step   BF16 x PAGED x WEIGHTS x BIAS x SPK                         32 launches: output, and the weights rows where asked for
  chunk  BF16 x PAGED x BIAS x SPK                                   16 launches: output
An option that is on: band (1, 0), gain 1.0, heads (1, 1), two speakers alternating inside each dialogue.
A wrong pick must not pass, so each case first asserts a PRECONDITION on its inputs, on the CPU: for every option flag, the reference
with that flag toggled differs from the case's reference by more than 10x the bound in use on at least one compared element.  The
three flags that do not change the reference are told apart by construction: a dense kernel on page pools (16 rows per page, the slots'
pages swapped) or a kernel of the other cache type reads other bytes, and the weights buffer is NaN until the weights form writes it."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import speaker_heads_ref as R  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402
from oracle import m2fnet_oracle as O  # noqa: E402
from test_context_window_kernels_gpu import _close, _probs_view  # noqa: E402
from test_speaker_heads_kernels_gpu import TOL_OUT  # noqa: E402

DEV = "cuda"
ON_OFF = [False, True]
B_, H_ = 2, 4
S_, C_, T_, R_, HD_ = 2, 8, 2, 16, 8          # stream: slots, capacity, chunk rows, rows per page, head dim
CACHED = 3                                    # utterances a slot holds before the launch
E_ = H_ * HD_


def _options(band, bias, spk):
    return ((1, 0) if band else (None, None)), (1.0 if bias else None), ((1, 1) if spk else None)


def _ref(q, k, v, key_pad, band, gain, speakers, heads):
    """float64 (out [B, L, E], P [B, H, i, j]) of the oracle's attention with the options swapped in"""
    with R.swapped_in(band, gain, speakers, heads):
        return O.attention(q.double(), k.double(), v.double(), key_pad, H_, return_probs=True)


def _told_apart(compared, flags, tol):
    """The precondition.  compared(*flags) -> the float64 reference elements the case compares; every flag toggled must move them by more
    than 10x the bound `_close` applies to them."""
    mine = compared(*flags)
    bound = 10 * (tol * max(mine.abs().max().item(), 1e-6) + 1e-7)
    for i in range(len(flags)):
        other = list(flags)
        other[i] = not other[i]
        moved = (compared(*other) - mine).abs().max().item()
        print(f"flag {i} toggled moves the reference by {moved:.3e} (10x bound: {bound:.3e})")
        assert moved > bound, f"the inputs do not tell flag {i} of {flags} apart: {moved:.3e} <= {bound:.3e}"


# ---- short kernels: NT x BAND x BIAS x SPK ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _short_inputs(L):
    """B = 2, lengths (L, 3): q, k, v [B*L, E], key_pad and speakers [B, L], on the CPU"""
    g = torch.Generator().manual_seed(900 + L)
    q, k, v = (torch.randn(B_ * L, E_, generator=g) for _ in range(3))
    key_pad = torch.zeros(B_, L, dtype=torch.bool)
    key_pad[1, 3:] = True
    return q, k, v, key_pad, (torch.arange(L) % 2)[None, :].repeat(B_, 1)


@functools.lru_cache(maxsize=None)
def _short_ref(L, band, bias, spk):
    q, k, v, key_pad, ids = _short_inputs(L)
    return _ref(*(t.reshape(B_, L, E_) for t in (q, k, v)), key_pad, *_options(band, bias, spk)[:2], ids, _options(band, bias, spk)[2])


@pytest.mark.parametrize("spk", ON_OFF, ids=["", "spk"])
@pytest.mark.parametrize("bias", ON_OFF, ids=["", "bias"])
@pytest.mark.parametrize("band", ON_OFF, ids=["", "band"])
@pytest.mark.parametrize("L", [5, 17, 33, 49])
def test_short_forward_instantiations(L, band, bias, spk):
    _told_apart(lambda *f: _short_ref(L, *f)[0], (band, bias, spk), TOL_OUT)
    q, k, v, key_pad, ids = (t.to(DEV) for t in _short_inputs(L))
    (past, future), gain, heads = _options(band, bias, spk)
    out, probs = F.attention_fwd(q, k, v, key_pad, B_, L, H_, past=past, future=future, bias=gain, speakers=ids if spk else None,
                                 speaker_heads=heads)
    ro, rp = _short_ref(L, band, bias, spk)
    _close(out.reshape(B_, L, E_).double().cpu(), ro, TOL_OUT, "out")
    _close(_probs_view(probs, B_, H_, L).double().cpu(), rp, TOL_OUT, "probs")


# ---- long-dialogue kernels: CTM x BAND x BIAS x SPK -------------------------------------------------------------------------------------
LONG_L, LONG_LENGTHS = 70, (70, 3)


@functools.lru_cache(maxsize=None)
def _long_inputs(hd):
    """packed rows: q, k, v [T, E] and speakers [T]; their padded images [B, L, E] / [B, L] with key_pad; cu - on the CPU"""
    E, T = H_ * hd, sum(LONG_LENGTHS)
    g = torch.Generator().manual_seed(950 + hd)
    rows = [torch.randn(T, E, generator=g) for _ in range(3)]
    cu = torch.tensor([0, LONG_LENGTHS[0], T], dtype=torch.int32)
    key_pad = torch.ones(B_, LONG_L, dtype=torch.bool)
    imgs = [torch.zeros(B_, LONG_L, E) for _ in range(3)]
    ids = (torch.arange(LONG_L) % 2)[None, :].repeat(B_, 1)
    id_rows = torch.zeros(T, dtype=torch.int64)
    for b, n in enumerate(LONG_LENGTHS):
        key_pad[b, :n] = False
        id_rows[int(cu[b]):int(cu[b]) + n] = ids[b, :n]
        for img, r in zip(imgs, rows):
            img[b, :n] = r[int(cu[b]):int(cu[b]) + n]
    return rows, id_rows, imgs, ids, key_pad, cu


@functools.lru_cache(maxsize=None)
def _long_ref(hd, band, bias, spk):
    """(out, P) of the valid query rows only, dialogue after dialogue: [T, E] and [T, H, L]"""
    _, _, imgs, ids, key_pad, _ = _long_inputs(hd)
    o, p = _ref(*imgs, key_pad, *_options(band, bias, spk)[:2], ids, _options(band, bias, spk)[2])
    return o[~key_pad], p.permute(0, 2, 1, 3)[~key_pad]


@pytest.mark.parametrize("spk", ON_OFF, ids=["", "spk"])
@pytest.mark.parametrize("bias", ON_OFF, ids=["", "bias"])
@pytest.mark.parametrize("band", ON_OFF, ids=["", "band"])
@pytest.mark.parametrize("hd", [8, 136], ids=["ctm8", "ctm16"])
def test_long_forward_instantiations(hd, band, bias, spk):
    _told_apart(lambda *f: _long_ref(hd, *f)[0], (band, bias, spk), TOL_OUT)
    rows, id_rows, _, _, key_pad, cu = _long_inputs(hd)
    q, k, v = (t.to(DEV) for t in rows)
    (past, future), gain, heads = _options(band, bias, spk)
    out, probs = F.attention_varlen_fwd(q, k, v, B_, LONG_L, H_, cu=cu.to(DEV), past=past, future=future, bias=gain,
                                        speakers=id_rows.to(DEV) if spk else None, speaker_heads=heads)
    ro, rp = _long_ref(hd, band, bias, spk)
    _close(out.double().cpu(), ro, TOL_OUT, "out")
    # (a fresh buffer: what the band's skipped blocks leave unwritten is the zero the reference has there)
    P = _probs_view(probs, B_, H_, LONG_L).permute(0, 2, 1, 3).double().cpu()[~key_pad]
    _close(P, rp, TOL_OUT, "probs")


# ---- the stream step and chunk: BF16 x PAGED x (WEIGHTS) x BIAS x SPK -------------------------------------------------------------------------
N_ = CACHED + T_


@functools.lru_cache(maxsize=None)
def _stream_inputs(bf16):
    """N_ utterances of S_ dialogues: q, k, v [N_, S_, E_] (bf16: exact bf16 values - what the kernels round to once), speakers [N_, S_]"""
    g = torch.Generator().manual_seed(980)
    q, k, v = (torch.randn(N_, S_, E_, generator=g) for _ in range(3))
    if bf16:
        q, k, v = (t.to(torch.bfloat16).float() for t in (q, k, v))
    return q, k, v, (torch.arange(N_)[:, None] + torch.arange(S_)[None, :]) % 2


@functools.lru_cache(maxsize=None)
def _stream_ref(bf16, bias, spk):
    """(out [S_, N_, E_], P [S_, H_, N_, N_]) of the whole dialogues under the causal band of a plain cache"""
    q, k, v, ids = _stream_inputs(bf16)
    _, gain, heads = _options(False, bias, spk)
    return _ref(*(t.permute(1, 0, 2) for t in (q, k, v)), torch.zeros(S_, N_, dtype=torch.bool), (None, 0), gain, ids.t().contiguous(), heads)


def _stream_state(bf16, paged):
    """caches (or pools and table) that hold the first CACHED utterances, their speaker bytes and counts"""
    _, k, v, ids = _stream_inputs(bf16)
    held = [t[:CACHED].reshape(CACHED, S_, H_, HD_).permute(1, 2, 0, 3).to(DEV) for t in (k, v)]          # [S, H, row, hd]
    table = None
    if paged:
        table = torch.tensor([[1], [0]], dtype=torch.int32, device=DEV)          # ceil(C_ / R_) = 1 page per slot, swapped
        kc, vc = F.attention_stream_pools(S_, H_, HD_, R_, bf16=bf16, device=DEV)
        for c, rows in zip((kc, vc), held):
            for s in range(S_):
                c[int(table[s, 0]), :, :CACHED, :HD_] = rows[s].to(c.dtype)
    else:
        kc, vc = F.attention_stream_caches(S_, H_, HD_, C_, bf16=bf16, device=DEV)
        for c, rows in zip((kc, vc), held):
            c[:, :, :CACHED, :HD_] = rows.to(c.dtype)
    cached_ids = torch.full((S_, C_), 77, dtype=torch.uint8, device=DEV)          # (stale bytes behind the live count: never read)
    cached_ids[:, :CACHED] = ids[:CACHED].t().to(torch.uint8).to(DEV)
    return kc, vc, table, cached_ids, torch.full((S_,), CACHED, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("spk", ON_OFF, ids=["", "spk"])
@pytest.mark.parametrize("bias", ON_OFF, ids=["", "bias"])
@pytest.mark.parametrize("weights", ON_OFF, ids=["", "weights"])
@pytest.mark.parametrize("paged", ON_OFF, ids=["dense", "paged"])
@pytest.mark.parametrize("bf16", ON_OFF, ids=["fp32", "bf16"])
def test_stream_step_instantiations(bf16, paged, weights, bias, spk):
    _told_apart(lambda *f: _stream_ref(bf16, *f)[0][:, CACHED], (bias, spk), TOL_OUT)
    q, k, v, ids = (t[CACHED].to(DEV) for t in _stream_inputs(bf16))
    kc, vc, table, cached_ids, lengths = _stream_state(bf16, paged)
    _, gain, heads = _options(False, bias, spk)
    w = torch.full((S_, H_, C_), float("nan"), device=DEV) if weights else None
    kw = dict(bf16=bf16, weights=w, bias=gain)
    if spk:
        kw.update(speakers=ids, speaker_cache=cached_ids, speaker_heads=heads)
    act = torch.ones(S_, device=DEV)
    if paged:
        out = F.attention_stream_paged(q, k, v, kc, vc, table, lengths, act, H_, C_, **kw)
    else:
        out = F.attention_stream(q, k, v, kc, vc, lengths, act, H_, **kw)
    ro, rp = _stream_ref(bf16, bias, spk)
    _close(out.double().cpu(), ro[:, CACHED], TOL_OUT, "out")
    if weights:
        live = CACHED + 1
        _close(w[:, :, :live].double().cpu(), rp[:, :, CACHED, :live], TOL_OUT, "weights")
        assert torch.all(w[:, :, live:] == 0)


@pytest.mark.parametrize("spk", ON_OFF, ids=["", "spk"])
@pytest.mark.parametrize("bias", ON_OFF, ids=["", "bias"])
@pytest.mark.parametrize("paged", ON_OFF, ids=["dense", "paged"])
@pytest.mark.parametrize("bf16", ON_OFF, ids=["fp32", "bf16"])
def test_stream_chunk_instantiations(bf16, paged, bias, spk):
    _told_apart(lambda *f: _stream_ref(bf16, *f)[0][:, CACHED:], (bias, spk), TOL_OUT)
    q, k, v, ids = _stream_inputs(bf16)
    q, k, v = (t[CACHED:].permute(1, 0, 2).reshape(S_ * T_, E_).contiguous().to(DEV) for t in (q, k, v))          # row s*T + t
    kc, vc, table, cached_ids, lengths = _stream_state(bf16, paged)
    _, gain, heads = _options(False, bias, spk)
    kw = dict(bf16=bf16, bias=gain)
    if spk:
        kw.update(speakers=ids[CACHED:].t().contiguous().to(DEV), speaker_cache=cached_ids, speaker_heads=heads)
    new = torch.full((S_,), T_, dtype=torch.int32, device=DEV)
    if paged:
        out = F.attention_stream_chunk_paged(q, k, v, kc, vc, table, lengths, new, H_, T_, C_, **kw)
    else:
        out = F.attention_stream_chunk(q, k, v, kc, vc, lengths, new, H_, T_, **kw)
    ro, _ = _stream_ref(bf16, bias, spk)
    _close(out.view(S_, T_, E_).double().cpu(), ro[:, CACHED:], TOL_OUT, "out")
