"""functional.attention_weights (m2f_attention_weights, csrc/attention_weights.hip): the saved P^T of one attention site -> torch's
need_weights layouts.  Per head it is the transposed, masked view of the probs tensor bit for bit; averaged it is the sequential fp32
sum over the heads times fp32(1 / H) bit for bit; both sit within the probs bound (2e-5, tests/test_kernels_gpu.py) of the float64
softmax of tests/golden/band_ref.py; an element outside the dialogue, at a padded key or hidden by the band is exactly 0 whatever the
probs buffer held there (long dialogues: the forward skips those blocks); two runs give the same bits."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_maps_ref as A  # noqa: E402
import band_ref as R  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402

DEV = "cuda"
TOL = 2e-5

# (B, L, H, hd, lengths): one 32-tile and part of one / exactly 16 / three 16-tiles + 1, two 32-tiles / two full 32-tiles, a length-1 dialogue
SHAPES = [(3, 5, 3, 20, [5, 3, 1]), (2, 16, 1, 128, [16, 9]), (2, 33, 5, 12, [33, 17]), (2, 64, 8, 96, [64, 1])]
BANDS = [(None, None), (None, 0), (2, 0), (0, 0), (1, 1)]


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def _close(a, b, tol, what=""):
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item()
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, bound {tol * scale + 1e-7:.3e}")
    assert err <= tol * scale + 1e-7, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def _key_pad(B, L, lengths):
    kp = torch.zeros(B, L, dtype=torch.bool)
    for b, n in enumerate(lengths):
        kp[b, n:] = True
    return kp.to(DEV)


@pytest.mark.parametrize("band", BANDS, ids=lambda b: f"band{b[0]}_{b[1]}")
@pytest.mark.parametrize("B,L,H,hd,lengths", SHAPES)
def test_padded_sites_exact_and_against_float64(B, L, H, hd, lengths, band):
    E = H * hd
    q, k, v = (_rand(B * L, E, seed=200 + i) for i in range(3))
    kp = _key_pad(B, L, lengths)
    _, probs = F.attention_fwd(q, k, v, kp, B, L, H, past=band[0], future=band[1])
    hide = A.hidden(kp, L, band)
    want = A.masked_view(probs, B, H, L, hide)
    per_head = F.attention_weights(probs, B, L, H, key_pad=kp, past=band[0], future=band[1], average_heads=False)
    assert per_head.shape == (B, H, L, L) and per_head.is_contiguous()
    assert torch.equal(per_head, want)
    avg = F.attention_weights(probs, B, L, H, key_pad=kp, past=band[0], future=band[1])
    assert avg.shape == (B, L, L) and avg.is_contiguous()
    assert torch.equal(avg, A.head_average(want))
    # float64 (pad-query rows keep their softmax numbers; a row that sees no key is zeros on both sides)
    img = lambda t: t.double().view(B, L, E)          # noqa: E731
    _, p64 = R.attention(img(q), img(k), img(v), kp, H, return_probs=True, band=band)
    _close(per_head.double(), p64, TOL, "per head")
    _close(avg.double(), p64.mean(dim=1), TOL, "averaged")
    assert torch.all(per_head[hide.expand(B, H, L, L)] == 0)
    empty = ~R.visible_rows(kp, band)                                     # [B, L]: queries that see no key
    assert torch.all(avg[empty] == 0)
    rows = per_head.sum(-1)[(~empty)[:, None].expand(B, H, L)]
    assert (rows - 1).abs().max().item() < 1e-5                           # every row that sees a key is a distribution
    # the same bits on every run
    assert torch.equal(F.attention_weights(probs, B, L, H, key_pad=kp, past=band[0], future=band[1], average_heads=False), per_head)
    assert torch.equal(F.attention_weights(probs, B, L, H, key_pad=kp, past=band[0], future=band[1]), avg)


def test_no_key_pad_means_every_key_valid_and_a_dirty_probs_tail_is_not_read():
    """L = 5 sits in a 16 x 16 tile of probs: what lies outside [0, L) x [0, L) never reaches the result."""
    B, L, H, hd = 2, 5, 2, 8
    q, k, v = (_rand(B * L, H * hd, seed=210 + i) for i in range(3))
    kp = torch.zeros(B, L, dtype=torch.bool, device=DEV)
    _, probs = F.attention_fwd(q, k, v, kp, B, L, H)
    want = A.masked_view(probs, B, H, L, A.hidden(kp, L, (None, None)))
    dirty = probs.clone()
    dirty.view(B, H, 16, 16)[:, :, L:, :] = float("nan")
    dirty.view(B, H, 16, 16)[:, :, :, L:] = float("nan")
    assert torch.equal(F.attention_weights(dirty, B, L, H, average_heads=False), want)
    assert torch.equal(F.attention_weights(dirty, B, L, H), A.head_average(want))


# ---- long dialogues (attention_dlong.hip), packed ----------------------------------------------------------------------------------------
def _packed_case(lengths, H, hd, seed):
    B, L, E = len(lengths), max(lengths), H * hd
    cu = torch.tensor([0] + list(itertools.accumulate(lengths)), dtype=torch.int32)
    T = int(cu[-1]) + 3
    row = torch.full((B, L), T - 1, dtype=torch.long)
    for b, n in enumerate(lengths):
        row[b, :n] = torch.arange(int(cu[b]), int(cu[b]) + n)
    q, k, v = (_rand(T, E, seed=seed + i) for i in range(3))
    return dict(B=B, L=L, H=H, E=E, T=T, cu=cu.to(DEV), row=row.to(DEV), kp=_key_pad(B, L, lengths), q=q, k=k, v=v)


@pytest.mark.parametrize("band", [(None, None), (3, 0)], ids=["offline", "window3"])
def test_long_packed_dialogues_over_a_used_probabilities_buffer(band):
    lengths, H, hd = [200, 70, 1], 2, 16
    other = _packed_case(lengths, H, hd, seed=300)
    c = _packed_case(lengths, H, hd, seed=310)
    B, L = c["B"], c["L"]
    _, probs = F.attention_varlen_fwd(other["q"], other["k"], other["v"], B, L, H, cu=other["cu"])          # unbanded, other data
    assert torch.all(A.masked_view(probs, B, H, L, torch.zeros(B, 1, L, L, dtype=torch.bool, device=DEV))[0, :, 199, 0] > 0)
    _, probs = F.attention_varlen_fwd(c["q"], c["k"], c["v"], B, L, H, cu=c["cu"], past=band[0], future=band[1], probs=probs)
    per_head = F.attention_weights(probs, B, L, H, cu=c["cu"], past=band[0], future=band[1], average_heads=False)
    avg = F.attention_weights(probs, B, L, H, cu=c["cu"], past=band[0], future=band[1])
    own = ~c["kp"]                                                               # [B, L]: slots inside the dialogue
    hide = A.hidden(c["kp"], L, band) | ~own[:, None, :, None]                   # ... hidden, or a query behind the dialogue's end
    assert torch.all(per_head[hide.expand(B, H, L, L)] == 0), "hidden or out-of-dialogue elements must be exactly 0"
    assert torch.all(avg[hide[:, 0]] == 0)
    if band != (None, None):                                                     # the forward left the other launch's values there
        assert A.masked_view(probs, B, H, L, torch.zeros_like(hide))[0, :, 199, 0].min().item() > 0
    img = lambda t: (t[c["row"]] * own[..., None]).double()          # noqa: E731
    _, p64 = R.attention(img(c["q"]), img(c["k"]), img(c["v"]), c["kp"], H, return_probs=True, band=band)
    p64 = torch.where(hide.expand(B, H, L, L), torch.zeros_like(p64), p64)
    _close(per_head.double(), p64, TOL, "per head")
    _close(avg.double(), p64.mean(dim=1), TOL, "averaged")
    assert torch.equal(per_head, A.masked_view(probs, B, H, L, hide))
    assert torch.equal(avg, A.head_average(per_head))
    assert torch.equal(F.attention_weights(probs, B, L, H, cu=c["cu"], past=band[0], future=band[1], average_heads=False), per_head)
    assert torch.equal(F.attention_weights(probs, B, L, H, cu=c["cu"], past=band[0], future=band[1]), avg)
