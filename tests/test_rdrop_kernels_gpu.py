"""The R-Drop criterion kernel on the device (functional.cross_entropy_rdrop) against the float64 reference (tests/golden/rdrop_ref.py)
and its exact properties: alpha = 0 is the plain criterion bit for bit, twins with equal logits cost exactly nothing, unlabelled rows
are selected away whatever their twin rows hold, a twin index out of range means no twin, saturated rows stay finite and right.
Tolerances are those of tests/test_distill_gpu.py for this kernel family.  Every comparison prints its figures before it asserts (-s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import rdrop_ref as ref  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402

DEV = "cuda"
ALPHAS = [0.3, 1.0, 5.0]
SHAPES = [2 * 150, 2 * 129 - 1]                 # two workgroups each; the odd count leaves one labelled row without a twin


def _close(a, b, tol, what=""):
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item()
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, bound {tol * scale + 1e-7:.3e}")
    assert err <= tol * scale + 1e-7, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def _against_ref(z, partner, y, w, alpha, what):
    loss_r, den_r, num_r, kl_r, grad_r = ref.rdrop_loss_and_grad(z, partner, y, w, 0.1, alpha)
    for normalise in (True, False):
        out, dl = F.cross_entropy_rdrop(z, partner, y, w, 0.1, alpha, normalise)
        assert torch.isfinite(out).all() and torch.isfinite(dl).all()
        err, bound = abs(out[0].item() - loss_r.item()), 2e-6 * max(1.0, abs(loss_r.item()))
        print(f"{what} alpha {alpha} normalise {normalise}: loss {out[0].item()!r} ref {loss_r.item()!r} err {err:.3e} bound {bound:.3e}; "
              f"kl {out[3].item()!r} ref {kl_r.item()!r}")
        assert err <= bound
        assert abs(out[1].item() - den_r.item()) <= 1e-6 * den_r.item()
        assert abs(out[2].item() - num_r.item()) <= 2e-6 * max(1.0, abs(num_r.item()))
        assert abs(out[3].item() - kl_r.item()) <= 2e-6 * max(1.0, abs(kl_r.item()))           # the KL share, reported on its own
        _close((dl if normalise else dl / out[1]).double(), grad_r, 1e-5, f"{what} dlogits")


# ---- 1. the kernel against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [2, 7, 16])
@pytest.mark.parametrize("T", SHAPES)
def test_kernel_matches_the_float64_reference(T, C, weighted):
    z, partner, y, w = ref.random_pairs(T, C, 100 * C + T, device=DEV)
    assert int((partner < 0).sum()) == T % 2 and 0.2 < float((y < 0).float().mean()) < 0.4
    assert not torch.equal(partner.long().cpu(), (torch.arange(T) + T // 2) % T)             # a permuted map, not merely + T / 2
    for alpha in ALPHAS:
        _against_ref(z, partner, y, w if weighted else None, alpha, f"T {T} C {C} weighted {weighted}")


# ---- 2. alpha = 0: the plain criterion's bits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("T,C", [(300, 7), (257, 2), (257, 16)])
def test_alpha_zero_is_the_plain_criterion_bit_for_bit(T, C, weighted):
    z, partner, y, w = ref.random_pairs(T, C, 7 * C + T, device=DEV)
    w = w if weighted else None
    for normalise in (True, False):
        out, dl = F.cross_entropy_rdrop(z, partner, y, w, 0.1, 0.0, normalise)
        out0, dl0 = F.cross_entropy(z, y, w, 0.1, normalise)
        assert torch.equal(out[:3], out0[:3]) and torch.equal(dl, dl0), (normalise, (dl - dl0).abs().max().item())
        assert out[3].item() > 0.0                                                            # the KL share is still reported


# ---- 3. twins with equal logits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,C", [(300, 7), (257, 16), (257, 2)])
def test_equal_twins_cost_exactly_nothing(T, C):
    z, partner, y, w = ref.random_pairs(T, C, 31 + C, device=DEV)
    has = partner >= 0
    lo = torch.minimum(torch.arange(T, device=DEV), partner.long())
    z[has] = z[lo[has]]                                                                       # both rows of a pair: the same logits
    for cw in (None, w):
        for normalise in (True, False):
            out, dl = F.cross_entropy_rdrop(z, partner, y, cw, 0.1, 5.0, normalise)
            out0, dl0 = F.cross_entropy(z, y, cw, 0.1, normalise)
            assert out[3].item() == 0.0
            assert torch.equal(out[:3], out0[:3]) and torch.equal(dl, dl0)


# ---- 4. invalid rows and missing twins are a select ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,C", [(300, 7), (257, 16)])
def test_unlabelled_rows_ignore_their_twin_rows(T, C):
    z, partner, y, w = ref.random_pairs(T, C, 41 + C, device=DEV)
    idx = ((y < 0) & (partner >= 0)).nonzero().flatten()                  # unlabelled rows; their twins are unlabelled too
    assert idx.numel() > 30
    tw = partner[idx].long()
    bad = z.clone()
    fill = torch.tensor([float("nan"), float("inf"), -float("inf")], device=DEV)
    bad[tw] = fill[torch.arange(tw.numel(), device=DEV) % 3][:, None]
    bad[tw[0], 0], bad[tw[0], 1:] = float("inf"), float("nan")              # (mixed within one row too)
    zeroed = z.clone()
    zeroed[tw] = 0.0
    for normalise in (True, False):
        a = F.cross_entropy_rdrop(bad, partner, y, w, 0.1, 1.0, normalise)
        b = F.cross_entropy_rdrop(zeroed, partner, y, w, 0.1, 1.0, normalise)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all() and float(a[1][idx].abs().max()) == 0.0
    # an out-of-range label is invalid as well: the pair's rows are selected away like the unlabelled ones
    y2 = y.clone()
    y2[idx[:5]] = C
    y2[tw[:5]] = C
    a = F.cross_entropy_rdrop(bad, partner, y2, w, 0.1, 1.0, True)
    b = F.cross_entropy_rdrop(zeroed, partner, y, w, 0.1, 1.0, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("T,C", [(300, 7), (257, 16)])
def test_a_twin_index_out_of_range_means_no_twin(T, C):
    """Labelled rows whose twin index is -1, T, T + 5 or far out get the plain term; the rest of the batch is untouched."""
    z, partner, y, w = ref.random_pairs(T, C, 61 + C, device=DEV)
    lab = ((y >= 0) & (partner >= 0)).nonzero().flatten()[:8]
    cut = partner.clone()
    for i, r in enumerate(lab.tolist()):                                   # both rows of the pair lose their twin
        t = int(partner[r])
        cut[r] = [-1, T, T + 5, 2 ** 31 - 1, -(2 ** 31), -7, T, -1][i]
        cut[t] = [T, -1, -3, T + 1, 2 ** 31 - 1, T, -1, T][i]
    none = partner.clone()
    none[lab] = -1
    none[partner[lab].long()] = -1
    a = F.cross_entropy_rdrop(z, cut, y, w, 0.1, 1.0, True)
    b = F.cross_entropy_rdrop(z, none, y, w, 0.1, 1.0, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.isfinite(a[1]).all()
    _against_ref(z, cut, y, w, 1.0, f"cut twins T {T} C {C}")
    # with every twin gone: the plain criterion, bit for bit, at any alpha
    out, dl = F.cross_entropy_rdrop(z, torch.full_like(partner, -1), y, w, 0.1, 5.0, True)
    out0, dl0 = F.cross_entropy(z, y, w, 0.1, True)
    assert torch.equal(out[:3], out0[:3]) and torch.equal(dl, dl0) and out[3].item() == 0.0


# ---- 5. saturated rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,C", [(300, 7), (257, 16), (257, 2)])
def test_saturated_rows_stay_finite_and_right(T, C):
    z, partner, y, w = ref.random_pairs(T, C, 51 + C, scale=200.0, device=DEV)                 # (logits of the usual scale, times 100)
    assert float(torch.softmax(z.double(), -1).float().min()) == 0.0                            # probabilities do underflow in fp32
    for cw in (None, w):
        for alpha in (1.0, 5.0):
            _against_ref(z, partner, y, cw, alpha, f"saturated T {T} C {C}")


def test_margins_of_120_are_finite_for_any_alpha():
    T, C = 256, 7
    z, partner, y, w = ref.random_pairs(T, C, 77, device=DEV)
    z = torch.where(torch.rand(T, C, device=DEV) < 0.5, torch.full_like(z, 120.0), torch.full_like(z, -120.0))
    for alpha in (0.0, 1.0, 1.0e4):
        out, dl = F.cross_entropy_rdrop(z, partner, y, w, 0.1, alpha, False)
        assert torch.isfinite(out).all() and torch.isfinite(dl).all()
