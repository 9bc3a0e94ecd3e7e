"""The supervised contrastive kernels on the device (functional.supcon, csrc/supcon.hip) against the float64 reference
(tests/golden/supcon_ref.py).

Bound, measured here and not chosen: the reference's own statements run as plain fp32 torch on the same inputs lie some distance from
float64; the kernels get 4 times the LARGEST such relative distance over the listed cases (the margin covers sum-order differences).
The gradient's distance is relative to the gradient's largest element, the loss's (con = sum of w l, summed in float64 from each
side's fp32 row terms) to the loss itself.  Exact properties: rows outside V and anchors without a positive give exactly 0, nothing is
NaN down to tau = 0.05 or for features scaled by 1e4, two runs give the same bits (the launch has no grid to choose: the tile and group
sizes are constants of the file).  Every comparison prints its figures before it asserts (-s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import supcon_ref as ref  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402

DEV = "cuda"
LAM = 0.7
# name: N, D, C, tau, ld, seed
CASES = {"1x8": (1, 8, 7, 0.1, None, 11), "2x8": (2, 8, 7, 0.1, None, 12), "33x20_ld24": (33, 20, 7, 0.07, 24, 13),
         "65x48": (65, 48, 7, 0.1, None, 14), "130x64": (130, 64, 3, 0.05, None, 15), "200x768": (200, 768, 7, 0.1, None, 16),
         "1040x768": (1040, 768, 7, 0.1, None, 17)}
DEGENERATE = ("1x8",)
_cache = {}


def _case(name):
    """inputs (on the device), float64 reference and the fp32-torch run of the same statements (both on the CPU), computed once."""
    if name not in _cache:
        N, D, C, tau, ld, seed = CASES[name]
        h, y, w = ref.random_case(N, D, C, seed, ld=ld)
        if name == "2x8":
            y[:] = 3                                   # the two rows are each other's positive
        r64 = ref.supcon(h, y, C, w, LAM, tau)
        r32 = ref.supcon(h, y, C, w, LAM, tau, dtype=torch.float32)
        hd = torch.zeros(N, ld or D, device=DEV)                   # (the row stride travels: a copy of the view alone would be contiguous)
        hd[:, :D] = h
        _cache[name] = (hd[:, :D], y.to(DEV), w.to(DEV), r64, r32)
    return _cache[name]


def _distances(rows, grad, r64):
    """(gradient distance / largest gradient element, loss distance / loss) of fp32 results from the float64 reference."""
    gmax = r64["grad"].abs().max().item()
    con = r64["con"].item()
    dg = (grad.double().cpu() - r64["grad"]).abs().max().item() / gmax if gmax > 0 else (grad.double().cpu() - r64["grad"]).abs().max().item()
    dl = abs(rows[:, 3].double().sum().item() - con) / abs(con) if con != 0 else abs(rows[:, 3].double().sum().item())
    return dg, dl


@pytest.fixture(scope="module")
def bound():
    """4 x the largest distance of the fp32 torch form over the listed cases: (gradient, loss)."""
    ds = {n: _distances(_case(n)[4]["rows"], _case(n)[4]["grad"], _case(n)[3]) for n in CASES}
    for n, (dg, dl) in ds.items():
        print(f"fp32 torch form, {n}: gradient {dg:.3e}, loss {dl:.3e}")
    bg, bl = 4 * max(d[0] for d in ds.values()), 4 * max(d[1] for d in ds.values())
    print(f"bound: gradient {bg:.3e}, loss {bl:.3e}")
    return bg, bl


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_match_the_float64_reference(name, bound):
    N, D, C, tau, ld, _ = CASES[name]
    h, y, w, r64, _ = _case(name)
    assert h.stride(0) == (ld or D)
    anchors = int(r64["has"].sum())
    print(f"{name}: {anchors} anchors with positives, {int(r64['valid'].sum())} rows in V of {N}")
    assert anchors >= 2 or name in DEGENERATE
    rows, grad = F.supcon(h, y, w, LAM, tau)
    assert torch.isfinite(rows).all() and torch.isfinite(grad).all()
    dg, dl = _distances(rows, grad, r64)
    print(f"{name}: kernels: gradient {dg:.3e} (bound {bound[0]:.3e}), loss {dl:.3e} (bound {bound[1]:.3e}); con {r64['con'].item()!r}")
    assert int((rows[:, 1] > 0).sum()) == anchors and torch.equal(rows[:, 1].double().cpu(), r64["rows"][:, 1])
    assert dg <= bound[0] and dl <= bound[1]
    rerr = (rows.double().cpu() - r64["rows"]).abs().max().item()
    print(f"{name}: row terms (lse, n, l, w l): largest difference {rerr:.3e}")
    assert rerr <= 1e-4
    # rows outside V: exact zeros everywhere; anchors of V without a positive: l and w l exactly 0
    out, lone = ~r64["valid"].to(DEV), ~r64["has"].to(DEV)
    assert not rows[out].any() and not grad[out].any()
    assert not rows[lone][:, 2:].any()
    if name not in DEGENERATE and N >= 8:
        assert bool(out.any()) and bool((lone & ~out).any())                   # the all-zero row / the single-member class are there


def test_two_runs_give_the_same_bits():
    for name in ("33x20_ld24", "200x768", "1040x768"):
        h, y, w, _, _ = _case(name)
        tau = CASES[name][3]
        a, b = F.supcon(h, y, w, LAM, tau), F.supcon(h, y, w, LAM, tau)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name


def test_all_unlabelled_and_all_singletons_cost_exactly_nothing():
    h, y, w, _, _ = _case("65x48")
    rows, grad = F.supcon(h, torch.full_like(y, -1), w, LAM, 0.1, n_classes=7)
    assert not rows.any() and not grad.any()
    h16 = h[:16]
    rows, grad = F.supcon(h16, torch.arange(16, device=DEV), None, LAM, 0.1, n_classes=16)      # every label once
    assert not rows[:, 1:].any() and not grad.any() and torch.isfinite(rows).all()
    rows0, grad0 = F.supcon(h, y, w, 0.0, 0.1)                                                  # weight 0: the terms, no gradient
    assert not grad0.any() and torch.equal(rows0, F.supcon(h, y, w, LAM, 0.1)[0])


@pytest.mark.parametrize("name", ["130x64", "200x768"])
def test_small_temperature_and_large_features_stay_finite_and_right(name, bound):
    N, D, C, _, _, _ = CASES[name]
    h, y, w, _, _ = _case(name)
    for scale, tau in ((1.0, 0.05), (1e4, 0.05), (1e4, 0.1)):
        hs = h * scale
        rows, grad = F.supcon(hs, y, w, LAM, tau)
        assert torch.isfinite(rows).all() and torch.isfinite(grad).all(), (scale, tau)
        r64 = ref.supcon(hs.cpu(), y.cpu(), C, w.cpu(), LAM, tau)
        r32 = ref.supcon(hs.cpu(), y.cpu(), C, w.cpu(), LAM, tau, dtype=torch.float32)
        dg, dl = _distances(rows, grad, r64)
        tg, tl = _distances(r32["rows"], r32["grad"], r64)
        print(f"{name} scale {scale:g} tau {tau}: kernels gradient {dg:.3e} loss {dl:.3e}; fp32 torch form gradient {tg:.3e} loss {tl:.3e}; "
              f"bound {bound[0]:.3e} / {bound[1]:.3e}")
        assert dg <= bound[0] and dl <= bound[1]
