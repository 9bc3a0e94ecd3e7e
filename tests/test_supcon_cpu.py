"""Host side of the supervised contrastive criterion: the float64 reference (tests/golden/supcon_ref.py) against float64 autograd of a
plain per-anchor loop, the argument checks (criterion.resolve), the drop-in parser (src/train.py supcon_settings) and the
shipped runtime.* keys.  No GPU."""
import os
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import supcon_ref as ref  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import runtime  # noqa: E402


@pytest.mark.parametrize("N,D,C,tau,weighted", [(1, 8, 7, 0.1, True), (2, 8, 7, 0.1, False), (33, 20, 7, 0.07, True), (65, 48, 7, 0.1, False),
                                                (130, 64, 3, 0.05, True)])
def test_reference_closed_form_is_autograd_of_the_anchor_loop(N, D, C, tau, weighted):
    h, y, w = ref.random_case(N, D, C, seed=7 * N)
    if N == 2:
        y[:] = 3
    w = w if weighted else None
    lam = 0.7
    r = ref.supcon(h, y, C, w, lam, tau)
    hd = h.double().clone().requires_grad_(True)
    loop = ref.loop_loss(hd, y, C, w, lam, tau)
    g = torch.autograd.grad(loop, hd)[0] if loop.grad_fn is not None else torch.zeros_like(hd)
    anchors = int(r["has"].sum())
    gmax = max(r["grad"].abs().max().item(), 1e-300)
    err_l, err_g = abs(loop.item() - lam * r["con"].item()), (g - r["grad"]).abs().max().item() / gmax
    print(f"N {N}: {anchors} anchors with positives; loss error {err_l:.3e}, gradient error {err_g:.3e} of its largest element")
    assert anchors >= 2 or N == 1
    assert err_l <= 1e-12 * max(1.0, abs(loop.item())) and err_g <= 1e-12
    # the reference's own autograd agrees with its closed form, and rows outside V / anchors without positives are exact zeros
    hd2 = h.double().clone().requires_grad_(True)
    r2 = ref.supcon(hd2, y, C, w, lam, tau)
    if r2["con"].grad_fn is not None:
        g2 = torch.autograd.grad(lam * r2["con"], hd2)[0]
        assert torch.isfinite(g2).all() and (g2 - r["grad"]).abs().max().item() <= 1e-12 * gmax
    assert not r["rows"][~r["valid"]].any() and not r["grad"][~r["valid"]].any() and not r["rows"][~r["has"]][:, 2:].any()
    if N >= 8:
        assert bool((~r["valid"] & (y >= 0)).any()) and bool((r["valid"] & ~r["has"]).any())     # the zero row, the single-member class


def test_reference_degenerate_batches_cost_nothing():
    h, y, w = ref.random_case(40, 16, 7, seed=1)
    r = ref.supcon(h, torch.full_like(y, -1), 7, w)
    assert not r["rows"].any() and not r["grad"].any() and r["den"].item() == 0.0
    r = ref.supcon(h[:7], torch.arange(7), 7, w)                       # singletons
    assert not r["rows"][:, 1:].any() and not r["grad"].any() and r["den"].item() > 0.0


def _check_supcon_args(who, supcon, **kw):
    """`supcon=` through criterion.resolve -> the checked (weight, temperature), or PLAIN for None"""
    from mer_amd.criterion import PLAIN, resolve
    spec = resolve(who, num_classes=7, cls_hidden=64, mask_shape=(4, 6), device="cpu", label_smoothing=0.0, class_weights=None,
                   supcon=supcon, **kw)
    return spec if spec is PLAIN else spec.supcon


def test_check_supcon_args():
    from mer_amd.crf import LinearChainCRF
    assert _check_supcon_args("step", None, focal_gamma=2.0) is None
    assert _check_supcon_args("step", (0, 1)) == (0.0, 1.0)
    assert _check_supcon_args("step", [0.25, 0.07]) == (0.25, 0.07)
    for bad in (0.1, (0.1,), (0.1, 0.1, 0.1), ("a", 0.1), (True, 0.1), (0.1, False), (-0.1, 0.1), (0.1, 0.0), (0.1, -1.0),
                (float("nan"), 0.1), (float("inf"), 0.1), (0.1, float("nan")), (0.1, float("inf"))):
        with pytest.raises(ValueError, match="step: supcon"):
            _check_supcon_args("step", bad)
    forms = {"teacher_logits": "distillation", "distill": "distillation", "focal_gamma": "focal", "crf": "CRF", "rdrop": "R-Drop"}
    # (valid values beside it: rdrop, which PRIORITY looks at before supcon, is checked before it)
    beside = {"teacher_logits": torch.zeros(4, 6, 7), "distill": (0.5, 2.0), "focal_gamma": 2.0, "crf": LinearChainCRF(7), "rdrop": 1.0}
    for name, form in forms.items():
        with pytest.raises(ValueError, match=f"step: supcon and {name} do not combine \\(the supervised contrastive criterion has no {form} form\\)"):
            _check_supcon_args("step", (0.1, 0.1), **{name: beside[name]})
    with pytest.raises(ValueError, match="DataParallelStep: supcon is refused"):
        _check_supcon_args("DataParallelStep", (0.1, 0.1), data_parallel=True)
    assert "m2f_plan_supcon" in runtime.SIGNATURES and "m2f_supcon" in runtime.SIGNATURES and "m2f_supcon_scratch_floats" in runtime.SIGNATURES
    assert (runtime.BUF_SUPCON, runtime.BUF_FEATURES) == (24, 25)


def test_header_and_bindings_agree():
    text = open(os.path.join(ROOT, "include", "m2fnet_hip.h")).read()
    assert "M2F_BUF_SUPCON = 24" in text and "M2F_BUF_FEATURES = 25" in text and "M2F_BUF_COUNT = 26" in text
    for name in ("m2f_plan_supcon", "m2f_supcon", "m2f_supcon_scratch_floats"):
        assert name + "(" in text


def test_drop_in_parser_and_shipped_keys(monkeypatch):
    monkeypatch.chdir(ROOT)
    import train as tr
    from utils import get_config
    cfg = get_config()
    assert dict(cfg.runtime.supcon) == {"enabled": False, "weight": 0.1, "temperature": 0.1, "warmup_steps": 0}
    assert tr.supcon_settings(cfg) is None and tr.supcon_settings({"runtime": {}}) is None
    on = {"enabled": True, "weight": 0.2, "temperature": 0.07, "warmup_steps": 4}
    assert tr.supcon_settings({"runtime": {"supcon": on}}) == {"weight": 0.2, "temperature": 0.07, "warmup_steps": 4}
    assert tr.supcon_settings({"runtime": {"supcon": {"enabled": True}}}) == {"weight": 0.1, "temperature": 0.1, "warmup_steps": 0}
    for bad, msg in (({"enabled": 1}, "enabled must be true or false"), ({"enabled": True, "weight": -1.0}, "weight"),
                     ({"enabled": False, "temperature": 0.0}, "temperature"), ({"enabled": True, "warmup_steps": -1}, "warmup_steps"),
                     ({"enabled": True, "warmup_steps": 1.5}, "warmup_steps"), ({"enabled": True, "alpha": 1.0}, "unknown key"),
                     ("yes", "must be a mapping")):
        with pytest.raises(ValueError, match="runtime.supcon.*" + msg):
            tr.supcon_settings({"runtime": {"supcon": bad}})
    base = {"enabled": True}
    with pytest.raises(ValueError, match="runtime.supcon.enabled needs runtime.fused_step: True"):
        tr.supcon_settings({"runtime": {"supcon": base, "fused_step": False}})
    with pytest.raises(ValueError, match="runtime.supcon.enabled needs solver.loss_fn: CE"):
        tr.supcon_settings({"runtime": {"supcon": base}, "solver": {"loss_fn": "Focal"}})
    with pytest.raises(ValueError, match="runtime.supcon.enabled does not combine with runtime.rdrop.enabled"):
        tr.supcon_settings({"runtime": {"supcon": base, "rdrop": {"enabled": True}}})
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="runtime.supcon.enabled runs in one process"):
        tr.supcon_settings({"runtime": {"supcon": base}})
    monkeypatch.delenv("WORLD_SIZE")
    # the schedule: weight * (step + 1) / n until n, the temperature constant
    m = type("M", (), {})()
    assert tr._supcon_kw(m, 0) == {}
    m.supcon = {"weight": 0.4, "temperature": 0.07, "warmup_steps": 4}
    assert [tr._supcon_kw(m, s)["supcon"] for s in (0, 1, 3, 9)] == [(0.1, 0.07), (0.2, 0.07), (0.4, 0.07), (0.4, 0.07)]
    m.supcon = {"weight": 0.4, "temperature": 0.07, "warmup_steps": 0}
    assert tr._supcon_kw(m, 0) == {"supcon": (0.4, 0.07)}
