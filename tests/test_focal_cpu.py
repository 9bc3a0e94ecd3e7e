"""The focal criterion on the host: the float64 reference (tests/golden/focal_ref.py) against plain formulas and finite differences,
and everything of the Python surface that needs no device - the gamma checks of train_step / eval_step / M2FFocalLoss, build_criterion
of the drop-in loop and its runtime.focal_gamma knob, the shipped config."""
import math
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import distill_ref  # noqa: E402
import focal_ref as ref  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import runtime  # noqa: E402
from mer_amd.optim import M2FCrossEntropyLoss, M2FFocalLoss  # noqa: E402

W7 = [0.3, 1.2, 2.1, 1.3, 1.2, 5.3, 5.2]
GAMMAS = [0.25, 0.5, 1.0, 2.0, 5.0]


def _case(T, C, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(T, C, generator=g, dtype=torch.float64) * 2.0
    y = torch.randint(0, C, (T,), generator=g)
    y[torch.rand(T, generator=g) < 0.3] = -1
    return z, y


# ---- the reference against plain formulas -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_gamma_zero_is_torch_cross_entropy(weighted, eps):
    z, y = _case(300, 7, 3)
    w = torch.tensor(W7, dtype=torch.float64) if weighted else None
    loss, den, _, grad = ref.focal_loss_and_grad(z, y, w, eps, 0.0)
    zr = z.clone().requires_grad_(True)
    ce = torch.nn.CrossEntropyLoss(weight=w, ignore_index=-1, label_smoothing=eps)(zr, y)
    ce.backward()
    assert abs(loss.item() - ce.item()) <= 1e-12 and (grad - zr.grad).abs().max().item() <= 1e-12
    assert abs(den.item() - (w[y[y >= 0]].sum().item() if weighted else float((y >= 0).sum()))) <= 1e-12


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("T,C", [(257, 2), (300, 7), (257, 16)])
def test_unweighted_unsmoothed_is_the_textbook_focal_loss(T, C, gamma):
    z, y = _case(T, C, 11 * C + T)
    loss, den, _, _ = ref.focal_loss_and_grad(z, y, None, 0.0, gamma)
    v = y >= 0
    py = F.softmax(z[v], -1).gather(1, y[v][:, None])[:, 0]
    want = (-(1.0 - py) ** gamma * py.log()).mean()
    assert abs(loss.item() - want.item()) <= 1e-12 * max(1.0, abs(want.item()))
    assert den.item() == float(v.sum())


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("gamma", GAMMAS)
def test_gradient_by_finite_differences(gamma, weighted):
    z, y = _case(12, 7, 5)
    w = torch.tensor(W7, dtype=torch.float64) if weighted else None
    _, _, _, grad = ref.focal_loss_and_grad(z, y, w, 0.1, gamma)

    def f(x):
        num, den = ref.focal_terms(x, y, w, 0.1, gamma)
        return (num / den).item()

    h, worst = 1e-6, 0.0
    for t in range(z.shape[0]):
        for c in range(z.shape[1]):
            zp, zm = z.clone(), z.clone()
            zp[t, c] += h
            zm[t, c] -= h
            worst = max(worst, abs((f(zp) - f(zm)) / (2 * h) - grad[t, c].item()))
    assert worst <= 1e-8, worst
    assert float(grad[y < 0].abs().max()) == 0.0


@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_teacher_blend_scales_the_hard_term_only(gamma):
    z, y = _case(300, 7, 6)
    u = torch.randn(300, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(8)) * 4.0
    alpha, tau = 0.3, 2.0
    num, den = ref.focal_terms(z, y, None, 0.1, gamma, u, alpha, tau)
    hard, _ = ref.focal_terms(z, y, None, 0.1, gamma)
    soft, _ = distill_ref.distill_terms(z, u, y, None, 0.1, 1.0, tau)                 # alpha = 1: the teacher term alone
    assert abs(num.item() - ((1 - alpha) * hard.item() + alpha * soft.item())) <= 1e-10
    if gamma == 0.0:
        want, _ = distill_ref.distill_terms(z, u, y, None, 0.1, alpha, tau)
        assert abs(num.item() - want.item()) <= 1e-10


def test_confident_rows_are_finite_in_the_ref():
    z, y = _case(100, 7, 7)
    y = y.clamp(min=0)
    z[torch.arange(100), y] = z.max(-1).values + torch.linspace(4, 120, 100, dtype=torch.float64)
    for gamma in GAMMAS:
        loss, _, _, grad = ref.focal_loss_and_grad(z, y, None, 0.1, gamma)
        assert math.isfinite(loss.item()) and torch.isfinite(grad).all()


# ---- argument checks (no device) -------------------------------------------------------------------------------------------------
BAD_GAMMAS = [-0.1, 8.5, float("nan"), float("inf"), "2", True, (2.0,), [2.0]]


@pytest.mark.parametrize("bad", BAD_GAMMAS)
def test_check_focal_gamma_refuses_and_names_the_argument(bad):
    with pytest.raises(ValueError, match="my_gamma"):
        runtime.check_focal_gamma(bad, "my_gamma", "here")


def test_check_focal_gamma_accepts_the_range():
    assert runtime.check_focal_gamma(0) == 0.0 and runtime.check_focal_gamma(8) == 8.0 and runtime.check_focal_gamma(0.25) == 0.25
    assert isinstance(runtime.check_focal_gamma(2), float)


def test_steps_refuse_a_bad_gamma_before_they_touch_a_device():
    """The checks run first: a CPU model raises the ValueError, not the 'no CPU path' error of its engine."""
    from mer_amd.model import M2FNet
    cfg = synth._cfg(48, 64, 64, 4, 4, 4, 1, 1, 1)
    m = M2FNet(cfg)
    t, a, kp, y = synth.make_inputs(cfg, 2, 5, None, "randn", seed=1)
    for bad in BAD_GAMMAS:
        with pytest.raises(ValueError, match="focal_gamma"):
            m.train_step(t, a, kp, y, focal_gamma=bad)
        with pytest.raises(ValueError, match="focal_gamma"):
            m.eval().eval_step(t, a, kp, y, None, focal_gamma=bad)
        m.train()
    assert m._engine is None


def test_focal_loss_module():
    assert issubclass(M2FFocalLoss, M2FCrossEntropyLoss)
    c = M2FFocalLoss()
    assert isinstance(c, M2FCrossEntropyLoss) and (c.gamma, c.label_smoothing, c.weight) == (2.0, 0.1, None)
    w = torch.tensor(W7)
    c = M2FFocalLoss(weight=w, label_smoothing=0.0, gamma=1)
    assert c.gamma == 1.0 and torch.equal(c.weight, w) and "weight" in dict(c.named_buffers())
    with pytest.raises(ValueError, match="ignore_index"):
        M2FFocalLoss(ignore_index=0)
    for bad in BAD_GAMMAS:
        with pytest.raises(ValueError, match="gamma"):
            M2FFocalLoss(gamma=bad)
    c.gamma = 0.5                                                                           # a schedule sets it
    assert c.gamma == 0.5
    c.gamma = 9.0                                                                           # ... and a bad value is refused at the call, on the host
    with pytest.raises(ValueError, match="gamma"):
        c(torch.zeros(2, 7, 5), torch.zeros(2, 5, dtype=torch.int64))


def test_functional_refuses_a_bad_gamma_on_the_host():
    from mer_amd import functional as MF
    for bad in BAD_GAMMAS:
        with pytest.raises(ValueError, match="gamma"):
            MF.cross_entropy_focal(torch.zeros(4, 7), torch.zeros(4, dtype=torch.int64), None, 0.1, bad, True)


# ---- the drop-in loop ----------------------------------------------------------------------------------------------------------------
class _Labels:
    def get_labels(self):
        return [0] * 10 + [1, 2, 3, 4, 5, 6]


def _solver(loss_fn, balance=False):
    return types.SimpleNamespace(loss_fn=loss_fn, balance_classes=balance)


def test_build_criterion():
    import train as tr
    cpu = torch.device("cpu")
    ce = tr.build_criterion(_solver("CE"), _Labels(), cpu)
    assert type(ce) is M2FCrossEntropyLoss and ce.weight is None and ce.label_smoothing == 0.1
    assert type(tr.build_criterion(_solver("CE"), _Labels(), cpu, focal_gamma=3.0)) is M2FCrossEntropyLoss       # ignored under CE
    fl = tr.build_criterion(_solver("Focal"), _Labels(), cpu)
    assert type(fl) is M2FFocalLoss and fl.gamma == 2.0 and fl.weight is None and fl.label_smoothing == 0.1
    fl = tr.build_criterion(_solver("Focal", True), _Labels(), cpu, focal_gamma=0.5)
    cw = tr.build_criterion(_solver("CE", True), _Labels(), cpu)
    assert fl.gamma == 0.5 and fl.weight is not None and torch.equal(fl.weight, cw.weight) and fl.weight.numel() == 7
    for other in ("focal", "BCE", "MSE", None):
        with pytest.raises(ValueError, match="Criterion not supported"):
            tr.build_criterion(_solver(other), _Labels(), cpu)
    assert tr._focal_kw(ce) == {} and tr._focal_kw(fl) == {"focal_gamma": 0.5}
    fl.gamma = 1.0
    assert tr._focal_kw(fl) == {"focal_gamma": 1.0}
    assert tr._step_mode(types.SimpleNamespace(train_step=None), fl)[0]                       # the fused step takes the focal criterion


def test_config_knob():
    import train as tr
    import yaml
    with open(os.path.join(ROOT, "src", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["runtime"]["focal_gamma"] == 2.0 and cfg["solver"]["loss_fn"] == "CE"
    assert tr.focal_gamma_setting(cfg) == 2.0 and tr.focal_gamma_setting({}) == 2.0 and tr.focal_gamma_setting({"runtime": {}}) == 2.0
    assert tr.focal_gamma_setting({"runtime": {"focal_gamma": 0}}) == 0.0 and tr.focal_gamma_setting({"runtime": {"focal_gamma": 8}}) == 8.0
    for bad in (-1, 8.01, "2.0", None, True, float("nan"), [2.0]):
        with pytest.raises(ValueError, match="focal_gamma"):
            tr.focal_gamma_setting({"runtime": {"focal_gamma": bad}})
