"""The distillation criterion on the host: the float64 reference (tests/golden/distill_ref.py) against torch's own composition and
against the closed-form gradient the kernel implements, and every refusal of the Python surface that needs no device - the argument
checks of train_step / Distiller, runtime.distill of the drop-in loop, the shipped config block."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import distill_ref as ref  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import distill as D  # noqa: E402
from mer_amd.layout import M2FConfig  # noqa: E402

W7 = [0.3, 1.2, 2.1, 1.3, 1.2, 5.3, 5.2]


def _model_cfg(d_a=48, d_t=64, d_f=64, n_out=7, **kw):
    cfg = synth._cfg(d_a, d_t, d_f, 4, 4, 4, 1, 1, 1, **kw)
    cfg["CLASSIFIER"]["output_size"] = n_out
    return cfg


def _case(T, C, seed, t_scale=4.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(T, C, generator=g, dtype=torch.float64) * 2.0
    u = torch.randn(T, C, generator=g, dtype=torch.float64) * t_scale
    y = torch.randint(0, C, (T,), generator=g)
    y[torch.rand(T, generator=g) < 0.3] = -1
    return z, u, y


@pytest.mark.parametrize("alpha,tau", [(0.5, 2.0), (1.0, 1.0), (0.3, 4.0)])
@pytest.mark.parametrize("T,C", [(257, 2), (300, 7), (257, 16)])
def test_ref_equals_torch_batchmean_composition(T, C, alpha, tau):
    z, u, y = _case(T, C, 11 * C + T)
    loss, den, num, _ = ref.distill_loss_and_grad(z, u, y, None, 0.1, alpha, tau)
    v = y >= 0
    want = ((1 - alpha) * torch.nn.CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)(z, y)
            + alpha * tau ** 2 * F.kl_div(F.log_softmax(z[v] / tau, -1), F.softmax(u[v] / tau, -1), reduction="batchmean"))
    assert abs(loss.item() - want.item()) <= 1e-12 * max(1.0, abs(want.item()))
    assert den.item() == float(v.sum())


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("alpha,tau", [(0.5, 2.0), (1.0, 1.0), (0.3, 4.0)])
def test_ref_autograd_equals_the_closed_form(alpha, tau, weighted):
    z, u, y = _case(300, 7, 5)
    w = torch.tensor(W7, dtype=torch.float64) if weighted else None
    _, den, _, grad = ref.distill_loss_and_grad(z, u, y, w, 0.1, alpha, tau)
    g = ref.closed_form_grad(z, u, y, w, 0.1, alpha, tau)
    assert (grad - g / den).abs().max().item() <= 1e-14
    assert float(g[y < 0].abs().max()) == 0.0


@pytest.mark.parametrize("weighted", [False, True])
def test_alpha_zero_is_the_plain_cross_entropy(weighted):
    z, u, y = _case(300, 7, 6)
    w = torch.tensor(W7, dtype=torch.float64) if weighted else None
    loss, _, _, grad = ref.distill_loss_and_grad(z, u, y, w, 0.1, 0.0, 3.0)
    zr = z.clone().requires_grad_(True)
    ce = torch.nn.CrossEntropyLoss(weight=w, ignore_index=-1, label_smoothing=0.1)(zr, y)
    ce.backward()
    assert abs(loss.item() - ce.item()) <= 1e-14 and (grad - zr.grad).abs().max().item() <= 1e-15


def test_saturated_teacher_is_finite_in_the_ref():
    z, u, y = _case(300, 7, 7, t_scale=100.0)
    loss, _, _, grad = ref.distill_loss_and_grad(z, u, y, None, 0.1, 0.5, 1.0)
    assert math.isfinite(loss.item()) and torch.isfinite(grad).all()


# ---- argument checks (no device) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [(-0.1, 2.0), (1.5, 2.0), (float("nan"), 2.0), ("0.5", 2.0), (True, 2.0), (0.5, 0.0), (0.5, -1.0),
                                 (0.5, float("inf")), (0.5, float("nan")), (0.5, None), (0.5,), 0.5, (0.5, 2.0, 1.0)])
def test_check_distill_refuses(bad):
    with pytest.raises(ValueError):
        D.check_distill(bad)


def test_check_distill_accepts_the_range():
    assert D.check_distill((0, 1)) == (0.0, 1.0) and D.check_distill((1.0, 0.25)) == (1.0, 0.25)
    assert D.check_distill([0.5, 2]) == (0.5, 2.0)


def test_resolve_distill_args_both_or_neither_and_the_teacher_tensor():
    u = torch.zeros(4, 9, 7)
    cpu = torch.device("cpu")
    assert D.resolve_distill_args(None, None, 4, 9, 7, cpu) is None
    assert D.resolve_distill_args(u, (0.5, 2.0), 4, 9, 7, cpu) == (0.5, 2.0)
    for t, d in ((u, None), (None, (0.5, 2.0))):
        with pytest.raises(ValueError, match="go together"):
            D.resolve_distill_args(t, d, 4, 9, 7, cpu)
    for bad, what in ((u.double(), "float32"), (u[:, :8], "cls_out"), (u.reshape(36, 7), "cls_out"), (u.numpy(), "tensor"),
                      (torch.zeros(4, 9, 6), "cls_out")):
        with pytest.raises(ValueError, match=what):
            D.resolve_distill_args(bad, (0.5, 2.0), 4, 9, 7, cpu)
    with pytest.raises(ValueError, match="model is on"):
        D.resolve_distill_args(u, (0.5, 2.0), 4, 9, 7, torch.device("cuda:0"))
    with pytest.raises(ValueError, match="alpha"):
        D.resolve_distill_args(u, (2.0, 2.0), 4, 9, 7, cpu)


def test_train_step_refuses_before_it_touches_a_device():
    """The checks run first: a CPU model raises the ValueError, not the 'no CPU path' error of its engine."""
    from mer_amd.model import M2FNet
    cfg = _model_cfg()
    m = M2FNet(cfg)
    t, a, kp, y = synth.make_inputs(cfg, 2, 5, None, "randn", seed=1)
    u = torch.zeros(2, 5, 7)
    for kw in ({"teacher_logits": u}, {"distill": (0.5, 2.0)}, {"teacher_logits": u, "distill": (0.5, 0.0)},
               {"teacher_logits": u[..., :6], "distill": (0.5, 2.0)}, {"teacher_logits": u.half(), "distill": (0.5, 2.0)}):
        with pytest.raises(ValueError):
            m.train_step(t, a, kp, y, **kw)
    assert m._engine is None


def test_distiller_pair_checks_name_the_field():
    base = M2FConfig.from_model_config(_model_cfg())
    D.check_pair(base, M2FConfig.from_model_config(synth._cfg(48, 64, 128, 4, 4, 8, 2, 2, 3, ncls=3)))       # widths / depth may differ
    for other, field in ((_model_cfg(n_out=5), "cls_out"), (_model_cfg(d_a=40), "d_audio"), (_model_cfg(d_t=32), "d_text"),
                         (_model_cfg(a_on=False, f_on=False), "audio_enabled")):
        with pytest.raises(ValueError, match=field):
            D.check_pair(base, M2FConfig.from_model_config(other))
    from mer_amd.model import M2FNet
    s, t = M2FNet(_model_cfg()), M2FNet(_model_cfg(n_out=5))
    with pytest.raises(ValueError, match="cls_out"):
        D.Distiller(s, t)
    t = M2FNet(_model_cfg()).train()
    for bad in ((1.5, 2.0), (0.5, 0.0)):
        with pytest.raises(ValueError):
            D.Distiller(s, t, *bad)
    d = D.Distiller(s, t, alpha=0.25, temperature=3.0)
    assert (d.alpha, d.temperature) == (0.25, 3.0) and not t.training and not any(p.requires_grad for p in t.parameters())
    d.alpha = 0.75                                                                          # a schedule sets it
    assert d.alpha == 0.75


def test_distillation_loss_module_refuses_bad_settings():
    from mer_amd.optim import M2FDistillationLoss
    with pytest.raises(ValueError):
        M2FDistillationLoss(ignore_index=0)
    with pytest.raises(ValueError):
        M2FDistillationLoss(alpha=1.5)
    with pytest.raises(ValueError):
        M2FDistillationLoss(temperature=0.0)
    c = M2FDistillationLoss()
    assert (c.alpha, c.temperature, c.label_smoothing) == (0.5, 2.0, 0.1)
    with pytest.raises(ValueError, match="shape"):
        c(torch.zeros(2, 7, 5), torch.zeros(2, 5, dtype=torch.int64), torch.zeros(2, 5, 7))


# ---- the drop-in loop's block ------------------------------------------------------------------------------------------------------
DEFAULTS = {"enabled": False, "teacher_checkpoint": None, "teacher_weights": "model", "alpha": 0.5, "temperature": 2.0,
            "teacher_context": {"past": None, "future": None}}


def test_config_yaml_carries_the_block_with_its_defaults(monkeypatch):
    monkeypatch.chdir(ROOT)
    import yaml
    with open(os.path.join(ROOT, "src", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["runtime"]["distill"] == DEFAULTS
    import train as tr
    assert tr.resolve_distill(cfg) is None and tr.resolve_distill({"runtime": {}}) is None and tr.resolve_distill({}) is None


def test_resolve_distill():
    import train as tr
    on = dict(DEFAULTS, enabled=True, teacher_checkpoint="ck/teacher.pth")
    got = tr.resolve_distill({"runtime": {"distill": on}})
    assert got == {"checkpoint": "ck/teacher.pth", "weights": "model", "alpha": 0.5, "temperature": 2.0, "context": (None, None)}
    got = tr.resolve_distill({"runtime": {"distill": dict(on, teacher_weights="ema", alpha=1, temperature=4,
                                                          teacher_context={"past": 3, "future": 1})}})
    assert got == {"checkpoint": "ck/teacher.pth", "weights": "ema", "alpha": 1.0, "temperature": 4.0, "context": (3, 1)}
    assert tr.resolve_distill({"runtime": {"distill": {"enabled": True, "teacher_checkpoint": "x.pth"}}})["alpha"] == 0.5
    for bad, what in ((dict(on, teacher=1), "unknown key"), (dict(on, teacher_checkpoint=None), "teacher_checkpoint"),
                      (dict(on, teacher_checkpoint=""), "teacher_checkpoint"), (dict(on, teacher_weights="best"), "teacher_weights"),
                      (dict(on, alpha=1.5), "alpha"), (dict(on, temperature=0), "temperature"), (dict(on, enabled="yes"), "enabled"),
                      (dict(on, teacher_context={"past": -1, "future": None}), "teacher_context"),
                      (dict(on, teacher_context={"window": 2}), "teacher_context"), ([1, 2], "mapping")):
        with pytest.raises(ValueError, match=what):
            tr.resolve_distill({"runtime": {"distill": bad}})
    with pytest.raises(ValueError, match="fused_step"):
        tr.resolve_distill({"runtime": {"distill": on, "fused_step": False}})
    # a disabled block is still checked for keys and values, and asks for nothing
    assert tr.resolve_distill({"runtime": {"distill": dict(DEFAULTS), "fused_step": False}}) is None
    with pytest.raises(ValueError, match="unknown key"):
        tr.resolve_distill({"runtime": {"distill": dict(DEFAULTS, techer=1)}})
