"""The R-Drop criterion on the host: the float64 reference (tests/golden/rdrop_ref.py) against the usual recipe and against its closed-form
gradient, the twin map of every plan kind (runtime.rdrop_partner), and everything of the Python surface that needs no device - the
alpha checks, the refusals beside the other criteria, the drop-in loop's runtime.rdrop block and the shipped config."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import rdrop_ref as ref  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import runtime  # noqa: E402
from mer_amd.optim import M2FCrossEntropyLoss, M2FRDropLoss  # noqa: E402

ALPHAS = [0.0, 0.3, 1.0, 5.0]


def _views(B, L, C, seed):
    """Two views [B, L, C] of one batch with shared labels [B, L] (about 30 % unlabelled), as one [2B * L, C] block with the +B map."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(2 * B, L, C, generator=g, dtype=torch.float64) * 2.0
    y = torch.randint(0, C, (B, L), generator=g)
    y[torch.rand(B, L, generator=g) < 0.3] = -1
    partner = runtime.rdrop_partner(B, L, 2 * B * L, L=L)
    return z, y, partner


# ---- the reference against the usual recipe ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,L,C", [(5, 6, 7), (3, 11, 2), (4, 9, 16)])
def test_unweighted_reference_is_the_usual_recipe(B, L, C, eps, alpha):
    z, y, partner = _views(B, L, C, 17 * C + L)
    loss, den, num, kl, _ = ref.rdrop_loss_and_grad(z.reshape(-1, C), partner, torch.cat([y, y]).reshape(-1), None, eps, alpha)
    v = y.reshape(-1) >= 0
    z0, z1 = z[:B].reshape(-1, C)[v], z[B:].reshape(-1, C)[v]
    ce0 = F.cross_entropy(z0, y.reshape(-1)[v], label_smoothing=eps)
    ce1 = F.cross_entropy(z1, y.reshape(-1)[v], label_smoothing=eps)
    lp0, lp1 = F.log_softmax(z0, -1), F.log_softmax(z1, -1)
    kl01 = F.kl_div(lp0, lp1, reduction="batchmean", log_target=True)
    kl10 = F.kl_div(lp1, lp0, reduction="batchmean", log_target=True)
    want = 0.5 * (ce0 + ce1) + alpha * 0.5 * (kl01 + kl10)
    assert abs(loss.item() - want.item()) <= 1e-12 * max(1.0, abs(want.item())), (loss.item(), want.item())
    assert den.item() == 2.0 * float(v.sum())
    assert abs(kl.item() / den.item() - 0.5 * (kl01 + kl10).item()) <= 1e-12
    assert abs(num.item() - loss.item() * den.item()) <= 1e-10


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("T,C", [(74, 7), (300, 7), (257, 2), (257, 16)])
def test_autograd_gradient_is_the_closed_form(T, C, weighted, alpha):
    """A permuted twin map, class weights, label smoothing 0.1: what the kernel evaluates per row is the gradient of the whole sum."""
    z, partner, y, w = ref.random_pairs(T, C, 5 * C + T)
    z, w = z.double(), (w.double() if weighted else None)
    loss, den, num, kl, grad = ref.rdrop_loss_and_grad(z, partner, y, w, 0.1, alpha)
    closed = ref.closed_form_grad(z, partner, y, w, 0.1, alpha)
    err = (grad * den - closed).abs().max().item()
    assert err <= 1e-12, err
    assert kl.item() > 0.0 and abs(loss.item() - num.item() / den.item()) <= 1e-15
    if T % 2:                                        # the row without a twin is labelled: the plain term
        lone = int((partner < 0).nonzero()[0])
        assert int(y[lone]) >= 0
        plain = ref.closed_form_grad(z, torch.full_like(partner, -1), y, w, 0.1, alpha)
        assert torch.equal(closed[lone], plain[lone])


def test_alpha_zero_and_equal_twins_are_the_cross_entropy():
    z, partner, y, w = ref.random_pairs(300, 7, 3)
    z = z.double()
    zr = z.clone().requires_grad_(True)
    ce = torch.nn.CrossEntropyLoss(weight=w.double(), ignore_index=-1, label_smoothing=0.1)(zr, y)
    ce.backward()
    loss, _, _, kl, grad = ref.rdrop_loss_and_grad(z, partner, y, w, 0.1, 0.0)
    assert abs(loss.item() - ce.item()) <= 1e-12 and (grad - zr.grad).abs().max().item() <= 1e-12 and kl.item() > 0.0
    same = z.clone()
    has = partner >= 0
    same[has] = 0.5 * (z[has] + z[partner[has].long()])           # both rows of a pair hold the same logits
    loss, _, _, kl, grad = ref.rdrop_loss_and_grad(same, partner, y, w, 0.1, 5.0)
    sr = same.clone().requires_grad_(True)
    ce = torch.nn.CrossEntropyLoss(weight=w.double(), ignore_index=-1, label_smoothing=0.1)(sr, y)
    ce.backward()
    assert kl.item() == 0.0 and abs(loss.item() - ce.item()) <= 1e-12 and (grad - sr.grad).abs().max().item() <= 1e-12


# ---- the twin map ---------------------------------------------------------------------------------------------------------------------
def _check_map(partner, labels, real_rows):
    """An involution over exactly `real_rows` that pairs rows of one label; every other row holds -1."""
    T = partner.numel()
    has = partner >= 0
    assert partner.dtype == torch.int32 and bool((partner < T).all())
    assert sorted(has.nonzero().flatten().tolist()) == sorted(real_rows)
    idx = has.nonzero().flatten()
    tw = partner[idx].long()
    assert torch.equal(partner[tw].long(), idx) and bool((tw != idx).all())
    assert torch.equal(labels[tw], labels[idx])


def test_partner_of_a_padded_plan():
    B, L = 4, 6
    g = torch.Generator().manual_seed(1)
    y = torch.randint(-1, 7, (B, L), generator=g)
    p = runtime.rdrop_partner(B, L, 2 * B * L, L=L)
    _check_map(p, torch.cat([y, y]).reshape(-1), range(2 * B * L))
    assert torch.equal(p.view(2 * B, L)[:B].long(), torch.arange(B * L, 2 * B * L).view(B, L))      # (b, i) <-> (b + B, i)
    assert torch.equal(p.view(2 * B, L)[B:].long(), torch.arange(B * L).view(B, L))


def test_partner_of_a_bucketed_plan():
    """A 2 * 3 x 5 batch inside a plan of 8 x 8 slots: rows of the batch pair up across the views, filler rows hold -1."""
    b, l, PB, PL = 3, 5, 8, 8
    g = torch.Generator().manual_seed(2)
    y = torch.randint(-1, 7, (b, l), generator=g)
    labels = torch.full((PB, PL), -1, dtype=torch.int64)
    labels[: 2 * b, :l] = torch.cat([y, y])
    p = runtime.rdrop_partner(b, l, PB * PL, L=PL)
    real = [r * PL + i for r in range(2 * b) for i in range(l)]
    _check_map(p, labels.reshape(-1), real)
    assert int(p[0 * PL + 2]) == (0 + b) * PL + 2 and int(p[(2 + b) * PL + 4]) == 2 * PL + 4
    assert bool((p.view(PB, PL)[2 * b:] == -1).all()) and bool((p.view(PB, PL)[:, l:] == -1).all())
    with pytest.raises(ValueError, match="rdrop_partner"):
        runtime.rdrop_partner(b, l, 2 * b * PL - 1, L=PL)
    with pytest.raises(ValueError, match="rdrop_partner"):
        runtime.rdrop_partner(b, l, PB * PL, L=l - 1)


def _packed_rows(lengths, l, T, fillers=0):
    """The row map of Plan._set_inputs_packed for a doubled batch of these lengths (dst, valid), and the labels by token row."""
    n = len(lengths)
    valid = torch.zeros(2 * n, l, dtype=torch.bool)
    for b, k in enumerate(lengths):
        valid[b, :k] = True
        valid[b + n, :k] = True
    rank = torch.cumsum(valid, 1, dtype=torch.int64) - 1
    cu = torch.zeros(2 * n + 1, dtype=torch.int64)
    cu[1:] = torch.cumsum(valid.sum(1), 0)
    dst = torch.where(valid, cu[:-1, None] + rank, torch.full_like(rank, T - 1))
    g = torch.Generator().manual_seed(sum(lengths))
    y = torch.randint(0, 7, (n, l), generator=g)
    y2 = torch.cat([y, y])
    labels = torch.full((T,), -1, dtype=torch.int64)
    labels[dst[valid]] = y2[valid]
    return dst, valid, labels, int(cu[-1])


def test_partner_of_a_packed_ragged_plan():
    lengths, l, T = [1, 5, 3], 5, 64
    dst, valid, labels, used = _packed_rows(lengths, l, T)
    assert used == 18
    p = runtime.rdrop_partner(3, l, T, dst=dst, valid=valid)
    _check_map(p, labels, range(used))
    assert p[:9].tolist() == list(range(9, 18)) and p[9:18].tolist() == list(range(9))
    assert bool((p[used:] == -1).all())                       # filler rows and the spare row


def test_partner_of_a_one_utterance_dialogue():
    dst, valid, labels, used = _packed_rows([1], 1, 64)
    p = runtime.rdrop_partner(1, 1, 64, dst=dst, valid=valid)
    _check_map(p, labels, [0, 1])
    assert p[:2].tolist() == [1, 0]
    q = runtime.rdrop_partner(1, 1, 2, L=1)                   # ... and as a padded plan of 2 x 1
    assert q.tolist() == [1, 0]


def test_partner_of_a_full_packed_plan_keeps_the_last_row():
    """Every dialogue full and T = 2B * l: no spare row, row T - 1 is a real row with a twin."""
    dst, valid, labels, used = _packed_rows([4, 4], 4, 16)
    assert used == 16
    p = runtime.rdrop_partner(2, 4, 16, dst=dst, valid=valid)
    _check_map(p, labels, range(16))
    assert int(p[15]) == 7
    with pytest.raises(ValueError, match="rdrop_partner"):
        runtime.rdrop_partner(2, 4, 16, dst=dst[:3], valid=valid[:3])


# ---- argument checks (no device) -----------------------------------------------------------------------------------------------------
BAD_ALPHAS = [-0.1, -1, float("nan"), float("inf"), -float("inf"), "1", True, (1.0,)]


@pytest.mark.parametrize("bad", BAD_ALPHAS)
def test_check_rdrop_alpha_refuses_and_names_the_argument(bad):
    with pytest.raises(ValueError, match="my_alpha"):
        runtime.check_rdrop_alpha(bad, "my_alpha", "here")


def test_check_rdrop_alpha_accepts():
    assert runtime.check_rdrop_alpha(0) == 0.0 and runtime.check_rdrop_alpha(5) == 5.0 and runtime.check_rdrop_alpha(0.3) == 0.3
    assert isinstance(runtime.check_rdrop_alpha(1), float)
    from mer_amd.criterion import resolve
    spec = resolve("here", num_classes=7, cls_hidden=64, mask_shape=(2, 5), device="cpu", label_smoothing=0.1, class_weights=None,
                   rdrop=None, focal_gamma=2.0)
    assert spec.rdrop is None and spec.gamma == 2.0                                   # off: nothing to refuse


def test_steps_refuse_before_they_touch_a_device():
    """The checks run first: a CPU model raises the ValueError, not the 'no CPU path' error of its engine."""
    from mer_amd.crf import LinearChainCRF
    from mer_amd.distill import Distiller
    from mer_amd.model import M2FNet
    cfg = synth._cfg(48, 64, 64, 4, 4, 4, 1, 1, 1)
    m = M2FNet(cfg)
    t, a, kp, y = synth.make_inputs(cfg, 2, 5, None, "randn", seed=1)
    for bad in BAD_ALPHAS:
        with pytest.raises(ValueError, match="rdrop"):
            m.train_step(t, a, kp, y, rdrop=bad)
    teacher = torch.zeros(2, 5, m.m2f_config.cls_out)
    for kw, name in (({"teacher_logits": teacher, "distill": (0.5, 2.0)}, "teacher_logits"), ({"distill": (0.5, 2.0)}, "distill"),
                     ({"focal_gamma": 2.0}, "focal_gamma"), ({"focal_gamma": 0.0}, "focal_gamma"),
                     ({"crf": LinearChainCRF(m.m2f_config.cls_out), "label_smoothing": 0.0}, "crf")):
        with pytest.raises(ValueError, match=f"M2FNet.train_step: rdrop and {name} do not combine"):
            m.train_step(t, a, kp, y, rdrop=1.0, **kw)
    assert m._engine is None
    d = Distiller(m, M2FNet(cfg), alpha=0.5, temperature=2.0)
    with pytest.raises(ValueError, match="Distiller.train_step: rdrop and distill do not combine"):
        d.train_step(t, a, kp, y, rdrop=1.0)
    assert m._engine is None


def test_rdrop_loss_module_and_functional_refuse_on_the_host():
    from mer_amd import functional as MF
    assert issubclass(M2FRDropLoss, M2FCrossEntropyLoss)
    c = M2FRDropLoss()
    assert (c.alpha, c.label_smoothing, c.weight) == (1.0, 0.1, None)
    with pytest.raises(ValueError, match="ignore_index"):
        M2FRDropLoss(ignore_index=0)
    for bad in BAD_ALPHAS:
        with pytest.raises(ValueError, match="alpha"):
            M2FRDropLoss(alpha=bad)
        with pytest.raises(ValueError, match="alpha"):
            MF.cross_entropy_rdrop(torch.zeros(4, 7), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), None, 0.1, bad)
    c.alpha = -1.0                                            # a schedule sets it; a bad value is refused at the call, on the host
    with pytest.raises(ValueError, match="alpha"):
        c(torch.zeros(2, 5, 7), torch.zeros(2, 5, dtype=torch.int64))
    c.alpha = 1.0
    with pytest.raises(ValueError, match="twice"):
        c(torch.zeros(3, 5, 7), torch.zeros(3, 5, dtype=torch.int64))


# ---- the drop-in loop ------------------------------------------------------------------------------------------------------------------
def test_config_keys_and_settings():
    import train as tr
    import types
    import yaml
    with open(os.path.join(ROOT, "src", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["runtime"]["rdrop"] == {"enabled": False, "alpha": 1.0, "warmup_steps": 0}
    assert "rdrop" not in cfg["solver"] and "rdrop" not in cfg
    assert tr.rdrop_settings(cfg) is None and tr.rdrop_settings({}) is None and tr.rdrop_settings({"runtime": {}}) is None
    assert tr.rdrop_settings({"runtime": {"rdrop": {"enabled": True}}}) == {"alpha": 1.0, "warmup_steps": 0}
    on = {"runtime": {"rdrop": {"enabled": True, "alpha": 0.5, "warmup_steps": 4}}, "solver": {"loss_fn": "CE"}}
    assert tr.rdrop_settings(on) == {"alpha": 0.5, "warmup_steps": 4}
    for key, bad in (("alpha", -1), ("alpha", float("nan")), ("alpha", float("inf")), ("alpha", "1"), ("warmup_steps", -1),
                     ("warmup_steps", 1.5), ("warmup_steps", True), ("enabled", 1), ("gamma", 1.0)):
        with pytest.raises(ValueError, match="runtime.rdrop"):
            tr.rdrop_settings({"runtime": {"rdrop": {"enabled": True, key: bad}}})
    with pytest.raises(ValueError, match="fused_step"):
        tr.rdrop_settings({"runtime": {"fused_step": False, "rdrop": {"enabled": True}}})
    for other in ("Focal", "CRF"):
        with pytest.raises(ValueError, match="solver.loss_fn: CE"):
            tr.rdrop_settings({"runtime": {"rdrop": {"enabled": True}}, "solver": {"loss_fn": other}})
    with pytest.raises(ValueError, match="runtime.distill"):
        tr.rdrop_settings({"runtime": {"rdrop": {"enabled": True}, "distill": {"enabled": True, "teacher_checkpoint": "x.pt"}}})
    # the schedule: off -> no argument at all; on -> alpha, through a linear warm-up
    assert tr._rdrop_kw(types.SimpleNamespace(), 0) == {} and tr._rdrop_kw(types.SimpleNamespace(rdrop=None), 3) == {}
    m = types.SimpleNamespace(rdrop={"alpha": 2.0, "warmup_steps": 0})
    assert tr._rdrop_kw(m, 0) == {"rdrop": 2.0} and tr._rdrop_kw(m, 100) == {"rdrop": 2.0}
    m = types.SimpleNamespace(rdrop={"alpha": 2.0, "warmup_steps": 4})
    assert [tr._rdrop_kw(m, s)["rdrop"] for s in range(6)] == [0.5, 1.0, 1.5, 2.0, 2.0, 2.0]
