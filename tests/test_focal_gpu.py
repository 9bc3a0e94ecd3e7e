"""The focal criterion on the device: the kernel against the float64 reference (tests/golden/focal_ref.py), confident rows (the other
classes' probabilities underflow), its exact properties (gamma = 0 is the plain / distillation criterion bit for bit, invalid rows are
selected away), the eval form, the train step against the autograd path on every plan kind, switching and gamma schedules under
graphs, every training mode, the Distiller and the drop-in loop.  Every comparison prints its figures before it asserts (-s)."""
import os
import sys

import numpy as np
import pandas as pd
import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import focal_ref as ref  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import dp  # noqa: E402
from mer_amd import functional as F  # noqa: E402
from mer_amd.distill import Distiller  # noqa: E402
from mer_amd.metrics import DeviceScores  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam, M2FFocalLoss  # noqa: E402

DEV = "cuda"
CFG = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2, ncls=7)          # dropout 0
GAMMAS = [0.25, 0.5, 1.0, 2.0, 5.0]
W7 = [0.3, 1.2, 2.1, 1.3, 1.2, 5.3, 5.2]


def _rows(T, C, seed, t_scale=4.0):
    """tests/test_distill_gpu.py's rows: 30 % of the labels -1."""
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(T, C, generator=g) * 2.0).to(DEV)
    u = (torch.randn(T, C, generator=g) * t_scale).to(DEV)
    y = torch.randint(0, C, (T,), generator=g)
    y[torch.rand(T, generator=g) < 0.3] = -1
    w = (0.3 + 5.0 * torch.rand(C, generator=g)).to(DEV)
    return z, u, y.to(DEV), w


def _confident(T, C, seed):
    """`_rows`, but 100 rows carry a valid label whose logit leads the others by linspace(4, 120): from a margin of about 17 on p_y
    rounds to 1 in fp32, from about 104 on every other class's expf underflows (omp == 0)."""
    z, u, y, w = _rows(T, C, seed)
    idx = torch.arange(0, 100, device=DEV) * (T // 100)
    g = torch.Generator().manual_seed(seed + 1)
    yc = torch.randint(0, C, (100,), generator=g).to(DEV)
    y[idx] = yc
    rows = z[idx]
    rows[torch.arange(100, device=DEV), yc] = -1e30
    lead = rows.max(-1).values + torch.linspace(4, 120, 100, device=DEV)
    z[idx, yc] = lead
    return z, u, y, w, idx


def _against_ref(z, y, w, gamma, what, teacher=None, alpha=0.0, tau=1.0):
    """The bounds of the issue: loss within 2e-6 * max(1, |loss|); gradient within 2e-5 of the reference's largest magnitude + 1e-7."""
    loss_r, den_r, num_r, grad_r = ref.focal_loss_and_grad(z, y, w, 0.1, gamma, teacher, alpha, tau)
    for normalise in (True, False):
        out, dl = F.cross_entropy_focal(z, y, w, 0.1, gamma, normalise, teacher, alpha, tau)
        assert torch.isfinite(out[:3]).all() and torch.isfinite(dl).all(), (what, gamma, normalise)
        err, bound = abs(out[0].item() - loss_r.item()), 2e-6 * max(1.0, abs(loss_r.item()))
        g = (dl if normalise else dl / out[1]).double()
        gerr, gbound = (g - grad_r).abs().max().item(), 2e-5 * grad_r.abs().max().item() + 1e-7
        print(f"{what} gamma {gamma} normalise {normalise}: loss {out[0].item()!r} ref {loss_r.item()!r} err {err:.3e} bound {bound:.3e}; "
              f"gradient err {gerr:.3e} bound {gbound:.3e} (of the largest: {gerr / grad_r.abs().max().item():.3e})")
        assert err <= bound
        assert abs(out[1].item() - den_r.item()) <= 1e-6 * den_r.item() and abs(out[2].item() - num_r.item()) <= 2e-6 * max(1.0, abs(num_r.item()))
        assert gerr <= gbound


# ---- 1. the kernel against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [2, 7, 16])
@pytest.mark.parametrize("T", [300, 257])
def test_kernel_matches_the_float64_reference(T, C, weighted):
    z, u, y, w = _rows(T, C, 100 * C + T)
    for gamma in GAMMAS:
        _against_ref(z, y, w if weighted else None, gamma, f"T {T} C {C} weighted {weighted}")
    _against_ref(z, y, w if weighted else None, 2.0, f"T {T} C {C} weighted {weighted} teacher", u, 0.5, 2.0)


# ---- 2. confident rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [2, 7, 16])
def test_confident_rows_are_finite_and_right(C, weighted):
    z, u, y, w, idx = _confident(300, C, 200 + C)
    p = torch.softmax(z[idx], -1)
    others = p.sum(-1) - p.gather(1, y[idx][:, None])[:, 0]
    assert float(p.max(-1).values.max()) == 1.0 and int((torch.softmax(z[idx], -1) == 0).any(-1).sum()) > 5      # p_y rounds to 1; others underflow
    print(f"C {C}: rows whose 1 - p_y is 0 in fp32: {int((others == 0).sum())} of 100")
    for gamma in GAMMAS:
        _against_ref(z, y, w if weighted else None, gamma, f"confident C {C} weighted {weighted}")
    _against_ref(z, y, w if weighted else None, 0.5, f"confident C {C} weighted {weighted} teacher", u, 0.5, 2.0)
    for gamma in (0.01, 0.1, 7.9, 8.0):                        # (the ends of the range: nothing overflows, nothing is NaN)
        out, dl = F.cross_entropy_focal(z, y, w if weighted else None, 0.1, gamma, True)
        assert torch.isfinite(out[:3]).all() and torch.isfinite(dl).all(), gamma


# ---- 3. exact properties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("T,C", [(300, 7), (257, 2), (257, 16)])
def test_gamma_zero_is_the_plain_and_the_distillation_criterion_bit_for_bit(T, C, weighted):
    for z, u, y, w in (_rows(T, C, 7 * C + T), _confident(300, C, 9 * C)[:4]):
        w = w if weighted else None
        for normalise in (True, False):
            out, dl = F.cross_entropy_focal(z, y, w, 0.1, 0.0, normalise)
            out0, dl0 = F.cross_entropy(z, y, w, 0.1, normalise)
            assert torch.equal(out, out0) and torch.equal(dl, dl0), (normalise, (dl - dl0).abs().max().item())
            for alpha, tau in ((0.5, 2.0), (0.3, 3.7), (0.0, 1.0)):
                out, dl = F.cross_entropy_focal(z, y, w, 0.1, 0.0, normalise, u, alpha, tau)
                out0, dl0 = F.cross_entropy_distill(z, u, y, w, 0.1, alpha, tau, normalise)
                assert torch.equal(out, out0) and torch.equal(dl, dl0), (normalise, alpha, tau, (dl - dl0).abs().max().item())


@pytest.mark.parametrize("T,C", [(300, 7), (257, 16)])
def test_invalid_rows_are_a_select_of_zeros(T, C):
    z, u, y, w = _rows(T, C, 41 + C)
    idx = (y < 0).nonzero().flatten()
    assert idx.numel() > 30
    fill = torch.tensor([float("nan"), float("inf"), -float("inf")], device=DEV)
    pattern = fill[torch.arange(idx.numel(), device=DEV) % 3][:, None]
    bad_z, bad_u = z.clone(), u.clone()
    bad_z[idx], bad_u[idx] = pattern, pattern.flip(0)
    bad_z[idx[0], 0], bad_z[idx[0], 1:] = float("inf"), float("nan")          # (mixed within one row too)
    zero_z, zero_u = z.clone(), u.clone()
    zero_z[idx], zero_u[idx] = 0.0, 0.0
    for gamma in (0.0, 0.5, 2.0):
        for teacher in (False, True):
            for normalise in (True, False):
                a = F.cross_entropy_focal(bad_z, y, w, 0.1, gamma, normalise, bad_u if teacher else None, 0.5, 2.0)
                b = F.cross_entropy_focal(zero_z, y, w, 0.1, gamma, normalise, zero_u if teacher else None, 0.5, 2.0)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (gamma, teacher, normalise)
                assert torch.isfinite(a[0][:3]).all() and torch.isfinite(a[1]).all() and float(a[1][idx].abs().max()) == 0.0
    # an out-of-range label is invalid as well
    y2 = y.clone()
    y2[idx[:5]] = C
    y2[idx[5:8]] = -7
    a = F.cross_entropy_focal(bad_z, y2, w, 0.1, 2.0, True, bad_u, 0.5, 2.0)
    b = F.cross_entropy_focal(zero_z, y, w, 0.1, 2.0, True, zero_u, 0.5, 2.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 4. the eval form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("T,C", [(300, 7), (257, 2), (257, 16), (33000, 7)])         # (33000 rows: more than 128 workgroups, the rows launch strides)
def test_eval_scores_carry_the_train_kernels_loss(T, C, weighted):
    z, _, y, w = _confident(T, C, 61 + C)[:4]
    w = w if weighted else None
    plain = DeviceScores(C, DEV)
    plain.update(z, y, w, 0.1)
    for gamma in [0.0] + GAMMAS:
        s = DeviceScores(C, DEV)
        s.update(z, y, w, 0.1, focal_gamma=gamma)
        out, _ = F.cross_entropy_focal(z, y, w, 0.1, gamma, True)
        print(f"T {T} C {C} gamma {gamma}: eval loss {s.last()[0].item()!r}, criterion loss {out[0].item()!r}")
        assert torch.equal(s.last()[0], out[0].double())
        assert torch.equal(s.last()[1:], plain.last()[1:]) and torch.equal(s.record[8:], plain.record[8:])      # accuracy, F1, confusion matrix
        if gamma == 0.0:
            assert torch.equal(s.record, plain.record)
    with pytest.raises(ValueError, match="focal_gamma"):
        plain.update(z, y, w, 0.1, focal_gamma=9.0)


# ---- models --------------------------------------------------------------------------------------------------------------------------------
def _model(precision="fp32", context=None, cfg=CFG, seed=None, packed=None):
    m = M2FNet(cfg, precision=precision, context=context, packed=packed)
    sd = synth.make_state_dict(cfg)
    if seed is not None:                                    # other weights of the same shapes (a teacher)
        g = torch.Generator().manual_seed(seed)
        sd = {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in sd.items()}
    m.load_state_dict(sd)
    return m.to(DEV).train()


def _batch(B, L, seed, lengths=None):
    if lengths is None:
        g = torch.Generator().manual_seed(seed)
        lengths = [L] + [int(x) for x in torch.randint(1, L + 1, (B - 1,), generator=g)]
    return [t.to(DEV) for t in synth.make_inputs(CFG, B, L, lengths, "randn", seed=seed)]


def _teacher_rows(B, L, seed, C=7):
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.randn(B, L, C, generator=g) * 2.0).to(DEV)


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _same_grads(ga, gb, what):
    """tests/test_distill_gpu.py's step tolerance."""
    worst = 0.0
    for k in ga:
        err, bound = (ga[k] - gb[k]).abs().max().item(), 1e-6 + 1e-4 * ga[k].abs().max().item()
        worst = max(worst, err / bound)
        assert err <= bound, (what, k, err, bound)
    print(f"{what}: worst gradient error / bound {worst:.3f}")


def _equal_grads(ma, mb, what):
    for (k, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(p.grad, q.grad), (what, k, (p.grad - q.grad).abs().max().item())


def _last_plan(m):
    return m.engine().plans[next(reversed(m.engine().plans))]


def test_eval_step_scores_the_focal_criterion():
    t, a, kp, em = _batch(6, 12, 3)
    m = _model().eval()
    with torch.no_grad():
        logits = m(t, a, kp)
    w = torch.tensor(W7, device=DEV)
    for cw in (None, w):
        got, want, plain = DeviceScores(7, DEV), DeviceScores(7, DEV), DeviceScores(7, DEV)
        for use_graph in (False, True, True):
            m.eval_step(t, a, kp, em, got, class_weights=cw, focal_gamma=2.0, use_graph=use_graph)
        want.update(logits, em, cw, 0.1, focal_gamma=2.0)
        m.eval_step(t, a, kp, em, plain, class_weights=cw, use_graph=True)
        # (the plan scores its own token rows - a bucket's filler rows add zeros -, so only the order of the sum differs)
        err = abs(got.last()[0].item() - want.last()[0].item())
        print(f"eval_step loss {got.last()[0].item()!r}, DeviceScores.update {want.last()[0].item()!r}, plain {plain.last()[0].item()!r}")
        assert err <= 2e-6 * max(1.0, abs(want.last()[0].item())) and got.n_batches == 3
        assert torch.equal(got.last()[1:], plain.last()[1:]) and not torch.equal(got.last()[0], plain.last()[0])
        # ... and None afterwards is the plain record again, bit for bit
        again, fresh = DeviceScores(7, DEV), DeviceScores(7, DEV)
        m.eval_step(t, a, kp, em, again, class_weights=cw, use_graph=True)
        _model().eval().eval_step(t, a, kp, em, fresh, class_weights=cw, use_graph=True)
        assert torch.equal(again.record, fresh.record)


# ---- 5. the train step against autograd ----------------------------------------------------------------------------------------------------
PLAN_KINDS = {"padded_6x12": (6, 12, 1, [12, 12, 11, 12, 12, 12], None), "packed_6x12": (6, 12, 2, [12, 3, 5, 1, 7, 2], True),
              "long_2x70": (2, 70, 3, [70, 23], None)}


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("kind", list(PLAN_KINDS))
def test_step_matches_the_autograd_path(kind, use_graph):
    B, L, seed, lengths, packed = PLAN_KINDS[kind]
    t, a, kp, em = _batch(B, L, seed, lengths)
    gamma = 2.0
    for cw in (None, torch.tensor(W7, device=DEV)):
        ma = _model(packed=packed)
        for _ in range(3 if use_graph else 1):               # eager warm-up, capture, replay
            la = ma.train_step(t, a, kp, em, class_weights=cw, focal_gamma=gamma, use_graph=use_graph)
        assert _last_plan(ma).packed == (kind != "padded_6x12")
        ga = _grads(ma)
        mb = _model()
        lb = M2FFocalLoss(weight=cw, gamma=gamma)(mb(t, a, kp).permute(0, 2, 1), em)
        lb.backward()
        print(f"{kind} graph {use_graph} weighted {cw is not None}: step loss {la.item()!r}, autograd loss {lb.item()!r}")
        assert abs(la.item() - lb.item()) <= 1e-5
        _same_grads(ga, _grads(mb), f"{kind} step vs M2FFocalLoss")
        if cw is None:                                       # ... and against torch's own composition
            mc = _model()
            out = mc(t, a, kp)
            v = em >= 0
            lp = TF.log_softmax(out[v], -1)
            py = lp.gather(1, em[v][:, None])[:, 0].exp()
            rows = TF.cross_entropy(out[v], em[v], reduction="none", label_smoothing=0.1)
            lc = ((1.0 - py) ** gamma * rows).mean()
            lc.backward()
            assert abs(la.item() - lc.item()) <= 1e-5
            _same_grads(ga, _grads(mc), f"{kind} step vs torch composition")


@pytest.mark.parametrize("use_graph", [False, True])
def test_step_with_a_teacher_matches_the_autograd_path(use_graph):
    t, a, kp, em = _batch(6, 12, 4)
    u = _teacher_rows(6, 12, 4)
    gamma, alpha, tau = 2.0, 0.5, 2.0
    ma = _model()
    for _ in range(3 if use_graph else 1):
        la = ma.train_step(t, a, kp, em, teacher_logits=u, distill=(alpha, tau), focal_gamma=gamma, use_graph=use_graph)
    mb = _model()
    out = mb(t, a, kp)
    v = em >= 0
    hard = M2FFocalLoss(gamma=gamma)(out.permute(0, 2, 1), em)
    kl = TF.kl_div(TF.log_softmax(out[v] / tau, -1), TF.softmax(u[v] / tau, -1), reduction="batchmean")
    lb = (1 - alpha) * hard + alpha * tau ** 2 * kl
    lb.backward()
    print(f"teacher, graph {use_graph}: step loss {la.item()!r}, autograd loss {lb.item()!r}")
    assert abs(la.item() - lb.item()) <= 1e-5
    _same_grads(_grads(ma), _grads(mb), "step with a teacher vs M2FFocalLoss + kl_div")


# ---- 6. switching ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
def test_none_after_focal_steps_is_the_model_that_never_saw_it(use_graph):
    t, a, kp, em = _batch(6, 12, 1)
    m, fresh = _model(), _model()
    lf = [m.train_step(t, a, kp, em, focal_gamma=2.0, use_graph=use_graph) for _ in range(3)][-1]
    want = [fresh.train_step(t, a, kp, em, use_graph=use_graph) for _ in range(3)][-1]
    for _ in range(3):
        got = m.train_step(t, a, kp, em, use_graph=use_graph)
        assert torch.equal(got, want) and not torch.equal(got, lf)
        assert torch.equal(_last_plan(m).logits, _last_plan(fresh).logits)
        _equal_grads(m, fresh, "plain after focal")
    assert torch.equal(m.train_step(t, a, kp, em, focal_gamma=2.0, use_graph=use_graph), lf)       # ... and back


def test_gamma_schedule_replays_the_captured_step():
    t, a, kp, em = _batch(6, 12, 1)
    mg = _model()
    for _ in range(3):                                     # eager warm-up, capture, replay
        mg.train_step(t, a, kp, em, focal_gamma=2.0, use_graph=True)
    plan = _last_plan(mg)
    n_plans, handle, ws = len(mg.engine().plans), plan.handle, plan.workspace.data_ptr()
    losses = []
    for gamma in (2.0, 1.0, 0.5, 0.0, 2.0):
        lg = mg.train_step(t, a, kp, em, focal_gamma=gamma, use_graph=True)
        me = _model()
        le = me.train_step(t, a, kp, em, focal_gamma=gamma, use_graph=False)
        print(f"gamma {gamma}: replayed loss {lg.item()!r}, eager loss {le.item()!r}")
        assert torch.equal(lg, le)
        _equal_grads(mg, me, f"replay at gamma {gamma}")
        assert plan.gamma_host == gamma and float(plan.focal_gamma[0]) == gamma
        losses.append(lg.item())
    assert len(set(losses[:4])) == 4 and losses[4] == losses[0]
    assert _last_plan(mg) is plan and (len(mg.engine().plans), plan.handle, plan.workspace.data_ptr()) == (n_plans, handle, ws)


# ---- 7. training modes ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_rank_group():
    import socket
    with socket.socket() as sk:                          # a free rendezvous port on this box
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    rank, world, _ = dp.init_distributed()
    assert (rank, world) == (0, 1) and dist.is_initialized()
    yield
    dist.destroy_process_group()
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        os.environ.pop(k, None)


def test_accumulation_equals_the_concatenated_batch():
    """tests/test_grad_accumulation_gpu.py's global-denominator test and its bounds (loss 1e-5, gradients 5e-6 of the largest element
    of their tensor), under the focal criterion: one denominator, so nothing else changes."""
    big = _batch(6, 12, 9)
    mbs = [[x[i * 3:(i + 1) * 3] for x in big] for i in range(2)]
    m_big, m_acc = _model(), _model()
    m_acc.set_grad_accumulation(True)
    loss_big = m_big.train_step(*big, focal_gamma=2.0, use_graph=False)
    m_acc.zero_grad(set_to_none=True)
    for mb in mbs:
        m_acc.train_step(*mb, normalise=False, focal_gamma=2.0, use_graph=False)
    den, num = m_acc.loss_terms()[1], m_acc.loss_terms()[2]
    worst = 0.0
    for (k, p), (_, q) in zip(m_acc.named_parameters(), m_big.named_parameters()):
        worst = max(worst, ((p.grad / den) - q.grad).abs().max().item() / max(q.grad.abs().max().item(), 1e-12))
    print(f"group loss {(num / den).item()!r}, big batch {loss_big.item()!r}; gradient error (of the largest element) {worst:.3e}")
    assert abs((num / den).item() - loss_big.item()) < 1e-5
    assert worst < 5e-6, worst


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_optimizer_inside_the_step(precision):
    """fp32 mode: the optimizer's kernel runs behind the step - bit for bit step + optimizer.step().  bf16 mode: the weight-gradient launch
    applies the update itself; the criterion in front of it is the stand-alone kernel on the plan's rows, bit for bit."""
    t, a, kp, em = _batch(6, 12, 1)
    ma, mb = _model(precision), _model(precision)
    oa, ob = FusedAdam(ma, lr=1e-3, weight_decay=0.01), FusedAdam(mb, lr=1e-3, weight_decay=0.01)
    la = ma.train_step(t, a, kp, em, focal_gamma=2.0, use_graph=False, optimizer=oa)
    lb = mb.train_step(t, a, kp, em, focal_gamma=2.0, use_graph=False)
    ob.step()
    assert torch.equal(la, lb)
    if precision == "fp32":
        for (n, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
            assert torch.equal(p, q), n
    plan = _last_plan(ma)
    out, dl = F.cross_entropy_focal(plan._logits.reshape(-1, 7).clone(), plan.labels_in.clone(), None, 0.1, 2.0, True)
    assert torch.equal(plan._dlogits.reshape(dl.shape), dl) and torch.equal(ma.loss_terms()[:3], out[:3])
    plain = _model(precision)
    lp = plain.train_step(t, a, kp, em, use_graph=False, optimizer=FusedAdam(plain, lr=1e-3, weight_decay=0.01))
    assert not torch.equal(la, lp) and any(not torch.equal(p, q) for p, q in zip(ma.parameters(), plain.parameters()))


@pytest.mark.parametrize("grad_bf16", [False, True])
def test_bf16_mode_runs_the_focal_kernel_on_its_own_rows(grad_bf16):
    """As the distillation test of the bf16 modes: the plan's dlogits and tail are the stand-alone kernel's on the plan's own logits,
    bit for bit; gamma = 0 gives the mode's own bits; and the loss is the fp32 model's within bf16 mode's 2e-3 (tests/test_dp_gpu.py)."""
    t, a, kp, em = _batch(6, 12, 1)

    def run(**kw):
        m = _model("bf16")
        if grad_bf16:
            assert m.set_grad_bf16(True)
        loss = m.train_step(t, a, kp, em, use_graph=False, **kw)
        return m, loss, (m.engine().grad_bf16_buf.clone() if grad_bf16 else torch.cat([g.flatten() for g in _grads(m).values()]))

    _, l_plain, g_plain = run()
    _, l_zero, g_zero = run(focal_gamma=0.0)
    assert torch.equal(l_plain, l_zero) and torch.equal(g_plain, g_zero)
    m, loss, g = run(focal_gamma=2.0)
    plan = _last_plan(m)
    out, dl = F.cross_entropy_focal(plan._logits.reshape(-1, 7).clone(), plan.labels_in.clone(), None, 0.1, 2.0, True)
    assert torch.equal(plan._dlogits.reshape(dl.shape), dl) and torch.equal(m.loss_terms()[:3], out[:3]) and torch.equal(loss, out[0])
    l32 = _model().train_step(t, a, kp, em, focal_gamma=2.0, use_graph=False)
    print(f"bf16 loss {loss.item()!r}, fp32 loss {l32.item()!r}")
    assert abs(loss.item() - l32.item()) <= 2e-3 and torch.isfinite(g.float()).all() and not torch.equal(loss, l_plain)


def test_data_parallel_step_on_one_rank(one_rank_group):
    """The rank's step is train_step(normalise=False) and the division by the (global = local) den inside the optimizer, bit for bit."""
    t, a, kp, em = _batch(6, 12, 1)
    m = _model()
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01)
    step = dp.DataParallelStep(m, opt, n_buckets=3, exchange="fp32")
    loss = step(t, a, kp, em, focal_gamma=2.0, use_graph=False)
    m2 = _model()
    opt2 = FusedAdam(m2, lr=1e-3, weight_decay=0.01)
    l2 = m2.train_step(t, a, kp, em, focal_gamma=2.0, normalise=False, use_graph=False)
    assert torch.equal(_last_plan(m)._dlogits, _last_plan(m2)._dlogits) and torch.equal(m.loss_terms()[:3], m2.loss_terms()[:3])
    opt2.grad_scale = m2.loss_terms()[1:2]
    opt2.step()
    print(f"data-parallel loss {loss.item()!r}, train_step loss {l2.item()!r}")
    assert torch.equal(loss, l2)
    worst = max((p - q).abs().max().item() for p, q in zip(m.parameters(), m2.parameters()))
    print(f"largest parameter difference after the update: {worst:.3e}")
    for (n, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(p, q), n
    with pytest.raises(ValueError, match="focal_gamma"):
        step(t, a, kp, em, focal_gamma=-1.0)


def test_distiller_hands_gamma_to_the_student():
    t, a, kp, em = _batch(6, 12, 1)
    teacher = _model(seed=5)
    student = _model(context=(None, 0))
    d = Distiller(student, teacher, alpha=0.5, temperature=2.0)
    loss = d.train_step(t, a, kp, em, focal_gamma=2.0, use_graph=False)
    other = _model(context=(None, 0))
    with torch.no_grad():
        u = teacher(t, a, kp)
    want = other.train_step(t, a, kp, em, teacher_logits=u, distill=(0.5, 2.0), focal_gamma=2.0, use_graph=False)
    assert torch.equal(loss, want)
    _equal_grads(student, other, "Distiller vs train_step with the teacher's logits")
    assert not torch.equal(loss, d.train_step(t, a, kp, em, use_graph=False))
    zero = d.train_step(t, a, kp, em, focal_gamma=0.0, use_graph=False)
    assert torch.equal(zero, d.train_step(t, a, kp, em, use_graph=False))
    with pytest.raises(ValueError, match="focal_gamma"):
        d.train_step(t, a, kp, em, focal_gamma=float("nan"))


# ---- 8. the drop-in loop ----------------------------------------------------------------------------------------------------------------------
def _dataset(n_dia, d_t, d_a, seed):
    import dataset as ds
    g = np.random.default_rng(seed)
    rows = [(f"utt {d}-{u}", list(ds.EMOTIONS)[int(g.integers(0, 7))], d, u) for d in range(n_dia) for u in range(int(g.integers(1, 10)))]
    table = pd.DataFrame(rows, columns=["Utterance", "Emotion", "Dialogue_ID", "Utterance_ID"])
    text = torch.from_numpy(g.standard_normal((len(rows), d_t)).astype(np.float32))
    audio = torch.from_numpy(g.standard_normal((len(rows), d_a)).astype(np.float32))
    lab = table["Emotion"].map(ds.EMOTIONS).to_numpy()
    text[np.arange(len(rows)), lab] += 3.0                  # the label is learnable from the text rows
    return ds.Dataset("train", text_embeddings=text, audio_embeddings=audio, table=table)


def test_loop_trains_and_validates_with_the_focal_criterion(tmp_path, monkeypatch):
    monkeypatch.chdir(ROOT)
    import dataset as ds
    import train as tr
    from utils import AttrDict, get_config
    device = torch.device("cuda:0")
    model_cfg = synth._cfg(40, 48, 64, 4, 4, 4, 1, 1, 1, dropout=0.0)
    sd = synth.make_state_dict(model_cfg)
    cfg = AttrDict(dict(get_config()))
    cfg.model = AttrDict(model_cfg)
    cfg.runtime = AttrDict(dict(cfg.runtime, focal_gamma=2.0))
    cfg.solver = AttrDict(dict(cfg.solver, epochs=2, lr=2e-3, weight_decay=0.01, loss_fn="Focal", balance_classes=True,
                               early_stopping=AttrDict(enabled=False, patience=5, restore_best_weights=False),
                               scheduler=AttrDict(enabled=False, scheduler_fn="ExponentialLR", gamma=0.9)))
    d_train, d_val = _dataset(24, 48, 40, 1), _dataset(8, 48, 40, 2)
    dl_train = torch.utils.data.DataLoader(d_train, collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    dl_val = torch.utils.data.DataLoader(d_val, collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    crit = tr.build_criterion(cfg.solver, d_train, device, focal_gamma=tr.focal_gamma_setting(cfg))
    assert type(crit) is M2FFocalLoss and crit.gamma == 2.0 and crit.weight is not None and crit.weight.numel() == 7

    def run(device_metrics, criterion):
        cfg.checkpoint = AttrDict(save_path=str(tmp_path / f"ck{int(device_metrics)}" / "m2fnet.pth"), load_path="", save_checkpoint=False,
                                  load_checkpoint=False)
        m = tr.build_model(cfg, device)
        m.load_state_dict({k: v.to(device) for k, v in sd.items()})
        m.device_metrics = device_metrics
        out = tr.training_loop(m, dl_train, dl_val, criterion, tr.build_optimizer(cfg, m), None, 0, cfg, device)
        return m, out

    m_host, host = run(False, crit)
    m_dev, devs = run(True, crit)
    print(f"train {host['loss_values']} / {devs['loss_values']}; validation host loop {host['val_loss_values']}, device {devs['val_loss_values']}")
    assert host["loss_values"] == devs["loss_values"]
    for p, q in zip(m_host.parameters(), m_dev.parameters()):
        assert torch.equal(p, q)
    for x, y in zip(host["val_loss_values"], devs["val_loss_values"]):
        assert np.isfinite(x) and abs(x - y) <= 2e-5, (x, y)
    assert host["loss_values"][1] < host["loss_values"][0] and host["val_loss_values"][1] < host["val_loss_values"][0]
    # the focal criterion is what trained and what validated: the CE loop ends elsewhere
    ce = tr.build_criterion(AttrDict(dict(cfg.solver, loss_fn="CE")), d_train, device)
    m_ce, plain = run(True, ce)
    assert plain["loss_values"][0] > host["loss_values"][0] and plain["val_loss_values"][0] > devs["val_loss_values"][0]
    assert any(not torch.equal(p, q) for p, q in zip(m_ce.parameters(), m_dev.parameters()))
