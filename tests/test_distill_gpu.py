"""The distillation criterion on the device: the kernel against the float64 reference (tests/golden/distill_ref.py), its exact
properties (alpha = 0 is the plain criterion bit for bit, a teacher equal to the student costs nothing, invalid rows are selected
away whatever their teacher row holds, an underflowing teacher stays finite), the train step against the autograd path on every plan
kind, graphs, every training mode, the Distiller and the drop-in loop.  Every comparison prints its figures before it asserts (-s)."""
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

import distill_ref as ref  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import dp  # noqa: E402
from mer_amd import functional as F  # noqa: E402
from mer_amd.distill import Distiller  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam, M2FDistillationLoss  # noqa: E402

DEV = "cuda"
CFG = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2, ncls=7)          # dropout 0
PAIRS = [(0.5, 2.0), (1.0, 1.0), (0.3, 4.0)]


def _close(a, b, tol, what=""):
    """tests/test_kernels_gpu.py's comparison: max error against tol * the reference's largest magnitude."""
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item()
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, bound {tol * scale + 1e-7:.3e}")
    assert err <= tol * scale + 1e-7, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def _rows(T, C, seed, t_scale=4.0):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(T, C, generator=g) * 2.0).to(DEV)
    u = (torch.randn(T, C, generator=g) * t_scale).to(DEV)
    y = torch.randint(0, C, (T,), generator=g)
    y[torch.rand(T, generator=g) < 0.3] = -1
    w = (0.3 + 5.0 * torch.rand(C, generator=g)).to(DEV)
    return z, u, y.to(DEV), w


def _against_ref(z, u, y, w, alpha, tau, what):
    loss_r, den_r, num_r, grad_r = ref.distill_loss_and_grad(z, u, y, w, 0.1, alpha, tau)
    for normalise in (True, False):
        out, dl = F.cross_entropy_distill(z, u, y, w, 0.1, alpha, tau, normalise)
        assert torch.isfinite(out[:3]).all() and torch.isfinite(dl).all()
        err, bound = abs(out[0].item() - loss_r.item()), 2e-6 * max(1.0, abs(loss_r.item()))
        print(f"{what} alpha {alpha} tau {tau} normalise {normalise}: loss {out[0].item()!r} ref {loss_r.item()!r} err {err:.3e} bound {bound:.3e}")
        assert err <= bound
        assert abs(out[1].item() - den_r.item()) <= 1e-6 * den_r.item() and abs(out[2].item() - num_r.item()) <= 2e-6 * max(1.0, abs(num_r.item()))
        _close((dl if normalise else dl / out[1]).double(), grad_r, 1e-5, f"{what} dlogits")


# ---- 1. the kernel against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [2, 7, 16])
@pytest.mark.parametrize("T", [300, 257])
def test_kernel_matches_the_float64_reference(T, C, weighted):
    z, u, y, w = _rows(T, C, 100 * C + T)
    for alpha, tau in PAIRS:
        _against_ref(z, u, y, w if weighted else None, alpha, tau, f"T {T} C {C} weighted {weighted}")


# ---- 2. alpha = 0: the plain criterion's bits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("T,C", [(300, 7), (257, 2), (257, 16)])
def test_alpha_zero_is_the_plain_criterion_bit_for_bit(T, C, weighted):
    z, u, y, w = _rows(T, C, 7 * C + T)
    w = w if weighted else None
    for tau in (1.0, 2.0, 3.7):
        for normalise in (True, False):
            out, dl = F.cross_entropy_distill(z, u, y, w, 0.1, 0.0, tau, normalise)
            out0, dl0 = F.cross_entropy(z, y, w, 0.1, normalise)
            assert torch.equal(out, out0) and torch.equal(dl, dl0), (tau, normalise, (dl - dl0).abs().max().item())


# ---- 3. a teacher that is the student ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,C", [(300, 7), (257, 16)])
def test_teacher_equal_to_the_student_costs_nothing(T, C):
    z, _, y, w = _rows(T, C, 31 + C)
    for cw in (None, w):
        out, dl = F.cross_entropy_distill(z, z.clone(), y, cw, 0.1, 1.0, 1.0, True)
        print(f"C {C}: |loss| {abs(out[0].item()):.3e}, max |gradient| {dl.abs().max().item():.3e}")
        assert abs(out[0].item()) <= 1e-6 and dl.abs().max().item() <= 1e-6


# ---- 4. invalid rows are a select ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,C", [(300, 7), (257, 16)])
def test_invalid_rows_ignore_their_teacher_row(T, C):
    z, u, y, w = _rows(T, C, 41 + C)
    bad = u.clone()
    idx = (y < 0).nonzero().flatten()
    assert idx.numel() > 30
    fill = torch.tensor([float("nan"), float("inf"), -float("inf")], device=DEV)
    bad[idx] = fill[torch.arange(idx.numel(), device=DEV) % 3][:, None]
    bad[idx[0], 0], bad[idx[0], 1:] = float("inf"), float("nan")              # (mixed within one row too)
    zeroed = u.clone()
    zeroed[idx] = 0.0
    for normalise in (True, False):
        a = F.cross_entropy_distill(z, bad, y, w, 0.1, 0.5, 2.0, normalise)
        b = F.cross_entropy_distill(z, zeroed, y, w, 0.1, 0.5, 2.0, normalise)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.isfinite(a[1]).all() and float(a[1][idx].abs().max()) == 0.0
    # an out-of-range label is invalid as well
    y2 = y.clone()
    y2[idx[:5]] = C
    a = F.cross_entropy_distill(z, bad, y2, w, 0.1, 0.5, 2.0, True)
    b = F.cross_entropy_distill(z, zeroed, y, w, 0.1, 0.5, 2.0, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 5. a saturated teacher ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,C", [(300, 7), (257, 16), (257, 2)])
def test_saturated_teacher_stays_finite_and_right(T, C):
    z, u, y, w = _rows(T, C, 51 + C, t_scale=100.0)
    assert float(torch.softmax(u.double(), -1).float().min()) == 0.0           # teacher probabilities do underflow in fp32
    for cw in (None, w):
        _against_ref(z, u, y, cw, 0.5, 1.0, f"saturated T {T} C {C}")
        _against_ref(z, u, y, cw, 1.0, 1.0, f"saturated T {T} C {C}")


# ---- 6. the step against the autograd path ---------------------------------------------------------------------------------------------
def _model(precision="fp32", context=None, cfg=CFG, seed=None):
    m = M2FNet(cfg, precision=precision, context=context)
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
    worst = 0.0
    for k in ga:
        err, bound = (ga[k] - gb[k]).abs().max().item(), 1e-6 + 1e-4 * ga[k].abs().max().item()
        worst = max(worst, err / bound)
        assert err <= bound, (what, k, err, bound)
    print(f"{what}: worst gradient error / bound {worst:.3f}")


PLAN_KINDS = {"full_8x16": (8, 16, 1, [16] * 8), "ragged_8x32": (8, 32, 2, None), "packed_2x80": (2, 80, 3, [80, 23]),
              "bucketed_5x9": (5, 9, 4, [9, 1, 4, 7, 2])}


@pytest.mark.parametrize("kind", list(PLAN_KINDS))
def test_step_matches_the_autograd_path(kind):
    B, L, seed, lengths = PLAN_KINDS[kind]
    t, a, kp, em = _batch(B, L, seed, lengths)
    u = _teacher_rows(B, L, seed)
    alpha, tau = 0.5, 2.0
    ma = _model()
    la = ma.train_step(t, a, kp, em, teacher_logits=u, distill=(alpha, tau), use_graph=False)
    plan = ma.engine().plans[next(reversed(ma.engine().plans))]
    assert kind != "bucketed_5x9" or (plan.B, plan.L) == (8, 16)
    assert plan.packed == (kind == "packed_2x80")
    v = em >= 0
    assert torch.equal(plan.teacher[v], u[v])               # the teacher rows travelled with the batch
    ga = _grads(ma)
    mb = _model()
    out = mb(t, a, kp)
    ce = torch.nn.CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)(out.permute(0, 2, 1), em)
    kl = TF.kl_div(TF.log_softmax(out[v] / tau, -1), TF.softmax(u[v] / tau, -1), reduction="batchmean")
    lb = (1 - alpha) * ce + alpha * tau ** 2 * kl
    lb.backward()
    print(f"{kind}: step loss {la.item()!r}, autograd loss {lb.item()!r}")
    assert abs(la.item() - lb.item()) <= 1e-5
    _same_grads(ga, _grads(mb), f"{kind} step vs torch composition")
    mc = _model()
    lc = M2FDistillationLoss(alpha=alpha, temperature=tau)(mc(t, a, kp).permute(0, 2, 1), em, u.permute(0, 2, 1))
    lc.backward()
    assert abs(la.item() - lc.item()) <= 1e-5
    _same_grads(ga, _grads(mc), f"{kind} step vs M2FDistillationLoss")


# ---- 7. graphs ---------------------------------------------------------------------------------------------------------------------------
def _equal_grads(ma, mb, what):
    for (k, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(p.grad, q.grad), (what, k, (p.grad - q.grad).abs().max().item())


def test_graph_replay_follows_the_pair_on_the_device():
    t, a, kp, em = _batch(8, 16, 1)
    u = _teacher_rows(8, 16, 1)
    me, mg = _model(), _model()
    le = me.train_step(t, a, kp, em, teacher_logits=u, distill=(0.5, 2.0), use_graph=False)
    for _ in range(3):                                     # eager warm-up, capture, replay
        lg = mg.train_step(t, a, kp, em, teacher_logits=u, distill=(0.5, 2.0), use_graph=True)
        assert torch.equal(lg, le)
        _equal_grads(mg, me, "graph vs eager")
    # alpha moves between two replays: the captured step reads the pair on the device
    lg = mg.train_step(t, a, kp, em, teacher_logits=u, distill=(0.8, 2.0), use_graph=True)
    m2 = _model()
    l2 = m2.train_step(t, a, kp, em, teacher_logits=u, distill=(0.8, 2.0), use_graph=False)
    assert torch.equal(lg, l2) and not torch.equal(lg, le)
    _equal_grads(mg, m2, "replay at the new alpha")
    # ... and a plain step after the distilled ones is the plain step (either order)
    m3 = _model()
    l3 = m3.train_step(t, a, kp, em, use_graph=False)
    for _ in range(3):
        lp = mg.train_step(t, a, kp, em, use_graph=True)
        assert torch.equal(lp, l3)
        _equal_grads(mg, m3, "plain after distilled")
    lg = mg.train_step(t, a, kp, em, teacher_logits=u, distill=(0.8, 2.0), use_graph=True)
    assert torch.equal(lg, l2)
    _equal_grads(mg, m2, "distilled after plain")


# ---- 8. every training mode ----------------------------------------------------------------------------------------------------------------
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


def _last_plan(m):
    return m.engine().plans[next(reversed(m.engine().plans))]


def _standalone(plan, pair, normalise):
    """The stand-alone kernel on the plan's own token rows: (loss_out, dlogits [T, C])."""
    C = plan.cfg.cls_out
    return F.cross_entropy_distill(plan._logits.reshape(-1, C).clone(), plan._teacher.reshape(-1, C).clone(), plan.labels_in.clone(), None,
                                   0.1, pair[0], pair[1], normalise)


def _run_mode(mode, kw):
    """One step (or group) of `mode` with the train_step keywords `kw`; -> (model, result tensors to compare, [(plan rows after each
    micro-batch: dlogits, standalone out, standalone dlogits)])."""
    batches = [(_batch(8, 16, 1), _teacher_rows(8, 16, 1)), (_batch(8, 16, 2), _teacher_rows(8, 16, 2))]
    pair = kw.get("distill")
    probes = []

    def probe(m, normalise):
        if pair is not None:
            plan = _last_plan(m)
            out, dl = _standalone(plan, pair, normalise)
            probes.append((plan._dlogits.reshape(dl.shape).clone(), out, dl))

    def kws(i):
        return dict(kw, teacher_logits=batches[i][1]) if pair is not None else {}

    if mode == "bf16":
        m = _model("bf16")
        loss = m.train_step(*batches[0][0], use_graph=False, **kws(0))
        probe(m, True)
        return m, [loss] + list(_grads(m).values()), probes
    if mode == "optimizer":
        m = _model("bf16")
        opt = FusedAdam(m, lr=1e-3, weight_decay=0.01)
        loss = m.train_step(*batches[0][0], use_graph=False, optimizer=opt, **kws(0))
        probe(m, True)
        return m, [loss] + [p.detach().clone() for p in m.parameters()], probes
    if mode == "grad_bf16":
        m = _model("bf16")
        assert m.set_grad_bf16(True)
        loss = m.train_step(*batches[0][0], use_graph=False, **kws(0))
        probe(m, True)
        return m, [loss, m.engine().grad_bf16_buf.clone()], probes
    if mode == "accumulation":
        m = _model()
        m.set_grad_accumulation(True)
        m.zero_grad(set_to_none=True)
        for i in range(2):
            m.train_step(*batches[i][0], normalise=False, use_graph=False, **kws(i))
            probe(m, False)
        return m, [m.loss_terms().clone()] + list(_grads(m).values()), probes
    assert mode == "data_parallel"
    m = _model()
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01)
    step = dp.DataParallelStep(m, opt, n_buckets=3)
    loss = step(*batches[0][0], use_graph=False, **kws(0))
    probe(m, False)
    return m, [loss] + [p.detach().clone() for p in m.parameters()], probes


@pytest.mark.parametrize("mode", ["bf16", "optimizer", "grad_bf16", "accumulation", "data_parallel"])
def test_every_training_mode(one_rank_group, mode):
    # alpha = 0: the mode's own bits
    _, plain, _ = _run_mode(mode, {})
    _, zero, _ = _run_mode(mode, {"distill": (0.0, 3.0)})
    assert len(plain) == len(zero)
    for i, (x, y) in enumerate(zip(plain, zero)):
        assert torch.equal(x, y), (mode, i, (x.float() - y.float()).abs().max().item())
    # alpha = 0.5: the step ran the distillation kernel on its own rows, and its tail holds the group's den / num
    m, half, probes = _run_mode(mode, {"distill": (0.5, 2.0)})
    assert not torch.equal(half[0], plain[0])
    den = num = 0.0
    for dl_plan, out, dl in probes:
        assert torch.equal(dl_plan, dl), (mode, (dl_plan - dl).abs().max().item())
        den, num = out[1] + den, out[2] + num
    tail = m.loss_terms()
    print(f"{mode}: tail {tail.tolist()}, stand-alone den {float(den)!r} num {float(num)!r}")
    assert torch.equal(tail[1], den) and torch.equal(tail[2], num)


# ---- 9. Distiller ----------------------------------------------------------------------------------------------------------------------------
def test_distiller_runs_the_teacher_and_leaves_it_alone():
    t, a, kp, em = _batch(8, 16, 1)
    teacher = _model(seed=5)                               # offline: sees the whole dialogue
    before = [p.detach().clone() for p in teacher.parameters()]
    student = _model(context=(None, 0))
    d = Distiller(student, teacher, alpha=0.5, temperature=2.0)
    assert not teacher.training and student.training
    loss = d.train_step(t, a, kp, em, use_graph=False)
    other = _model(context=(None, 0))
    with torch.no_grad():                                  # (the teacher's plan was made by the Distiller's inference-mode forward)
        u = teacher(t, a, kp)
    want = other.train_step(t, a, kp, em, teacher_logits=u, distill=(0.5, 2.0), use_graph=False)
    assert torch.equal(loss, want)
    _equal_grads(student, other, "Distiller vs train_step with the teacher's logits")
    plain = _model(context=(None, 0)).train_step(t, a, kp, em, use_graph=False)
    assert not torch.equal(loss, plain)
    d.alpha = 0.0                                          # a schedule: alpha = 0 is the hard-label step
    assert torch.equal(d.train_step(t, a, kp, em, use_graph=False), plain)
    for p, q in zip(teacher.parameters(), before):
        assert torch.equal(p, q) and p.grad is None and not p.requires_grad
    small = synth._cfg(48, 64, 64, 4, 4, 4, 1, 1, 1)
    small["CLASSIFIER"]["output_size"] = 5
    with pytest.raises(ValueError, match="cls_out"):
        Distiller(student, M2FNet(small))


# ---- 10. the drop-in loop ----------------------------------------------------------------------------------------------------------------------
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


def test_loop_takes_the_teacher_from_the_checkpoints_average(tmp_path, monkeypatch):
    """runtime.distill.teacher_weights: ema - the teacher gets the parameters of the checkpoint's ema_state_dict, not the live weights;
    a checkpoint without an average is refused."""
    monkeypatch.chdir(ROOT)
    import train as tr
    from utils import AttrDict, get_config
    device = torch.device("cuda:0")
    model_cfg = synth._cfg(40, 48, 64, 4, 4, 4, 1, 1, 1, dropout=0.0)
    src = tr.M2FNet(model_cfg)
    src.load_state_dict(synth.make_state_dict(model_cfg))
    src = src.to(device).train()
    opt = tr.FusedAdam(src, lr=1e-2, weight_decay=0.0, ema_decay=0.5)
    batch = [x.to(device) for x in synth.make_inputs(model_cfg, 4, 9, [9, 4, 1, 7], "randn", seed=3)]
    for _ in range(2):
        opt.zero_grad()
        src.train_step(*batch, use_graph=False)
        opt.step()
    path = str(tmp_path / "teacher.pth")
    tr.write_checkpoint(path, 0, src, opt)
    ck = torch.load(path)
    assert tr.EMA_KEY in ck

    def cfg_for(ckpt, weights):
        cfg = AttrDict(dict(get_config()))
        cfg.model = AttrDict(model_cfg)
        cfg.runtime = AttrDict(dict(cfg.runtime, distill={"enabled": True, "teacher_checkpoint": ckpt, "teacher_weights": weights}))
        return cfg

    student = tr.build_model(cfg_for(path, "ema"), device)
    d = tr.attach_distiller(cfg_for(path, "ema"), student, device)
    live_differs = False
    for k, p in d.teacher.state_dict().items():
        assert torch.equal(p, ck[tr.EMA_KEY]["parameters"][k].to(device)), k
        live_differs |= not torch.equal(p, ck["model_state_dict"][k].to(device))
    assert live_differs
    d_live = tr.attach_distiller(cfg_for(path, "model"), tr.build_model(cfg_for(path, "model"), device), device)
    for k, p in d_live.teacher.state_dict().items():
        assert torch.equal(p, ck["model_state_dict"][k].to(device)), k
    plain = str(tmp_path / "plain.pth")
    torch.save({k: ck[k] for k in tr.CHECKPOINT_KEYS}, plain)
    with pytest.raises(ValueError, match="ema_state_dict"):
        tr.attach_distiller(cfg_for(plain, "ema"), tr.build_model(cfg_for(plain, "ema"), device), device)


def test_loop_distils_and_checkpoints_the_student_only(tmp_path, monkeypatch):
    monkeypatch.chdir(ROOT)
    import dataset as ds
    import train as tr
    from utils import AttrDict, get_config
    device = torch.device("cuda:0")
    model_cfg = synth._cfg(40, 48, 64, 4, 4, 4, 1, 1, 1, dropout=0.0)
    sd = synth.make_state_dict(model_cfg)
    g = torch.Generator().manual_seed(9)
    teacher_sd = {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in sd.items()}
    # the teacher's checkpoint, as this loop writes one
    teacher = tr.M2FNet(model_cfg)
    teacher.load_state_dict(teacher_sd)
    teacher = teacher.to(device)
    teacher_path = str(tmp_path / "teacher" / "m2fnet.pth")
    os.makedirs(os.path.dirname(teacher_path))
    tr.write_checkpoint(teacher_path, 3, teacher, tr.FusedAdam(teacher, lr=1e-3))

    cfg = AttrDict(dict(get_config()))
    cfg.model = AttrDict(model_cfg)
    cfg.runtime = AttrDict(dict(cfg.runtime, context={"past": None, "future": 0},
                                distill={"enabled": True, "teacher_checkpoint": teacher_path, "teacher_weights": "model", "alpha": 0.6,
                                         "temperature": 3.0, "teacher_context": {"past": None, "future": None}}))
    cfg.solver = AttrDict(dict(cfg.solver, epochs=1, lr=2e-3, weight_decay=0.01,
                               early_stopping=AttrDict(enabled=False, patience=5, restore_best_weights=False),
                               scheduler=AttrDict(enabled=False, scheduler_fn="ExponentialLR", gamma=0.9)))
    cfg.checkpoint = AttrDict(save_path=str(tmp_path / "ck" / "m2fnet.pth"), load_path=str(tmp_path / "ck" / "m2fnet.pth"),
                              save_checkpoint=True, load_checkpoint=False)
    d_train, d_val = _dataset(24, 48, 40, 1), _dataset(8, 48, 40, 2)
    dl_train = torch.utils.data.DataLoader(d_train, collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    dl_val = torch.utils.data.DataLoader(d_val, collate_fn=ds.collate_fn, batch_size=8, shuffle=False)

    def student():
        m = tr.build_model(cfg, device)
        m.load_state_dict({k: v.to(device) for k, v in sd.items()})
        return m

    model = student()
    assert model.context == (None, 0)
    d = tr.attach_distiller(cfg, model, device)
    assert d is model.distiller and (d.alpha, d.temperature) == (0.6, 3.0) and d.teacher.context == (None, None)
    assert "distiller" not in dict(model.named_modules()) and list(model.state_dict()) == list(sd)
    for k, p in d.teacher.state_dict().items():
        assert torch.equal(p.cpu(), teacher_sd[k]), k
    crit = tr.M2FCrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    opt = tr.build_optimizer(cfg, model)
    out = tr.training_loop(model, dl_train, dl_val, crit, opt, None, 0, cfg, device)

    # the same epoch by hand over Distiller.train_step
    model2 = student()
    teacher2 = tr.M2FNet(model_cfg)
    teacher2.load_state_dict(torch.load(teacher_path)["model_state_dict"])
    d2 = Distiller(model2, teacher2.to(device), alpha=0.6, temperature=3.0)
    opt2 = tr.build_optimizer(cfg, model2)
    model2.train()
    losses = []
    for batch in dl_train:
        text, audio, emotion, mask = (batch[k].to(device) for k in ("text", "audio", "emotion", "padding_mask"))
        opt2.zero_grad()
        losses.append(d2.train_step(text, audio, mask, emotion, label_smoothing=0.1).item())
        opt2.step()
    print(f"loop epoch loss {out['loss_values'][0]!r}, by hand {float(np.mean(losses))!r}")
    assert out["loss_values"][0] == float(np.mean(losses)) or abs(out["loss_values"][0] - float(np.mean(losses))) < 1e-12
    for (n, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(p, q), n
    # distillation changed the training (the hard-label loop ends elsewhere) ...
    model3 = student()
    opt3 = tr.build_optimizer(cfg, model3)
    tr.train(model3, dl_train, crit, opt3, 0, False, device)
    assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), model3.parameters()))
    # ... validation stays the hard-label criterion, and the checkpoint holds the student only: it loads into a plain model
    assert np.isfinite(out["val_loss_values"]).all()
    ck = torch.load(cfg.checkpoint.save_path)
    assert set(ck) == set(tr.CHECKPOINT_KEYS) and list(ck["model_state_dict"]) == list(sd)
    plain = tr.M2FNet(cfg.model)
    plain.load_state_dict(ck["model_state_dict"])
    for (n, p), (_, q) in zip(plain.named_parameters(), model.named_parameters()):
        assert torch.equal(p, q.cpu()), n
