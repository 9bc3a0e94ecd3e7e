"""The linear-chain CRF inside the model: ``train_step(crf=)`` against forward + ``LinearChainCRF`` + backward on every plan kind (graph
and eager), switching back to the plain criterion, a torch optimizer on the module under a replayed graph, ``eval_step(crf=)`` (the train
kernel's loss bits, the Viterbi path's confusion matrix), a frozen module under every training mode, and every refusal by name.
Every comparison prints its figures before it asserts (-s)."""
import os

import pytest
import torch
import torch.distributed as dist

pytestmark = pytest.mark.gpu

import crf_cases as cases  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import dp  # noqa: E402
from mer_amd import functional as F  # noqa: E402
from mer_amd.crf import LinearChainCRF  # noqa: E402
from mer_amd.metrics import DeviceScores  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam  # noqa: E402

DEV = "cuda"
CFG = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2, ncls=7)          # dropout 0 (tests/test_focal_gpu.py's)
C = 7
# name: B, L, seed, lengths, packed
PLAN_KINDS = {"padded_6x12": (6, 12, 1, [12, 12, 11, 12, 12, 12], None), "bucketed_5x11": (5, 11, 4, [11, 4, 9, 1, 11], None),
              "packed_6x12": (6, 12, 2, [12, 3, 5, 1, 7, 2], True), "long_2x70": (2, 70, 3, [70, 23], None)}


def _model(precision="fp32", packed=None):
    m = M2FNet(CFG, precision=precision, packed=packed)
    m.load_state_dict(synth.make_state_dict(CFG))
    return m.to(DEV).train()


def _crf(trainable=True, seed=11, scale=0.5):
    crf = LinearChainCRF(C).to(DEV)
    with torch.no_grad():
        crf.params.copy_(cases.params_block(C, seed, scale))
    crf.params.requires_grad_(trainable)
    return crf


def _batch(B, L, seed, lengths=None):
    if lengths is None:
        g = torch.Generator().manual_seed(seed)
        lengths = [L] + [int(x) for x in torch.randint(1, L + 1, (B - 1,), generator=g)]
    return [t.to(DEV) for t in synth.make_inputs(CFG, B, L, lengths, "randn", seed=seed)]


def _last_plan(m):
    return m.engine().plans[next(reversed(m.engine().plans))]


def _equal_grads(ma, mb, what):
    for (k, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(p.grad, q.grad), (what, k, (p.grad - q.grad).abs().max().item())


# ---- 1. the train step against the autograd path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind", list(PLAN_KINDS))
def test_step_matches_the_autograd_path(kind, use_graph):
    B, L, seed, lengths, packed = PLAN_KINDS[kind]
    t, a, kp, em = _batch(B, L, seed, lengths)
    ma, ca = _model(packed=packed), _crf()
    for _ in range(3 if use_graph else 1):               # eager warm-up, capture, replay
        la = ma.train_step(t, a, kp, em, label_smoothing=0.0, crf=ca, use_graph=use_graph)
    plan = _last_plan(ma)
    mb, cb = _model(packed=packed), _crf()
    lb = cb(mb(t, a, kp).permute(0, 2, 1), em)
    lb.backward()
    gerr = max((p.grad - q.grad).abs().max().item() for p, q in zip(ma.parameters(), mb.parameters()))
    print(f"{kind} graph {use_graph} (plan {plan.B} x {plan.L}, packed {plan.packed}): step loss {la.item()!r}, autograd loss {lb.item()!r}; "
          f"largest parameter-gradient difference {gerr:.3e}; crf.grad difference {(ca.params.grad - cb.params.grad).abs().max().item():.3e}")
    assert plan.packed == (kind in ("packed_6x12", "long_2x70"))
    assert torch.equal(la, lb.detach())
    _equal_grads(ma, mb, kind)
    assert torch.equal(ca.params.grad, cb.params.grad)
    assert ca.params.grad.data_ptr() == ca._grad_buf.data_ptr()           # a view of the buffer the step overwrites
    assert "params" not in dict(ma.named_parameters()) and all("crf" not in k for k in ma.state_dict())


def test_frozen_module_gets_no_gradient_and_the_same_step():
    t, a, kp, em = _batch(6, 12, 1)
    ma, mb = _model(), _model()
    cf, ct = _crf(trainable=False), _crf()
    lf = ma.train_step(t, a, kp, em, label_smoothing=0.0, crf=cf, use_graph=False)
    lt = mb.train_step(t, a, kp, em, label_smoothing=0.0, crf=ct, use_graph=False)
    assert torch.equal(lf, lt) and cf.params.grad is None and ct.params.grad is not None
    _equal_grads(ma, mb, "frozen vs trainable")


# ---- 2. switching ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_none_after_crf_steps_is_the_model_that_never_saw_it(use_graph):
    t, a, kp, em = _batch(6, 12, 1)
    m, fresh, crf = _model(), _model(), _crf()
    lc = [m.train_step(t, a, kp, em, label_smoothing=0.0, crf=crf, use_graph=use_graph) for _ in range(3)][-1]
    want = [fresh.train_step(t, a, kp, em, use_graph=use_graph) for _ in range(3)][-1]
    for _ in range(3):
        got = m.train_step(t, a, kp, em, use_graph=use_graph)
        assert torch.equal(got, want) and not torch.equal(got, lc)
        assert torch.equal(_last_plan(m).logits, _last_plan(fresh).logits)
        _equal_grads(m, fresh, "plain after crf")
    assert torch.equal(m.train_step(t, a, kp, em, label_smoothing=0.0, crf=crf, use_graph=use_graph), lc)       # ... and back
    # the focal criterion after it, and the CRF after the focal criterion: each switch clears the other
    lf = m.train_step(t, a, kp, em, focal_gamma=2.0, use_graph=use_graph)
    assert torch.equal(lf, _model().train_step(t, a, kp, em, focal_gamma=2.0, use_graph=use_graph))
    assert torch.equal(m.train_step(t, a, kp, em, label_smoothing=0.0, crf=crf, use_graph=use_graph), lc)


def test_torch_adam_on_the_module_under_a_replayed_graph():
    """The block's values are read on the device: a captured step replays while a torch optimizer updates them in place, and follows the
    eager trajectory bit for bit; the model's own optimizer runs inside the step beside it."""
    t, a, kp, em = _batch(6, 12, 1)
    runs = {}
    for use_graph in (True, False):
        m, crf = _model(), _crf()
        opt_m, opt_c = FusedAdam(m, lr=1e-3), torch.optim.Adam(crf.parameters(), lr=1e-2)
        losses = []
        for _ in range(6):
            losses.append(m.train_step(t, a, kp, em, label_smoothing=0.0, crf=crf, use_graph=use_graph, optimizer=opt_m).item())
            opt_c.step()
        runs[use_graph] = (losses, crf.params.detach().clone(), [p.detach().clone() for p in m.parameters()])
        if use_graph:
            plan = _last_plan(m)
            assert len(m.engine().plans) == 1 and plan._crf_key[0] == crf.params.data_ptr()
    print("replayed:", runs[True][0], "\neager:   ", runs[False][0])
    assert runs[True][0] == runs[False][0] and torch.equal(runs[True][1], runs[False][1])
    assert all(torch.equal(p, q) for p, q in zip(runs[True][2], runs[False][2]))
    assert runs[True][0][-1] < runs[True][0][0] and not torch.equal(runs[True][1], cases.params_block(C, 11, 0.5).to(DEV))


# ---- 3. the eval step ---------------------------------------------------------------------------------------------------------------------
def _confusion(scores):
    return scores.record[8:].view(torch.int64).view(C, C).cpu()


@pytest.mark.parametrize("kind", ["padded_6x12", "packed_6x12", "long_2x70"])
def test_eval_step_scores_the_crf_loss_and_the_viterbi_path(kind):
    B, L, seed, lengths, packed = PLAN_KINDS[kind]
    t, a, kp, em = _batch(B, L, seed, lengths)
    m = _model(packed=packed).eval()
    crf = _crf(trainable=False, scale=0.0)
    with torch.no_grad():                                  # staying in a class costs 50: the path must move where the argmax repeats itself
        crf.transitions.copy_(-50.0 * torch.eye(C))
        logits = m(t, a, kp)
    got, plain = DeviceScores(C, DEV), DeviceScores(C, DEV)
    for use_graph in (False, True, True):
        m.eval_step(t, a, kp, em, got, label_smoothing=0.0, crf=crf, use_graph=use_graph)
    m.eval_step(t, a, kp, em, plain, label_smoothing=0.0, use_graph=True)
    # the loss: the train kernel's bits on the plan's own rows
    mt = _model(packed=packed)
    lt = mt.train_step(t, a, kp, em, label_smoothing=0.0, crf=crf, use_graph=False)
    print(f"{kind}: eval loss {got.last()[0].item()!r}, train step loss {lt.item()!r}, plain criterion {plain.last()[0].item()!r}")
    assert got.n_batches == 3 and got.last()[0].item() == float(lt.item())
    # the confusion matrix: the host's count of decode() against the labels
    path = crf.decode(logits, kp)
    assert (path[kp] == -1).all() and (path[~kp] >= 0).all()
    want = torch.zeros(C, C, dtype=torch.int64)
    v = (em >= 0).cpu()
    want.view(-1).index_add_(0, (em.cpu()[v] * C + path.cpu()[v]), torch.ones(int(v.sum()), dtype=torch.int64))
    arg = torch.zeros(C, C, dtype=torch.int64)
    arg.view(-1).index_add_(0, (em.cpu()[v] * C + logits.argmax(-1).cpu()[v]), torch.ones(int(v.sum()), dtype=torch.int64))
    cm = _confusion(got)
    print(f"{kind}: labelled rows {int(v.sum())}, positions where the path differs from the argmax {int((path != logits.argmax(-1))[~kp].sum())}")
    assert torch.equal(cm, 3 * want) and torch.equal(_confusion(plain), arg) and not torch.equal(want, arg)
    # ... and None afterwards is the plain record again, bit for bit
    again = DeviceScores(C, DEV)
    m.eval_step(t, a, kp, em, again, label_smoothing=0.0, use_graph=True)
    assert torch.equal(again.record, plain.record)


# ---- 4. a frozen module under every training mode -----------------------------------------------------------------------------------------
def _standalone(plan, crf, normalise=True):
    """The stand-alone kernel on the plan's own logits and labels (padded plans)."""
    return F.crf_nll(plan._logits.reshape(-1, C).clone(), plan.labels_in.clone(), crf.params.detach(), batch=plan.B, normalise=normalise,
                     param_grad=False)


def test_frozen_under_accumulation():
    big = _batch(6, 12, 9)
    mbs = [[x[i * 3:(i + 1) * 3] for x in big] for i in range(2)]
    crf = _crf(trainable=False)
    m_big, m_acc = _model(), _model()
    m_acc.set_grad_accumulation(True)
    loss_big = m_big.train_step(*big, label_smoothing=0.0, crf=crf, use_graph=False)
    m_acc.zero_grad(set_to_none=True)
    for mb in mbs:
        m_acc.train_step(*mb, label_smoothing=0.0, normalise=False, crf=crf, use_graph=False)
    den, num = m_acc.loss_terms()[1], m_acc.loss_terms()[2]
    worst = 0.0
    for (k, p), (_, q) in zip(m_acc.named_parameters(), m_big.named_parameters()):
        worst = max(worst, ((p.grad / den) - q.grad).abs().max().item() / max(q.grad.abs().max().item(), 1e-12))
    print(f"group loss {(num / den).item()!r}, big batch {loss_big.item()!r}; gradient error (of the largest element) {worst:.3e}")
    assert abs((num / den).item() - loss_big.item()) < 1e-5 and worst < 5e-6
    with pytest.raises(ValueError, match="gradient accumulation"):
        m_acc.train_step(*mbs[0], label_smoothing=0.0, crf=_crf(), use_graph=False)


@pytest.mark.parametrize("grad_bf16", [False, True])
def test_frozen_in_bf16_mode_and_with_clipping_and_the_optimizer_inside(grad_bf16):
    t, a, kp, em = _batch(6, 12, 1)
    crf = _crf(trainable=False)
    ma, mb = _model("bf16"), _model("bf16")
    if grad_bf16:
        assert ma.set_grad_bf16(True) and mb.set_grad_bf16(True)
    oa, ob = FusedAdam(ma, lr=1e-3, max_grad_norm=1e-4), FusedAdam(mb, lr=1e-3, max_grad_norm=1e-4)
    la = ma.train_step(t, a, kp, em, label_smoothing=0.0, crf=crf, use_graph=False, optimizer=oa)
    lb = mb.train_step(t, a, kp, em, label_smoothing=0.0, crf=crf, use_graph=False)
    ob.step()
    plan = _last_plan(ma)
    out, dl, _, _ = _standalone(plan, crf)
    l32 = _model().train_step(t, a, kp, em, label_smoothing=0.0, crf=crf, use_graph=False)
    print(f"bf16 (bf16 gradients {grad_bf16}) loss {la.item()!r}, fp32 loss {l32.item()!r}, clip coefficient {oa.clip_coef().item()!r}")
    assert torch.equal(la, lb) and torch.equal(la, out[0]) and torch.equal(plan._dlogits.reshape(dl.shape), dl)
    assert abs(la.item() - l32.item()) <= 2e-3 and oa.clip_coef().item() < 1.0
    assert all(torch.isfinite(p).all() for p in ma.parameters())


@pytest.fixture(scope="module")
def one_rank_group():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    rank, world, _ = dp.init_distributed()
    assert (rank, world) == (0, 1) and dist.is_initialized()
    yield
    dist.destroy_process_group()
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        os.environ.pop(k, None)


def test_frozen_under_one_rank_data_parallel(one_rank_group):
    t, a, kp, em = _batch(6, 12, 1)
    crf = _crf(trainable=False)
    m = _model()
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01)
    step = dp.DataParallelStep(m, opt, n_buckets=3, exchange="fp32", crf=crf)
    loss = step(t, a, kp, em, label_smoothing=0.0, use_graph=False)
    m2 = _model()
    opt2 = FusedAdam(m2, lr=1e-3, weight_decay=0.01)
    l2 = m2.train_step(t, a, kp, em, label_smoothing=0.0, normalise=False, crf=crf, use_graph=False)
    assert torch.equal(_last_plan(m)._dlogits, _last_plan(m2)._dlogits) and torch.equal(m.loss_terms()[:3], m2.loss_terms()[:3])
    opt2.grad_scale = m2.loss_terms()[1:2]
    opt2.step()
    print(f"data-parallel loss {loss.item()!r}, train_step loss {l2.item()!r}")
    assert torch.equal(loss, l2)
    for (n, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(p, q), n
    with pytest.raises(ValueError, match="DataParallelStep"):
        dp.DataParallelStep(m, opt, crf=_crf())
    for kw, name in (({"label_smoothing": 0.1}, "label_smoothing"), ({"label_smoothing": 0.0, "focal_gamma": 2.0}, "focal_gamma"),
                     ({"label_smoothing": 0.0, "class_weights": torch.ones(C, device=DEV)}, "class_weights")):
        with pytest.raises(ValueError, match=name):
            step(t, a, kp, em, use_graph=False, **kw)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_pair():
    t, a, kp, em = _batch(6, 12, 1)
    m, crf = _model(), _crf()
    u = torch.zeros(6, 12, C, device=DEV)
    for kw, name in (({"class_weights": torch.ones(C, device=DEV), "label_smoothing": 0.0}, "class_weights"),
                     ({"teacher_logits": u, "distill": (0.5, 2.0), "label_smoothing": 0.0}, "teacher_logits / distill"),
                     ({"focal_gamma": 2.0, "label_smoothing": 0.0}, "focal_gamma"),
                     ({}, "label_smoothing"), ({"label_smoothing": 0.05}, "label_smoothing")):
        with pytest.raises(ValueError, match="crf= does not combine with " + name):
            m.train_step(t, a, kp, em, crf=crf, use_graph=False, **kw)
    with pytest.raises(ValueError, match="classes"):
        m.train_step(t, a, kp, em, label_smoothing=0.0, crf=LinearChainCRF(5).to(DEV), use_graph=False)
    with pytest.raises(ValueError, match="LinearChainCRF"):
        m.train_step(t, a, kp, em, label_smoothing=0.0, crf=torch.zeros(63), use_graph=False)
    with pytest.raises(ValueError, match="move the module"):
        m.train_step(t, a, kp, em, label_smoothing=0.0, crf=LinearChainCRF(C), use_graph=False)
    sc = DeviceScores(C, DEV)
    m.eval()
    with pytest.raises(ValueError, match="focal_gamma"):
        m.eval_step(t, a, kp, em, sc, label_smoothing=0.0, focal_gamma=1.0, crf=crf)
    with pytest.raises(ValueError, match="label_smoothing"):
        m.eval_step(t, a, kp, em, sc, crf=crf)
    m.train()
    # the C entries refuse each other by name too (a plan driven by hand)
    m.train_step(t, a, kp, em, label_smoothing=0.0, crf=crf, use_graph=False)
    plan = _last_plan(m)
    from mer_amd import runtime
    for call, name in ((lambda: plan.set_focal(2.0), "m2f_plan_focal.*m2f_plan_crf"), (lambda: plan.distill(True), "m2f_plan_distill.*m2f_plan_crf"),
                       (lambda: plan.accumulate_grads(True), "m2f_plan_accumulate_grads.*m2f_plan_crf")):
        with pytest.raises(runtime.HipError, match=name):
            call()
    plan.set_crf(None)
    plan.set_focal(2.0)
    with pytest.raises(runtime.HipError, match="m2f_plan_crf.*m2f_plan_focal"):
        plan.set_crf(crf.params.detach(), None)
    plan.set_focal(None)


# ---- 6. the drop-in loop -----------------------------------------------------------------------------------------------------------------
def _dataset(n_dia, d_t, d_a, seed):
    """tests/test_focal_gpu.py's dataset, with sticky labels: an utterance keeps its predecessor's emotion three times out of four."""
    import numpy as np
    import pandas as pd
    import dataset as ds
    g = np.random.default_rng(seed)
    names = list(ds.EMOTIONS)
    rows = []
    for d in range(n_dia):
        cur = int(g.integers(0, 7))
        for u in range(int(g.integers(2, 10))):
            if g.random() > 0.75:
                cur = int(g.integers(0, 7))
            rows.append((f"utt {d}-{u}", names[cur], d, u))
    table = pd.DataFrame(rows, columns=["Utterance", "Emotion", "Dialogue_ID", "Utterance_ID"])
    text = torch.from_numpy(g.standard_normal((len(rows), d_t)).astype(np.float32))
    audio = torch.from_numpy(g.standard_normal((len(rows), d_a)).astype(np.float32))
    lab = table["Emotion"].map(ds.EMOTIONS).to_numpy()
    text[np.arange(len(rows)), lab] += 3.0                  # the label is learnable from the text rows
    return ds.Dataset("train", text_embeddings=text, audio_embeddings=audio, table=table)


def test_loop_trains_validates_checkpoints_and_tests_with_the_crf(tmp_path, monkeypatch):
    import sys
    import numpy as np
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    sys.path.insert(0, os.path.join(root, "src"))
    monkeypatch.chdir(root)
    import dataset as ds
    import test as te
    import train as tr
    from utils import AttrDict, get_config
    device = torch.device("cuda:0")
    model_cfg = synth._cfg(40, 48, 64, 4, 4, 4, 1, 1, 1, dropout=0.0)
    sd = synth.make_state_dict(model_cfg)
    cfg = AttrDict(dict(get_config()))
    cfg.model = AttrDict(model_cfg)
    cfg.runtime = AttrDict(dict(cfg.runtime, crf=AttrDict(init="bigram", smoothing=1.0, trainable=True, lr=1.0e-2)))
    cfg.solver = AttrDict(dict(cfg.solver, epochs=2, lr=2e-3, weight_decay=0.01, loss_fn="CRF", balance_classes=False,
                               early_stopping=AttrDict(enabled=False, patience=5, restore_best_weights=False),
                               scheduler=AttrDict(enabled=False, scheduler_fn="ExponentialLR", gamma=0.9)))
    d_train, d_val = _dataset(24, 48, 40, 1), _dataset(8, 48, 40, 2)
    dl_train = torch.utils.data.DataLoader(d_train, collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    dl_val = torch.utils.data.DataLoader(d_val, collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    settings = tr.crf_settings(cfg)
    assert settings == {"init": "bigram", "smoothing": 1.0, "trainable": True, "lr": 1.0e-2}
    with pytest.raises(ValueError, match="balance_classes"):
        tr.build_criterion(AttrDict(dict(cfg.solver, balance_classes=True)), d_train, device, crf=settings)

    def run(device_metrics, save=False):
        crit = tr.build_criterion(cfg.solver, d_train, device, crf=settings)
        assert type(crit) is LinearChainCRF and crit.trainable and isinstance(crit.optimizer, torch.optim.Adam)
        assert torch.allclose(crit.transitions.exp().sum(1), torch.ones(7, device=device), atol=1e-5)          # init: bigram
        assert float(crit.transitions.diagonal().mean()) > float(crit.transitions.mean())                      # ... of sticky labels
        cfg.checkpoint = AttrDict(save_path=str(tmp_path / f"ck{int(device_metrics)}" / "m2fnet.pth"), load_path="", save_checkpoint=save,
                                  load_checkpoint=False)
        m = tr.build_model(cfg, device)
        m.load_state_dict({k: v.to(device) for k, v in sd.items()})
        m.device_metrics = device_metrics
        tr.attach_crf(m, crit)
        start = crit.params.detach().clone()
        out = tr.training_loop(m, dl_train, dl_val, crit, tr.build_optimizer(cfg, m), None, 0, cfg, device)
        assert not torch.equal(crit.params.detach(), start), "the second Adam steps the block"
        return m, crit, out

    m_host, c_host, host = run(False)
    m_dev, c_dev, devs = run(True, save=True)
    print(f"train {host['loss_values']} / {devs['loss_values']}; validation host loop {host['val_loss_values']}, device {devs['val_loss_values']}")
    assert host["loss_values"] == devs["loss_values"] and torch.equal(c_host.params, c_dev.params)
    for p, q in zip(m_host.parameters(), m_dev.parameters()):
        assert torch.equal(p, q)
    for x, y in zip(host["val_loss_values"], devs["val_loss_values"]):
        assert np.isfinite(x) and abs(x - y) <= 2e-5, (x, y)
    # the loop minimises the criterion over the training dialogues: its running loss falls, and validate() over the TRAINING loader scores
    # the trained model and block below the untrained ones.  (Held-out loss is printed, not asserted: 24 synthetic dialogues and six
    # optimizer steps promise nothing about generalisation - measured: 1.350 untrained, 1.408 / 1.413 after epochs 1 / 2.)
    m0 = tr.build_model(cfg, device)
    m0.load_state_dict({k: v.to(device) for k, v in sd.items()})
    m0.device_metrics = False
    c0 = tr.build_criterion(cfg.solver, d_train, device, crf=settings)
    before, after = tr.validate(m0, dl_train, c0, device)[0], tr.validate(m_host, dl_train, c_host, device)[0]
    print(f"criterion over the training dialogues: untrained {before}, trained {after}; held-out, untrained {tr.validate(m0, dl_val, c0, device)[0]}")
    assert host["loss_values"][1] < host["loss_values"][0] and after < before
    assert all("crf" not in k for k in m_dev.state_dict())
    # host loop and device metrics decode alike: the Viterbi path, not the argmax
    acc_h = tr.validate(m_host, dl_val, c_host, device)
    acc_d = tr.validate(m_dev, dl_val, c_dev, device)
    print(f"validate: host loop {acc_h}, device metrics {acc_d}")
    assert abs(acc_h[1] - acc_d[1]) <= 1e-9 and abs(acc_h[2] - acc_d[2]) <= 1e-9
    # the checkpoint carries the block; test.py loads it and scores the Viterbi path
    state = torch.load(cfg.checkpoint.save_path, map_location="cpu")
    assert set(state) == {"epoch", "model_state_dict", "optimizer_state_dict", "crf_state_dict"}
    assert torch.equal(state["crf_state_dict"]["params"], c_dev.params.detach().cpu())
    for device_metrics in (False, True):
        mt = tr.build_model(cfg, device)
        mt.device_metrics = device_metrics
        tr.attach_crf(mt, tr.build_crf(dict(settings, init="zeros", trainable=False), None, device))
        te.load_model_weights(mt, cfg.checkpoint.save_path, device)
        assert torch.equal(mt.crf.params, c_dev.params.detach()) and not mt.crf.trainable
        got = te.test(mt, dl_val, device)
        print(f"test.py (device metrics {device_metrics}): {got}")
        assert abs(got[0] - acc_d[1]) <= 1e-9 and abs(got[1] - acc_d[2]) <= 1e-9
    # a strong prior changes the decoded path: staying costs 50, so the path differs from the argmax pass of a model without crf
    with torch.no_grad():
        mt.crf.transitions.copy_(-50.0 * torch.eye(7))
    object.__setattr__(mt, "device_metrics", False)
    moved = te.test(mt, dl_val, device)
    tr.attach_crf(mt, None)
    plain = te.test(mt, dl_val, device)
    print(f"test.py with a prior that forbids staying {moved}, without a CRF {plain}")
    assert moved != plain
    # resume: the block comes back from the checkpoint
    cfg.checkpoint = AttrDict(dict(cfg.checkpoint, load_path=cfg.checkpoint.save_path, load_checkpoint=True))
    m2 = tr.build_model(cfg, device)
    tr.attach_crf(m2, tr.build_crf(dict(settings, init="zeros"), None, device))
    assert tr.resume_if_requested(cfg, m2, tr.build_optimizer(cfg, m2), device) == 2
    assert torch.equal(m2.crf.params.detach(), c_dev.params.detach())
    # the streamed test pass scores the emission logits' argmax and gets the filter: crf_posterior() is there for the caller
    tr.attach_crf(mt, tr.build_crf(dict(settings, init="zeros", trainable=False), None, device))
    mt.set_context(None, 0)
    mt.streaming = True
    streamed = te.test(mt, dl_val, device)
    phi = mt._test_stream.crf_posterior()
    print(f"streamed test pass {streamed}; posterior rows sum to {phi.exp().sum(1).tolist()}")
    assert mt._test_stream.crf is mt.crf and torch.allclose(phi.exp().sum(1), torch.ones(phi.shape[0], device=device), atol=1e-5)
    mt._test_stream.close()
    with pytest.raises(ValueError, match="crf_state_dict"):
        torch.save({k: v for k, v in state.items() if k != "crf_state_dict"}, str(tmp_path / "no_crf.pth"))
        te.load_model_weights(m2, str(tmp_path / "no_crf.pth"), device)
