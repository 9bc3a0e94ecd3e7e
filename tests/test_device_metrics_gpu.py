"""Device-side evaluation scoring (csrc/metrics.hip, m2f_eval_scores / m2f_eval_step, mer_amd.metrics.DeviceScores, M2FNet.eval_step,
runtime.device_metrics): the kernels against scikit-learn and torch on the same logits, the plan path against a no-grad forward, and
validate() / test() with the switch on against off.

Bounds: confusion matrices are integers and must be EQUAL; accuracy and weighted F1 are float64 and must be within 1e-12 of sklearn
(a rounding guard: the float64 restatement of the rule differs from sklearn in 0 of 20,000 batches, tests/test_device_metrics_cpu.py);
the loss must be within 2e-5 of torch.nn.CrossEntropyLoss (the bound DESIGN.md section 4 holds the criterion to) and BIT-EQUAL to the
train path's criterion (m2f_cross_entropy) on the same rows.  Every comparison prints its figures before it asserts (run with -s)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import eval_ref as ref  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402
from mer_amd import runtime  # noqa: E402
from mer_amd.metrics import HEAD, DeviceScores  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam, M2FCrossEntropyLoss  # noqa: E402

CFG = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2)                      # dropout 0, 7 classes
CFG_DROP = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2, dropout=0.4)
ACC_TOL, LOSS_TOL = 1e-12, 2e-5


def _close(a, b, tol):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _weights(C):
    return (0.5 + torch.arange(C, dtype=torch.float32) / C).cuda()


def _read(sc):
    """-> (head of the record as a list of floats, confusion matrix as a numpy int64 array)."""
    h = sc.record.cpu()
    C = sc.n_classes
    return h[:HEAD].tolist(), h[HEAD:].view(torch.int64).view(C, C).numpy().copy()


def _torch_loss(logits, labels, cw, ls):
    crit = torch.nn.CrossEntropyLoss(weight=cw, ignore_index=-1, label_smoothing=ls)
    return float(crit(logits, labels))


# ---- the kernels on seeded logits --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unlabelled", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [2, 7, 16])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 1000, 32768])
def test_kernel_against_sklearn_and_torch(T, C, weighted, ls, unlabelled):
    logits, labels = ref.logits_batch(T, C, seed=1000 * C + T, unlabelled=unlabelled)
    logits, labels = logits.cuda(), labels.cuda()
    cw = _weights(C) if weighted else None
    sc = DeviceScores(C, "cuda")
    sc.update(logits, labels, cw, ls)
    head, cm = _read(sc)
    valid = (labels != -1).cpu()
    target = labels.cpu()[valid].numpy()
    predicted = logits.argmax(1).cpu()[valid].numpy()
    acc_s, f1_s = ref.sk_scores(target, predicted)
    loss_t = _torch_loss(logits, labels, cw, ls)
    ce = float(F.cross_entropy(logits, labels, cw, ls)[0][0])
    print(f"T={T} C={C} w={weighted} ls={ls} unl={unlabelled}: acc {head[5]!r} / {acc_s!r}  f1 {head[6]!r} / {f1_s!r}  "
          f"loss {head[4]!r} torch {loss_t!r} m2f_cross_entropy {ce!r}")
    assert (cm == ref.sk_confusion(target, predicted, C)).all()
    if unlabelled >= 1.0 or len(target) == 0:                        # (T = 1 at 30 % may draw no labelled row either)
        assert math.isnan(head[4]) and math.isnan(head[5]) and math.isnan(head[6])
    assert _close(head[5], acc_s, ACC_TOL) and _close(head[6], f1_s, ACC_TOL)
    assert _close(head[4], loss_t, LOSS_TOL)
    assert _same(head[4], ce)                                        # the train path's criterion, bit for bit
    assert _same(head[0], head[4]) and _same(head[1], head[5]) and _same(head[2], head[6]) and head[3] == 1.0


def _special_rows(C):
    nan = float("nan")
    rows = [
        [0.0] * C,                                # all equal: class 0
        [1.0] * C,
        [-0.0] + [0.0] * (C - 1),                 # -0.0 == 0.0: the first one
        [0.0] + [-0.0] * (C - 1),
        [-1.0, 2.0] + [2.0] * (C - 2),            # repeated maximum: its first index
        [3.0] + [1.0] * (C - 2) + [3.0],
        [1.0] * (C - 1) + [nan],                  # a NaN counts as maximal
        [nan] + [5.0] * (C - 1),
        [1.0, nan] + [nan] * (C - 2),             # the first NaN
        [-float("inf")] * C,
        [float("inf"), 1.0] + [float("inf")] * (C - 2),
    ]
    return torch.tensor(rows, dtype=torch.float32)


@pytest.mark.parametrize("C", [2, 7, 16])
def test_ties_and_specials_follow_torch_argmax(C):
    g = torch.Generator().manual_seed(C)
    logits = torch.cat([_special_rows(C), torch.randint(-2, 3, (500, C), generator=g).float()]).cuda()
    T = logits.shape[0]
    labels = torch.randint(0, C, (T,), generator=g).cuda()
    sc = DeviceScores(C, "cuda")
    sc.update(logits, labels)
    _, cm = _read(sc)
    predicted = torch.argmax(logits, dim=1)                          # on the same device tensor
    want = torch.zeros(C, C, dtype=torch.int64)
    for t, p in zip(labels.cpu().tolist(), predicted.cpu().tolist()):
        want[t, p] += 1
    assert (cm == want.numpy()).all(), (cm, want)
    # every special row on its own as well: a one-row batch's matrix names the prediction
    for i in range(_special_rows(C).shape[0]):
        one = DeviceScores(C, "cuda")
        one.update(logits[i: i + 1], labels[i: i + 1])
        _, cm1 = _read(one)
        assert cm1[int(labels[i]), int(predicted[i])] == 1 and cm1.sum() == 1, (i, cm1)


@pytest.mark.parametrize("T", [65, 1000, 32768])
def test_same_batch_twice_gives_identical_bytes(T):
    logits, labels = ref.logits_batch(T, 7, seed=T)
    logits, labels = logits.cuda(), labels.cuda()
    recs = []
    for _ in range(2):
        sc = DeviceScores(7, "cuda")
        sc.update(logits, labels, _weights(7), 0.1)
        recs.append(sc.record.cpu().view(torch.int64))
    assert torch.equal(recs[0], recs[1])


def test_accumulation_over_a_pass():
    from metrics import BatchScores
    g = torch.Generator().manual_seed(3)
    sc, host = DeviceScores(7, "cuda"), BatchScores()
    cm_want = np.zeros((7, 7), dtype=np.int64)
    loss_sum = 0.0
    n = 12
    for i in range(n):
        B, L = int(torch.randint(1, 9, (1,), generator=g)), int(torch.randint(1, 34, (1,), generator=g))
        logits = (torch.randn(B, L, 7, generator=g) * 2).cuda()
        lens = torch.randint(1, L + 1, (B,), generator=g)
        emotion = torch.randint(0, 7, (B, L), generator=g)
        emotion[torch.arange(L)[None, :] >= lens[:, None]] = -1
        emotion = emotion.cuda()
        sc.update(logits, emotion)
        host.update(logits, emotion)
        valid = emotion != -1
        cm_want += ref.sk_confusion(emotion[valid].cpu().numpy(), logits.argmax(2)[valid].cpu().numpy(), 7)
        loss_sum += float(F.cross_entropy(logits.reshape(-1, 7), emotion.reshape(-1), None, 0.1)[0][0])
        assert float(sc.last()[0]) == float(F.cross_entropy(logits.reshape(-1, 7), emotion.reshape(-1), None, 0.1)[0][0])
    acc_sum, f1_sum = sc.sums()
    print(f"acc_sum {acc_sum!r} / {host.sums()[0]!r}  f1_sum {f1_sum!r} / {host.sums()[1]!r}")
    assert abs(acc_sum - host.sums()[0]) <= n * ACC_TOL and abs(f1_sum - host.sums()[1]) <= n * ACC_TOL
    assert sc.n_batches == host.n_batches == n
    assert (sc.confusion().numpy() == cm_want).all()
    assert sc.totals()[0] == loss_sum and sc.mean_loss() == loss_sum / n
    assert abs(sc.result()[0] - host.result()[0]) <= ACC_TOL and abs(sc.result()[1] - host.result()[1]) <= ACC_TOL
    rep = sc.report()
    assert rep["support"] == cm_want.sum(1).tolist()
    sc.reset()
    assert sc.n_batches == 0 and int(sc.confusion().sum()) == 0 and sc.totals() == (0.0, 0.0, 0.0, 0.0)


# ---- eval_step against forward ---------------------------------------------------------------------------------------------
def _model(cfg=CFG, precision="fp32", **kw):
    m = M2FNet(cfg, precision=precision, **kw)
    m.load_state_dict(synth.make_state_dict(cfg))
    return m.to("cuda").eval()


def _batch(B, L, seed, lengths=None, cfg=CFG):
    if lengths is None:
        g = torch.Generator().manual_seed(seed)
        lengths = [L] + [int(x) for x in torch.randint(1, L + 1, (B - 1,), generator=g)]
    return [t.cuda() for t in synth.make_inputs(cfg, B, L, lengths, "randn", seed=seed)]


def _compare_with_forward(m, batch, use_graph=True, loss_bits=False):
    text, audio, mask, emotion = batch
    a, b = DeviceScores(7, "cuda"), DeviceScores(7, "cuda")
    m.eval_step(text, audio, mask, emotion, a, use_graph=use_graph)
    with torch.no_grad():
        b.update(m(text, audio, mask), emotion)
    (ha, cma), (hb, cmb) = _read(a), _read(b)
    print(f"eval_step loss {ha[4]!r} acc {ha[5]!r} f1 {ha[6]!r} | forward + update loss {hb[4]!r} acc {hb[5]!r} f1 {hb[6]!r}")
    assert cma.sum() == int((emotion != -1).sum()) and cma.sum() > 0
    assert (cma == cmb).all()
    assert ha[5] == hb[5] and ha[6] == hb[6]
    assert abs(ha[4] - hb[4]) <= LOSS_TOL
    if loss_bits:
        assert ha[4] == hb[4]
    return ha, cma


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["padded", "packed", "long", "partial_last"])
def test_eval_step_against_forward(kind, precision):
    m = _model(precision=precision, packed=(kind == "packed"))
    if kind == "long":
        batches = [_batch(2, 100, 5, lengths=[100, 37])]
    elif kind == "partial_last":
        batches = [_batch(8, 16, 6), _batch(8, 16, 7), _batch(3, 9, 8)]          # the last one lands in the 4 x 16 bucket
    elif kind == "packed":
        batches = [_batch(8, 32, 9, lengths=[32, 3, 5, 1, 9, 2, 4, 7]), _batch(8, 32, 10, lengths=[32, 2, 6, 1, 8, 3, 5, 7])]
    else:
        batches = [_batch(8, 16, 11), _batch(8, 16, 12)]
    for rounds in range(2):                                            # (the second round replays the captured graphs)
        for batch in batches:
            _compare_with_forward(m, batch)
    plans = list(m.engine().plans.values())
    if kind in ("packed", "long"):
        assert any(p.packed for p in plans)
    if kind == "partial_last":
        assert len({(p.B, p.L) for p in plans}) == 2
    assert all(not p.train for p in plans)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_exact_plan_gives_the_forward_loss_bit_for_bit(precision):
    """shape_buckets=False and a full batch: eval_step sums exactly the rows forward hands back."""
    m = _model(precision=precision, shape_buckets=False)
    batch = _batch(5, 9, 13, lengths=[9, 9, 9, 9, 9])
    for _ in range(3):
        _compare_with_forward(m, batch, loss_bits=True)
    ragged = _batch(5, 9, 14, lengths=[9, 1, 4, 7, 2])                 # the same plan, pad slots inside: labels -1 at the same rows
    _compare_with_forward(m, ragged, loss_bits=True)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_eager_and_replay_give_identical_records(precision):
    m = _model(precision=precision)
    b1, b2 = _batch(8, 16, 21), _batch(8, 16, 22)
    order = [b1, b1, b2, b1, b2, b2]
    recs, scs = {}, {}
    for use_graph in (True, False):
        sc = DeviceScores(7, "cuda")
        lasts = []
        for b in order:
            m.eval_step(*b, sc, use_graph=use_graph)
            lasts.append(sc.last().cpu().clone())
        recs[use_graph], scs[use_graph] = (sc.record.cpu().view(torch.int64), lasts), sc
    assert torch.equal(recs[True][0], recs[False][0])
    for x, y in zip(recs[True][1], recs[False][1]):
        assert torch.equal(x, y)
    # the replay scored the batch it was given: b2's numbers are those of b2 alone, and differ from b1's
    alone = {}
    for name, b in (("b1", b1), ("b2", b2)):
        sc = DeviceScores(7, "cuda")
        m.eval_step(*b, sc, use_graph=False)
        alone[name] = sc.last().cpu().clone()
    assert not torch.equal(alone["b1"], alone["b2"])
    for b, last in zip(order, recs[True][1]):
        assert torch.equal(last, alone["b1" if b is b1 else "b2"])
    # a second record: the captured graph is not replayed into the first one
    sc2 = DeviceScores(7, "cuda")
    m.eval_step(*b1, sc2, use_graph=True)
    m.eval_step(*b2, sc2, use_graph=True)
    assert sc2.n_batches == 2 and torch.equal(sc2.last().cpu(), alone["b2"])
    assert torch.equal(scs[True].record.cpu().view(torch.int64), recs[True][0])


def test_class_weights_and_smoothing_reach_the_plan():
    m = _model()
    batch = _batch(8, 16, 31)
    text, audio, mask, emotion = batch
    w = _weights(7)
    for use_graph in (False, True, True):
        a, b = DeviceScores(7, "cuda"), DeviceScores(7, "cuda")
        m.eval_step(text, audio, mask, emotion, a, class_weights=w, label_smoothing=0.05, use_graph=use_graph)
        with torch.no_grad():
            logits = m(text, audio, mask)
        b.update(logits, emotion, w, 0.05)
        assert abs(a.mean_loss() - b.mean_loss()) <= LOSS_TOL
        assert abs(a.mean_loss() - _torch_loss(logits.reshape(-1, 7), emotion.reshape(-1), w, 0.05)) <= LOSS_TOL
        c = DeviceScores(7, "cuda")
        m.eval_step(text, audio, mask, emotion, c, use_graph=use_graph)
        assert abs(c.mean_loss() - a.mean_loss()) > 1e-4              # (the unweighted, 0.1-smoothed loss is another number)


# ---- the training state ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_train_state_untouched_by_eval_step(precision):
    def run(with_eval):
        torch.manual_seed(0)
        m = M2FNet(CFG, precision=precision)
        m.load_state_dict(synth.make_state_dict(CFG))
        m = m.to("cuda").train()                                      # dropout 0: eval_step is legal in training mode
        opt = FusedAdam(m, lr=1e-3)
        tb, eb = _batch(8, 16, 41), _batch(8, 16, 42)
        sc = DeviceScores(7, "cuda")
        losses = []
        for i in range(5):
            losses.append(m.train_step(*tb, use_graph=True).item())
            opt.step()
            if with_eval and i >= 1:
                m.eval_step(*eb, sc, use_graph=True)
        torch.cuda.synchronize()
        return losses, {n: p.grad.detach().clone() for n, p in m.named_parameters()}, m.flat_parameters().clone()

    la, ga, pa = run(True)
    lb, gb, pb = run(False)
    assert la == lb
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    assert torch.equal(pa, pb)


def test_eval_step_draws_no_dropout_masks():
    m = _model(CFG_DROP)
    eng = m.engine()
    batch = _batch(8, 16, 51, cfg=CFG_DROP)
    sc = DeviceScores(7, "cuda")
    before = eng.rng.clone()
    for _ in range(3):
        m.eval_step(*batch, sc)
    torch.cuda.synchronize()
    assert torch.equal(eng.rng, before) and sc.n_batches == 3


def test_refusals():
    m = _model(CFG_DROP)
    batch = _batch(8, 16, 52, cfg=CFG_DROP)
    sc = DeviceScores(7, "cuda")
    m.train()
    with pytest.raises(RuntimeError, match="training mode with dropout"):
        m.eval_step(*batch, sc)
    # the C entry refuses a train plan whose dropout is active, and a NULL / closed plan
    eng = m.engine()
    plan = eng.plan(8, 16, True, True)
    plan.set_inputs(batch[0], batch[1], batch[2], batch[3])
    with pytest.raises(runtime.HipError, match="dropout"):
        plan.eval_step(sc.record)
    assert runtime.lib().m2f_eval_step(None, 0.1, 0, sc.record.data_ptr(), 1, None) != 0
    assert "NULL plan" in runtime.lib().m2f_last_error().decode()
    plan.close()
    with pytest.raises(runtime.HipError, match="closed"):
        plan.eval_step(sc.record)
    assert sc.n_batches == 0
    with pytest.raises(ValueError):
        m.eval().eval_step(*batch, DeviceScores(5, "cuda"))
    with pytest.raises(ValueError):
        sc.update(torch.zeros(4, 6, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"))


# ---- the drop-in loops -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("weighted", [False, True])
def test_validate_and_test_with_the_switch_on_against_off(weighted, precision):
    import train as tr
    import test as te
    device = torch.device("cuda:0")
    m = M2FNet(CFG_DROP, precision=precision)
    m.load_state_dict(synth.make_state_dict(CFG_DROP))
    m = m.to(device)
    loader = ref.collated_batches(7, 64, 48, 7, seed=61)
    w = _weights(7) if weighted else None
    crit = M2FCrossEntropyLoss(weight=w, ignore_index=-1, label_smoothing=0.1)
    out = {}
    for on in (False, True, True):                                     # (the second pass with the switch on replays the graphs)
        m.device_metrics = on
        out[on] = (tr.validate(m, loader, crit, device), te.test(m, loader, device))
    (loss0, acc0, f10), (tacc0, tf10) = out[False]
    (loss1, acc1, f11), (tacc1, tf11) = out[True]
    print(f"validate off {out[False][0]!r} on {out[True][0]!r}; test off {out[False][1]!r} on {out[True][1]!r}")
    assert abs(acc1 - acc0) <= ACC_TOL and abs(f11 - f10) <= ACC_TOL and abs(loss1 - loss0) <= LOSS_TOL
    assert abs(tacc1 - tacc0) <= ACC_TOL and abs(tf11 - tf10) <= ACC_TOL
    assert 0.0 < acc1 <= 1.0 and math.isfinite(loss1)
    # the pass's confusion matrix and per-class report (test.py prints it)
    rep = m.test_scores.report()
    n_valid = sum(int((b["emotion"] != -1).sum()) for b in loader)
    assert sum(rep["support"]) == n_valid == int(m.test_scores.confusion().sum())
