"""The supervised contrastive criterion inside the train step (M2FNet.train_step(supcon=(weight, temperature))) on the four plan kinds
of tests/test_rdrop_model_gpu.py: the step against the float64 reference (tests/golden/supcon_ref.py) on the plan's own features and
against the oracle's float64 autograd of CE + the reference term; weight 0; schedules under a replayed graph; every training mode;
dropout (the gate factor); bf16 mode (the shadow of the hidden gradient); last_features(); refusals; the drop-in loop.
Every comparison prints its figures before it asserts (-s)."""
import os
import sys
import types

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))
sys.path.insert(0, ROOT)

import supcon_ref as ref  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import dp  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam, M2FCrossEntropyLoss, M2FSupConLoss  # noqa: E402
from oracle import m2fnet_oracle as O  # noqa: E402

DEV = "cuda"
CFG = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2, ncls=7)          # dropout 0 (tests/test_rdrop_model_gpu.py's)
CFG_DROP = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2, ncls=7, dropout=0.4)
C, HID = 7, 64
PLAN_KINDS = {"padded_4x6": (4, 6, 1, [6, 6, 5, 6], None), "bucketed_3x5": (3, 5, 4, [5, 2, 4], None),
              "packed_5x9": (5, 9, 2, [9, 1, 5, 3, 2], True), "long_2x70": (2, 70, 3, [70, 5], None)}
FIRST = "output_layer.0.weight"


def _model(precision="fp32", packed=None, cfg=CFG, **kw):
    m = M2FNet(cfg, precision=precision, packed=packed, **kw)
    m.load_state_dict(synth.make_state_dict(cfg))
    return m.to(DEV).train()


def _batch(B, L, seed, lengths=None, cfg=CFG):
    if lengths is None:
        g = torch.Generator().manual_seed(seed)
        lengths = [L] + [int(x) for x in torch.randint(1, L + 1, (B - 1,), generator=g)]
    t, a, kp, em = [x.to(DEV) for x in synth.make_inputs(cfg, B, L, lengths, "randn", seed=seed)]
    # labels by hand: three classes in turn, so that every labelled utterance has positives whatever the synthetic labels were
    hand = (torch.arange(B * L, device=DEV).reshape(B, L) % 3) + 2
    return t, a, kp, torch.where(em >= 0, hand, em)


def _last_plan(m):
    return m.engine().plans[next(reversed(m.engine().plans))]


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _equal_grads(ma, mb, what):
    for (k, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(p.grad, q.grad), (what, k, (p.grad - q.grad).abs().max().item())


def _reference_on_features(feats, em, lam, tau, cw=None):
    """The float64 reference on [B, L, hid] features and [B, L] labels (the contrast set is every dialogue of the batch)."""
    r = ref.supcon(feats.detach().cpu().reshape(-1, feats.shape[-1]), em.cpu().reshape(-1), C, None if cw is None else cw.cpu(), lam, tau)
    anchors = int(r["has"].sum())
    assert anchors >= 2, anchors
    return r, anchors


def _oracle_grads(cfg, t, a, kp, em, lam, tau, cw=None):
    """float64 autograd through the oracle of CE + lam * con / den, the features captured by the oracle's `drop` hook under
    "classifier" -> (loss, con / den, features, {name: grad})."""
    leaves, sd = {}, {}
    for k, v in synth.make_state_dict(cfg).items():           # (one leaf per unique tensor, as oracle.loss_and_grads)
        if id(v) not in leaves:
            leaves[id(v)] = v.detach().double().requires_grad_(True)
        sd[k] = leaves[id(v)]
    seen = {}

    def drop(name, x):
        if name == "classifier":
            seen["h"] = x
        return x

    logits = O.forward(sd, cfg, t.cpu().double(), a.cpu().double(), kp.cpu(), drop=drop)
    cwd = None if cw is None else cw.cpu().double()
    ce = O.cross_entropy(logits, em.cpu(), cwd)
    h = seen["h"]
    r = ref.supcon(h.reshape(-1, h.shape[-1]), em.cpu().reshape(-1), C, cwd, lam, tau)
    loss = ce + lam * r["con"] / r["den"]
    loss.backward()
    return loss.detach(), (r["con"] / r["den"]).detach(), h.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}


# ---- 1. the step against the reference and the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", list(PLAN_KINDS))
def test_step_matches_the_reference_and_the_oracle(kind, weighted):
    """Parameter gradients: the bound tests/test_model_gpu.py applies to the plain criterion's gradients against the oracle,
    3e-5 + 1e-3 x the reference tensor's largest element.  The oracle WITHOUT the term must miss that bound (printed), so the test fails
    without the feature."""
    B, L, seed, lengths, packed = PLAN_KINDS[kind]
    t, a, kp, em = _batch(B, L, seed, lengths)
    cw = (0.3 + torch.arange(C, device=DEV) * 0.7) if weighted else None
    lam, tau = 0.8, 0.1
    m = _model(packed=packed)
    loss = m.train_step(t, a, kp, em, class_weights=cw, supcon=(lam, tau), use_graph=False)
    plan = _last_plan(m)
    assert plan.packed == (kind in ("packed_5x9", "long_2x70")) and plan._supcon
    feats = m.last_features()
    r, anchors = _reference_on_features(feats, em, lam, tau, cw)
    ce, con = m.supcon_terms()
    plain = _model(packed=packed).train_step(t, a, kp, em, class_weights=cw, use_graph=False)
    con_ref = (r["con"] / r["den"]).item()
    err_con = abs(con.item() - con_ref)
    err_loss = abs(loss.item() - (plain.item() + lam * con_ref))
    print(f"{kind} weighted {weighted} (plan {plan.B} x {plan.L}, T {plan.T}): {anchors} anchors with positives; loss {loss.item()!r}, "
          f"plain {plain.item()!r}, con {con.item()!r} ref {con_ref!r} (err {err_con:.3e}), ce {ce.item()!r}; loss err {err_loss:.3e}")
    assert err_con <= 2e-6 * max(1.0, abs(con_ref)) and err_loss <= 4e-6 * max(1.0, abs(loss.item()))
    assert abs(ce.item() - plain.item()) <= 4e-6 * max(1.0, abs(plain.item()))
    assert abs(m.loss_terms()[1].item() - r["den"].item()) <= 1e-6 * r["den"].item()
    lo, con_o, h_o, g_o = _oracle_grads(CFG, t, a, kp, em, lam, tau, cw)
    _, _, _, g_plain = _oracle_grads(CFG, t, a, kp, em, 0.0, tau, cw)
    ferr = (feats.cpu().double() - h_o)[~kp.cpu()].abs().max().item()          # (pad slots: 0 in last_features, whatever the oracle holds)
    print(f"{kind}: features against the oracle's: {ferr:.3e}; oracle loss {lo.item()!r} (err {abs(lo.item() - loss.item()):.3e})")
    assert ferr <= 1e-4 and abs(lo.item() - loss.item()) <= 2e-5
    worst, worst_plain, missed = 0.0, 0.0, 0
    for k, p in m.named_parameters():
        g, want = p.grad.detach().cpu().double(), g_o[k]
        bound = 3e-5 + 1e-3 * want.abs().max().item()
        err, err_plain = (g - want).abs().max().item(), (g_plain[k] - want).abs().max().item()
        worst, worst_plain = max(worst, err / bound), max(worst_plain, err_plain / bound)
        missed += err_plain > bound
        assert err <= bound, (k, err, bound)
    print(f"{kind}: worst gradient error / bound {worst:.3f}; the oracle without the term lies at {worst_plain:.1f} x the bound "
          f"({missed} tensors outside it)")
    assert missed > 0 and (g_plain[FIRST] - g_o[FIRST]).abs().max().item() > 3e-5 + 1e-3 * g_o[FIRST].abs().max().item()


def test_loss_module_is_the_steps_term():
    """M2FCrossEntropyLoss + weight * M2FSupConLoss on the model's own logits and features is the step's loss; its autograd gradient
    is the reference's."""
    t, a, kp, em = _batch(4, 6, 1, [6, 6, 5, 6])
    lam, tau = 0.8, 0.1
    m = _model()
    loss = m.train_step(t, a, kp, em, supcon=(lam, tau), use_graph=False)
    feats = m.last_features().requires_grad_(True)
    crit = M2FSupConLoss(temperature=tau, n_classes=C)
    term = crit(feats, em)
    term.backward()
    r, _ = _reference_on_features(feats, em, 1.0, tau)
    gerr = (feats.grad.cpu().double().reshape(-1, HID) - r["grad"] / r["den"]).abs().max().item() / (r["grad"] / r["den"]).abs().max().item()
    ce = M2FCrossEntropyLoss()(_last_plan(m).logits.permute(0, 2, 1), em)
    print(f"module term {term.item()!r}, reference {(r['con'] / r['den']).item()!r}; gradient error {gerr:.3e}; "
          f"CE + weight * term {(ce + lam * term).item()!r}, step {loss.item()!r}")
    assert abs(term.item() - (r["con"] / r["den"]).item()) <= 2e-6 * term.item() and gerr <= 1e-5
    assert abs((ce + lam * term).item() - loss.item()) <= 4e-6 * loss.item()


# ---- 2. weight 0 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(PLAN_KINDS))
def test_weight_zero_is_the_plain_step(kind):
    B, L, seed, lengths, packed = PLAN_KINDS[kind]
    t, a, kp, em = _batch(B, L, seed, lengths)
    ma, mb = _model(packed=packed), _model(packed=packed)
    la = ma.train_step(t, a, kp, em, supcon=(0.0, 0.1), use_graph=False)
    lb = mb.train_step(t, a, kp, em, use_graph=False)
    assert torch.equal(la, lb) and ma.supcon_terms()[1].item() > 0.0           # (the share is still reported)
    _equal_grads(ma, mb, kind)


# ---- 3. schedules under a replayed graph ---------------------------------------------------------------------------------------------------
def test_weight_schedule_and_plain_calls_replay_the_captured_step():
    t, a, kp, em = _batch(4, 6, 1, [6, 6, 5, 6])
    mg, fresh = _model(), _model()
    for _ in range(3):                                     # eager warm-up, capture, replay
        mg.train_step(t, a, kp, em, supcon=(0.5, 0.1), use_graph=True)
    plan = _last_plan(mg)
    n_plans, handle, ws = len(mg.engine().plans), plan.handle, plan.workspace.data_ptr()
    for lam, tau in ((0.5, 0.1), (2.0, 0.1), (0.0, 0.1), (2.0, 0.07)):
        lg = mg.train_step(t, a, kp, em, supcon=(lam, tau), use_graph=True)
        me = _model()
        le = me.train_step(t, a, kp, em, supcon=(lam, tau), use_graph=False)
        print(f"weight {lam} temperature {tau}: replayed loss {lg.item()!r}, eager loss of a fresh model {le.item()!r}")
        assert torch.equal(lg, le) and plan.supcon_host == (lam, tau)
        _equal_grads(mg, me, f"replay vs eager at {lam}")
        # a plain call in between is the model that never saw the term
        got, want = mg.train_step(t, a, kp, em, use_graph=True), fresh.train_step(t, a, kp, em, use_graph=True)
        assert torch.equal(got, want) and not plan._supcon
        _equal_grads(mg, fresh, "plain between contrastive calls")
    assert _last_plan(mg) is plan and (len(mg.engine().plans), plan.handle, plan.workspace.data_ptr()) == (n_plans, handle, ws)
    # the autograd path on the same plan does not inherit the term
    mg.train_step(t, a, kp, em, supcon=(2.0, 0.1), use_graph=True)
    mg.zero_grad(set_to_none=True)
    fresh.zero_grad(set_to_none=True)
    crit = M2FCrossEntropyLoss()
    crit(mg(t, a, kp).permute(0, 2, 1), em).backward()
    crit(fresh(t, a, kp).permute(0, 2, 1), em).backward()
    _equal_grads(mg, fresh, "forward + backward after a contrastive step")


# ---- 4. training modes ------------------------------------------------------------------------------------------------------------------
def test_accumulation_contrasts_each_micro_batch_within_itself():
    """The group's gradient / den is the sum of the two micro-batches' own normalised-by-hand steps: tests/test_grad_accumulation_gpu.py's
    bound, 5e-6 of the largest element of the tensor."""
    big = _batch(6, 12, 9)
    mbs = [[x[i * 3:(i + 1) * 3] for x in big] for i in range(2)]
    pair = (0.8, 0.1)
    m_acc = _model()
    m_acc.set_grad_accumulation(True)
    m_acc.zero_grad(set_to_none=True)
    singles, cons, dens = [], [], []
    for mb in mbs:
        m_acc.train_step(*mb, normalise=False, supcon=pair, use_graph=False)
        m1 = _model()
        m1.train_step(*mb, normalise=False, supcon=pair, use_graph=False)
        singles.append(_grads(m1))
        r, _ = _reference_on_features(m1.last_features(), mb[3], *pair)
        cons.append(r["con"].item())
        dens.append(r["den"].item())
    ce, con = m_acc.supcon_terms()
    worst = 0.0
    for k, p in m_acc.named_parameters():
        want = singles[0][k] + singles[1][k]
        worst = max(worst, (p.grad - want).abs().max().item() / max(want.abs().max().item(), 1e-12))
    con_ref = sum(cons) / sum(dens)
    print(f"group: con {con.item()!r}, the two micro-batches' own references {con_ref!r}; gradient error (of the largest element) {worst:.3e}")
    assert worst < 5e-6 and abs(con.item() - con_ref) <= 2e-6 * con_ref
    assert abs(m_acc.loss_terms()[1].item() - sum(dens)) <= 1e-6 * sum(dens)


@pytest.mark.parametrize("mode", ["grad_bf16", "optimizer", "clip", "speakers"])
def test_modes_carry_the_term(mode):
    t, a, kp, em = _batch(4, 6, 1, [6, 6, 5, 6])
    pair = (1.2, 0.1)
    precision = "bf16" if mode in ("grad_bf16", "optimizer") else "fp32"
    kw_model = {"speaker_heads": (1, 1)} if mode == "speakers" else {}
    g = torch.Generator().manual_seed(5)
    spk = torch.randint(0, 3, (4, 6), generator=g).to(torch.uint8).to(DEV)

    def run(**kw):
        m = _model(precision, **kw_model)
        opt = None
        if mode == "grad_bf16":
            assert m.set_grad_bf16(True)
        if mode in ("optimizer", "clip"):
            opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, max_grad_norm=1e-3 if mode == "clip" else None)
            kw = dict(kw, optimizer=opt)
        if mode == "speakers":
            kw = dict(kw, speakers=spk)
        loss = m.train_step(t, a, kp, em, use_graph=False, **kw)
        if mode == "grad_bf16":
            res = m.engine().grad_bf16_buf.clone()
        elif opt is not None:
            res = torch.cat([p.detach().flatten() for p in m.parameters()])
        else:
            res = torch.cat([x.flatten() for x in _grads(m).values()])
        return m, loss, res, opt

    _, l_plain, r_plain, _ = run()
    _, l_zero, r_zero, _ = run(supcon=(0.0, 0.1))
    assert torch.equal(l_plain, l_zero) and torch.equal(r_plain, r_zero)
    m, loss, res, opt = run(supcon=pair)
    r, anchors = _reference_on_features(m.last_features(), em, *pair)
    ce, con = m.supcon_terms()
    con_ref = (r["con"] / r["den"]).item()
    print(f"{mode}: loss {loss.item()!r}, plain {l_plain.item()!r}, con {con.item()!r} ref on the plan's features {con_ref!r}, {anchors} anchors")
    assert abs(con.item() - con_ref) <= 2e-6 * con_ref and abs(loss.item() - (ce + pair[0] * con).item()) <= 4e-6 * loss.item()
    assert torch.isfinite(res.float()).all() and not torch.equal(loss, l_plain) and not torch.equal(res, r_plain)
    if mode in ("optimizer", "clip"):                       # the step with the optimizer inside = the step, then optimizer.step()
        m2 = _model(precision)
        o2 = FusedAdam(m2, lr=1e-3, weight_decay=0.01, max_grad_norm=1e-3 if mode == "clip" else None)
        l2 = m2.train_step(t, a, kp, em, supcon=pair, use_graph=False)
        o2.step()
        assert torch.equal(loss, l2)
        if precision == "fp32":
            for (n, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
                assert torch.equal(p, q), n
        if mode == "clip":
            assert float(opt.clip_coef()) < 1.0 and torch.equal(opt.grad_norm(), o2.grad_norm())


# ---- 5. dropout: the stored features carry the masks, the gradient passes the gate ---------------------------------------------------------
@pytest.mark.parametrize("kind", ["padded_4x6", "packed_5x9"])
def test_dropout_step_on_its_own_features_and_the_gate_factor(kind):
    """Two models built under one seed draw the same masks.  The contrastive step's loss is the plain step's plus the reference term on
    the features the step stored (zeros where the mask fell); and the bias gradient of the layer that produces them moves by exactly
    sum_i [h_i > 0] * (1 / (1 - p)) * dh_i / den, dh the reference's gradient: the gate and its scale, checked against the closed form
    at the kernel tests' measured fp32 level (1e-5 of the largest element)."""
    B, L, seed, lengths, packed = PLAN_KINDS[kind]
    t, a, kp, em = _batch(B, L, seed, lengths, cfg=CFG_DROP)
    lam, tau = 1.5, 0.1
    torch.manual_seed(1234)
    ma = _model(packed=packed, cfg=CFG_DROP)
    torch.manual_seed(1234)
    mb = _model(packed=packed, cfg=CFG_DROP)
    la = ma.train_step(t, a, kp, em, supcon=(lam, tau), use_graph=False)
    lb = mb.train_step(t, a, kp, em, use_graph=False)
    fa, fb = ma.last_features(), mb.last_features()
    assert torch.equal(fa, fb), "the same masks in both models"
    live = fa[em >= 0]
    zeros = float((live == 0).float().mean())
    assert 0.4 < zeros < 0.95 and float(live.max()) > 0                     # ReLU and the 0.4 mask
    r, anchors = _reference_on_features(fa, em, lam, tau)
    con_ref = (r["con"] / r["den"]).item()
    print(f"{kind}: {anchors} anchors, {zeros:.2f} of the labelled features are 0; loss {la.item()!r}, plain {lb.item()!r} + {lam} * {con_ref!r}")
    assert abs(la.item() - (lb.item() + lam * con_ref)) <= 4e-6 * la.item()
    names = [n for n, _ in ma.named_parameters() if n.startswith("output_layer.") and n.endswith(".bias")]
    name = names[-2]                                                       # the bias of the Linear in front of the last ReLU + dropout
    ga, gb = dict(ma.named_parameters())[name].grad, dict(mb.named_parameters())[name].grad
    h = fa.cpu().double().reshape(-1, HID)
    want = ((h > 0) * (1.0 / (1.0 - 0.4)) * r["grad"] / r["den"]).sum(0)
    got = (ga - gb).cpu().double()
    err = (got - want).abs().max().item() / want.abs().max().item()
    ungated = (r["grad"] / r["den"]).sum(0)
    print(f"{kind}: {name} moved by (largest element) {want.abs().max().item():.3e}; error {err:.3e}; without the gate factor the closed form "
          f"lies {(ungated - want).abs().max().item() / want.abs().max().item():.3e} away")
    assert err <= 1e-5


# ---- 6. bf16 precision ----------------------------------------------------------------------------------------------------------------------
def test_bf16_mode_rewrites_the_shadow_of_the_hidden_gradient():
    """Weight 0: the plain bf16 step, bit for bit.  A large weight moves the first classifier layer's weight gradient, and it tracks the
    fp32-mode step within the relative L2 of 25 % that tests/test_model_gpu.py applies to bf16 gradients against fp32 mode - a stale
    shadow would leave the plain step's gradient there (its distance is printed and must miss the bound)."""
    t, a, kp, em = _batch(4, 6, 1, [6, 6, 5, 6])
    pair = (20.0, 0.1)
    m0, mp = _model("bf16"), _model("bf16")
    l0 = m0.train_step(t, a, kp, em, supcon=(0.0, 0.1), use_graph=False)
    lp = mp.train_step(t, a, kp, em, use_graph=False)
    assert torch.equal(l0, lp)
    _equal_grads(m0, mp, "bf16 weight 0")
    m16, m32 = _model("bf16"), _model("fp32")
    l16 = m16.train_step(t, a, kp, em, supcon=pair, use_graph=False)
    l32 = m32.train_step(t, a, kp, em, supcon=pair, use_graph=False)
    rel = lambda x, y: ((x - y).norm() / y.norm()).item()          # noqa: E731
    worst = 0.0
    for (k, p), (_, q) in zip(m16.named_parameters(), m32.named_parameters()):
        if k.startswith("output_layer.") and k.endswith(".weight"):
            d = rel(p.grad.double(), q.grad.double())
            worst = max(worst, d)
            print(f"bf16 vs fp32 mode, {k}: relative L2 {d:.3e}")
            assert d <= 0.25, k
    g16, g32, gpl = (dict(x.named_parameters())[FIRST].grad.double() for x in (m16, m32, mp))
    stale = rel(gpl, g32)
    print(f"loss bf16 {l16.item()!r} fp32 {l32.item()!r}; {FIRST}: bf16 vs fp32 {rel(g16, g32):.3e}, the plain bf16 step (a stale shadow) {stale:.3e}")
    assert abs(l16.item() - l32.item()) <= 2e-2 * max(1.0, abs(l32.item())) and stale > 0.25


# ---- 7. last_features -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(PLAN_KINDS))
def test_last_features_match_the_oracles_activation(kind):
    B, L, seed, lengths, packed = PLAN_KINDS[kind]
    t, a, kp, em = _batch(B, L, seed, lengths)
    m = _model(packed=packed).eval()
    with torch.no_grad():
        m(t, a, kp)
    f = m.last_features()
    _, _, h_o, _ = _oracle_grads(CFG, t, a, kp, em, 0.0, 0.1)
    err = (f.cpu().double() - h_o)[~kp.cpu()].abs().max().item()
    print(f"{kind}: last_features {tuple(f.shape)} against the oracle's activation: {err:.3e}")
    assert f.shape == (B, L, HID) and not f.requires_grad and err <= 1e-4
    assert not f[kp].any() and bool((f[~kp] >= 0).all())
    m.train()
    m.train_step(t, a, kp, em, use_graph=False)
    ferr = (m.last_features() - f).abs().max().item()                          # dropout 0: the train step stores the same activation
    assert ferr <= 1e-5, ferr


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_rank_group():
    import socket
    import torch.distributed as dist
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


def test_every_refusal_raises_by_name(one_rank_group):
    from mer_amd.crf import LinearChainCRF
    t, a, kp, em = _batch(4, 6, 1, [6, 6, 5, 6])
    m = _model()
    teacher = torch.zeros(4, 6, C, device=DEV)
    for kw, name in (({"teacher_logits": teacher, "distill": (0.5, 2.0)}, "teacher_logits"), ({"focal_gamma": 2.0}, "focal_gamma"),
                     ({"crf": LinearChainCRF(C).to(DEV), "label_smoothing": 0.0}, "crf"), ({"rdrop": 1.0}, "rdrop")):
        with pytest.raises(ValueError, match=f"M2FNet.train_step: supcon and {name} do not combine"):
            m.train_step(t, a, kp, em, supcon=(0.1, 0.1), **kw)
    for bad in ((-1.0, 0.1), (0.1, 0.0), (float("nan"), 0.1), (0.1, float("inf")), 0.1, (0.1,), (True, 0.1)):
        with pytest.raises(ValueError, match="supcon"):
            m.train_step(t, a, kp, em, supcon=bad)
    assert not m.engine().plans, "refused before any plan was built"
    step = dp.DataParallelStep(m, FusedAdam(m, lr=1e-3), n_buckets=3, exchange="fp32")
    with pytest.raises(ValueError, match="DataParallelStep: supcon is refused"):
        step(t, a, kp, em, supcon=(0.1, 0.1))
    # the C entries refuse each other by name
    m.train_step(t, a, kp, em, supcon=(0.1, 0.1), use_graph=False)
    plan = _last_plan(m)
    for entry, name in ((plan.distill, "m2f_plan_distill"), (plan.focal, "m2f_plan_focal"), (plan.rdrop, "m2f_plan_rdrop")):
        with pytest.raises(Exception, match=name + ": the supervised contrastive criterion is on"):
            entry(True)
    with pytest.raises(Exception, match="m2f_plan_crf: the supervised contrastive criterion is on"):
        plan.set_crf(*LinearChainCRF(C).to(DEV).step_buffers(plan.workspace.device, want_grad=False))
    plan.supcon(False)
    plan.focal(True)
    with pytest.raises(Exception, match="m2f_plan_supcon: the focal criterion is on"):
        plan.supcon(True)
    plan.focal(False)
    ev = m.engine().plan(4, 6, False, False)
    with pytest.raises(Exception, match="m2f_plan_supcon"):
        ev.supcon(True)                                     # eval plans keep the hard-label criterion


# ---- 9. the drop-in loop ------------------------------------------------------------------------------------------------------------------------
def _dataset(n_dia, d_t, d_a, seed):
    import dataset as ds
    g = np.random.default_rng(seed)
    rows = [(f"utt {d}-{u}", list(ds.EMOTIONS)[int(g.integers(0, 7))], d, u) for d in range(n_dia) for u in range(int(g.integers(1, 10)))]
    table = pd.DataFrame(rows, columns=["Utterance", "Emotion", "Dialogue_ID", "Utterance_ID"])
    text = torch.from_numpy(g.standard_normal((len(rows), d_t)).astype(np.float32))
    audio = torch.from_numpy(g.standard_normal((len(rows), d_a)).astype(np.float32))
    return ds.Dataset("train", text_embeddings=text, audio_embeddings=audio, table=table)


def test_loop_logs_both_shares_and_is_unchanged_with_the_key_off(monkeypatch):
    monkeypatch.chdir(ROOT)
    import dataset as ds
    import train as tr
    from utils import AttrDict, get_config
    device = torch.device("cuda:0")
    model_cfg = synth._cfg(40, 48, 64, 4, 4, 4, 1, 1, 1, dropout=0.4)
    sd = synth.make_state_dict(model_cfg)
    weight = 0.5
    cfg = AttrDict(dict(get_config()))
    cfg.model = AttrDict(model_cfg)
    cfg.solver = AttrDict(dict(cfg.solver, lr=2e-3, weight_decay=0.01))
    logs = []
    monkeypatch.setattr(tr, "wandb", types.SimpleNamespace(log=lambda d: logs.append(dict(d))))
    dl_train = torch.utils.data.DataLoader(_dataset(16, 48, 40, 1), collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    assert len(dl_train) == 2
    crit = tr.M2FCrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)

    def run(supcon, attach=True):
        cfg.runtime = AttrDict(dict(get_config().runtime, supcon=supcon))
        m = tr.build_model(cfg, device)
        m.load_state_dict({k: v.to(device) for k, v in sd.items()})
        if attach:
            object.__setattr__(m, "supcon", tr.supcon_settings(cfg))
        del logs[:]
        mean = tr.train(m, dl_train, crit, tr.build_optimizer(cfg, m), 0, True, device)
        return m, mean, [dict(d) for d in logs]

    m_on, mean_on, on = run({"enabled": True, "weight": weight, "temperature": 0.1, "warmup_steps": 0})
    assert m_on.supcon == {"weight": weight, "temperature": 0.1, "warmup_steps": 0} and len(on) == 2
    for d in on:
        full = d["Train/CE"] + weight * d["Train/SupCon"]
        print(f"Train/Running_loss {d['Train/Running_loss']!r} = CE {d['Train/CE']!r} + {weight} * SupCon {d['Train/SupCon']!r} = {full!r}")
        assert d["Train/SupCon"] > 0.0 and abs(full - d["Train/Running_loss"]) <= 2e-6 * abs(d["Train/Running_loss"])
    assert abs(mean_on - on[-1]["Train/Running_loss"]) <= 1e-12
    # the key off (the shipped default), absent, and a model main() never touched: the loop as it was
    m_off, mean_off, off = run({"enabled": False, "weight": weight, "temperature": 0.1, "warmup_steps": 0})
    m_none, mean_none, none = run(None, attach=False)
    assert m_off.supcon is None and not hasattr(m_none, "supcon")
    assert mean_off == mean_none and off == none and all("Train/CE" not in d and "Train/SupCon" not in d for d in off)
    for p, q in zip(m_off.parameters(), m_none.parameters()):
        assert torch.equal(p, q)
    assert mean_on != mean_off
