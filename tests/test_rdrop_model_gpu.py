"""R-Drop inside the train step (M2FNet.train_step(rdrop=alpha)): with dropout 0 the step against the autograd path (forward on the
doubled batch, M2FRDropLoss, backward) on every plan kind; with dropout 0.4 the two views under the device's own masks against the
float64 reference (tests/golden/rdrop_ref.py) on the step's own logits; alpha schedules under a replayed graph; plain calls between
R-Drop calls; every training mode; speaker heads; the drop-in loop.  Every comparison prints its figures before it asserts (-s)."""
import os
import sys
import types

import numpy as np
import pandas as pd
import pytest
import torch
import torch.distributed as dist

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import rdrop_ref as ref  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import dp  # noqa: E402
from mer_amd import functional as F  # noqa: E402
from mer_amd import runtime  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam, M2FRDropLoss  # noqa: E402

DEV = "cuda"
CFG = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2, ncls=7)          # dropout 0 (tests/test_distill_gpu.py's)
CFG_DROP = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2, ncls=7, dropout=0.4)
C = 7
# name: B, L, seed, lengths, packed      (the bucketed batch runs inside the padded one's plan: 2 * 4 x 6 and 2 * 3 x 5 -> 8 x 16)
PLAN_KINDS = {"padded_4x6": (4, 6, 1, [6, 6, 5, 6], None), "bucketed_3x5": (3, 5, 4, [5, 2, 4], None),
              "packed_5x9": (5, 9, 2, [9, 1, 5, 3, 2], True), "long_2x70": (2, 70, 3, [70, 5], None)}


def _model(precision="fp32", packed=None, cfg=CFG, **kw):
    m = M2FNet(cfg, precision=precision, packed=packed, **kw)
    m.load_state_dict(synth.make_state_dict(cfg))
    return m.to(DEV).train()


def _batch(B, L, seed, lengths=None, cfg=CFG):
    if lengths is None:
        g = torch.Generator().manual_seed(seed)
        lengths = [L] + [int(x) for x in torch.randint(1, L + 1, (B - 1,), generator=g)]
    return [t.to(DEV) for t in synth.make_inputs(cfg, B, L, lengths, "randn", seed=seed)]


def _twice(*xs):
    return [torch.cat([x, x], 0) for x in xs]


def _last_plan(m):
    return m.engine().plans[next(reversed(m.engine().plans))]


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _equal_grads(ma, mb, what):
    for (k, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(p.grad, q.grad), (what, k, (p.grad - q.grad).abs().max().item())


def _autograd_path(m, t, a, kp, em, alpha, **fw):
    """forward on the doubled batch, M2FRDropLoss on its [2B, L, C] logits, backward."""
    t2, a2, kp2, em2 = _twice(t, a, kp, em)
    crit = M2FRDropLoss(alpha=alpha, channels_last=True)
    loss = crit(m(t2, a2, kp2, **fw), em2)
    loss.backward()
    return loss.detach(), crit.last_terms


def _reference_on_the_plans_logits(plan, em, alpha, cw=None):
    """The float64 reference on the logits the step left in the plan, on the PADDED surface [2B, L, C]: the twin of (b, i) is (b + B, i),
    whatever rows the plan keeps them in.  -> (loss, den, num, kl, normalised gradient [2B, L, C])."""
    z = plan.logits.detach().clone()
    n, L, _ = z.shape
    em2 = torch.cat([em, em], 0)
    partner = runtime.rdrop_partner(n // 2, L, n * L, L=L, device=z.device)
    loss, den, num, kl, grad = ref.rdrop_loss_and_grad(z.reshape(-1, C), partner, em2.reshape(-1), cw, 0.1, alpha)
    return loss, den, num, kl, grad.reshape(n, L, C)


def _close(a, b, tol, what=""):
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item()
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, bound {tol * scale + 1e-7:.3e}")
    assert err <= tol * scale + 1e-7, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


# ---- 1. dropout 0: the step against the autograd path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(PLAN_KINDS))
def test_step_matches_the_autograd_path(kind):
    """torch.equal in the loss and in every parameter gradient.  The row terms and the (integer: no class weights) denominator are the same
    bits on both paths, and so are the gradients, whatever rows the plan keeps the batch in.  The two numerators are fp32 sums of the
    same terms in two row layouts (the plan's own token rows through the tail's reduce, the module's [2B * L] rows through the same
    reduce): equal on these four cases, not by construction."""
    B, L, seed, lengths, packed = PLAN_KINDS[kind]
    t, a, kp, em = _batch(B, L, seed, lengths)
    alpha = 0.7
    ma = _model(packed=packed)
    la = ma.train_step(t, a, kp, em, rdrop=alpha, use_graph=False)
    plan = _last_plan(ma)
    assert plan.packed == (kind in ("packed_5x9", "long_2x70")) and (plan.in_B, plan.in_L) == (2 * B, L)
    assert kind not in ("padded_4x6", "bucketed_3x5") or (plan.B, plan.L) == (8, 16)
    mb = _model(packed=packed)
    lb, terms = _autograd_path(mb, t, a, kp, em, alpha)
    gerr = max((p.grad - q.grad).abs().max().item() for p, q in zip(ma.parameters(), mb.parameters()))
    ce, kl = ma.rdrop_terms()
    print(f"{kind} (plan {plan.B} x {plan.L}, T {plan.T}, packed {plan.packed}): step loss {la.item()!r}, autograd loss {lb.item()!r}; "
          f"largest parameter-gradient difference {gerr:.3e}; ce {ce.item()!r} kl {kl.item()!r}")
    assert torch.equal(la, lb)
    _equal_grads(ma, mb, kind)
    # dropout 0: the twins agree, the term vanishes exactly - the loss is the cross entropy of the batch, and the plain step's gradients
    assert kl.item() == 0.0 and terms[3].item() == 0.0
    mc = _model(packed=packed)
    lc = mc.train_step(t, a, kp, em, use_graph=False)
    assert abs(la.item() - lc.item()) <= 1e-5
    for (k, p), (_, q) in zip(ma.named_parameters(), mc.named_parameters()):
        bound = 1e-6 + 1e-4 * q.grad.abs().max().item()
        assert (p.grad - q.grad).abs().max().item() <= bound, k


# ---- 2. dropout 0.4: two views under the device's own masks ---------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", list(PLAN_KINDS))
def test_two_views_under_dropout_follow_the_reference(kind, weighted):
    B, L, seed, lengths, packed = PLAN_KINDS[kind]
    t, a, kp, em = _batch(B, L, seed, lengths, cfg=CFG_DROP)
    cw = (0.3 + torch.arange(C, device=DEV) * 0.7) if weighted else None
    alpha = 1.5
    m = _model(packed=packed, cfg=CFG_DROP)
    loss = m.train_step(t, a, kp, em, class_weights=cw, rdrop=alpha, use_graph=False)
    plan = _last_plan(m)
    assert plan.packed == (kind in ("packed_5x9", "long_2x70"))
    z = plan.logits
    v = em >= 0
    differ = (z[:B][v] != z[B:][v]).any(-1)
    assert bool(differ.all()), "the two views of every labelled utterance run under different masks"
    loss_r, den_r, num_r, kl_r, grad_r = _reference_on_the_plans_logits(plan, em, alpha, cw)
    tail = m.loss_terms()
    ce, kl = m.rdrop_terms()
    err, bound = abs(loss.item() - loss_r.item()), 2e-6 * max(1.0, abs(loss_r.item()))
    print(f"{kind} weighted {weighted}: loss {loss.item()!r} ref {loss_r.item()!r} err {err:.3e} bound {bound:.3e}; den {tail[1].item()!r} "
          f"ref {den_r.item()!r}; kl {kl.item()!r} ref {(kl_r / den_r).item()!r}; ce {ce.item()!r}")
    assert kl.item() > 0.0
    assert err <= bound and torch.equal(loss, tail[0])
    assert abs(tail[1].item() - den_r.item()) <= 1e-6 * den_r.item()
    assert abs(tail[2].item() - num_r.item()) <= 2e-6 * max(1.0, abs(num_r.item()))
    assert abs(kl.item() - (kl_r / den_r).item()) <= 2e-6 * max(1.0, abs((kl_r / den_r).item()))
    assert abs(ce.item() - ((num_r - alpha * kl_r) / den_r).item()) <= 4e-6 * max(1.0, abs(loss_r.item()))
    _close(plan.dlogits.double(), grad_r, 1e-5, f"{kind} M2F_BUF_DLOGITS")
    # the map the step wrote is an involution over the labelled rows that pairs rows of one label
    p = plan.partner_in.long()
    lab = plan.labels_in
    rows = (lab >= 0).nonzero().flatten()
    assert bool((p[rows] >= 0).all()) and torch.equal(p[p[rows]], rows) and torch.equal(lab[p[rows]], lab[rows])


def test_eval_mode_and_dropout_zero_are_allowed_and_cost_nothing():
    t, a, kp, em = _batch(4, 6, 1, [6, 6, 5, 6], cfg=CFG_DROP)
    m = _model(cfg=CFG_DROP).eval()
    loss = m.train_step(t, a, kp, em, rdrop=3.0, use_graph=False)
    ce, kl = m.rdrop_terms()
    assert kl.item() == 0.0 and torch.isfinite(loss) and abs(ce.item() - loss.item()) <= 1e-6


# ---- 3. graphs --------------------------------------------------------------------------------------------------------------------------------
def test_alpha_schedule_replays_the_captured_step():
    t, a, kp, em = _batch(4, 6, 1, [6, 6, 5, 6], cfg=CFG_DROP)
    mg = _model(cfg=CFG_DROP)
    for _ in range(3):                                     # eager warm-up, capture, replay
        mg.train_step(t, a, kp, em, rdrop=0.5, use_graph=True)
    plan = _last_plan(mg)
    n_plans, handle, ws = len(mg.engine().plans), plan.handle, plan.workspace.data_ptr()
    seen = []
    for alpha in (0.5, 2.0, 0.0, 2.0):                     # consecutive steps at different alphas: the kernel reads alpha on the device
        loss = mg.train_step(t, a, kp, em, rdrop=alpha, use_graph=True)
        loss_r, den_r, _, kl_r, grad_r = _reference_on_the_plans_logits(plan, em, alpha)
        err, bound = abs(loss.item() - loss_r.item()), 2e-6 * max(1.0, abs(loss_r.item()))
        print(f"alpha {alpha}: replayed loss {loss.item()!r}, reference {loss_r.item()!r} err {err:.3e} bound {bound:.3e}")
        assert err <= bound
        _close(plan.dlogits.double(), grad_r, 1e-5, f"alpha {alpha} dlogits")
        assert plan.alpha_host == alpha and float(plan.rdrop_alpha[0]) == alpha
        seen.append((kl_r / den_r).item())
    assert min(seen) > 0.0
    assert _last_plan(mg) is plan and (len(mg.engine().plans), plan.handle, plan.workspace.data_ptr()) == (n_plans, handle, ws)
    # dropout 0: replay and eager agree bit for bit at each alpha
    t, a, kp, em = _batch(4, 6, 1, [6, 6, 5, 6])
    mg = _model()
    for alpha in (0.5, 0.5, 0.5, 2.0):
        lg = mg.train_step(t, a, kp, em, rdrop=alpha, use_graph=True)
    me = _model()
    le = me.train_step(t, a, kp, em, rdrop=2.0, use_graph=False)
    assert torch.equal(lg, le)
    _equal_grads(mg, me, "replay vs eager")


# ---- 4. plain calls between R-Drop calls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_plain_calls_between_rdrop_calls_are_the_model_that_never_saw_it(use_graph):
    t, a, kp, em = _batch(4, 6, 1, [6, 6, 5, 6])
    t2, a2, kp2, em2 = _twice(t, a, kp, em)                # (the doubled batch as a PLAIN batch shares the R-Drop step's plan)
    m, fresh = _model(), _model()
    for i in range(3):
        lr = m.train_step(t, a, kp, em, rdrop=1.0, use_graph=use_graph)
        for batch in ((t, a, kp, em), (t2, a2, kp2, em2)):
            got = m.train_step(*batch, use_graph=use_graph)
            want = fresh.train_step(*batch, use_graph=use_graph)
            assert torch.equal(got, want), (i, got.item(), want.item())
            assert torch.equal(_last_plan(m).logits, _last_plan(fresh).logits)
            _equal_grads(m, fresh, "plain after R-Drop")
    assert torch.equal(m.train_step(t, a, kp, em, rdrop=1.0, use_graph=use_graph), lr)


# ---- 5. every training mode --------------------------------------------------------------------------------------------------------------------
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


def _standalone(plan, alpha, normalise):
    """The stand-alone kernel on the plan's own token rows and its own twin map: (loss_out, dlogits [T, C])."""
    return F.cross_entropy_rdrop(plan._logits.reshape(-1, C).clone(), plan.partner_in.clone(), plan.labels_in.clone(), None, 0.1, alpha,
                                 normalise)


def _split_check(m, alpha, outs):
    """rdrop_terms() against the stand-alone kernel's tails `outs` (one per micro-batch): ce + alpha * kl = num / den."""
    den, num, klsum = sum(o[1] for o in outs), sum(o[2] for o in outs), sum(o[3] for o in outs)
    ce, kl = m.rdrop_terms()
    print(f"rdrop_terms: ce {ce.item()!r} kl {kl.item()!r}; stand-alone den {den.item()!r} num {num.item()!r} kl sum {klsum.item()!r}")
    assert klsum.item() > 0.0 and torch.equal(kl, klsum / den)
    assert abs((ce + alpha * kl).item() - (num / den).item()) <= 2e-6 * max(1.0, abs((num / den).item()))


def test_accumulation_over_two_micro_batches():
    """tests/test_grad_accumulation_gpu.py's global-denominator bounds (loss 1e-5, gradients 5e-6 of the largest element of their tensor):
    two R-Drop micro-batches of 3 dialogues are the R-Drop step on the 6 (dropout 0: the comparison is deterministic)."""
    big = _batch(6, 12, 9)
    mbs = [[x[i * 3:(i + 1) * 3] for x in big] for i in range(2)]
    alpha = 0.8
    m_big, m_acc = _model(), _model()
    m_acc.set_grad_accumulation(True)
    loss_big = m_big.train_step(*big, rdrop=alpha, use_graph=False)
    m_acc.zero_grad(set_to_none=True)
    for mb in mbs:
        m_acc.train_step(*mb, normalise=False, rdrop=alpha, use_graph=False)
    den, num = m_acc.loss_terms()[1], m_acc.loss_terms()[2]
    worst = 0.0
    for (k, p), (_, q) in zip(m_acc.named_parameters(), m_big.named_parameters()):
        worst = max(worst, ((p.grad / den) - q.grad).abs().max().item() / max(q.grad.abs().max().item(), 1e-12))
    print(f"group loss {(num / den).item()!r}, big batch {loss_big.item()!r}; gradient error (of the largest element) {worst:.3e}")
    assert abs((num / den).item() - loss_big.item()) < 1e-5 and worst < 5e-6
    assert torch.equal(den, m_big.loss_terms()[1])
    # under dropout the group's tail holds both micro-batches' shares
    m = _model(cfg=CFG_DROP)
    m.set_grad_accumulation(True)
    m.zero_grad(set_to_none=True)
    outs = []
    for i, mb in enumerate(mbs):
        m.train_step(*mb, normalise=False, rdrop=alpha, use_graph=False)
        out, dl = _standalone(_last_plan(m), alpha, False)
        assert torch.equal(_last_plan(m)._dlogits.reshape(dl.shape), dl)
        outs.append(out)
    tail = m.loss_terms()
    assert torch.equal(tail[1], outs[0][1] + outs[1][1]) and torch.equal(tail[2], outs[0][2] + outs[1][2])
    _split_check(m, alpha, outs)


@pytest.mark.parametrize("mode", ["bf16", "grad_bf16", "optimizer", "clip"])
def test_bf16_clipping_and_the_optimizer_inside_the_step(mode):
    """As the distillation and focal tests of these modes: the plan's dlogits and tail are the stand-alone kernel's on the plan's own logits
    and twin map, bit for bit; alpha = 0 on the doubled batch gives the mode's own bits for that batch; and the loss is the fp32
    model's within bf16 mode's 2e-3 (tests/test_dp_gpu.py).  optimizer / clip: step + optimizer.step(), bit for bit."""
    t, a, kp, em = _batch(4, 6, 1, [6, 6, 5, 6], cfg=CFG_DROP)
    alpha = 1.2
    precision = "fp32" if mode == "clip" else "bf16"

    def run(batch, **kw):
        m = _model(precision, cfg=CFG_DROP)
        opt = None
        if mode == "grad_bf16":
            assert m.set_grad_bf16(True)
        if mode in ("optimizer", "clip"):
            opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, max_grad_norm=1e-3 if mode == "clip" else None)
            kw = dict(kw, optimizer=opt)
        loss = m.train_step(*batch, use_graph=False, **kw)
        if mode == "grad_bf16":
            res = m.engine().grad_bf16_buf.clone()
        elif opt is not None:
            res = torch.cat([p.detach().flatten() for p in m.parameters()])
        else:
            res = torch.cat([g.flatten() for g in _grads(m).values()])
        return m, loss, res, opt

    _, l_plain, r_plain, _ = run(_twice(t, a, kp, em))
    _, l_zero, r_zero, _ = run((t, a, kp, em), rdrop=0.0)
    assert torch.equal(l_plain, l_zero) and torch.equal(r_plain, r_zero)
    m, loss, res, opt = run((t, a, kp, em), rdrop=alpha)
    plan = _last_plan(m)
    out, dl = _standalone(plan, alpha, True)
    assert torch.equal(plan._dlogits.reshape(dl.shape), dl) and torch.equal(m.loss_terms()[:3], out[:3]) and torch.equal(loss, out[0])
    _split_check(m, alpha, [out])
    assert torch.isfinite(res.float()).all() and not torch.equal(loss, l_plain) and not torch.equal(res, r_plain)
    if mode in ("optimizer", "clip"):                       # the step with the optimizer inside = the step, then optimizer.step()
        m2 = _model(precision, cfg=CFG_DROP)
        o2 = FusedAdam(m2, lr=1e-3, weight_decay=0.01, max_grad_norm=1e-3 if mode == "clip" else None)
        l2 = m2.train_step(t, a, kp, em, rdrop=alpha, use_graph=False)
        o2.step()
        assert torch.equal(loss, l2)
        if precision == "fp32":
            for (n, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
                assert torch.equal(p, q), n
        if mode == "clip":
            assert float(opt.clip_coef()) < 1.0 and torch.equal(opt.grad_norm(), o2.grad_norm())
    else:
        l32 = _model(cfg=CFG_DROP).train_step(t, a, kp, em, rdrop=alpha, use_graph=False)
        print(f"{mode}: loss {loss.item()!r}, fp32 loss {l32.item()!r}")
        assert abs(loss.item() - l32.item()) <= 2e-3 * max(1.0, abs(l32.item()))


def test_data_parallel_step_on_one_rank(one_rank_group):
    """The rank's step is train_step(normalise=False, rdrop=) and the division by the (global = local) den inside the optimizer, bit for
    bit; the all-reduced tail gives rdrop_terms() the global shares."""
    t, a, kp, em = _batch(4, 6, 1, [6, 6, 5, 6], cfg=CFG_DROP)
    alpha = 0.9
    m = _model(cfg=CFG_DROP)
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01)
    step = dp.DataParallelStep(m, opt, n_buckets=3, exchange="fp32")
    loss = step(t, a, kp, em, rdrop=alpha, use_graph=False)
    m2 = _model(cfg=CFG_DROP)
    opt2 = FusedAdam(m2, lr=1e-3, weight_decay=0.01)
    l2 = m2.train_step(t, a, kp, em, rdrop=alpha, normalise=False, use_graph=False)
    assert torch.equal(_last_plan(m)._dlogits, _last_plan(m2)._dlogits) and torch.equal(m.loss_terms()[:3], m2.loss_terms()[:3])
    assert torch.equal(_last_plan(m).partner_in, _last_plan(m2).partner_in)
    out, _ = _standalone(_last_plan(m), alpha, False)
    _split_check(m, alpha, [out])
    opt2.grad_scale = m2.loss_terms()[1:2]
    opt2.step()
    print(f"data-parallel loss {loss.item()!r}, train_step loss {l2.item()!r}")
    assert torch.equal(loss, l2)
    for (n, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(p, q), n
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="rdrop"):
            step(t, a, kp, em, rdrop=bad)
    with pytest.raises(ValueError, match="DataParallelStep: rdrop and focal_gamma do not combine"):
        step(t, a, kp, em, rdrop=1.0, focal_gamma=2.0)


def test_c_entry_points_refuse_each_other_by_name():
    t, a, kp, em = _batch(4, 6, 1, [6, 6, 5, 6])
    m = _model()
    m.train_step(t, a, kp, em, rdrop=1.0, use_graph=False)
    plan = _last_plan(m)
    for entry, name in ((plan.distill, "m2f_plan_distill"), (plan.focal, "m2f_plan_focal")):
        with pytest.raises(Exception, match=name + ": the R-Drop criterion is on"):
            entry(True)
    from mer_amd.crf import LinearChainCRF
    crf = LinearChainCRF(C).to(DEV)
    with pytest.raises(Exception, match="m2f_plan_crf: the R-Drop criterion is on"):
        plan.set_crf(*crf.step_buffers(plan.workspace.device, want_grad=False))
    plan.rdrop(False)
    plan.focal(True)
    with pytest.raises(Exception, match="m2f_plan_rdrop: the focal criterion is on"):
        plan.rdrop(True)
    plan.focal(False)
    ev = m.engine().plan(8, 6, False, False)
    with pytest.raises(Exception, match="m2f_plan_rdrop"):
        ev.rdrop(True)                                      # eval plans keep the hard-label criterion


# ---- 6. speaker heads -----------------------------------------------------------------------------------------------------------------------------
def test_speaker_ids_are_doubled_with_the_batch():
    B, L, lengths = 4, 6, [6, 6, 5, 6]
    t, a, kp, em = _batch(B, L, 1, lengths)
    g = torch.Generator().manual_seed(5)
    spk = torch.randint(0, 3, (B, L), generator=g).to(torch.uint8).to(DEV)
    ma = _model(speaker_heads=(1, 1))
    la = ma.train_step(t, a, kp, em, speakers=spk, rdrop=0.7, use_graph=False)
    plan = _last_plan(ma)
    assert torch.equal(plan.speakers_in.view(plan.B, plan.L)[: 2 * B, :L], torch.cat([spk, spk], 0))
    mb = _model(speaker_heads=(1, 1))
    lb, _ = _autograd_path(mb, t, a, kp, em, 0.7, speakers=torch.cat([spk, spk], 0))
    # the row terms and the (integer) denominator are the same bits on both paths, so the gradients are; the two numerators are fp32 sums
    # of the same n labelled rows' terms in two orders (the plan's 8 x 16 rows, the module's 8 x 6): each within n * 2^-24 of the exact sum
    n = 2 * int((em >= 0).sum())
    bound = 2 * n * 2.0 ** -24 * abs(lb.item())
    print(f"speaker heads: step loss {la.item()!r}, autograd loss {lb.item()!r}, bound {bound:.3e}")
    assert abs(la.item() - lb.item()) <= bound
    _equal_grads(ma, mb, "speaker heads")
    other = _model(speaker_heads=(1, 1)).train_step(t, a, kp, em, speakers=(spk + 1) % 3 * (spk > 0), rdrop=0.7, use_graph=False)
    assert not torch.equal(la, other)                       # the ids matter


# ---- 7. the drop-in loop ----------------------------------------------------------------------------------------------------------------------------
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
    alpha = 1.5
    cfg = AttrDict(dict(get_config()))
    cfg.model = AttrDict(model_cfg)
    cfg.solver = AttrDict(dict(cfg.solver, lr=2e-3, weight_decay=0.01))
    logs = []
    monkeypatch.setattr(tr, "wandb", types.SimpleNamespace(log=lambda d: logs.append(dict(d))))
    dl_train = torch.utils.data.DataLoader(_dataset(16, 48, 40, 1), collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    assert len(dl_train) == 2
    crit = tr.M2FCrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)

    def run(rdrop, attach=True):
        cfg.runtime = AttrDict(dict(get_config().runtime, rdrop=rdrop))
        m = tr.build_model(cfg, device)
        m.load_state_dict({k: v.to(device) for k, v in sd.items()})
        if attach:
            object.__setattr__(m, "rdrop", tr.rdrop_settings(cfg))
        del logs[:]
        mean = tr.train(m, dl_train, crit, tr.build_optimizer(cfg, m), 0, True, device)
        return m, mean, [dict(d) for d in logs]

    m_on, mean_on, on = run({"enabled": True, "alpha": alpha, "warmup_steps": 0})
    assert m_on.rdrop == {"alpha": alpha, "warmup_steps": 0} and len(on) == 2
    for d in on:
        full = d["Train/CE"] + alpha * d["Train/RDrop_KL"]
        print(f"Train/Running_loss {d['Train/Running_loss']!r} = CE {d['Train/CE']!r} + {alpha} * KL {d['Train/RDrop_KL']!r} = {full!r}")
        assert d["Train/RDrop_KL"] > 0.0 and abs(full - d["Train/Running_loss"]) <= 1e-6 * abs(d["Train/Running_loss"])
    assert abs(mean_on - on[-1]["Train/Running_loss"]) <= 1e-12
    # the key off (the shipped default), absent, and a model main() never touched: the loop as it was
    m_off, mean_off, off = run({"enabled": False, "alpha": alpha, "warmup_steps": 0})
    m_none, mean_none, none = run(None, attach=False)
    assert m_off.rdrop is None and not hasattr(m_none, "rdrop")
    assert mean_off == mean_none and off == none and all("Train/CE" not in d and "Train/RDrop_KL" not in d for d in off)
    for p, q in zip(m_off.parameters(), m_none.parameters()):
        assert torch.equal(p, q)
    # ... which is train_step + optimizer.step() per batch, by hand
    cfg.runtime = AttrDict(dict(get_config().runtime))
    m_hand = tr.build_model(cfg, device)
    m_hand.load_state_dict({k: v.to(device) for k, v in sd.items()})
    opt = tr.build_optimizer(cfg, m_hand)
    total = 0.0
    for batch in dl_train:
        text, audio, emotion, mask = tr.move_batch(batch, device)
        opt.zero_grad()
        total += m_hand.train_step(text, audio, mask, emotion, label_smoothing=0.1, class_weights=None, use_graph=True).item()
        opt.step()
    assert total / 2 == mean_off
    for p, q in zip(m_off.parameters(), m_hand.parameters()):
        assert torch.equal(p, q)
    assert mean_on != mean_off
