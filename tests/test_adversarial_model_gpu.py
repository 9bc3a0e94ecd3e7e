"""M2FNet.adversarial_step, train_step(input_grads=) and last_input_grads / last_perturbation on the device: padded, bucketed, packed and
long-dialogue plans of a small synthetic configuration.  The composition checks are bit for bit (torch.equal) against the loop a user can
write from the public pieces; the oracle check holds the summed gradient to the bound the fp32 train-step gradient tests use (3e-5 + 1e-3
x the reference tensor's largest element: tests/test_model_gpu.py, tests/test_aux_head_model_gpu.py) and demands that K x the oracle's
CLEAN gradient misses the device result by at least 10 x that bound - the test that fails without the feature.  Figures are printed
before they are asserted (-s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
import adversarial_oracle as AO  # noqa: E402
from mer_amd import functional as F  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam  # noqa: E402

DEV = "cuda"
CFG = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2, ncls=7)          # dropout 0 (tests/test_aux_head_model_gpu.py's)
CFG_DROP = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2, ncls=7, dropout=0.4)
# name: B, L, seed, lengths, packed
PLAN_KINDS = {"padded_4x16": (4, 16, 1, [16, 16, 9, 16], None), "bucketed_3x5": (3, 5, 4, [5, 2, 4], None),
              "packed_5x9": (5, 9, 2, [9, 1, 5, 3, 2], True), "long_2x70": (2, 70, 3, [70, 5], None)}
BOTH = ("text", "audio")


def _model(precision="fp32", packed=None, cfg=CFG, **kw):
    m = M2FNet(cfg, precision=precision, packed=packed, **kw)
    m.load_state_dict(synth.make_state_dict(cfg))
    return m.to(DEV).train()


def _batch(kind, cfg=CFG):
    B, L, seed, lengths, _ = PLAN_KINDS[kind]
    return [v.to(DEV) for v in synth.make_inputs(cfg, B, L, lengths, "randn", seed=seed)]


def _last_plan(m):
    return m.engine().plans[next(reversed(m.engine().plans))]


def _flat(m):
    return m.flat_gradients().detach().clone()


def _manual(m, t, a, kp, em, eps, steps, step=None, norm="utterance", modalities=BOTH, **kw):
    """The documented loop over the public pieces; -> (loss of pass 0, {modality: delta})."""
    m.set_grad_accumulation(True)
    for p in m.parameters():
        p.grad = None
    clean = {"text": t, "audio": a}
    delta = {n: torch.zeros_like(clean[n]) for n in modalities}
    first = None
    for k in range(steps):
        if k:
            g = m.last_input_grads()
            for n in modalities:
                F.adversarial_ascend(clean[n], g[n], delta[n], None, kp, eps, step, norm)
        x = {n: clean[n] + delta[n] if n in delta else clean[n] for n in clean}
        loss = m.train_step(x["text"], x["audio"], kp, em, normalise=False, input_grads=modalities, **kw)
        first = loss if first is None else first
    m.set_grad_accumulation(False)
    return first, delta


# ---- a. the call is the documented loop, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", list(PLAN_KINDS))
def test_adversarial_step_is_the_documented_loop(kind, precision):
    t, a, kp, em = _batch(kind)
    packed = PLAN_KINDS[kind][4]
    for norm, mods in (("utterance", BOTH), ("batch", ("text",))) if kind == "padded_4x16" else (("utterance", BOTH),):
        ma, mb = _model(precision, packed), _model(precision, packed)
        la = ma.adversarial_step(t, a, kp, em, epsilon=0.75, steps=3, step_size=0.5, norm=norm, modalities=mods)
        lb, delta = _manual(mb, t, a, kp, em, 0.75, 3, 0.5, norm, mods)
        assert torch.equal(la, lb), (kind, norm, la.item(), lb.item())
        assert torch.equal(_flat(ma), _flat(mb)), (kind, norm, (_flat(ma) - _flat(mb)).abs().max().item())
        assert torch.equal(ma.loss_terms()[1:], mb.loss_terms()[1:])
        got = ma.last_perturbation()
        assert sorted(got) == sorted(mods)
        for n in mods:
            assert got[n].shape == delta[n].shape and torch.equal(got[n], delta[n]), (kind, norm, n)
            assert not got[n][kp].any() and bool(got[n][~kp].any())
            rows = got[n][~kp].double().norm(dim=-1)
            print(f"{kind} {precision} {norm} {n}: final row norms {rows.min().item():.4f} .. {rows.max().item():.4f}; den {ma.loss_terms()[1].item()}")
            if norm == "utterance":
                assert bool((rows <= 0.75 * (1 + 1e-6)).all())
        pl = _last_plan(ma)
        assert pl.input_mask == sum({"text": 1, "audio": 2}[n] for n in mods) and pl.param_grads and not pl._acc
        assert ma.loss_terms()[1].item() == 3 * float((em != -1).sum())


# ---- b. fp32 against the oracle's float64 autograd; K x the clean gradient must miss ------------------------------------------------------
@pytest.mark.parametrize("kind", ["padded_4x16", "bucketed_3x5", "packed_5x9"])
def test_summed_gradient_matches_the_oracle_and_the_clean_gradient_misses(kind):
    t, a, kp, em = _batch(kind)
    K = 3
    cpu = [v.cpu() for v in (t, a, kp, em)]
    # epsilon: chosen on the CPU with the oracle alone - the smallest of the list at which K x the clean gradient lies at least 20 x
    # the bound from the adversarial sum (twice what the assertion below demands)
    chosen = None
    for eps in (1.0, 3.0, 9.0):
        o = AO.adversarial_grads(CFG, *cpu, eps, K)
        factor = max((K * o["clean"][k] - o["grads"][k]).abs().max().item() / (3e-5 + 1e-3 * o["grads"][k].abs().max().item()) for k in o["grads"])
        print(f"{kind}: epsilon {eps}: K x clean lies at {factor:.1f} x the bound from the oracle's adversarial sum")
        if factor >= 20:
            chosen = (eps, o)
            break
    assert chosen is not None, kind
    eps, o = chosen
    m = _model("fp32", PLAN_KINDS[kind][4])
    loss = m.adversarial_step(t, a, kp, em, epsilon=eps, steps=K)
    assert abs(loss.item() - (o["num"][0] / o["den"]).item()) <= 2e-5
    assert abs(m.loss_terms()[2].item() - sum(o["num"]).item()) <= 1e-4 * sum(o["num"]).item()
    worst, worst_clean = 0.0, 0.0
    for k, p in m.named_parameters():
        want = o["grads"][k]
        bound = 3e-5 + 1e-3 * want.abs().max().item()
        err = (p.grad.detach().cpu().double() - want).abs().max().item()
        miss = (p.grad.detach().cpu().double() - K * o["clean"][k]).abs().max().item()
        worst, worst_clean = max(worst, err / bound), max(worst_clean, miss / bound)
        assert err <= bound, (kind, k, err, bound)
    d_err = max((m.last_perturbation()[n].cpu().double() - o["delta"][n]).abs().max().item() for n in BOTH)
    print(f"{kind}: epsilon {eps}: worst gradient error / bound {worst:.3f}; K x the oracle's clean gradient misses the device result by "
          f"{worst_clean:.1f} x the bound; final delta against the oracle's {d_err:.3e}")
    assert worst_clean >= 10.0, (kind, worst_clean)
    assert d_err <= 1e-3 * eps


# ---- c. one pass is the plain un-normalised step ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["padded_4x16", "packed_5x9"])
def test_one_pass_is_the_plain_step(kind):
    t, a, kp, em = _batch(kind, CFG_DROP)
    packed = PLAN_KINDS[kind][4]
    torch.manual_seed(5)
    ma = _model("fp32", packed, CFG_DROP)
    torch.manual_seed(5)
    mb = _model("fp32", packed, CFG_DROP)
    la = ma.train_step(t, a, kp, em, normalise=False)
    lb = mb.adversarial_step(t, a, kp, em, epsilon=1.0, steps=1)
    assert torch.equal(la, lb) and torch.equal(_flat(ma), _flat(mb)) and torch.equal(ma.loss_terms(), mb.loss_terms())
    assert torch.equal(ma.engine().rng, mb.engine().rng)
    assert not any(v.any() for v in mb.last_perturbation().values())


# ---- d. dropout: the masks of pass 0 in every pass, or fresh ones; the state one step leaves --------------------------------------------------
def test_same_dropout_repeats_the_masks_and_leaves_one_steps_state():
    t, a, kp, em = _batch("padded_4x16", CFG_DROP)
    models = []
    for _ in range(3):
        torch.manual_seed(9)
        models.append(_model("fp32", None, CFG_DROP))
    m1, ms, mf = models
    m1.train_step(t, a, kp, em, normalise=False)
    ms.adversarial_step(t, a, kp, em, epsilon=0.0, steps=2, same_dropout=True)
    mf.adversarial_step(t, a, kp, em, epsilon=0.0, steps=2, same_dropout=False)
    assert torch.equal(_flat(ms), 2 * _flat(m1))                                    # g + g is exact in fp32
    assert not torch.equal(_flat(mf), 2 * _flat(m1))                                # the second pass drew its own masks
    assert torch.equal(ms.engine().rng, m1.engine().rng) and torch.equal(mf.engine().rng, m1.engine().rng)
    assert torch.equal(ms.loss_terms()[1:], 2 * m1.loss_terms()[1:])


# ---- e. the default step is untouched -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_default_step_is_what_it_was(precision):
    t, a, kp, em = _batch("padded_4x16", CFG_DROP)
    torch.manual_seed(3)
    used = _model(precision, None, CFG_DROP)
    torch.manual_seed(3)
    fresh = _model(precision, None, CFG_DROP)
    l0, f0 = used.train_step(t, a, kp, em), fresh.train_step(t, a, kp, em)
    assert torch.equal(l0, f0) and torch.equal(_flat(used), _flat(fresh))
    eng = used.engine()
    key = eng.plan_key(4, 16, None, True, True, eng.precision) + (0,)
    assert key in eng.plans and len(eng.plans) == 1
    used.adversarial_step(t, a, kp, em, epsilon=0.5, steps=2)
    fresh.train_step(t, a, kp, em)                          # (the dropout state moves as one step moves it)
    assert len(eng.plans) == 2 and key in eng.plans
    l1, f1 = used.train_step(t, a, kp, em), fresh.train_step(t, a, kp, em)
    assert torch.equal(l1, f1) and torch.equal(_flat(used), _flat(fresh)) and torch.equal(used.loss_terms(), fresh.loss_terms())
    assert eng.plans[key].num_launches() == fresh.engine().plans[key].num_launches()
    assert eng.plans[key].adv_mask == 0 and eng.plans[key]._adv_state is None
    assert eng.plans[key].nbytes() == fresh.engine().plans[key].nbytes()


# ---- f. last_input_grads against the autograd surface ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(PLAN_KINDS))
def test_last_input_grads_against_autograd(kind):
    t, a, kp, em = _batch(kind)
    packed = PLAN_KINDS[kind][4]
    m = _model("fp32", packed)
    loss = m.train_step(t, a, kp, em, input_grads=BOTH)
    got = m.last_input_grads()
    params = _flat(m)
    plain = _model("fp32", packed)
    assert torch.equal(plain.train_step(t, a, kp, em), loss) and torch.equal(_flat(plain), params)   # the parameter gradients keep their bits
    ta, aa = t.clone().requires_grad_(True), a.clone().requires_grad_(True)
    ref_m = _model("fp32", packed)
    logits = ref_m(ta, aa, kp)
    torch.nn.functional.cross_entropy(logits.permute(0, 2, 1), em, ignore_index=-1, label_smoothing=0.1).backward()
    for n, want in (("text", ta.grad), ("audio", aa.grad)):
        assert got[n].shape == want.shape and not got[n][kp].any()
        err = (got[n] - want)[~kp].abs().max().item()
        bound = 3e-5 + 1e-3 * want[~kp].abs().max().item()
        print(f"{kind}: d loss / d {n}: against the autograd surface {err:.3e}, bound {bound:.3e} (largest element {want[~kp].abs().max().item():.3e})")
        assert err <= bound and bool(got[n][~kp].any())
    only = m.train_step(t, a, kp, em, input_grads="audio")
    assert torch.equal(only, loss) and sorted(m.last_input_grads()) == ["audio"] and torch.equal(m.last_input_grads()["audio"], got["audio"])
    # un-normalised: den x the normalised gradient, to rounding
    m.train_step(t, a, kp, em, input_grads=BOTH, normalise=False)
    den = m.loss_terms()[1].item()
    un = m.last_input_grads()["text"]
    assert (un - den * got["text"]).abs().max().item() <= 1e-5 * un.abs().max().item()


# ---- g. graphs: replay equals eager, a schedule of epsilon replays ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graph_replay_and_epsilon_schedule(precision):
    t, a, kp, em = _batch("packed_5x9")
    mg = _model(precision, True)
    for _ in range(2):                                      # (after the second call on a shape every pass replays)
        mg.adversarial_step(t, a, kp, em, epsilon=0.5, steps=3, use_graph=True)
    plan = _last_plan(mg)
    n_plans, handle, ws, state = len(mg.engine().plans), plan.handle, plan.workspace.data_ptr(), plan._adv_state.data_ptr()
    for eps in (0.5, 0.25, 1.0, 0.5):
        lg = mg.adversarial_step(t, a, kp, em, epsilon=eps, steps=3, use_graph=True)
        me = _model(precision, True)
        le = me.adversarial_step(t, a, kp, em, epsilon=eps, steps=3, use_graph=False)
        print(f"{precision}: epsilon {eps}: replayed loss {lg.item()!r}, eager loss {le.item()!r}")
        assert torch.equal(lg, le) and torch.equal(_flat(mg), _flat(me)) and torch.equal(mg.loss_terms(), me.loss_terms())
        for n in BOTH:
            assert torch.equal(mg.last_perturbation()[n], me.last_perturbation()[n])
        assert plan.uploaded["adv_hyper"] == (eps, eps) and plan.adv_hyper.tolist() == [eps, eps]
        assert _last_plan(mg) is plan
        assert (len(mg.engine().plans), plan.handle, plan.workspace.data_ptr(), plan._adv_state.data_ptr()) == (n_plans, handle, ws, state)


# ---- h. with the optimizer: the manual loop followed by grad_scale = den; step() --------------------------------------------------------------
def test_optimizer_step_inside_the_call():
    t, a, kp, em = _batch("bucketed_3x5")
    ma, mb = _model("bf16"), _model("bf16")
    oa = FusedAdam(ma, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    ob = FusedAdam(mb, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    held = torch.full((1,), 1.0, device=DEV)
    oa.grad_scale = held
    for _ in range(2):
        ma.adversarial_step(t, a, kp, em, oa, epsilon=0.5, steps=2)
        assert oa.grad_scale is held
        _manual(mb, t, a, kp, em, 0.5, 2)
        ob.grad_scale = mb.loss_terms()[1:2]
        ob.step()
        assert torch.equal(ma.flat_parameters(), mb.flat_parameters())
    assert not torch.equal(ma.flat_parameters().cpu(), _model("bf16").flat_parameters().cpu())
