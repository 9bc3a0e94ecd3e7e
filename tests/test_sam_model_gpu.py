"""Sharpness-aware minimisation through the model (FusedAdam(sam_rho=), first_step / step / restore, M2FNet.sam_step) on the four
plan kinds of tests/test_aux_head_model_gpu.py: the second pass's gradient against the float64 reference (tests/sam_ref.py: the oracle
at w + e) where the oracle's PLAIN gradient must miss by >= 20 bounds; bf16 mode against the bf16-emulating oracle at w + e; the restore
to the bit (a twin optimizer fed the same second gradient); graphs; dropout; the training modes; a three-step trajectory;
sam_rho=None; every refusal and state error.  Dropout 0 unless said.  Every comparison prints its figures before it asserts (-s)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))
sys.path.insert(0, ROOT)

import bf16_emulation as E  # noqa: E402
import focal_ref  # noqa: E402
import sam_ref as ref  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import dp  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam, FusedAdamW  # noqa: E402
from oracle import m2fnet_oracle as O  # noqa: E402

DEV = "cuda"
CFG = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2, ncls=7)          # dropout 0 (tests/test_aux_head_model_gpu.py's)
CFG_DROP = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2, ncls=7, dropout=0.4)
PLAN_KINDS = {"padded_4x6": (4, 6, 1, [6, 6, 5, 6], None), "bucketed_3x5": (3, 5, 4, [5, 2, 4], None),
              "packed_5x9": (5, 9, 2, [9, 1, 5, 3, 2], True), "long_2x70": (2, 70, 3, [70, 5], None)}
RHO = 0.5                                                       # (tests/test_sam_cpu.py: every kind's plain gradient misses by >= 260 bounds)
EPS32 = torch.finfo(torch.float32).eps
LAST = [k for k in synth.make_state_dict(CFG) if k.startswith("output_layer.") and k.endswith(".weight")][-1]


def _threads():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))


def _model(precision="fp32", packed=None, cfg=CFG, sd=None):
    m = M2FNet(cfg, precision=precision, packed=packed)
    m.load_state_dict(synth.make_state_dict(cfg) if sd is None else sd)
    return m.to(DEV).train()


def _batch(kind, cfg=CFG):
    B, L, seed, lengths, packed = PLAN_KINDS[kind]
    cpu = synth.make_inputs(cfg, B, L, lengths, "randn", seed=seed)
    return cpu, [v.to(DEV) for v in cpu], packed


def _as64(cpu):
    t, a, kp, em = cpu
    return t.double(), a.double(), kp, em


_REF = {}


def _reference(kind):
    """tests/sam_ref.py on the kind's batch at RHO, once per kind (float64 CPU time) and never changed."""
    if kind not in _REF:
        _threads()
        _REF[kind] = ref.sam_gradient(ref.as_float64(synth.make_state_dict(CFG)), CFG, _as64(_batch(kind)[0]), RHO)
    return _REF[kind]


def _last_plan(m):
    return m.engine().plans[next(reversed(m.engine().plans))]


def _check_grads(label, m, want, scale=1.0):
    """Every flat-buffer gradient (times `scale`) within 3e-5 + 1e-3 x the largest element of the reference's tensor."""
    worst, at = 0.0, None
    for k, p in m.named_parameters():
        bound = 3e-5 + 1e-3 * want[k].abs().max().item()
        err = (p.grad.detach().cpu().double() * scale - want[k]).abs().max().item()
        if err / bound > worst:
            worst, at = err / bound, k
    print(f"{label}: worst gradient error / bound {worst:.3f} ({at})")
    assert worst <= 1.0, (label, at, worst)
    return worst


# ---- 1. against the oracle, fp32 mode -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(PLAN_KINDS))
def test_second_pass_gradient_is_the_oracles_at_w_plus_e(kind):
    """train_step; first_step; train_step: every flat-buffer gradient within 3e-5 + 1e-3 x max of the reference's SAM gradient, while the
    oracle's PLAIN gradient misses that bound on the last classifier weight by >= 20 x - a step that skipped the perturbation fails."""
    cpu, dev, packed = _batch(kind)
    r = _reference(kind)
    m = _model(packed=packed)
    opt = FusedAdam(m, lr=1e-3, sam_rho=RHO)
    before = m.engine().flat.clone()
    l1 = m.train_step(*dev, use_graph=False)
    g1 = {k: p.grad.detach().cpu().double() for k, p in m.named_parameters()}
    opt.first_step()
    assert opt.sam_pending
    l2 = m.train_step(*dev, use_graph=False)
    moved = (m.engine().flat - before).double().norm().item()
    norm = float(opt.sam_norm())
    bound = 3e-5 + 1e-3 * r["sam"][LAST].abs().max().item()
    factor = (r["plain"][LAST] - r["sam"][LAST]).abs().max().item() / bound
    own = (g1[LAST] - r["sam"][LAST]).abs().max().item() / bound
    print(f"{kind}: loss {l1.item()!r} (float64 {float(r['loss'])!r}) -> {l2.item()!r} at w + e (float64 {float(r['loss_at'])!r}); ||g|| {norm!r} "
          f"(float64 {r['norm']!r}); ||w' - w|| {moved!r}; the oracle's plain gradient misses on {LAST} by {factor:.0f} x the bound, the "
          f"step's own first gradient by {own:.0f} x")
    assert abs(l1.item() - float(r["loss"])) <= 2e-5 and abs(l2.item() - float(r["loss_at"])) <= 2e-5
    assert abs(norm - r["norm"]) <= 1e-3 * r["norm"] and abs(moved - RHO) <= 1e-4 * RHO
    _check_grads(kind, m, r["sam"])
    assert factor >= 20.0 and own >= 20.0
    assert opt.restore() is True and not opt.sam_pending and torch.equal(m.engine().flat, before)


# ---- 2. bf16 mode ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,backward", [("tiny_audio_only", True), ("tiny_text_only", False)])
def test_bf16_mode_matches_the_emulation_at_w_plus_e(name, backward):
    """tests/test_bf16_emulation_gpu.py's rule (max |plan - emulation| <= TOL x max |emulation| per tensor, logits and loss included), the
    emulation run at ITS OWN w + e (e from its own first gradient, w + e rounded to fp32 as the master copy holds it).
    engine.shadows_fresh() stays true: the second pass reads the shadows the perturbation wrote, and the emulation at w misses by far.

    Which cases.  That file holds its rule only on cases a GPU run showed free of rounding flips, and says why: a value within fp32 noise
    of a bf16 midpoint rounds one way in the kernels and the other way in float64.  Whether a case is free of them is a property of the
    weights, so it has to be found again at w + e.  Measured on MI355X at rho = 0.5: tiny_audio_only meets the rule on all 34 tensors
    (worst 3.7e-7).  tiny_text_only meets it in the forward (logits 9.0e-8, loss 2.1e-8: every bf16 weight the second pass read is the
    emulation's, 0 of them round differently) but its backward departs on text_encoders.0.layers.0.linear1.weight by 3.5e-3.  That is a
    flip of the existing backward at that point, not of the perturbation: the emulation fed the DEVICE's own w' departs by the same
    3.5e-3 on the same tensors, and the emulation against itself under one fp32 ulp of noise (Bf16Rounding(jitter=2^-24), four seeds, CPU)
    moves that very tensor by 2.8e-3 .. 3.8e-3.  So tiny_text_only is held to the forward (backward=False; its gradient figure is
    printed), tiny_audio_only to everything."""
    cfg, B, L, lengths, kind = synth.CASES[name]
    sd = synth.make_state_dict(cfg)
    cpu = synth.make_inputs(cfg, B, L, lengths, kind)
    _threads()
    r = ref.sam_gradient(sd, cfg, cpu, RHO, rounding=O.Bf16Rounding(), to_fp32=True)
    m = _model("bf16", cfg=cfg, sd=sd)
    opt = FusedAdam(m, lr=1e-3, sam_rho=RHO)
    dev = [v.to(DEV) for v in cpu]
    m.train_step(*dev, use_graph=False)
    opt.first_step()
    eng = m.engine()
    assert eng.wshadow is not None and eng.shadows_fresh()
    loss = m.train_step(*dev, use_graph=False)
    assert eng.shadows_fresh()
    plan = _last_plan(m)
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    valid = ~cpu[2]
    errs = E.errors(plan.logits.cpu(), loss.item(), grads, (r["logits_at"], r["loss_at"], r["sam"]), valid)
    w, k = E.worst(errs)
    _, loss_w, plain = ref.loss_and_grads(sd, cfg, cpu, rounding=O.Bf16Rounding())
    errs_plain = E.errors(plan.logits.cpu(), loss.item(), grads, (r["logits_at"], loss_w, plain), valid)
    wp, kp_ = E.worst({n: v for n, v in errs_plain.items() if n != "logits"})
    differ = sum(int((p.detach().cpu().bfloat16() != r["at"][n].bfloat16()).sum()) for n, p in m.named_parameters() if p.dim() == 2)
    print(f"{name}: worst against the emulation at w + e {w:.3e} ({k}) over {len(errs)} tensors, logits {errs['logits']:.3e}, loss {errs['loss']:.3e}; "
          f"{differ} bf16 weights round differently; against the emulation at w {wp:.3e} ({kp_}); TOL {E.TOL}")
    assert len(errs) >= 4 and errs["logits"] <= E.TOL and errs["loss"] <= E.TOL and differ == 0
    assert not backward or w <= E.TOL, (k, w)
    assert wp >= 20 * E.TOL


# ---- 3. exactness of the restore ---------------------------------------------------------------------------------------------------------------
def _optimizers(ms, mt, grouped, **kw):
    if not grouped:
        return FusedAdam(ms, sam_rho=RHO, **kw), FusedAdam(mt, **kw)

    def groups(m):                                                # AdamW groups that cover everything
        head = [p for n, p in m.named_parameters() if n.startswith("output_layer.")]
        rest = [p for n, p in m.named_parameters() if not n.startswith("output_layer.")]
        return [{"params": head, "lr": 2e-2, "weight_decay": 0.0}, {"params": rest}]

    return FusedAdamW(ms, params=groups(ms), sam_rho=RHO, **kw), FusedAdamW(mt, params=groups(mt), **kw)


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_restore_is_exact_a_twin_stepping_on_the_same_gradient_agrees_bit_for_bit(precision, grouped):
    cpu, dev, _ = _batch("padded_4x6")
    ms, mt = _model(precision), _model(precision)
    os_, ot = _optimizers(ms, mt, grouped, lr=1e-2, weight_decay=0.01, ema_decay=0.9)
    for step in range(2):
        ms.sam_step(*dev, os_, use_graph=False)
        mt.train_step(*dev, use_graph=False)                      # (the twin's engine, gradient buffer and .grad views; its values are replaced)
        mt.flat_gradients().copy_(ms.flat_gradients())
        ot.step()
        torch.cuda.synchronize()
        es, et = ms.engine(), mt.engine()
        what = f"{precision} grouped {grouped} step {step}"
        assert torch.equal(es.flat, et.flat), what
        assert torch.equal(os_._m, ot._m) and torch.equal(os_._v, ot._v), what
        assert torch.equal(os_.ema_parameters(), ot.ema_parameters()) and os_.n_averaged == ot.n_averaged == step + 1, what
        if precision == "bf16":
            assert es.shadows_fresh() and et.shadows_fresh() and torch.equal(es.wshadow, et.wshadow), what
        assert not os_.sam_pending
    moved = (ms.engine().flat - _model(precision).engine().flat).abs().max().item()
    print(f"{precision} grouped {grouped}: parameters, moments, shadows and the EMA equal the twin's after two steps (largest move {moved:.3e})")
    assert moved > 1e-3


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_step_that_moves_nothing_leaves_every_bit(precision):
    _, dev, _ = _batch("packed_5x9")
    m = _model(precision, packed=True)
    opt = FusedAdam(m, lr=0.0, weight_decay=0.0, sam_rho=RHO)
    before = m.engine().flat.clone()
    m.sam_step(*dev, opt, use_graph=False)
    torch.cuda.synchronize()
    assert torch.equal(m.engine().flat, before) and float(opt.sam_norm()) > 0.0


# ---- 4. graphs ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sam_step_replays_the_one_captured_graph(precision, monkeypatch):
    """use_graph=True equals the eager step bit for bit.  Both passes run the one plan: the plan count, the plan, its handle and its
    workspace are what they were, and between the two passes no plan entry is called but m2f_step - every switch entry would drop the
    captured step, so the graph that replays for pass 2 is the one pass 1 replayed."""
    _, dev, _ = _batch("padded_4x6")
    mg, me = _model(precision), _model(precision)
    og, oe = FusedAdam(mg, lr=1e-3, weight_decay=0.01, sam_rho=RHO), FusedAdam(me, lr=1e-3, weight_decay=0.01, sam_rho=RHO)
    for i in range(3):                                       # eager warm-up, capture, replay
        lg, le = mg.sam_step(*dev, og, use_graph=True), me.sam_step(*dev, oe, use_graph=False)
        assert torch.equal(lg, le) and torch.equal(mg.engine().flat, me.engine().flat), (precision, i)
    plan = _last_plan(mg)
    state = (len(mg.engine().plans), plan.handle, plan.workspace.data_ptr())
    seen, orig = [], mer_amd.runtime.check
    monkeypatch.setattr(mer_amd.runtime, "check", lambda rc, what="": (seen.append(what), orig(rc, what))[1])
    lg = mg.sam_step(*dev, og, use_graph=True)
    monkeypatch.undo()
    le = me.sam_step(*dev, oe, use_graph=False)
    print(f"{precision}: entries called during one sam_step: {seen}")
    assert torch.equal(lg, le) and torch.equal(mg.engine().flat, me.engine().flat)
    assert _last_plan(mg) is plan and (len(mg.engine().plans), plan.handle, plan.workspace.data_ptr()) == state
    adam = "m2f_adam_step_shadowed_range" if precision == "bf16" else "m2f_adam_step"
    assert seen == ["m2f_step", "m2f_grad_sumsq", "m2f_sam_perturb", "m2f_step", "m2f_sam_restore", adam], seen


# ---- 5. dropout -------------------------------------------------------------------------------------------------------------------------------
def test_dropout_sam_step_is_the_four_calls_by_hand():
    _, dev, _ = _batch("padded_4x6", CFG_DROP)
    torch.manual_seed(1234)
    ma = _model(cfg=CFG_DROP)
    torch.manual_seed(1234)
    mb = _model(cfg=CFG_DROP)
    oa, ob = FusedAdam(ma, lr=1e-3, sam_rho=RHO), FusedAdam(mb, lr=1e-3, sam_rho=RHO)
    for _ in range(2):
        la = ma.sam_step(*dev, oa, use_graph=False)
        lb = mb.train_step(*dev, use_graph=False)
        ob.first_step()
        l2 = mb.train_step(*dev, use_graph=False)
        ob.step()
        assert torch.equal(la, lb) and not torch.equal(l2, lb)
        assert torch.equal(ma.engine().flat, mb.engine().flat) and torch.equal(ma.flat_gradients(), mb.flat_gradients())
    # fresh masks in the second pass: at rho -> 0 the two passes of ONE step would otherwise return the same loss
    mc = _model(cfg=CFG_DROP)
    oc = FusedAdam(mc, lr=1e-3, sam_rho=1e-9)
    l1 = mc.train_step(*dev, use_graph=False)
    oc.first_step()
    l2 = mc.train_step(*dev, use_graph=False)
    print(f"dropout 0.4, rho 1e-9: first pass {l1.item()!r}, second pass {l2.item()!r}")
    assert abs(l1.item() - l2.item()) > 1e-4


# ---- 6. training modes --------------------------------------------------------------------------------------------------------------------------
def test_accumulation_group_in_two_sweeps_against_the_oracle_on_the_concatenated_batch():
    B, L = 6, 12
    g = torch.Generator().manual_seed(9)
    lengths = [L] + [int(x) for x in torch.randint(1, L + 1, (B - 1,), generator=g)]
    cpu = synth.make_inputs(CFG, B, L, lengths, "randn", seed=9)
    _threads()
    r = ref.sam_gradient(ref.as_float64(synth.make_state_dict(CFG)), CFG, _as64(cpu), RHO)
    mbs = [[x[i * 3:(i + 1) * 3].to(DEV) for x in cpu] for i in range(2)]
    m = _model()
    m.set_grad_accumulation(True)
    opt = FusedAdam(m, lr=1e-3, sam_rho=RHO)

    def sweep():
        opt.zero_grad()
        for mb in mbs:
            m.train_step(*mb, normalise=False, use_graph=False)

    sweep()
    opt.grad_scale = m.loss_terms()[1:2]
    opt.first_step()
    sweep()
    den = m.loss_terms()[1].item()
    norm = float(opt.sam_norm())
    print(f"two micro-batches, two sweeps: den {den}, ||g / den|| {norm!r} (float64 on the concatenated batch {r['norm']!r})")
    assert abs(norm - r["norm"]) <= 1e-3 * r["norm"]
    _check_grads("accumulation", m, r["sam"], scale=1.0 / den)
    before = m.engine().flat.clone()
    opt.step()
    assert not opt.sam_pending and not torch.equal(m.engine().flat, before)


def test_bf16_gradients_carry_the_perturbation():
    """set_grad_bf16: first_step reads the bf16 buffer step() reads; the buffer after the second pass against the bf16-emulating oracle at
    w + e (sam_ref, as the bf16-mode test above), by the first test's bound.  The reference states what this mode stores
    (sam_ref.sam_gradient(grad_bf16=True)): both gradients rounded to bf16, the norm and e taken from the ROUNDED first gradient - the
    buffer the optimizer reads.  Measured on MI355X: worst error 0.79 of the bound (in_proj_weight), the norm equal to 1.3e-8, none
    of the bf16 weights at w + e rounds differently.  With e from the UNROUNDED first gradient instead the reference's ||g|| differs by
    5e-6, 8,701 bf16 weights at w + e round the other way and linear1.weight lies 23 bounds away: the test would see a first_step that
    read the fp32 buffer."""
    name = "tiny_audio_only"
    cfg, B, L, lengths, kind = synth.CASES[name]
    sd = synth.make_state_dict(cfg)
    cpu = synth.make_inputs(cfg, B, L, lengths, kind)
    _threads()
    r = ref.sam_gradient(sd, cfg, cpu, RHO, rounding=O.Bf16Rounding(), to_fp32=True, grad_bf16=True)
    m = _model("bf16", cfg=cfg, sd=sd)
    assert m.set_grad_bf16(True)
    opt = FusedAdam(m, lr=1e-3, sam_rho=RHO)
    dev = [v.to(DEV) for v in cpu]
    m.train_step(*dev, use_graph=False)
    buf = m.engine().grad_bf16_buf
    first = buf.clone()
    opt.first_step()
    m.train_step(*dev, use_graph=False)
    norm = float(opt.sam_norm())
    want_norm = float(torch.sqrt(sum((first[o: o + n].double() ** 2).sum() for (_, o, n, _) in m.engine().items)))
    worst, at = 0.0, None
    names = {id(p): k for k, p in m.named_parameters()}
    for (p, o, n, s) in m.engine().items:
        k = names[id(p)]
        want = r["sam"][k]
        bound = 3e-5 + 1e-3 * want.abs().max().item()
        err = (buf[o: o + n].view(s).cpu().double() - want).abs().max().item()
        if err / bound > worst:
            worst, at = err / bound, k
    print(f"bf16 gradients: ||g|| {norm!r} (float64 over the bf16 buffer {want_norm!r}, the emulation's {r['norm']!r}); worst error / bound "
          f"{worst:.3f} ({at})")
    assert abs(norm - want_norm) <= EPS32 * want_norm and abs(norm - r["norm"]) <= E.TOL * r["norm"]
    assert worst <= 1.0, (at, worst)
    opt.step()


def test_clipping_reads_the_second_gradient():
    kind = "padded_4x6"
    _, dev, _ = _batch(kind)
    r = _reference(kind)
    m = _model()
    opt = FusedAdam(m, lr=1e-3, max_grad_norm=1e-3, sam_rho=RHO)
    m.sam_step(*dev, opt, use_graph=False)
    _check_grads("clip", m, r["sam"])
    g2 = m.flat_gradients()
    n2 = float(torch.sqrt(sum((g2[o: o + n].double() ** 2).sum() for (_, o, n, _) in m.engine().items)))
    coef64 = min(1.0, 1e-3 / (n2 + 1e-6))
    n2_ref = ref.grad_norm(r["sam"], r["sam"])
    print(f"clip: grad_norm {float(opt.grad_norm())!r} (float64 of the second gradient {n2!r}, the oracle's {n2_ref!r}), sam_norm "
          f"{float(opt.sam_norm())!r} (the oracle's first {r['norm']!r}); clip_coef {float(opt.clip_coef())!r} (float64 {coef64!r})")
    assert coef64 < 1.0 and abs(float(opt.clip_coef()) - coef64) <= 2 * EPS32 * coef64
    assert abs(float(opt.grad_norm()) - n2_ref) <= 1e-3 * n2_ref and abs(float(opt.sam_norm()) - r["norm"]) <= 1e-3 * r["norm"]
    assert abs(float(opt.grad_norm()) - float(opt.sam_norm())) > 1e-3 * r["norm"]       # two norms: g1 for SAM, g2 for the clip


def test_a_criterion_argument_passes_through_both_passes():
    kind = "padded_4x6"
    cpu, dev, _ = _batch(kind)

    def focal(logits, target):
        num, den = focal_ref.focal_terms(logits.reshape(-1, logits.shape[-1]), target.reshape(-1), None, 0.1, 2.0)
        return num / den

    _threads()
    r = ref.sam_gradient(ref.as_float64(synth.make_state_dict(CFG)), CFG, _as64(cpu), RHO, criterion=focal)
    plain = _reference(kind)
    m = _model()
    opt = FusedAdam(m, lr=1e-3, sam_rho=RHO)
    loss = m.sam_step(*dev, opt, focal_gamma=2.0, use_graph=False)
    bound = 3e-5 + 1e-3 * r["sam"][LAST].abs().max().item()
    other = (plain["sam"][LAST] - r["sam"][LAST]).abs().max().item() / bound
    print(f"focal_gamma 2: loss {loss.item()!r} (float64 {float(r['loss'])!r}); the cross entropy's SAM gradient lies {other:.0f} x the bound away")
    assert abs(loss.item() - float(r["loss"])) <= 2e-5 and other > 5.0
    _check_grads("focal", m, r["sam"])


# ---- 7. trajectory ------------------------------------------------------------------------------------------------------------------------------
def test_three_sam_steps_track_the_float64_trajectory():
    """tests/test_aux_head_model_gpu.py's three-step rule: losses to 1e-4, parameter norms to rtol 1e-4 / atol 1e-6; graph on."""
    kind = "padded_4x6"
    cpu, dev, _ = _batch(kind)
    lr, wd = 1e-3, 0.01
    _threads()
    want, w64 = ref.trajectory(synth.make_state_dict(CFG), CFG, _as64(cpu), RHO, 3, lr, wd)
    plain, _ = ref.trajectory(synth.make_state_dict(CFG), CFG, _as64(cpu), 1e-12, 3, lr, wd)
    m = _model()
    opt = FusedAdam(m, lr=lr, weight_decay=wd, sam_rho=RHO)
    losses = [m.sam_step(*dev, opt, use_graph=True).item() for _ in range(3)]
    print(f"losses {losses} against float64 {want} (without the perturbation {plain})")
    assert np.allclose(losses, want, rtol=0, atol=1e-4) and losses[2] < losses[0]
    norms, norms64, done = [], [], set()
    for k, p in m.state_dict(keep_vars=True).items():
        if id(p) not in done:
            done.add(id(p))
            norms.append(float(p.detach().double().norm()))
            norms64.append(float(w64[k].norm()))
    assert np.allclose(norms, norms64, rtol=1e-4, atol=1e-6)
    worst = max((p.detach().cpu().double() - w64[k]).abs().max().item() for k, p in m.named_parameters())
    print(f"parameters after three steps against float64: {worst:.3e} (an element whose gradient is fp32 noise may step the other way: printed only)")


# ---- 8. sam_rho=None ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,inside", [("fp32", False), ("bf16", False), ("bf16", True)])
def test_sam_rho_none_is_the_optimizer_that_never_saw_the_keyword(precision, inside):
    _, dev, _ = _batch("padded_4x6")
    ma, mb = _model(precision), _model(precision)
    oa, ob = FusedAdam(ma, lr=1e-3, weight_decay=0.01, sam_rho=None), FusedAdam(mb, lr=1e-3, weight_decay=0.01)
    for _ in range(3):
        for m, o in ((ma, oa), (mb, ob)):
            if inside:
                m.train_step(*dev, optimizer=o)
            else:
                m.train_step(*dev)
                o.step()
    assert torch.equal(ma.engine().flat, mb.engine().flat) and torch.equal(oa._m, ob._m) and torch.equal(oa._v, ob._v)
    assert oa._sam_saved is None and oa._sam_record is None


# ---- 9. refusals and state errors -----------------------------------------------------------------------------------------------------------------
def test_every_refusal_and_state_error_raises_by_name():
    _, dev, _ = _batch("padded_4x6")
    m = _model("bf16")
    opt = FusedAdam(m, lr=1e-3, ema_decay=0.9, sam_rho=RHO)
    with pytest.raises(RuntimeError, match=r"M2FNet\.train_step: optimizer= .*optimizer\.sam_rho"):
        m.train_step(*dev, optimizer=opt)
    assert not m.engine().plans, "refused before any plan was built"
    m.train_step(*dev, use_graph=False)
    with pytest.raises(RuntimeError, match=r"FusedAdam\.step\(\): sam_rho is set and no perturbation is pending"):
        opt.step()
    with pytest.raises(RuntimeError, match=r"FusedAdam\.step_ranges\(\): sharpness-aware"):
        opt.step_ranges([(0, m.engine().flat.numel())])
    with pytest.raises(RuntimeError, match="DataParallelStep: sharpness-aware minimisation"):
        dp.DataParallelStep(m, opt)
    assert opt.prepare_fused(_last_plan(m)) is False
    before = m.engine().flat.clone()
    opt.first_step()
    assert m.engine().shadows_fresh() and not torch.equal(m.engine().flat, before)
    with pytest.raises(RuntimeError, match=r"FusedAdam\.first_step\(\): a perturbation is already pending"):
        opt.first_step()
    with pytest.raises(RuntimeError, match=r"FusedAdam\.prepare_fused\(\) while a sharpness-aware perturbation is pending"):
        opt.prepare_fused(_last_plan(m))
    with pytest.raises(RuntimeError, match="M2FNet.sam_step: a perturbation is already pending"):
        m.sam_step(*dev, opt)
    # restore() abandons it: w's bits, the shadows invalidated
    assert opt.restore() is True and torch.equal(m.engine().flat, before) and not m.engine().shadows_fresh()
    assert opt.restore() is False
    with pytest.raises(RuntimeError, match=r"FusedAdam\.step\(\): sam_rho is set"):
        opt.step()
    # ... with an average under way
    m.sam_step(*dev, opt, use_graph=False)
    m.train_step(*dev, use_graph=False)
    opt.first_step()
    with pytest.raises(RuntimeError, match=r"FusedAdam\.averaged_parameters\(\) while a sharpness-aware perturbation is pending"):
        with opt.averaged_parameters():
            pass
    with pytest.raises(RuntimeError, match=r"FusedAdam\.ema_state_dict\(\) while a sharpness-aware perturbation is pending"):
        opt.ema_state_dict()
    opt.sam_rho = None                                             # a pending perturbation is still restored by step()
    m.train_step(*dev, use_graph=False)
    opt.step()
    assert not opt.sam_pending and opt.n_averaged == 2
    with opt.averaged_parameters():
        pass
    # a grouped optimizer that leaves a tensor in no group
    m2 = _model()
    part = FusedAdamW(m2, params=[{"params": [p for n, p in m2.named_parameters() if n.startswith("output_layer.")]}], sam_rho=RHO)
    m2.train_step(*dev, use_graph=False)
    before = m2.engine().flat.clone()
    with pytest.raises(RuntimeError, match=r"FusedAdam\.first_step\(\): .*cover every tensor"):
        part.first_step()
    assert torch.equal(m2.engine().flat, before)
    m2.set_grad_accumulation(True)
    with pytest.raises(RuntimeError, match="M2FNet.sam_step: under gradient accumulation"):
        m2.sam_step(*dev, part)
