"""bf16 mode against a float64 oracle that rounds to bf16 exactly where the kernels do (oracle/m2fnet_oracle.py, Bf16Rounding).

The other bf16 checks compare with the UNROUNDED fp32 oracle and so need bounds wide enough for honest bf16 rounding (6-8 % of a
gradient's norm, cosine 0.995).  Here like is compared with like: logits (valid rows), the loss and EVERY gradient tensor element
by element, max |plan - emulation| <= TOL x max |emulation| (bf16_emulation.TOL, shared with tests/test_bf16_emulation_cpu.py,
which shows that switching off any one rounding rule moves some tensor by >= 3 TOL).  Dropout 0 throughout.

Where it can be this tight.  A bf16 rounding decision is a step function of an fp32 value: an operand within fp32 noise of a
rounding midpoint rounds one way on the GPU (fp32 sums in the kernels' order) and the other way in float64, the one-ulp change
reaches later rounding points and ReLU gates, and it spreads - through attention to the rest of its dialogue, through the weight
gradients to every tensor.  At width: the emulation's own inputs moved by ONE fp32 ulp move the emulation itself, on c2_slice,
by 2.8e-3 of the logits and 0.46 of fusion_layers.0.linear.weight's largest element - what the plan measured against it, and as
much as the unrounded oracle is away; c2_slice and the bench geometries are therefore not compared here.  The strict cases below
are ones the GPU run showed free of such flips.  The small cases that do flip (FLIPPED) are held to what a flip leaves
intact: the dialogues it did not reach agree to fp32 noise, and the full bound is a strict xfail that records the disagreement.

Measured on MI355X (worst tensor of each test, relative to its largest element):
  tiny_audio_only  2.9e-7 (audio_encoders.0.layers.0.norm1.weight), eager and graph replay;
  tiny_text_only   1.9e-5 (text_encoders.0.layers.1.linear1.weight), same;
  tiny_odd_width   1.6e-5 (width 60 -> ld 64, head dim 15: the fp32-slab attention rule), same;
  M2F_TABLE_TILE=131 and M2F_ATTN_BF16=0 (against the emulation without attention rounding): the same values;
  FusedAdam, lr 1e-2, step 1 (shadows written by m2f_adam_shadow_kernel): 2.8e-7; the emulation fed the step-0 parameters
  instead: 2.5 (a stale parameter shadow cannot pass);
  grad_bf16 buffer: every element within one bf16 ulp of the emulated gradient (excess 0).
TOL = 1e-4: about 4x the worst of these (1.9e-5, rounded up).
Findings: (1) M2F_WGRAD_TABLE=0 missed the bound on the last classifier bias (2.8e-3 / 1.0e-3): the fp32-source grouped
weight-gradient form, which takes the criterion gradient (no bf16 shadow) in that variant, sums the fp32 values for the bias
gradient (its documented contract, test_kernels_gpu.py::test_gemm_layouts) while the table forms sum the bf16 rounding; the
emulation states that rule (Bf16Rounding(wgrad_table=False)) and the variant meets TOL with it.  (2) Plans with L > 64 (long_tiny, a text-only L = 80
plan) miss the full bound in the same per-dialogue pattern as the short cases that flip: the other dialogues' logits agree to
5e-8, and the L = 80 plan in fp32 mode matches the fp32 oracle to 9e-7; rounding the attention operands in the emulation makes
long_tiny worse (median relative L2 1.1e-2 -> 3.8e-2), which supports "no attention rounding at L > 64" (attention_dlong.hip reads
fp32 operands).  A one-layer L = 80 plan has exact logits but gradients 3.8e-4 off: not located, recorded in FLIPPED.
(3) After a second fused optimizer step (train_step(optimizer=...)) a plain step is 1.1e-3 off: not located, a strict xfail.
"""
import pytest
import torch

import synth
import long_cases
import bf16_emulation as E
from mer_amd.model import M2FNet
from mer_amd.optim import FusedAdam
from oracle import m2fnet_oracle as O

pytestmark = pytest.mark.gpu

TOL = E.TOL
CLEAN = ["tiny_audio_only", "tiny_text_only", "tiny_odd_width"]
# cases beyond synth.CASES: name -> (cfg, B, L, dialogue lengths)
EXTRA = {
    # width 60 (ld 64) and head dim 15: hd % 4 != 0 keeps the attention on fp32 slabs with the bf16 contractions only
    "tiny_odd_width": (synth._cfg(44, 60, 60, 4, 4, 4, 1, 1, 1, a_on=False, f_on=False), 3, 7, [7, 2, 5]),
    # M2FNet(packed=True) on a batch ragged enough to pack (46 valid rows of 8 x 16 slots -> T = 64): attention.hip and its
    # bf16 forms on the packed layout (plan.hip picks the kernel by L, not by the layout)
    "packed_tiny": (synth._cfg(48, 64, 64, 4, 4, 4, 1, 1, 1), 6, 16, [16, 3, 9, 1, 12, 5]),
    # L = 80 and 110 > 64: packed plans on the long-dialogue kernels (fp32 attention operands)
    "long_text": (synth._cfg(64, 64, 64, 4, 8, 4, 1, 2, 1, a_on=False, f_on=False), 2, 80, [80, 45]),
    "long_text_1layer": (synth._cfg(64, 64, 64, 4, 8, 4, 1, 1, 1, a_on=False, f_on=False), 2, 80, [80, 45]),
}


def _threads():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))


def _case(name):
    """(cfg, state dict, (text, audio, key_pad, emotion)) of a synth case, a long_cases case or an EXTRA case."""
    if name in synth.CASES:
        cfg, B, L, lengths, kind = synth.CASES[name]
        return cfg, synth.make_state_dict(cfg), synth.make_inputs(cfg, B, L, lengths, kind)
    if name in long_cases.CASES:
        cfg, *batch = long_cases.inputs(name)
        return cfg, synth.make_state_dict(cfg), tuple(batch)
    cfg, B, L, lengths = EXTRA[name]
    return cfg, synth.make_state_dict(cfg), synth.make_inputs(cfg, B, L, lengths, "randn")


_ORACLE = {}


def _oracle(name, attn=True, wgrad_table=True):
    """The emulation's (logits, loss, grads) on the case's own weights - once per case (float64 CPU time)."""
    key = (name, attn, wgrad_table)
    if key not in _ORACLE:
        cfg, sd, batch = _case(name)
        _threads()
        _ORACLE[key] = O.loss_and_grads(sd, cfg, *batch, rounding=O.Bf16Rounding(attn=attn, wgrad_table=wgrad_table))
    return _ORACLE[key]


def _model(cfg, sd, packed=None):
    m = M2FNet(cfg, precision="bf16", packed=packed)
    m.load_state_dict(sd)
    return m.to("cuda:0").train()


def _grads(m):
    return {k: p.grad.detach().cpu() for k, p in m.named_parameters()}


def _check(label, logits, loss, grads, ref, valid, tol=TOL):
    errs = E.errors(logits, loss, grads, ref, valid)
    w, k = E.worst(errs)
    top = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
    print(f"{label}: worst {w:.3e} ({k}) over {len(errs)} tensors; next {', '.join(f'{n} {v:.2e}' for n, v in top[1:])}")
    assert len(errs) >= 4, errs
    assert w <= tol, (label, k, w, top)
    return errs


def _run(name, packed=None, graph=False):
    cfg, sd, batch = _case(name)
    packed = True if name.startswith("packed") else packed
    m = _model(cfg, sd, packed)
    dev = [t.cuda() for t in batch]
    loss = m.train_step(*dev, use_graph=graph)
    if graph:
        loss = m.train_step(*dev, use_graph=True)
    torch.cuda.synchronize()
    return m, next(iter(m.engine().plans.values())), loss.item(), batch


def _step(name, packed=None, graph=False, attn=True, wgrad_table=True):
    cfg, sd, batch = _case(name)
    m = _model(cfg, sd, packed)
    dev = [t.cuda() for t in batch]
    loss = m.train_step(*dev, use_graph=graph)
    if graph:
        loss = m.train_step(*dev, use_graph=True)           # the replayed graph, as bench.py runs it
    torch.cuda.synchronize()
    plan = next(iter(m.engine().plans.values()))
    return _check(f"{name}{' packed' if packed else ''}{' graph' if graph else ''}", plan.logits.cpu(), loss.item(), _grads(m),
                  _oracle(name, attn, wgrad_table), ~batch[2])


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("name", CLEAN)
def test_padded_plan_matches_bf16_emulation(name, graph):
    _step(name, graph=graph)


# Cases whose rounding decisions are not stable: a value within fp32 noise of a bf16 rounding midpoint rounds the other way on the
# GPU, and the one-ulp change spreads through attention to the rest of ITS dialogue (and through the weight gradients to every
# tensor) but not to the other dialogues.  Measured on MI355X, worst logit error per dialogue relative to the logits' scale:
#   tiny_ragged  4.6e-8 1.4e-8 3.2e-8 1.1e-3 2.8e-8  (the FAM: two-segment operand, cross-attention with K from audio)
#   tiny_no_fam  5.5e-8 2.5e-3 2.3e-8                (one token of dialogue 1)
#   long_tiny    2.6e-3 2.4e-3 5.0e-8 9.1e-9         (L = 110: the two long dialogues)
#   long_text    dialogue 0 exact, dialogue 1 (45 utterances) off from its second row on; the same plan with one encoder
#                layer (long_text_1layer above) meets TOL everywhere, and in fp32 mode this plan matches the fp32 oracle to 9e-7
#   packed_tiny  5.2e-8 4.2e-8 4.5e-8 3.7e-8 5.3e-8 3.3e-8  (packed, T = 64; the gradients: 2.4e-3, audio in_proj_weight)
#   a text-only packed batch of the same lengths: 2.0e-3 on text_encoders.0.layers.0.linear1.weight (not kept)
#   long_text_1layer  logits of both dialogues within 5e-8; the gradients differ by up to 3.8e-4 (linear2.weight, 1.1e-4
#                in_proj_weight), so something in the backward of the L = 80 plan rounds differently; it is not located yet
# A wrong rounding rule or a kernel bug would move every dialogue; so here at least half of the dialogues must meet TOL, and the
# full bound is a strict xfail that records the disagreement (it passes only if the flips go away).
FLIPPED = ["tiny_ragged", "tiny_no_fam", "long_tiny", "long_text", "packed_tiny", "long_text_1layer"]


def _per_dialogue(logits, ref_logits, key_pad):
    scale = ref_logits[~key_pad].abs().max().item()
    d = (logits.double() - ref_logits.double()).abs().amax(-1)
    d[key_pad] = 0
    return (d.amax(1) / scale).tolist()


@pytest.mark.parametrize("name", FLIPPED)
def test_flipped_cases_agree_outside_the_flipped_dialogues(name):
    m, plan, loss, batch = _run(name)
    B, L = batch[2].shape
    if name.startswith(("packed", "long")):                 # packed plans for real: fewer token rows than the padded bucket
        Bb, Lb = m.engine().bucket(B, L)
        assert plan.packed and plan.T < Bb * Lb, (plan.packed, plan.T)
    per = _per_dialogue(plan.logits.cpu(), _oracle(name)[0], batch[2])
    print(f"{name} (packed {plan.packed}): per-dialogue logit error {', '.join(f'{x:.1e}' for x in per)}")
    assert sum(x <= TOL for x in per) >= len(per) / 2, per
    assert max(per) < 1e-2, per                         # a flip, not a wrong rule: those move logits by 1e-1 and more


@pytest.mark.xfail(strict=True, reason="bf16 rounding flips spread through one dialogue (see FLIPPED)")
@pytest.mark.parametrize("name", FLIPPED)
def test_flipped_cases_full_bound(name):
    m, plan, loss, batch = _run(name)
    _check(name, plan.logits.cpu(), loss, _grads(m), _oracle(name), ~batch[2])


@pytest.mark.parametrize("name", CLEAN)
@pytest.mark.parametrize("var,val", [("M2F_WGRAD_TABLE", "0"), ("M2F_TABLE_TILE", "131"), ("M2F_ATTN_BF16", "0")])
def test_plan_variants_match_bf16_emulation(name, var, val, monkeypatch):
    """The grouped weight-gradient launches (M2F_WGRAD_TABLE=0: against the emulation with that variant's bias-gradient rule,
    see the findings above) and the ring form of the table (M2F_TABLE_TILE=131) meet the
    bound on their own; M2F_ATTN_BF16=0 keeps fp32 attention in bf16 mode and must match the emulation with its attention
    rounding switched off (the attention rule checked from the other side).  All read when a plan is built."""
    monkeypatch.setenv(var, val)
    _step(name, attn=(var != "M2F_ATTN_BF16"), wgrad_table=(var != "M2F_WGRAD_TABLE"))


def _snapshot(m):
    """The model's fp32 parameters as a CPU state dict, aliases kept aliased (the oracle sums their gradients)."""
    seen, out = {}, {}
    for k, v in m.state_dict(keep_vars=True).items():
        if id(v) not in seen:
            seen[id(v)] = v.detach().cpu().clone()
        out[k] = seen[id(v)]
    return out


def test_optimizer_written_shadows_match_bf16_emulation():
    """Three FusedAdam steps (lr 1e-2) with graph replay: the forward reads the bf16 parameter shadows m2f_adam_shadow_kernel
    wrote, so each step's gradients must match the emulation fed the plan's OWN fp32 parameters of that moment - and must
    NOT match it fed the previous step's parameters (a shadow one step stale would be caught).  Between the second and the
    third step a load_state_dict writes new parameters through torch: the cast launch must come back."""
    name = "tiny_text_only"
    cfg, sd0, batch = _case(name)
    m = _model(cfg, sd0)
    opt = FusedAdam(m, lr=1e-2, weight_decay=0.01)
    dev = [t.cuda() for t in batch]
    valid = ~batch[2]
    _threads()
    stale = []
    for step in range(3):
        now = _snapshot(m)
        opt.zero_grad()
        loss = m.train_step(*dev, use_graph=True)
        torch.cuda.synchronize()
        plan = next(iter(m.engine().plans.values()))
        logits, grads = plan.logits.cpu(), _grads(m)
        ref = O.loss_and_grads(now, cfg, *batch, rounding=O.Bf16Rounding())
        _check(f"adam step {step}", logits, loss.item(), grads, ref, valid)
        for what, old in stale:
            w, k = E.worst(E.errors(logits, loss.item(), grads, O.loss_and_grads(old, cfg, *batch, rounding=O.Bf16Rounding()), valid))
            print(f"adam step {step} against the {what}: worst {w:.3e} ({k})")
            assert w > 3 * TOL, (step, what, k, w)
        opt.step()
        stale = [("parameters of the step before", now)]
        if step == 1:
            adam = _snapshot(m)
            m.load_state_dict(sd0)                          # back to the initial weights (two lr 1e-2 steps away)
            stale.append(("parameters before load_state_dict", adam))


@pytest.mark.parametrize("steps", [1, pytest.param(2, marks=pytest.mark.xfail(strict=True, reason="second fused step: 1.1e-3, not located"))])
def test_fused_optimizer_written_shadows_match_bf16_emulation(steps):
    """train_step(optimizer=opt): in bf16 mode the weight-gradient launch applies the Adam update itself (FusedAdam.prepare_fused,
    gemm_p8.h EPI 3) and writes the parameter shadows.  The matrices' .grad is not written in that form, so the check is on the
    step AFTER each fused one: a plain step must match the emulation fed the plan's own parameters, and must not match it fed
    the parameters of before the fused update.  Measured: after one fused step 2.8e-7 (against the parameters before the
    update: 2.5); after a second fused step 1.1e-3 (text_encoders.0.layers.0.linear1.weight) - above TOL, below a stale
    shadow by three orders of magnitude; whether a rounding flip or a fused-path difference is not settled, kept as a strict
    xfail."""
    name = "tiny_text_only"
    cfg, sd0, batch = _case(name)
    m = _model(cfg, sd0)
    opt = FusedAdam(m, lr=1e-2, weight_decay=0.01)
    dev = [t.cuda() for t in batch]
    valid = ~batch[2]
    _threads()
    for step in range(steps):
        before = _snapshot(m)
        m.train_step(*dev, use_graph=True, optimizer=opt)
        now = _snapshot(m)
        assert any(not torch.equal(before[k], now[k]) for k in now)
        loss = m.train_step(*dev, use_graph=True)
        torch.cuda.synchronize()
        plan = next(iter(m.engine().plans.values()))
        logits, grads = plan.logits.cpu(), _grads(m)
        _check(f"fused adam step {step}", logits, loss.item(), grads, O.loss_and_grads(now, cfg, *batch, rounding=O.Bf16Rounding()),
               valid)
        w, k = E.worst(E.errors(logits, loss.item(), grads, O.loss_and_grads(before, cfg, *batch, rounding=O.Bf16Rounding()), valid))
        print(f"fused adam step {step} against the parameters before the update: worst {w:.3e} ({k})")
        assert w > 3 * TOL, (step, k, w)


def test_grad_bf16_buffer_matches_bf16_emulation():
    """M2FNet.set_grad_bf16: the step leaves every gradient rounded once to bf16 in one flat buffer (the weight-gradient launch
    writes dW as bf16, one cast launch rounds the rest).  Each element must equal the emulated gradient to TOL x the tensor's
    scale plus one bf16 ulp of that element."""
    name = "tiny_text_only"
    cfg, sd, batch = _case(name)
    m = _model(cfg, sd)
    assert m.set_grad_bf16(True)
    dev = [t.cuda() for t in batch]
    m.train_step(*dev, use_graph=True)
    m.train_step(*dev, use_graph=True)
    torch.cuda.synchronize()
    eng = m.engine()
    buf = eng.grad_bf16_buf.float().cpu()
    by_id = {id(p): k for k, p in m.named_parameters()}
    _, _, rg = _oracle(name)
    worst, checked = (0.0, ""), 0
    for (p, o, n, s) in eng.items:
        k = by_id[id(p)]
        want = rg[k].double()
        scale = want.abs().max().item()
        if scale < E.ZERO_GRAD:
            continue
        got = buf[o: o + n].view(s).double()
        ulp = torch.where(got != 0, torch.exp2(torch.floor(torch.log2(got.abs())) - 7), torch.zeros_like(got))
        excess = ((got - want).abs() - ulp).max().item() / scale
        worst = max(worst, (excess, k))
        checked += 1
        assert excess <= TOL, (k, excess)
    print(f"grad_bf16 buffer: worst excess over one ulp {worst[0]:.3e} ({worst[1]}) over {checked} tensors")
    assert checked >= 20
