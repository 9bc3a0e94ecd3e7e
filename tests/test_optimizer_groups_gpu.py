"""Parameter groups and decoupled weight decay on the device: FusedAdam(params=[...]) / FusedAdamW (csrc/adam.hip: the grouped
shadow-writing and slice kernels, the hyper table; csrc/gemm_p8.h EPI 6: the grouped in-launch optimizer).

What is compared against what:
  * torch.optim.AdamW - the decoupled arithmetic, at kernel level (max abs difference 1e-6, the bound
    tests/test_kernels_gpu.py::test_adam_matches_torch holds the coupled kernel to) and at model level (deviation relative to the norm
    of the update below 1e-4, the bound of tests/test_grad_clip_gpu.py::test_clipped_step_against_torch_clip_grad_norm_and_adam);
  * today's single-group kernels - BIT FOR BIT: a coupled group's tensors get what FusedAdam(model, lr, wd) gives them;
  * the grouped forms against each other - bit for bit: step() / step_ranges() / the in-launch optimizer, eager and replayed;
  * nothing at all: a tensor of no group keeps every bit.
The grouped kernels walk the flat buffer of a model layout (tensor by tensor), not a bare array, so the kernel-level test seeds every
element of the tiny layout (about 1e6 elements, tensors with 1-3 element tails among them) where test_adam_matches_torch seeds 4096 + 64."""
import io
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import dp, layout, runtime  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam, FusedAdamW  # noqa: E402

TINY = synth.CASES["tiny_ragged"][0]                     # dropout 0; a 2-element classifier bias (odd tail)
ENCODERS = ("audio_encoders", "text_encoders")
TABLE = 32 * 1024                                        # behind the shadows: the optimizer's tensor table (uint16 elements)


def _model(cfg=TINY, precision="fp32"):
    m = M2FNet(cfg, precision=precision)
    m.load_state_dict(synth.make_state_dict(cfg))
    return m.to("cuda:0").train()


def _batch(cfg=TINY, B=8, L=16, seed=1):
    g = torch.Generator().manual_seed(seed)
    lengths = [L] + [int(x) for x in torch.randint(1, L + 1, (B - 1,), generator=g)]
    return [t.cuda() for t in synth.make_inputs(cfg, B, L, lengths, "randn", seed=seed)]


def _split(m):
    named = dict(m.named_parameters())
    return ([p for n, p in named.items() if n.startswith(ENCODERS)], [p for n, p in named.items() if not n.startswith(ENCODERS)])


def _state(m, opt):
    torch.cuda.synchronize()
    eng = m.engine()
    out = {"p": eng.flat.detach().clone(), "m": opt._m.clone(), "v": opt._v.clone()}
    if eng.wshadow is not None:
        out["sh"] = eng.wshadow[: eng.wshadow.numel() - TABLE].clone()
    return out


def _same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


def _element_mask(m, params):
    """bool mask over the flat buffer: the elements of `params`."""
    eng = m.engine()
    ids = {id(p) for p in params}
    mask = torch.zeros(eng.flat.numel(), dtype=torch.bool, device="cuda")
    for (p, o, n, _) in eng.items:
        if id(p) in ids:
            mask[o: o + n] = True
    return mask


def _recast_shadows(m, batch):
    """The shadow buffer after a forward that was FORCED to cast every parameter again (what the shadows must hold), and that
    forward's logits."""
    eng = m.engine()
    eng.invalidate_shadows()
    m.eval()
    with torch.inference_mode():
        logits = m(batch[0], batch[1], batch[2]).clone()
    m.train()
    torch.cuda.synchronize()
    return eng.wshadow[: eng.wshadow.numel() - TABLE].clone(), logits


# ---- 5. against torch, kernel level ---------------------------------------------------------------------------------------------------
def _bare_layout(seed):
    """Flat buffers of TINY's layout with every real element seeded (pads zero), and the (offset, numel) of the tensors."""
    c = layout.M2FConfig.from_model_config(TINY)
    specs, total = layout.param_specs(c)
    items = [(s.offset, s.numel) for s in specs if not s.alias_of]
    g = torch.Generator().manual_seed(seed)
    buf = torch.zeros(total)
    for o, n in items:
        buf[o: o + n] = torch.randn(n, generator=g)
    return c, buf, items, total


@pytest.mark.parametrize("lr,wd", [(1e-3, 0.01), (5e-4, 5e-4)])
@pytest.mark.parametrize("form", ["slices", "shadowed"])
def test_decoupled_update_matches_torch_adamw(form, lr, wd):
    c, p0, items, total = _bare_layout(80)
    _, g, _, _ = _bare_layout(81)
    real = torch.zeros(total, dtype=torch.bool)
    for o, n in items:
        real[o: o + n] = True
    assert int(real.sum()) >= 4096 + 64
    ref_p = torch.nn.Parameter(p0[real].clone().cuda())          # (torch on the device, as test_adam_matches_torch runs it)
    opt = torch.optim.AdamW([ref_p], lr=lr, weight_decay=wd)
    p, m, v = p0.cuda(), torch.zeros(total, device="cuda"), torch.zeros(total, device="cuda")
    shadow = runtime.param_shadow_buffer(c, "cuda") if form == "shadowed" else None
    table = torch.zeros(16, 8, device="cuda")
    import ctypes
    tg = (ctypes.c_int * len(items))(*([0] * len(items)))
    for step in range(1, 5):
        gg = g * step
        ref_p.grad = gg[real].clone().cuda()
        opt.step()
        runtime.adam_hyper_groups(table, [(lr, (0.9, 0.999), 1e-8, wd, True, step)])
        runtime.adam_step_grouped(c, p, gg.cuda(), m, v, shadow, tg, table)
    torch.cuda.synchronize()
    err = float((p.cpu()[real] - ref_p.detach().cpu()).abs().max())
    print(f"AdamW kernel ({form}) lr {lr} wd {wd}: max abs difference from torch.optim.AdamW after 4 steps {err:.3e} "
          f"over {int(real.sum())} elements (|p| max {float(p0.abs().max()):.2f})")
    assert err <= 1e-6
    assert not bool(p.cpu()[~real].any()) and not bool(m.cpu()[~real].any())          # pads: still zero
    row = table[0].cpu()
    assert float(row[4]) == 0.0 and float(row[6]) == float(np.float32(1.0 - lr * wd))  # coupled wd 0, decay rounded once from double


@pytest.mark.parametrize("form", ["slices", "shadowed"])
def test_bf16_gradient_input_equals_fp32_kernel_on_the_rounded_gradients(form):
    c, p0, items, total = _bare_layout(80)
    _, g, _, _ = _bare_layout(81)
    import ctypes
    tg = (ctypes.c_int * len(items))(*([i % 2 for i in range(len(items))]))
    table = torch.zeros(16, 8, device="cuda")
    den = torch.tensor([4.0], device="cuda")
    g16 = g.to(torch.bfloat16).cuda()
    runs = []
    for grads in (g16, g16.float()):
        p, m, v = p0.cuda(), torch.zeros(total, device="cuda"), torch.zeros(total, device="cuda")
        shadow = runtime.param_shadow_buffer(c, "cuda") if form == "shadowed" else None
        for step in range(1, 4):
            runtime.adam_hyper_groups(table, [(1e-3, (0.9, 0.999), 1e-8, 0.01, True, step), (5e-4, (0.8, 0.99), 1e-6, 0.1, False, step)])
            runtime.adam_step_grouped(c, p, grads, m, v, shadow, tg, table, grad_scale=den)
        torch.cuda.synchronize()
        runs.append((p, m, v) + ((shadow[: shadow.numel() - TABLE],) if shadow is not None else ()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], p0.cuda())


# ---- 6. against today's kernels, bit for bit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16_grads"])
def test_coupled_two_group_step_equals_the_single_group_steps(mode):
    precision = "fp32" if mode == "fp32" else "bf16"
    (lr1, wd1), (lr2, wd2) = (1e-3, 0.01), (3e-4, 0.05)
    mg, ma, mb = (_model(TINY, precision) for _ in range(3))
    if mode == "bf16_grads":
        for m in (mg, ma, mb):
            assert m.set_grad_bf16(True)
    enc, rest = _split(mg)
    og = FusedAdam(mg, params=[{"params": enc, "lr": lr1, "weight_decay": wd1}, {"params": rest, "lr": lr2, "weight_decay": wd2}])
    oa, ob = FusedAdam(ma, lr=lr1, weight_decay=wd1), FusedAdam(mb, lr=lr2, weight_decay=wd2)
    assert og._grouped and not oa._grouped
    enc_mask = _element_mask(mg, enc)
    rest_mask = _element_mask(mg, rest)
    assert bool(enc_mask.any()) and bool(rest_mask.any()) and not bool((enc_mask & rest_mask).any())
    for i in range(3):
        batch = _batch(seed=1 + i)
        mg.train_step(*batch)
        torch.cuda.synchronize()
        eg = mg.engine()
        og._bind()
        for m, o in ((ma, oa), (mb, ob)):
            e = m.engine()
            o._bind()
            m.train_step(*batch)                               # (publishes .grad as views of the flat gradient buffer)
            torch.cuda.synchronize()
            with torch.no_grad():
                e.flat.copy_(eg.flat)                          # the grouped run's parameters, moments, step count, gradients
                o._m.copy_(og._m)
                o._v.copy_(og._v)
                o._step = i
                e.ensure_grad().copy_(eg.ensure_grad())
                if mode == "bf16_grads":
                    e.grad_bf16_buf.copy_(eg.grad_bf16_buf)
        assert og._gsteps == [i, i]
        og.step()
        oa.step()
        ob.step()
        sg, sa, sb = _state(mg, og), _state(ma, oa), _state(mb, ob)
        for k in ("p", "m", "v"):
            assert torch.equal(sg[k][enc_mask], sa[k][enc_mask]), (mode, i, k, "encoders")
            assert torch.equal(sg[k][rest_mask], sb[k][rest_mask]), (mode, i, k, "rest")
        assert not torch.equal(sg["p"][rest_mask], sa["p"][rest_mask])          # (the two settings do differ)
        if precision == "bf16":
            # both shadows: where the two single-group runs agree with each other they hold an unowned pad; everywhere else the grouped
            # buffer holds A's value or B's
            assert eg.shadows_fresh()
            assert bool(((sg["sh"] == sa["sh"]) | (sg["sh"] == sb["sh"])).all())
            assert not torch.equal(sg["sh"], sa["sh"]) and not torch.equal(sg["sh"], sb["sh"])
    if precision == "bf16":
        got = _state(mg, og)["sh"]
        want, _ = _recast_shadows(mg, _batch(seed=1))
        assert torch.equal(got, want)                          # W and W^T of every matrix = the cast of the updated parameter


# ---- 7. one explicit group with the defaults = FusedAdam(model) ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16_in_launch"])
def test_one_explicit_group_equals_the_plain_optimizer(mode):
    precision = "fp32" if mode == "fp32" else "bf16"
    cfg, B, L, lengths, kind = synth.CASES["tiny_ragged"]
    batch = [t.cuda() for t in synth.make_inputs(cfg, B, L, lengths, kind)]
    runs = []
    for grouped in (True, False):
        m = _model(cfg, precision)
        opt = FusedAdam(m, params=[{"params": list(m.parameters())}]) if grouped else FusedAdam(m)
        assert opt._grouped == grouped
        losses = []
        for i in range(3):
            if mode == "bf16_in_launch":
                losses.append(float(m.train_step(*batch, use_graph=i > 0, optimizer=opt)))
            else:
                losses.append(float(m.train_step(*batch, use_graph=i > 0)))
                opt.step()
        plan = next(p for p in m.engine().plans.values() if p.train)
        if mode == "bf16_in_launch":
            assert getattr(plan, "_fused_key", None) is not None, getattr(plan, "_fused_err", None)
        runs.append((losses, _state(m, opt), m.engine().shadows_fresh()))
    assert runs[0][0] == runs[1][0]
    _same(runs[0][1], runs[1][1], mode)
    assert runs[0][2] == runs[1][2] == (precision == "bf16")


# ---- 8. tensors of no group ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16_grads", "bf16_in_launch_asked"])
def test_unowned_tensors_keep_every_bit(mode):
    precision = "fp32" if mode == "fp32" else "bf16"
    m = _model(TINY, precision)
    if mode == "bf16_grads":
        assert m.set_grad_bf16(True)
    enc, rest = _split(m)
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.1, params=rest)            # both encoders in no group
    enc_mask, rest_mask = _element_mask(m, enc), _element_mask(m, rest)
    m.train_step(*_batch(seed=1))
    opt._bind()
    opt._m[enc_mask | rest_mask] = 0.25                                     # (a sentinel: an unowned moment must not even be decayed)
    opt._v[enc_mask | rest_mask] = 0.5
    before = _state(m, opt)
    for i in range(3):
        if mode == "bf16_in_launch_asked":
            # the weight-gradient table holds the encoders' matrices, which no group owns: prepare_fused declines, two launches run
            m.train_step(*_batch(seed=1 + i), optimizer=opt)
            plan = next(p for p in m.engine().plans.values() if p.train)
            assert getattr(plan, "_fused_key", None) is None and "owned by no parameter group" in plan._fused_err
        else:
            m.train_step(*_batch(seed=1 + i))
            opt.step()
        if precision == "bf16":
            assert m.engine().shadows_fresh()
    after = _state(m, opt)
    for k in ("p", "m", "v"):
        assert torch.equal(before[k][enc_mask], after[k][enc_mask]), k
        assert not torch.equal(before[k][rest_mask], after[k][rest_mask]), k
    pads = ~(enc_mask | rest_mask)
    assert not bool(after["p"][pads].any()) and not bool(after["m"][pads].any())         # pads: zero as before
    if precision == "bf16":
        b = _batch(seed=9)
        m.eval()
        with torch.inference_mode():
            fresh_logits = m(b[0], b[1], b[2]).clone()                                 # skips its parameter casts
        m.train()
        got = after["sh"]
        assert torch.equal(got, m.engine().wshadow[: got.numel()])
        want, recast_logits = _recast_shadows(m, b)
        assert torch.equal(got, want)
        assert torch.equal(fresh_logits, recast_logits)
        assert not torch.equal(before["sh"], after["sh"])


# ---- 9. against torch, model level ----------------------------------------------------------------------------------------------------
def _cat(ts):
    return torch.cat([t.reshape(-1).double() for t in ts])


@pytest.mark.parametrize("max_norm", [None, 0.02])
def test_fused_adamw_groups_and_warmup_against_torch(max_norm):
    m = _model()
    named = list(m.named_parameters())
    decay = [p for _, p in named if p.dim() > 1]
    no_decay = [p for _, p in named if p.dim() == 1]
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.01, max_grad_norm=max_norm,
                     params=[{"params": decay}, {"params": no_decay, "weight_decay": 0.0, "lr": 2e-3}])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, [lambda s: min(1.0, (s + 1) / 3.0), lambda s: min(1.0, (s + 1) / 2.0)])
    order = decay + no_decay
    worst = 0.0
    for i in range(3):
        m.train_step(*_batch(seed=1 + i))
        torch.cuda.synchronize()
        start = [p.detach().cpu().double().clone() for p in order]
        grads = [p.grad.detach().cpu().double().clone() for p in order]
        sd = _through_a_file(opt.state_dict(), "cpu")
        cpu = [torch.nn.Parameter(s.clone()) for s in start]
        t = torch.optim.AdamW([{"params": cpu[: len(decay)]}, {"params": cpu[len(decay):]}])
        t.load_state_dict(sd)
        assert [g["lr"] for g in t.param_groups] == [g["lr"] for g in opt.param_groups]
        assert t.param_groups[0]["lr"] == pytest.approx(1e-3 * min(1.0, (i + 1) / 3.0)) and t.param_groups[1]["weight_decay"] == 0.0
        for p, g in zip(cpu, grads):
            p.grad = g
        if max_norm is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(cpu, max_norm))
        t.step()
        opt.step()
        sched.step()
        torch.cuda.synchronize()
        got, want = _cat([p.detach().cpu() for p in order]), _cat([p.detach() for p in cpu])
        dev = float((got - want).norm() / (want - _cat(start)).norm())
        worst = max(worst, dev)
        print(f"FusedAdamW step {i + 1} (max_grad_norm {max_norm}): deviation from torch.optim.AdamW relative to the update's norm {dev:.3e}")
        if max_norm is not None:
            assert float(opt.clip_coef()) < 1.0 and abs(float(opt.grad_norm()) - norm) / norm <= 2.0 ** -23
        assert dev < 1e-4
    assert opt._gsteps == [3, 3]


# ---- 10. step_ranges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16_exchange"])
def test_step_ranges_over_the_reducers_buckets_equals_step(mode):
    precision = "fp32" if mode == "fp32" else "bf16"
    pair = []
    for _ in range(2):
        m = _model(TINY, precision)
        enc, rest = _split(m)
        pair.append((m, FusedAdamW(m, lr=1e-3, params=[{"params": enc, "weight_decay": 0.1}, {"params": rest, "lr": 5e-4}])))
    (m1, o1), (m2, o2) = pair
    eng = m2.engine()
    n = eng.flat.numel()
    eng.ensure_grad()
    red = dp.GradReducer(eng.flat_grad_ext, n, n_buckets=3)
    red.align_to(o for (_, o, _, _) in eng.items)
    ranges = list(red.param_chunks)
    assert len(ranges) == 3 and ranges[0][0] == 0 and ranges[-1][1] == n
    for i in range(3):
        batch = _batch(seed=1 + i)
        m1.train_step(*batch)
        m2.train_step(*batch)
        if mode == "bf16_exchange":
            o1.grads_bf16 = m1.engine().flat_grad.to(torch.bfloat16)
            o1.step()
            seen = []
            o2.step_ranges(ranges, before_each=seen.append, grads=m2.engine().flat_grad.to(torch.bfloat16))
            assert seen == [0, 1, 2]
        else:
            o1.step()
            o2.step_ranges(ranges)
        _same(_state(m1, o1), _state(m2, o2), (mode, i))
        assert m1.engine().shadows_fresh() == m2.engine().shadows_fresh() == (precision == "bf16")
    assert o2._gsteps == [3, 3]
    # a range that cuts a tensor: refused by a grouped optimizer, before anything is stepped ...
    mid = next(o for (_, o, numel, _) in eng.items if o > 0 and numel > 128) + 64
    cut = [(0, mid), (mid, n)]
    assert mid not in {o for (_, o, _, _) in eng.items}
    before = _state(m2, o2)
    with pytest.raises(ValueError, match="cuts a parameter tensor"):
        o2.step_ranges(cut)
    _same(before, _state(m2, o2))
    assert o2._gsteps == [3, 3]
    # ... and still taken by today's single coupled group (its flat kernel)
    m3 = _model(TINY, precision)
    o3 = FusedAdam(m3, lr=1e-3, weight_decay=0.01)
    m3.train_step(*_batch())
    o3.step_ranges(cut)
    torch.cuda.synchronize()
    assert o3._step == 1 and not m3.engine().shadows_fresh()


# ---- 11. the in-launch form ----------------------------------------------------------------------------------------------------------------
def _run_in_launch(name, groups, fused, steps=6, lr_change=False):
    cfg, B, L, lengths, kind = synth.CASES[name]
    batch = [t.cuda() for t in synth.make_inputs(cfg, B, L, lengths, kind)]
    m = _model(cfg, "bf16")
    enc, rest = _split(m)
    if groups == "one_decoupled":
        opt = FusedAdamW(m, lr=1e-3, weight_decay=0.05)
    else:
        opt = FusedAdamW(m, lr=1e-3, params=[{"params": enc, "lr": 2e-4, "weight_decay": 0.1}, {"params": rest, "decoupled_weight_decay": False}])
    losses = []
    for i in range(steps):
        if lr_change and i == 4:                                # between two replays of the captured step
            opt.param_groups[0]["lr"] = 5e-3
        if fused:
            losses.append(float(m.train_step(*batch, use_graph=i > 0, optimizer=opt)))
        else:
            losses.append(float(m.train_step(*batch, use_graph=i > 0)))
            opt.step()
    plan = next(p for p in m.engine().plans.values() if p.train)
    return {"losses": losses, "state": _state(m, opt), "fresh": m.engine().shadows_fresh(),
            "armed": getattr(plan, "_fused_key", None) is not None, "err": getattr(plan, "_fused_err", None), "steps": opt._gsteps}


@pytest.mark.parametrize("name", ["tiny_ragged", "c2_slice"])
@pytest.mark.parametrize("groups", ["one_decoupled", "two_groups"])
def test_in_launch_optimizer_with_groups_equals_step_then_step(name, groups):
    """The register gate passed for the grouped epilogue (EPI 6: zero scratch, no VGPR spills), so prepare_fused arms it."""
    a, b = _run_in_launch(name, groups, True), _run_in_launch(name, groups, False)
    assert a["armed"] and not b["armed"], a["err"]
    assert a["losses"] == b["losses"], (a["losses"], b["losses"])
    _same(a["state"], b["state"], (name, groups))
    assert a["fresh"] and b["fresh"] and a["steps"] == b["steps"]


def test_lr_change_between_replays_reaches_the_grouped_graph():
    a, b = _run_in_launch("tiny_ragged", "two_groups", True, lr_change=True), _run_in_launch("tiny_ragged", "two_groups", False, lr_change=True)
    assert a["armed"], a["err"]
    _same(a["state"], b["state"])
    c = _run_in_launch("tiny_ragged", "two_groups", True)
    assert not torch.equal(a["state"]["p"], c["state"]["p"])


def test_a_grouped_optimizer_takes_over_a_captured_plan():
    """A second setup on a plan with a captured graph drops that graph: the plain optimizer's in-launch steps, then FusedAdamW's."""
    cfg, B, L, lengths, kind = synth.CASES["tiny_ragged"]
    batch = [t.cuda() for t in synth.make_inputs(cfg, B, L, lengths, kind)]
    runs = []
    for fused in (True, False):
        m = _model(cfg, "bf16")
        first, second = FusedAdam(m, lr=1e-3, weight_decay=0.01), FusedAdamW(m, lr=1e-3, weight_decay=0.05)
        for i in range(6):
            opt = first if i < 3 else second
            if fused:
                m.train_step(*batch, use_graph=i > 0, optimizer=opt)
            else:
                m.train_step(*batch, use_graph=i > 0)
                opt.step()
        runs.append((_state(m, first), _state(m, second)))
    _same(runs[0][0], runs[1][0])
    _same(runs[0][1], runs[1][1])


# ---- 12. checkpoints ---------------------------------------------------------------------------------------------------------------------
def _grouped_adamw(m):
    enc, rest = _split(m)
    return FusedAdamW(m, lr=1e-3, params=[{"params": rest, "weight_decay": 0.05}, {"params": enc, "lr": 3e-4}])


def _through_a_file(obj, device="cuda:0"):
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return torch.load(buf, map_location=device)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_save_and_resume_is_the_uninterrupted_run(precision):
    whole = _model(TINY, precision)
    o_whole = _grouped_adamw(whole)
    for i in range(4):
        whole.train_step(*_batch(seed=1 + i))
        o_whole.step()
    part = _model(TINY, precision)
    o_part = _grouped_adamw(part)
    for i in range(2):
        part.train_step(*_batch(seed=1 + i))
        o_part.step()
    ck = _through_a_file({"model": part.state_dict(), "opt": o_part.state_dict()})
    assert sorted(ck["opt"]["state"]) == list(range(len(list(part.parameters()))))
    assert all(float(st["step"]) == 2.0 for st in ck["opt"]["state"].values())
    resumed = M2FNet(TINY, precision=precision).to("cuda:0").train()
    o_res = _grouped_adamw(resumed)
    resumed.load_state_dict(ck["model"])
    o_res.load_state_dict(ck["opt"])
    assert o_res._gsteps == [2, 2]
    for i in range(2, 4):
        resumed.train_step(*_batch(seed=1 + i))
        o_res.step()
    _same(_state(whole, o_whole), _state(resumed, o_res), precision)
    assert o_res._gsteps == o_whole._gsteps == [4, 4]


def test_a_torch_adamw_state_dict_loads():
    m = _model()
    opt = _grouped_adamw(m)
    cpu = [[torch.nn.Parameter(p.detach().cpu().clone()) for p in g["params"]] for g in opt.param_groups]
    t = torch.optim.AdamW([{"params": cpu[0], "weight_decay": 0.05}, {"params": cpu[1], "lr": 3e-4}], lr=1e-3)
    g = torch.Generator().manual_seed(3)
    for p in cpu[0] + cpu[1]:
        p.grad = torch.randn(p.shape, generator=g)
    t.step()
    t.step()
    opt.load_state_dict(t.state_dict())
    assert opt._gsteps == [2, 2]
    assert [g["lr"] for g in opt.param_groups] == [1e-3, 3e-4] and all(g["decoupled_weight_decay"] for g in opt.param_groups)
    at = {id(p): (o, n) for (p, o, n, _) in m.engine().items}
    for grp, cgrp in zip(opt.param_groups, cpu):
        for p, q in zip(grp["params"], cgrp):
            o, n = at[id(p)]
            assert torch.equal(opt._m[o: o + n].cpu(), t.state[q]["exp_avg"].reshape(-1))
            assert torch.equal(opt._v[o: o + n].cpu(), t.state[q]["exp_avg_sq"].reshape(-1))
    m.train_step(*_batch())
    opt.step()                                                  # and steps on from there
    assert opt._gsteps == [3, 3]
    back = opt.state_dict()
    t.load_state_dict(_through_a_file(back, "cpu"))             # ... and back into torch's
    assert float(t.state[cpu[0][0]]["step"]) == 3.0


# ---- 13. the drop-in driver ------------------------------------------------------------------------------------------------------------
def _dataset(n_dia, d_t, d_a, seed):
    import pandas as pd
    import dataset as ds
    g = np.random.default_rng(seed)
    rows = [(f"utt {d}-{u}", list(ds.EMOTIONS)[int(g.integers(0, 7))], d, u) for d in range(n_dia) for u in range(int(g.integers(1, 10)))]
    table = pd.DataFrame(rows, columns=["Utterance", "Emotion", "Dialogue_ID", "Utterance_ID"])
    text = torch.from_numpy(g.standard_normal((len(rows), d_t)).astype(np.float32))
    audio = torch.from_numpy(g.standard_normal((len(rows), d_a)).astype(np.float32))
    lab = table["Emotion"].map(ds.EMOTIONS).to_numpy()
    text[np.arange(len(rows)), lab] += 3.0
    return ds.Dataset("train", text_embeddings=text, audio_embeddings=audio, table=table)


def test_training_loop_with_runtime_optimizer_block(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "src"))
    monkeypatch.chdir(ROOT)
    import dataset as ds
    import train as tr
    from utils import AttrDict, get_config
    cfg = AttrDict(dict(get_config()))
    cfg.model = AttrDict(synth._cfg(40, 48, 64, 4, 4, 4, 1, 1, 1, dropout=0.1))
    cfg.runtime = AttrDict(dict(cfg.runtime, optimizer={"name": "adamw", "no_decay_1d": True, "frozen": ["audio_encoders"]}))
    cfg.solver = AttrDict(dict(cfg.solver, epochs=2, lr=2e-3, weight_decay=0.01,
                               early_stopping=AttrDict(enabled=False, patience=2, restore_best_weights=False),
                               scheduler=AttrDict(enabled=True, scheduler_fn="ExponentialLR", gamma=0.9)))
    cfg.checkpoint = AttrDict(save_path=str(tmp_path / "ck" / "m2fnet.pth"), load_path=str(tmp_path / "ck" / "m2fnet.pth"),
                              save_checkpoint=True, load_checkpoint=True)
    dl_train = torch.utils.data.DataLoader(_dataset(40, 48, 40, 1), collate_fn=ds.collate_fn, batch_size=8, shuffle=True)
    dl_val = torch.utils.data.DataLoader(_dataset(12, 48, 40, 2), collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = tr.M2FNet(cfg.model).to(device)
    start = {n: p.detach().clone() for n, p in model.named_parameters()}
    crit = tr.M2FCrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    opt = tr.build_optimizer(cfg, model)
    assert isinstance(opt, FusedAdamW) and len(opt.param_groups) == 2
    sched = tr.build_scheduler(cfg.solver, opt)
    out = tr.training_loop(model, dl_train, dl_val, crit, opt, sched, 0, cfg, device)
    losses = out["loss_values"]
    assert len(losses) == 2 and losses[1] < losses[0], losses
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        assert torch.equal(p, start[n]) == n.startswith("audio_encoders"), n       # frozen: unchanged; everything else moved
    assert [g["lr"] for g in opt.param_groups] == [pytest.approx(2e-3 * 0.81)] * 2    # ExponentialLR scales every group
    steps = opt._gsteps
    assert steps[0] == steps[1] == 2 * len(dl_train)
    # the checkpoint resumes: same groups, counts and moments
    model2 = tr.M2FNet(cfg.model).to(device)
    opt2 = tr.build_optimizer(cfg, model2)
    assert tr.resume_if_requested(cfg, model2, opt2, device) == 2
    assert opt2._gsteps == steps
    for (n, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(p, q), n
    opt._bind()
    assert torch.equal(opt2._m, opt._m) and torch.equal(opt2._v, opt._v)
    audio_mask = _element_mask(model2, [p for n, p in model2.named_parameters() if n.startswith("audio_encoders")])
    assert not bool(opt2._m[audio_mask].any())
    l2 = tr.train(model2, dl_train, crit, opt2, 2, False, device)
    assert np.isfinite(l2) and opt2._gsteps[0] == 3 * len(dl_train)
