"""Gradient clipping by global L2 norm on the device (FusedAdam(max_grad_norm=...), csrc/gradnorm.hip): the norm of the gradient
buffer the optimizer reads - fp32, bf16, accumulated - reduced in float64 by two launches, and torch.nn.utils.clip_grad_norm_'s
coefficient folded into the divisor the Adam kernels already apply.

Reference values: torch on the CPU in float64 (clip_grad_norm_, torch.optim.Adam) and its restatement tests/golden/grad_clip_ref.py.
Bounds: the published norm is one rounding to fp32 (2^-24) of a float64 sum whose own error is orders below that - 2^-23 relative;
coef and divisor are the float64 formulas of the published inputs rounded once - one fp32 ulp; everything that compares two device
runs is bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import grad_clip_ref as ref  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402
from mer_amd import layout, runtime  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam  # noqa: E402

CFG = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2)          # dropout 0
WIDE = synth.CASES["c2_slice"][0]                        # C2 widths (300 / 768 / 768), depth 2: thousands of slices, odd tensor tails
REL_NORM = 2.0 ** -23


def _model(cfg=CFG, precision="fp32"):
    m = M2FNet(cfg, precision=precision)
    m.load_state_dict(synth.make_state_dict(cfg))
    return m.to("cuda").train()


def _batch(cfg=CFG, B=8, L=16, seed=1):
    g = torch.Generator().manual_seed(seed)
    lengths = [L] + [int(x) for x in torch.randint(1, L + 1, (B - 1,), generator=g)]
    return [t.cuda() for t in synth.make_inputs(cfg, B, L, lengths, "randn", seed=seed)]


def _items(m):
    return [(o, n) for (_, o, n, _) in m.engine().items]


def _read_buffer(m):
    """The buffer FusedAdam.step reads: the bf16 gradients of set_grad_bf16, else the fp32 flat gradient buffer."""
    eng = m.engine()
    return eng.grad_bf16_buf if eng.grad_bf16_buf is not None else eng.ensure_grad()


def _ref_norm(buf, items, den=1.0):
    return ref.norm(ref.tensors_of(buf.detach().cpu(), items), den)


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def _record(opt):
    torch.cuda.synchronize()
    return [float(x) for x in opt._clip_record.cpu()]


def _pad_mask(total, items):
    pad = torch.ones(total, dtype=torch.bool)
    for o, n in items:
        pad[o: o + n] = False
    return pad


def _spread_buffer(cfg, dtype, seed=5):
    """A bare flat buffer of cfg's layout: values spread over twelve decades, element by element."""
    c = layout.M2FConfig.from_model_config(cfg)
    specs, total = layout.param_specs(c)
    items = [(s.offset, s.numel) for s in specs if not s.alias_of]
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(total, generator=g) * torch.pow(10.0, torch.rand(total, generator=g) * 12.0 - 8.0)
    return c, buf.to(dtype).cuda(), items


# ---- 1. the norm's value --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fp32", "bf16_grads", "fp32_wide", "bf16_grads_wide"])
def test_norm_of_the_gradients_the_optimizer_read(case):
    cfg = WIDE if case.endswith("wide") else CFG
    m = _model(cfg, "bf16" if case.startswith("bf16") else "fp32")
    if case.startswith("bf16"):
        assert m.set_grad_bf16(True)
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, max_grad_norm=1e-3)
    m.train_step(*_batch(cfg))
    torch.cuda.synchronize()
    buf = _read_buffer(m)
    assert buf.dtype == (torch.bfloat16 if case.startswith("bf16") else torch.float32)
    want = _ref_norm(buf, _items(m))
    opt.step()
    got = float(opt.grad_norm())
    rel = abs(got - want) / want
    print(f"grad_norm {case}: device {got!r} float64 {want!r} relative error {rel:.3e}")
    assert want > 0 and rel <= REL_NORM
    assert float(opt.clip_coef()) < 1.0
    assert opt.grad_norm().is_cuda and opt.clip_coef().is_cuda


def test_norm_of_an_accumulation_group_is_divided_by_its_den():
    m = _model()
    m.set_grad_accumulation(True)
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, max_grad_norm=1e-3)
    opt.zero_grad()
    for seed in (1, 2):
        m.train_step(*_batch(seed=seed), normalise=False)
    terms = m.loss_terms()
    opt.grad_scale = terms[1:2]
    torch.cuda.synchronize()
    den = float(terms[1])
    assert den > 1.0
    want = _ref_norm(_read_buffer(m), _items(m), den)
    opt.step()
    norm, coef, div, root = _record(opt)
    rel = abs(norm - want) / want
    print(f"grad_norm of a two-micro-batch group: device {norm!r} float64 {want!r} den {den} relative error {rel:.3e}")
    assert rel <= REL_NORM
    assert abs(root - want * den) / (want * den) <= REL_NORM
    assert coef < 1.0 and abs(div - ref.divisor(den, coef)) <= _ulp(ref.divisor(den, coef))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_norm_of_a_bare_buffer_spread_over_many_decades(dtype):
    c, buf, items = _spread_buffer(WIDE, dtype)
    den = torch.tensor([3.0], device="cuda")
    for d in (None, den):
        rec = F.grad_norm(c, buf, 1.0, den=d).cpu()
        want = _ref_norm(buf, items, 1.0 if d is None else 3.0)
        rel = abs(float(rec[0]) - want) / want
        print(f"bare {dtype} buffer, den {d is not None}: device {float(rec[0])!r} float64 {want!r} relative error {rel:.3e}")
        assert rel <= REL_NORM


# ---- 2. pads do not count -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pads_between_tensors_do_not_count(precision):
    for cfg in (CFG, WIDE):
        m = _model(cfg, precision)
        if precision == "bf16":
            assert m.set_grad_bf16(True)
        m.train_step(*_batch(cfg))
        torch.cuda.synchronize()
        buf = _read_buffer(m).detach().clone()
        c = m.engine().cfg
        clean = F.grad_norm(c, buf, 0.5).cpu()
        pad = _pad_mask(buf.numel(), _items(m)).cuda()
        assert int(pad.sum()) > 0
        buf[pad] = 1e6
        dirty = F.grad_norm(c, buf, 0.5).cpu()
        assert torch.equal(clean, dirty), (clean, dirty)
        assert float(clean[0]) < 1e3


# ---- 3. reproducible ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_same_bits_on_every_call_and_for_every_grid(dtype):
    c, buf, _ = _spread_buffer(WIDE, dtype, seed=9)
    first = F.grad_norm(c, buf, 1.0).cpu()
    for grid, nt in ((0, None), (0, None), (1, False), (7, True), (333, False), (2048, True), (100000, False)):
        again = F.grad_norm(c, buf, 1.0, grid=grid, nontemporal=nt).cpu()
        assert torch.equal(first, again), (grid, nt, first, again)
    # the partials themselves, slice by slice
    a, b = runtime.grad_norm_scratch(c, "cuda"), runtime.grad_norm_scratch(c, "cuda")
    runtime.grad_sumsq(c, buf, a)
    runtime.grad_sumsq(c, buf, b, grid=13, nontemporal=True)
    assert a.numel() > 2048 and torch.equal(a, b)


# ---- 4. no clip = no change -----------------------------------------------------------------------------------------------------
def _state(m, opt):
    torch.cuda.synchronize()
    eng = m.engine()
    out = {"p": eng.flat.detach().clone(), "m": opt._m.clone(), "v": opt._v.clone()}
    if eng.wshadow is not None:
        out["sh"] = eng.wshadow[: eng.wshadow.numel() - 32 * 1024].clone()      # (behind the shadows: the optimizer's tensor table)
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16_grads"])
def test_a_norm_below_max_grad_norm_changes_nothing(mode):
    precision = "fp32" if mode == "fp32" else "bf16"
    pair = []
    for max_norm in (1e9, None):
        m = _model(CFG, precision)
        if mode == "bf16_grads":
            assert m.set_grad_bf16(True)
        pair.append((m, FusedAdam(m, lr=1e-3, weight_decay=0.01, max_grad_norm=max_norm)))
    for i in range(3):
        for m, opt in pair:
            opt.zero_grad()
            m.train_step(*_batch(seed=1 + i))
            opt.step()
    (m_clip, o_clip), (m_ref, o_ref) = pair
    _same(_state(m_clip, o_clip), _state(m_ref, o_ref))
    assert (precision == "bf16") == ("sh" in _state(m_clip, o_clip))
    assert m_clip.engine().shadows_fresh() == m_ref.engine().shadows_fresh()
    norm, coef, div, _ = _record(o_clip)
    assert coef == 1.0 and div == 1.0 and 0.0 < norm < 1e9
    with pytest.raises(RuntimeError, match="no step has clipped"):
        o_ref.grad_norm()


def test_no_clip_keeps_the_bits_of_den():
    pair = []
    for max_norm in (1e9, None):
        m = _model()
        pair.append((m, FusedAdam(m, lr=1e-3, weight_decay=0.01, max_grad_norm=max_norm)))
    for m, opt in pair:
        m.train_step(*_batch(), normalise=False)
        opt.grad_scale = m.loss_terms()[1:2]
        opt.step()
    (m_clip, o_clip), (m_ref, o_ref) = pair
    _same(_state(m_clip, o_clip), _state(m_ref, o_ref))
    assert torch.equal(o_clip._clip_record[2:3], m_clip.loss_terms()[1:2])


# ---- 5. clip = the step with the published divisor, exactly -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16_grads", "fp32_den"])
def test_a_clipped_step_is_the_step_scaled_by_the_published_divisor(mode):
    precision = "fp32" if mode.startswith("fp32") else "bf16"
    with_den = mode == "fp32_den"
    models = [_model(CFG, precision) for _ in range(2)]
    if mode == "bf16_grads":
        for m in models:
            assert m.set_grad_bf16(True)
    (m_clip, m_twin) = models
    max_norm = 0.01
    o_clip = FusedAdam(m_clip, lr=1e-3, weight_decay=0.01, max_grad_norm=max_norm)
    o_twin = FusedAdam(m_twin, lr=1e-3, weight_decay=0.01)
    for i in range(3):
        b = _batch(seed=1 + i)
        m_clip.train_step(*b, normalise=not with_den)
        m_twin.train_step(*b, normalise=not with_den)
        if with_den:
            o_clip.grad_scale = m_clip.loss_terms()[1:2]
        o_clip.step()
        norm, coef, div, _ = _record(o_clip)
        den = float(m_clip.loss_terms()[1]) if with_den else 1.0
        # the formulas in float64 from the published inputs, one fp32 ulp
        want_coef = ref.coef(norm, max_norm)
        want_div = ref.divisor(den, coef)
        print(f"{mode} step {i}: norm {norm!r} coef {coef!r} (float64 {want_coef!r}) divisor {div!r} (float64 {want_div!r})")
        assert coef < 1.0, "max_grad_norm must be below the norm in this test"
        assert abs(coef - want_coef) <= _ulp(want_coef)
        assert abs(div - want_div) <= _ulp(want_div)
        o_twin.grad_scale = o_clip._clip_record[2:3].clone()
        o_twin.step()
        _same(_state(m_clip, o_clip), _state(m_twin, o_twin))


# ---- 6. against torch -------------------------------------------------------------------------------------------------------------
def _torch_step(start, grads, max_norm, lr, wd):
    """clip_grad_norm_ then one torch.optim.Adam step (coupled weight decay, as the reference builds it) in float64 on the CPU."""
    params = [torch.nn.Parameter(p.double().clone()) for p in start]
    for p, g in zip(params, grads):
        p.grad = g.double().clone()
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(params, max_norm)
    torch.optim.Adam(params, lr=lr, weight_decay=wd).step()
    return [p.detach() for p in params]


def _cat(ts):
    return torch.cat([t.reshape(-1).double() for t in ts])


def test_clipped_step_against_torch_clip_grad_norm_and_adam():
    stats = {}
    for name, max_norm in (("unclipped", None), ("clipped", 0.02)):
        m = _model()
        opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, max_grad_norm=max_norm)
        m.train_step(*_batch())
        torch.cuda.synchronize()
        start = [p.detach().cpu().clone() for p in m.parameters()]
        grads = [p.grad.detach().cpu().clone() for p in m.parameters()]
        opt.step()
        torch.cuda.synchronize()
        got = _cat([p.detach().cpu() for p in m.parameters()])
        want = _cat(_torch_step(start, grads, max_norm, 1e-3, 0.01))
        stats[name] = float((got - want).norm() / (want - _cat(start)).norm())
        if max_norm is not None:
            assert float(opt.clip_coef()) < 1.0
            assert abs(float(opt.grad_norm()) - ref.norm(grads)) / ref.norm(grads) <= REL_NORM
    print(f"deviation from torch relative to the update's norm: unclipped {stats['unclipped']:.3e} clipped {stats['clipped']:.3e}")
    assert stats["unclipped"] < 1e-4 and stats["clipped"] < 1e-4, stats


# ---- 7. the fused path falls back ---------------------------------------------------------------------------------------------------
def test_train_step_with_optimizer_takes_the_two_launch_path_when_clipping():
    cfg, B, L, lengths, kind = synth.CASES["tiny_ragged"]
    batch = [t.cuda() for t in synth.make_inputs(cfg, B, L, lengths, kind)]
    runs = []
    for inside in (True, False):
        m = _model(cfg, "bf16")
        opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, max_grad_norm=0.01)
        losses = []
        for i in range(3):
            if inside:
                losses.append(float(m.train_step(*batch, use_graph=i > 0, optimizer=opt)))
            else:
                losses.append(float(m.train_step(*batch, use_graph=i > 0)))
                opt.step()
        plan = next(p for p in m.engine().plans.values() if p.train)
        assert opt.prepare_fused(plan) is False
        assert getattr(plan, "_fused_key", None) is None       # never armed
        assert float(opt.clip_coef()) < 1.0
        runs.append((losses, _state(m, opt), _record(opt)))
    assert runs[0][0] == runs[1][0]
    _same(runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2]
    # without clipping the same model still arms the in-launch optimizer
    m = _model(cfg, "bf16")
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01)
    m.train_step(*batch, optimizer=opt)
    plan = next(p for p in m.engine().plans.values() if p.train)
    assert getattr(plan, "_fused_key", None) is not None, getattr(plan, "_fused_err", None)
    assert opt.prepare_fused(plan) is True
    opt.finish_fused(plan)
    # ... and switching clipping on between steps leaves that path at once
    opt.max_grad_norm = 0.01
    assert opt.prepare_fused(plan) is False


def test_max_grad_norm_is_a_plain_attribute_checked_at_the_step():
    m = _model()
    opt = FusedAdam(m, lr=1e-3, max_grad_norm=0.01)
    m.train_step(*_batch())
    opt.step()
    assert float(opt.clip_coef()) < 1.0
    opt.max_grad_norm = None
    m.train_step(*_batch())
    opt.step()                                               # today's path; the record keeps the last clipping step's values
    for bad in (0.0, -1.0, float("nan")):
        opt.max_grad_norm = bad
        with pytest.raises(ValueError, match="positive"):
            opt.step()
    assert "max_grad_norm" not in opt.state_dict()["param_groups"][0]


# ---- 8. drop-in -----------------------------------------------------------------------------------------------------------------
def _dataset(n_dia, d_t, d_a, seed):
    import pandas as pd
    import dataset as ds
    g = np.random.default_rng(seed)
    rows = [(f"utt {d}-{u}", list(ds.EMOTIONS)[int(g.integers(0, 7))], d, u) for d in range(n_dia) for u in range(int(g.integers(1, 10)))]
    table = pd.DataFrame(rows, columns=["Utterance", "Emotion", "Dialogue_ID", "Utterance_ID"])
    text = torch.from_numpy(g.standard_normal((len(rows), d_t)).astype(np.float32))
    audio = torch.from_numpy(g.standard_normal((len(rows), d_a)).astype(np.float32))
    return ds.Dataset("train", text_embeddings=text, audio_embeddings=audio, table=table)


def test_train_loop_with_clip_grad_norm_equals_hand_loop(monkeypatch):
    """src/train.py::train for one epoch with runtime.clip_grad_norm set the way main() sets it, against a hand-written loop that uses
    the API directly: the same parameters bit for bit, and every step clipped."""
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    sys.path.insert(0, os.path.join(root, "src"))
    monkeypatch.chdir(root)
    import dataset as ds
    import train as tr
    from utils import AttrDict
    cfg = AttrDict(runtime=AttrDict(clip_grad_norm=0.05))
    max_norm = tr.clip_grad_norm(cfg, 1)
    assert max_norm == 0.05
    model_cfg = AttrDict(synth._cfg(40, 48, 64, 4, 4, 4, 1, 1, 1))
    dl = torch.utils.data.DataLoader(_dataset(28, 48, 40, 1), collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    device = torch.device("cuda:0")
    crit = tr.M2FCrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    models = []
    for _ in range(2):
        torch.manual_seed(0)
        models.append(tr.M2FNet(model_cfg).to(device))
    m_loop, m_hand = models
    o_loop = tr.FusedAdam(m_loop, lr=2e-3, weight_decay=0.01)
    o_loop.max_grad_norm = max_norm                          # main(): optimizer.max_grad_norm = clip_grad_norm(config, world)
    mean = tr.train(m_loop, dl, crit, o_loop, 0, False, device)
    o_hand = tr.FusedAdam(m_hand, lr=2e-3, weight_decay=0.01, max_grad_norm=0.05)
    m_hand.train()
    losses, coefs = [], []
    for batch in dl:
        text, audio, emotion, pad = tr.move_batch(batch, device)
        o_hand.zero_grad()
        losses.append(m_hand.train_step(text, audio, pad, emotion, label_smoothing=0.1).item())
        o_hand.step()
        coefs.append(float(o_hand.clip_coef()))
    torch.cuda.synchronize()
    assert max(coefs) < 1.0, coefs
    for (n, p), (_, q) in zip(m_loop.named_parameters(), m_hand.named_parameters()):
        assert torch.equal(p, q), n
    assert abs(mean - sum(losses) / len(losses)) < 1e-6
    assert torch.equal(o_loop.grad_norm(), o_hand.grad_norm())
    assert tr._grad_norm_log(o_loop) == {"Train/Grad_norm": float(o_hand.grad_norm())}
    o_loop.max_grad_norm = None
    assert tr._grad_norm_log(o_loop) == {}
