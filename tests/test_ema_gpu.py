"""The exponential moving average of the weights inside the optimizer kernels (FusedAdam(ema_decay=...); csrc/adam.hip: the EMA
forms of the flat, shadow-writing, grouped and slice kernels, ema4, the exchange kernel).

What is compared against what:
  * tests/golden/ema_ref.py - the rule in float64, from the exact fp32 parameters read back after every step, element by element
    within 8 k 2^-24 M (k updates, M the largest magnitude the element's parameter took; derivation in ema_ref.py, pinned to torch's
    AveragedModel in tests/test_ema_cpu.py);
  * the optimizer without ema_decay - BIT FOR BIT: parameters, moments and shadows do not know the average exists;
  * the forms against each other - bit for bit: step() / step_ranges() over whole tensors and over cut ranges, single group / grouped,
    fp32 / bf16 gradient input;
  * a second model that loaded ema_state_dict()["parameters"] - bit for bit: logits and scores inside averaged_parameters();
  * nothing at all: a tensor of no group keeps every bit of its parameter, its shadows and its EMA slice."""
import io
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

import ema_ref as ref  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import dp  # noqa: E402
from mer_amd.metrics import DeviceScores  # noqa: E402
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


def _state(m, opt, ema=True):
    torch.cuda.synchronize()
    eng = m.engine()
    out = {"p": eng.flat.detach().clone(), "m": opt._m.clone(), "v": opt._v.clone()}
    if eng.wshadow is not None:
        out["sh"] = eng.wshadow[: eng.wshadow.numel() - TABLE].clone()
    if ema and opt._ema is not None:
        out["ema"] = opt.ema_parameters().clone()
    return out


def _same(a, b, what=""):
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


def _element_mask(m, params):
    eng = m.engine()
    ids = {id(p) for p in params}
    mask = torch.zeros(eng.flat.numel(), dtype=torch.bool, device="cuda")
    for (p, o, n, _) in eng.items:
        if id(p) in ids:
            mask[o: o + n] = True
    return mask


def _check_rule(avg, m, opt, what, mask=None):
    """One more update of the float64 average from the parameters as they are now, then the optimizer's buffer against it."""
    torch.cuda.synchronize()
    avg.step(m.engine().flat.detach(), mask)
    ratio = avg.error_ratio(opt.ema_parameters())
    print(f"{what}: update {avg.n}: largest |ema - float64 rule| / (8 k 2^-24 M) = {ratio:.4f}")
    assert opt.n_averaged == avg.n
    assert ratio <= 1.0, (what, avg.n, ratio)


def _eval_logits(m, batch):
    was = m.training
    m.eval()
    with torch.inference_mode():
        out = m(batch[0], batch[1], batch[2]).clone()
    m.train(was)
    return out


def _through_a_file(obj, device="cuda:0"):
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return torch.load(buf, map_location=device)


# ---- 1. the rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay,warmup", [(0.9, False), (0.999, True)])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_average_follows_the_rule(precision, decay, warmup):
    m = _model(TINY, precision)
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, ema_decay=decay, ema_warmup=warmup)
    avg = ref.Average(decay, warmup)
    real = _element_mask(m, list(m.parameters()))
    assert bool((~real).any())
    for i in range(8):
        m.train_step(*_batch(seed=1 + i))
        opt.step()
        _check_rule(avg, m, opt, f"{precision} decay {decay} warmup {warmup}")
        ema = opt.ema_parameters()
        assert not bool(ema[~real].any())                                    # the pads between tensors: still zero
        if i == 0:
            assert torch.equal(ema, m.engine().flat)                         # update 0 copies, bit for bit
        else:
            assert not torch.equal(ema, m.engine().flat)
    assert opt.n_averaged == 8


def test_decay_may_change_and_none_stops_updating():
    m = _model()
    opt = FusedAdam(m, lr=1e-3, ema_decay=0.5)
    avg = ref.Average(0.5)
    for i in range(2):
        m.train_step(*_batch(seed=1 + i))
        opt.step()
        _check_rule(avg, m, opt, "decay 0.5")
    opt.ema_decay = None
    kept = opt.ema_parameters().clone()
    m.train_step(*_batch(seed=3))
    opt.step()
    torch.cuda.synchronize()
    assert opt.n_averaged == 2 and torch.equal(opt.ema_parameters(), kept)   # the buffer is kept, not updated
    opt.ema_decay = avg.decay = 0.25
    m.train_step(*_batch(seed=4))
    opt.step()
    _check_rule(avg, m, opt, "decay 0.25")
    opt.ema_decay = 1.5
    with pytest.raises(ValueError, match="ema_decay"):
        opt.step()


# ---- 2. no side effect ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16_grads", "fp32_grouped", "bf16_grouped"])
def test_parameters_moments_and_shadows_do_not_know_the_average(mode):
    precision = "fp32" if mode.startswith("fp32") else "bf16"
    runs = []
    for decay in (0.9, None):
        m = _model(TINY, precision)
        if mode == "bf16_grads":
            assert m.set_grad_bf16(True)
        if mode.endswith("grouped"):
            enc, rest = (lambda named: ([p for n, p in named if n.startswith(ENCODERS)], [p for n, p in named if not n.startswith(ENCODERS)]))(
                list(m.named_parameters()))
            opt = FusedAdamW(m, lr=1e-3, params=[{"params": enc, "weight_decay": 0.1}, {"params": rest, "lr": 5e-4}], ema_decay=decay)
        else:
            opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, ema_decay=decay)
        losses = []
        for i in range(4):
            losses.append(float(m.train_step(*_batch(seed=1 + i), use_graph=i > 0)))
            opt.step()
        runs.append((losses, _state(m, opt, ema=False), m.engine().shadows_fresh(), opt.n_averaged))
    assert runs[0][0] == runs[1][0]
    _same(runs[0][1], runs[1][1], mode)
    assert runs[0][2] == runs[1][2] == (precision == "bf16")
    assert (runs[0][3], runs[1][3]) == (4, 0)


# ---- 3. one result from every form ------------------------------------------------------------------------------------------------------
def _buckets(m, n_buckets=3):
    eng = m.engine()
    n = eng.flat.numel()
    eng.ensure_grad()
    red = dp.GradReducer(eng.flat_grad_ext, n, n_buckets=n_buckets)
    red.align_to(o for (_, o, _, _) in eng.items)
    ranges = list(red.param_chunks)
    assert len(ranges) == n_buckets and ranges[0][0] == 0 and ranges[-1][1] == n
    return ranges


def _cuts(m):
    """Ranges that cut tensors at multiples of 4 (and are not tensor-aligned)."""
    eng = m.engine()
    n = eng.flat.numel()
    starts = {o for (_, o, _, _) in eng.items}
    big = [o for (_, o, numel, _) in eng.items if numel > 256]
    a, b = big[1] + 36, big[len(big) // 2] + 132
    assert a % 4 == 0 and b % 4 == 0 and a not in starts and b not in starts and 0 < a < b < n
    return [(0, a), (a, b), (b, n)]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_every_form_gives_the_same_average(precision):
    forms = ["step", "ranges_aligned", "ranges_cut", "grouped", "grouped_ranges"]
    results = {}
    for form in forms:
        m = _model(TINY, precision)
        if form.startswith("grouped"):
            opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, params=[{"params": list(m.parameters())}], ema_decay=0.9, ema_warmup=True)
            assert opt._grouped
        else:
            opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, ema_decay=0.9, ema_warmup=True)
        ranges = {"ranges_aligned": _buckets, "grouped_ranges": _buckets, "ranges_cut": _cuts}.get(form, lambda _m: None)(m)
        for i in range(3):
            m.train_step(*_batch(seed=1 + i))
            if ranges is None:
                opt.step()
            else:
                seen = []
                opt.step_ranges(ranges, before_each=seen.append)
                assert seen == [0, 1, 2]
        st = _state(m, opt)
        st.pop("sh", None)                                                   # (cut ranges leave the shadows to the next forward)
        results[form] = st
        assert opt.n_averaged == 3
    for form in forms[1:]:
        _same(results["step"], results[form], (precision, form))
    assert not torch.equal(results["step"]["ema"], results["step"]["p"])


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_bf16_gradient_input_gives_the_average_of_the_fp32_input(precision, grouped):
    """The G16 forms fed bf16 gradients against the fp32 forms fed the same values (exactly representable in bf16)."""
    runs = []
    for g16 in (False, True):
        m = _model(TINY, precision)
        kw = {"params": [{"params": list(m.parameters())}]} if grouped else {}
        opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, ema_decay=0.75, **kw)
        for i in range(3):
            m.train_step(*_batch(seed=1 + i))
            fg = m.engine().flat_grad
            rounded = fg.to(torch.bfloat16)
            if g16:
                opt.grads_bf16 = rounded
            else:
                fg.copy_(rounded.float())
            opt.step()
        runs.append(_state(m, opt))
    _same(runs[0], runs[1], (precision, grouped))
    assert "ema" in runs[0]


# ---- 4. groups, and tensors of no group ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_groups_are_averaged_and_unowned_tensors_keep_every_bit(precision):
    m = _model(TINY, precision)
    named = list(m.named_parameters())
    text = [p for n, p in named if n.startswith("text_encoders")]
    audio = [p for n, p in named if n.startswith("audio_encoders")]           # in NO group
    rest = [p for n, p in named if not n.startswith(ENCODERS)]
    opt = FusedAdamW(m, lr=1e-3, params=[{"params": text, "weight_decay": 0.1}, {"params": rest, "lr": 4e-4, "weight_decay": 0.0}],
                     ema_decay=0.9)
    owned, unowned = _element_mask(m, text + rest), _element_mask(m, audio)
    assert bool(owned.any()) and bool(unowned.any())
    avg = ref.Average(0.9)
    m.train_step(*_batch(seed=1))
    opt.step()
    _check_rule(avg, m, opt, f"{precision} groups", owned)
    assert not bool(opt.ema_parameters()[unowned].any())                     # never written: the zeros it was allocated with
    opt.ema_parameters()[unowned] = 0.125                                    # a sentinel: an unowned slice must not even be read
    avg.value[unowned] = 0.125
    before = _state(m, opt)
    for i in range(1, 5):
        m.train_step(*_batch(seed=1 + i))
        opt.step()
        _check_rule(avg, m, opt, f"{precision} groups", owned)
    after = _state(m, opt)
    for k in ("p", "ema"):
        assert torch.equal(before[k][unowned], after[k][unowned]), k
        assert not torch.equal(before[k][owned], after[k][owned]), k
    assert bool((after["ema"][unowned] == 0.125).all())
    assert not bool(after["ema"][~(owned | unowned)].any())                  # pads
    if precision == "bf16":
        assert m.engine().shadows_fresh()
    # a round trip through averaged_parameters(): the exchange skips the unowned tensors and the pads
    b = _batch(seed=9)
    logits = _eval_logits(m, b)
    with opt.averaged_parameters():
        torch.cuda.synchronize()
        inside = m.engine().flat.detach().clone()
        assert torch.equal(inside[owned], after["ema"][owned])
        assert torch.equal(inside[unowned], after["p"][unowned])
        assert torch.equal(opt._ema[owned], after["p"][owned]) and bool((opt._ema[unowned] == 0.125).all())
        assert not m.engine().shadows_fresh()
        inside_logits = _eval_logits(m, b)
    assert not torch.equal(inside_logits, logits)
    assert not m.engine().shadows_fresh()
    assert torch.equal(_eval_logits(m, b), logits)                           # re-cast shadows of restored parameters
    _same(_state(m, opt), after, "round trip")                               # parameters, shadows (re-cast), the average: every bit


def test_a_group_added_later_starts_its_average_from_the_parameters():
    m = _model()
    named = list(m.named_parameters())
    enc = [p for n, p in named if n.startswith(ENCODERS)]
    rest = [p for n, p in named if not n.startswith(ENCODERS)]
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, params=rest, ema_decay=0.9)
    late = _element_mask(m, enc)
    for i in range(2):
        m.train_step(*_batch(seed=1 + i))
        opt.step()
    torch.cuda.synchronize()
    assert not bool(opt.ema_parameters()[late].any())                        # unowned so far: never written
    opt.add_param_group({"params": enc, "lr": 5e-4})
    torch.cuda.synchronize()
    p_old = m.engine().flat.detach().clone()
    assert torch.equal(opt.ema_parameters()[late], p_old[late])              # seeded: the copy a first update makes
    m.train_step(*_batch(seed=3))
    opt.step()
    torch.cuda.synchronize()
    p_new = m.engine().flat.detach()
    assert not torch.equal(p_new[late], p_old[late])
    want = ref.update(p_old.double(), p_new, 0.9, 2)[late]                   # update 2 (from 0) of a slice that held p_old
    mag = torch.maximum(p_old.abs(), p_new.abs()).double()[late]
    err = (opt.ema_parameters()[late].double() - want).abs()
    assert bool((err <= ref.bound(1, mag)).all()), float((err / ref.bound(1, mag).clamp_min(1e-300)).max())
    with opt.averaged_parameters():
        with pytest.raises(RuntimeError, match="averaged_parameters"):
            opt.add_param_group({"params": []})


# ---- 5. evaluation with the average ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_evaluation_inside_averaged_parameters(precision):
    pair = []
    for _ in range(2):
        m = _model(TINY, precision)
        pair.append((m, FusedAdam(m, lr=2e-3, weight_decay=0.01, ema_decay=0.5)))
    (m, opt), (twin, otwin) = pair
    with pytest.raises(RuntimeError, match="no average yet"):
        with opt.averaged_parameters():
            pass
    for i in range(3):
        for mm, oo in pair:
            mm.train_step(*_batch(seed=1 + i))
            oo.step()
    b = _batch(seed=9)
    before = _state(m, opt)
    logits_before = _eval_logits(m, b)
    with opt.averaged_parameters():
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        esd = opt.ema_state_dict()
        assert list(sd) == list(esd["parameters"]) == list(synth.make_state_dict(TINY))
        for k in sd:
            assert torch.equal(sd[k], esd["parameters"][k]), k
        assert (esd["decay"], esd["warmup"], esd["n_averaged"]) == (0.5, False, 3)
        second = M2FNet(TINY, precision=precision)
        second.load_state_dict(_through_a_file(esd["parameters"], "cpu"))
        second = second.to("cuda:0").eval()
        logits_in = _eval_logits(m, b)
        assert torch.equal(logits_in, _eval_logits(second, b))
        assert not torch.equal(logits_in, logits_before)
        n_cls = m.m2f_config.cls_out
        s1, s2 = DeviceScores(n_cls, torch.device("cuda:0")), DeviceScores(n_cls, torch.device("cuda:0"))
        m.eval()
        with torch.inference_mode():
            m.eval_step(*b, s1)
            second.eval_step(*b, s2)
        m.train()
        assert s1.totals() == s2.totals() and s1.totals()[3] == 1.0
        with pytest.raises(RuntimeError, match="averaged_parameters"):
            opt.step()
        with pytest.raises(RuntimeError, match="averaged_parameters"):
            opt.step_ranges([(0, 64)])
        with pytest.raises(RuntimeError, match="averaged_parameters"):
            opt.prepare_fused(None)
        with pytest.raises(RuntimeError, match="averaged_parameters"):
            with opt.averaged_parameters():
                pass
    # outside the context the same dictionary comes from the optimizer's buffer
    esd_out = opt.ema_state_dict()["parameters"]
    for k in sd:
        assert torch.equal(sd[k], esd_out[k]), k
    after = _state(m, opt)
    before.pop("sh", None)
    after.pop("sh", None)
    _same(before, after, "restored")
    assert torch.equal(_eval_logits(m, b), logits_before)
    for i in range(3, 5):                                                    # training goes on as if the context had never been entered
        for mm, oo in pair:
            mm.train_step(*_batch(seed=1 + i))
            oo.step()
    _same(_state(m, opt), _state(twin, otwin), "continued")
    assert opt.n_averaged == otwin.n_averaged == 5


# ---- 6. checkpoint round trip ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_save_and_resume_is_the_uninterrupted_run(precision):
    def make(m):
        return FusedAdam(m, lr=1e-3, weight_decay=0.01, ema_decay=0.99, ema_warmup=True)
    whole = _model(TINY, precision)
    o_whole = make(whole)
    for i in range(6):
        whole.train_step(*_batch(seed=1 + i))
        o_whole.step()
    part = _model(TINY, precision)
    o_part = make(part)
    for i in range(2):
        part.train_step(*_batch(seed=1 + i))
        o_part.step()
    ck = _through_a_file({"model": part.state_dict(), "opt": o_part.state_dict(), "ema": o_part.ema_state_dict()})
    assert set(ck["ema"]) == {"decay", "warmup", "n_averaged", "parameters"}
    assert list(ck["ema"]["parameters"]) == list(ck["model"]) and ck["ema"]["n_averaged"] == 2
    assert all(ck["ema"]["parameters"][k].shape == ck["model"][k].shape for k in ck["model"])
    resumed = M2FNet(TINY, precision=precision).to("cuda:0").train()
    o_res = FusedAdam(resumed, lr=1e-3, weight_decay=0.01)                   # decay and warm-up come from the dictionary
    resumed.load_state_dict(ck["model"])
    o_res.load_state_dict(ck["opt"])
    o_res.load_ema_state_dict(ck["ema"])
    assert (o_res.n_averaged, o_res.ema_decay, o_res.ema_warmup) == (2, 0.99, True)
    assert torch.equal(o_res.ema_parameters(), o_part.ema_parameters())
    for i in range(2, 6):
        resumed.train_step(*_batch(seed=1 + i))
        o_res.step()
    _same(_state(whole, o_whole), _state(resumed, o_res), precision)
    assert o_res.n_averaged == o_whole.n_averaged == 6
    # strict about names and shapes
    bad = dict(ck["ema"], parameters={k: v for k, v in list(ck["ema"]["parameters"].items())[1:]})
    with pytest.raises(KeyError, match="names differ"):
        o_res.load_ema_state_dict(bad)
    k0 = next(iter(ck["ema"]["parameters"]))
    bad = dict(ck["ema"], parameters=dict(ck["ema"]["parameters"], **{k0: ck["ema"]["parameters"][k0].reshape(-1)[:-1]}))
    with pytest.raises(ValueError, match="shape"):
        o_res.load_ema_state_dict(bad)
    # the state dict of the optimizer itself is torch's, as ever
    torch.optim.Adam(list(resumed.parameters())).load_state_dict(_through_a_file(o_res.state_dict(), "cpu"))


# ---- 7. accumulation and clipping ----------------------------------------------------------------------------------------------------------
def test_one_update_per_optimizer_step_under_accumulation():
    m = _model()
    m.set_grad_accumulation(True)
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, ema_decay=0.9)
    avg = ref.Average(0.9)
    for s in range(3):
        opt.zero_grad()
        for j in range(3):
            m.train_step(*_batch(seed=1 + 3 * s + j), normalise=False)
        opt.grad_scale = m.loss_terms()[1:2]
        opt.step()
        assert opt.n_averaged == s + 1
        _check_rule(avg, m, opt, "accumulation k = 3")
    opt.grad_scale = None


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_average_follows_the_clipped_parameters(precision):
    m = _model(TINY, precision)
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, max_grad_norm=0.05, ema_decay=0.9)
    avg = ref.Average(0.9)
    for i in range(4):
        m.train_step(*_batch(seed=1 + i))
        opt.step()
        _check_rule(avg, m, opt, f"{precision} clipped")
    assert float(opt.clip_coef()) < 1.0


# ---- 9. the in-launch optimizer is refused --------------------------------------------------------------------------------------------------
def test_prepare_fused_declines_and_train_step_still_trains_and_averages():
    cfg, B, L, lengths, kind = synth.CASES["tiny_ragged"]
    batch = [t.cuda() for t in synth.make_inputs(cfg, B, L, lengths, kind)]
    m = _model(cfg, "bf16")
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, ema_decay=0.9)
    twin = _model(cfg, "bf16")
    otwin = FusedAdam(twin, lr=1e-3, weight_decay=0.01, ema_decay=0.9)
    avg = ref.Average(0.9)
    losses = []
    for i in range(3):
        losses.append(float(m.train_step(*batch, use_graph=i > 0, optimizer=opt)))
        plan = next(p for p in m.engine().plans.values() if p.train)
        assert opt.prepare_fused(plan) is False and getattr(plan, "_fused_key", None) is None
        _check_rule(avg, m, opt, "train_step(optimizer=)")
        twin.train_step(*batch, use_graph=i > 0)
        otwin.step()
    assert losses[-1] < losses[0]
    _same(_state(m, opt), _state(twin, otwin), "two-launch branch")
    opt.ema_decay = None                                                     # without the average the plan is armed again
    m.train_step(*batch, optimizer=opt)
    assert getattr(plan, "_fused_key", None) is not None, getattr(plan, "_fused_err", None)
