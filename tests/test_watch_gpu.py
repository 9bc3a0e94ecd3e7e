"""The model watch on the device (mer_amd.watch.ModelWatch, csrc/tensor_stats.hip): per-tensor statistics and histograms of the flat
buffers an optimizer step uses.

Reference: the buffer copied to the host, tests/golden/watch_ref.py applied per tensor (float64 fields, torch.histc's rule in fp32).
Bounds: counts, min, max and every histogram count are exact.  sumsq: all terms are non-negative and accumulated in float64, in any
order the result stays within numel * 2^-52 relative of the float64 reference.  sum: absolute error at most numel * 2^-52 * sum(|x|).
Fields read() derives (l2 = sqrt(sumsq) / den, mean = sum / finite / den) add a few float64 roundings of 2^-53 each; the tests allow
four (2^-51 relative).  Everything that compares two device runs is byte for byte."""
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import synth  # noqa: E402
import watch_ref as ref  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import layout, runtime  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam, FusedAdamW  # noqa: E402
from mer_amd.watch import ModelWatch  # noqa: E402

CFG = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2)          # dropout 0
WIDE = synth.CASES["c2_slice"][0]                        # C2 widths (300 / 768 / 768), depth 2: thousands of slices, odd tensor tails
EPS = 2.0 ** -52
H, NF = runtime.TSTATS_HEADER, runtime.TSTATS_FIELDS


def _layout(cfg):
    c = layout.M2FConfig.from_model_config(cfg)
    specs, total = layout.param_specs(c)
    return c, [(s.offset, s.numel) for s in specs if not s.alias_of], total


def _pad_mask(total, items):
    pad = torch.ones(total, dtype=torch.bool)
    for o, n in items:
        pad[o: o + n] = False
    return pad


def _collect(c, buf, bins, other=None, den=None, grid=0, nontemporal=None):
    scratch, record = runtime.tensor_stats_buffers(c, bins, buf.device)
    record.fill_(float("nan"))                              # (contents irrelevant before the call)
    runtime.tensor_stats(c, buf, scratch, record, bins, b=other, den=den, grid=grid, nontemporal=nontemporal)
    torch.cuda.synchronize()
    return record.cpu().numpy()


def _rows(rec, n_tensors, bins):
    assert int(rec[1]) == n_tensors and int(rec[2]) == bins and rec.size == H + n_tensors * (NF + bins)
    rows = rec[H:].reshape(n_tensors, NF + bins)
    return rows[:, :NF], rows[:, NF:].view(np.int64)


def _check_rows(what, rows, counts, refs):
    """Record rows against watch_ref, tensor by tensor, at the bounds of the module docstring; prints the worst errors."""
    worst_q = worst_s = 0.0
    for t, r in enumerate(refs):
        row = rows[t]
        assert [int(v) for v in row[:5]] == [r["numel"], r["finite"], r["nan"], r["inf"], r["zeros"]], (what, t, row[:5], r)
        if r["finite"] == 0:
            assert all(math.isnan(v) for v in row[5:9]) and int(counts[t].sum()) == 0, (what, t, row)
            continue
        assert row[5] == r["min"] and row[6] == r["max"], (what, t, row[5:7], r["min"], r["max"])
        eq = abs(row[8] - r["sumsq"]) / r["sumsq"] if r["sumsq"] > 0 else abs(row[8])
        es = abs(row[7] - r["sum"])
        assert eq <= r["numel"] * EPS, (what, t, "sumsq", row[8], r["sumsq"], eq)
        assert es <= r["numel"] * EPS * r["abs_sum"], (what, t, "sum", row[7], r["sum"], es)
        worst_q = max(worst_q, eq / (r["numel"] * EPS))
        worst_s = max(worst_s, es / (r["numel"] * EPS * r["abs_sum"]) if r["abs_sum"] > 0 else 0.0)
        differing = int((torch.from_numpy(counts[t].copy()) != r["hist"]).sum())
        assert differing == 0, (what, t, f"{differing} differing counts", counts[t], r["hist"])
        assert int(counts[t].sum()) == r["finite"]
    print(f"{what}: {len(refs)} tensors; worst sumsq error {worst_q:.3e} of its bound, worst sum error {worst_s:.3e} of its bound; "
          "counts, min, max, histograms exact")


def _wide_buffer(dtype, seed=5):
    """A bare flat buffer of c2_slice's layout: randn times a scale of its own per tensor (1e-6 .. 10), NaN in every pad."""
    c, items, total = _layout(WIDE)
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((total,), float("nan"))
    for i, (o, n) in enumerate(items):
        buf[o: o + n] = torch.randn(n, generator=g) * 10.0 ** (i % 8 - 6)
    assert int(_pad_mask(total, items).sum()) > 0 and len(items) > 50
    return c, buf.to(dtype).cuda(), items


# ---- 1. every tensor of c2_slice ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_every_tensor_of_c2_slice_with_nan_in_the_pads(dtype):
    c, buf, items = _wide_buffer(dtype)
    assert sum((n + 8191) // 8192 for _, n in items) > 2000
    host = buf.cpu()
    for bins in (2, 64, 256):
        rows, counts = _rows(_collect(c, buf, bins), len(items), bins)
        _check_rows(f"c2_slice {dtype} bins {bins}", rows, counts, ref.buffer_stats(host, items, bins))
        assert all(int(r[2]) == 0 for r in rows), "a pad's NaN was read"


# ---- 2. planted values ----------------------------------------------------------------------------------------------------------------
def test_planted_nan_inf_zeros_and_the_special_tensors():
    c, items, total = _layout(CFG)
    g = torch.Generator().manual_seed(7)
    buf = torch.full((total,), float("nan"))
    for o, n in items:
        buf[o: o + n] = torch.randn(n, generator=g) * 0.02
    big = sorted(range(len(items)), key=lambda i: -items[i][1])
    t_nan, t_inf, t_zero, t_const, t_dead, t_dyadic = big[:6]
    small = sorted(range(len(items)), key=lambda i: items[i][1])[0]

    def view(t):
        o, n = items[t]
        return buf[o: o + n]
    view(t_nan)[[0, 5, view(t_nan).numel() - 1]] = float("nan")
    view(t_inf)[[1, 2]] = float("inf")
    view(t_inf)[[3, view(t_inf).numel() - 1]] = float("-inf")
    view(t_inf)[4] = float("nan")
    view(t_zero)[::3] = 0.0
    view(t_zero)[1] = -0.0
    view(t_const)[:] = 0.5
    view(t_dead)[0::2] = float("nan")
    view(t_dead)[1::2] = float("inf")
    view(t_dyadic)[:] = torch.randint(-512, 513, (view(t_dyadic).numel(),), generator=g).float() / 64.0
    dev = buf.cuda()
    for bins in (64, 7):
        rows, counts = _rows(_collect(c, dev, bins), len(items), bins)
        _check_rows(f"planted values, bins {bins}", rows, counts, ref.buffer_stats(buf, items, bins))
        assert [int(v) for v in rows[t_nan][1:4]] == [items[t_nan][1] - 3, 3, 0]
        assert [int(v) for v in rows[t_inf][1:4]] == [items[t_inf][1] - 5, 1, 4]
        assert int(rows[t_zero][4]) == len(range(0, items[t_zero][1], 3)) + 1
        assert int(counts[t_const][bins // 2]) == items[t_const][1] and rows[t_const][5] == rows[t_const][6] == 0.5
        assert int(rows[t_dead][1]) == 0 and int(counts[t_dead].sum()) == 0 and all(math.isnan(v) for v in rows[t_dead][5:9])
        d = view(t_dyadic)
        want = torch.histc(d, bins, min=float(d.min()), max=float(d.max())).to(torch.int64)
        assert torch.equal(torch.from_numpy(counts[t_dyadic].copy()), want), "dyadic-grid tensor against torch.histc"
    # one finite element: the smallest tensor's first element, the rest of it made non-finite
    o, n = items[small]
    buf[o + 1: o + n] = float("nan")
    buf[o] = -3.25
    rows, counts = _rows(_collect(c, buf.cuda(), 64), len(items), 64)
    _check_rows("one finite element", rows, counts, ref.buffer_stats(buf, items, 64))
    assert int(rows[small][1]) == 1 and rows[small][5] == rows[small][6] == rows[small][7] == -3.25 and int(counts[small][32]) == 1


# ---- 3. the difference form -----------------------------------------------------------------------------------------------------------
def test_difference_form_is_a_minus_b_in_fp32():
    c, a, items = _wide_buffer(torch.float32, seed=11)
    g = torch.Generator().manual_seed(12)
    b = (a.cpu() + torch.randn(a.numel(), generator=g) * 1e-3 * a.cpu().abs()).cuda()
    b[_pad_mask(a.numel(), items).cuda()] = float("nan")
    rows, counts = _rows(_collect(c, a, 64, other=b), len(items), 64)
    _check_rows("a - b", rows, counts, ref.buffer_stats(a.cpu(), items, 64, other=b.cpu()))
    with pytest.raises(runtime.HipError, match="fp32"):
        _collect(c, a.bfloat16(), 64, other=b)


# ---- 4. reproducible ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_same_bytes_on_every_call_and_for_every_grid(dtype):
    c, buf, items = _wide_buffer(dtype, seed=9)
    den = torch.tensor([3.0], device="cuda")
    first = _collect(c, buf, 64, den=den)
    assert first[0] == 3.0
    for grid, nt in ((0, None), (1, False), (7, True), (333, False), (100000, True)):
        again = _collect(c, buf, 64, den=den, grid=grid, nontemporal=nt)
        assert first.tobytes() == again.tobytes(), (grid, nt)
    assert _collect(c, buf, 64)[0] == 1.0                   # no den: 1.0 in the header


# ---- 5 - 7. through the optimizer -------------------------------------------------------------------------------------------------------
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


def _names(m):
    first = {}
    for name, p in m.named_parameters():
        first.setdefault(id(p), name)
    return [first[id(p)] for (p, _, _, _) in m.engine().items]


def _state(m, opt):
    torch.cuda.synchronize()
    eng = m.engine()
    out = {"p": eng.flat.detach().clone(), "m": opt._m.clone(), "v": opt._v.clone()}
    if eng.wshadow is not None:
        out["sh"] = eng.wshadow[: eng.wshadow.numel() - 32 * 1024].clone()      # (behind the shadows: the optimizer's tensor table)
    if opt._ema is not None:
        out["ema"] = opt._ema.clone()
    return out


def _check_kind(what, got, host, items, names, bins, den=1.0, other=None):
    """One kind of a read() record against watch_ref on the host copy of the buffer (divided by den where read() divides)."""
    assert list(got) == names
    refs = ref.buffer_stats(host, items, bins, other=other)
    for name, r in zip(names, refs):
        st = got[name]
        assert (st.numel, st.finite, st.nan, st.inf, st.zeros) == (r["numel"], r["finite"], r["nan"], r["inf"], r["zeros"]), (what, name)
        assert st.hist.dtype == np.int64 and st.hist.tolist() == r["hist"].tolist(), (what, name)
        assert st.edges.shape == (bins + 1,) and st.edges.dtype == np.float64
        assert r["finite"] > 0
        assert st.min == r["min"] / den and st.max == r["max"] / den, (what, name)
        assert st.edges[0] == r["lo"] / den and abs(st.edges[-1] - r["hi"] / den) <= 4 * EPS * abs(r["hi"] / den), (what, name)
        want_l2 = r["l2"] / den
        assert abs(st.l2 - want_l2) <= (r["numel"] + 4) * EPS * want_l2, (what, name, st.l2, want_l2)
        assert abs(st.rms - r["rms"] / den) <= (r["numel"] + 4) * EPS * r["rms"] / den, (what, name)
        assert abs(st.mean - r["mean"] / den) <= (r["numel"] + 4) * EPS * r["abs_sum"] / r["finite"] / den, (what, name, st.mean, r["mean"] / den)
    print(f"{what}: {len(names)} tensors agree with the host reference")


MODES = ["fp32", "bf16", "bf16_grads", "accumulation", "groups", "step_ranges"]


def _optimizer(mode, m, watch):
    if mode == "groups":
        ps = list(m.parameters())
        groups = [{"params": ps[1:9], "lr": 2e-3}, {"params": ps[9:], "weight_decay": 0.0}]      # ps[0] is in no group
        return FusedAdamW(m, lr=1e-3, weight_decay=0.01, params=groups, ema_decay=0.9, watch=watch)
    return FusedAdam(m, lr=1e-3, weight_decay=0.01, ema_decay=0.9 if mode == "fp32" else None, watch=watch)


@pytest.mark.parametrize("mode", MODES)
def test_watch_through_the_optimizer_and_nothing_else_moves(mode):
    """log_freq = 2 over 5 steps: records for steps 0, 2, 4 only; gradients / parameters / updates equal the reference on snapshots of
    the buffers the step read and wrote; and parameters, moments, shadows, EMA are bit for bit those of a twin without a watch."""
    precision = "fp32" if mode in ("fp32", "accumulation", "groups") else "bf16"
    bins = 64
    m, twin = _model(CFG, precision), _model(CFG, precision)
    kinds = ["gradients", "parameters", "updates"] + (["exp_avg", "exp_avg_sq", "ema"] if mode in ("fp32", "groups") else [])
    w = ModelWatch(m, log=kinds, log_freq=2, bins=bins)
    opt, opt_twin = _optimizer(mode, m, w), _optimizer(mode, twin, None)
    assert opt.watch is w and opt_twin.watch is None
    if mode == "bf16_grads":
        assert m.set_grad_bf16(True) and twin.set_grad_bf16(True)
    if mode == "accumulation":
        m.set_grad_accumulation(True)
        twin.set_grad_accumulation(True)
    items, names, n = _items(m), _names(m), m.engine().flat.numel()
    assert sorted(names) == sorted(k for k, _ in m.named_parameters())
    unowned = next(k for k, p in m.named_parameters() if p is next(iter(m.parameters())))
    starts = [o for o, _ in items]
    ranges = [(0, starts[5]), (starts[5], starts[20]), (starts[20], n)]
    log = []
    collect = w.collect
    w.collect = lambda kind, *a, **k: (log.append(("collect", kind)), collect(kind, *a, **k))[1]
    steps_read = []
    for i in range(5):
        den = 1.0
        used = []
        for mm, oo in ((m, opt), (twin, opt_twin)):
            eng = mm.engine()
            oo.zero_grad()
            if mode == "accumulation":
                for seed in (10 + 2 * i, 11 + 2 * i):
                    mm.train_step(*_batch(seed=seed), normalise=False)
                oo.grad_scale = mm.loss_terms()[1:2]
            else:
                mm.train_step(*_batch(seed=10 + i))
            if mode == "step_ranges":
                used.append(eng.ensure_grad().bfloat16())    # the reduced buffer of a bf16 exchange
            elif eng.grad_bf16_buf is not None:
                used.append(eng.grad_bf16_buf)
            else:
                used.append(eng.ensure_grad())
        torch.cuda.synchronize()
        if mode == "accumulation":
            den = float(m.loss_terms()[1])
            assert den > 1.0
        grad_host = used[0].detach().cpu().clone()
        assert grad_host.dtype == (torch.bfloat16 if mode in ("bf16_grads", "step_ranges") else torch.float32)
        pre = m.engine().flat.detach().cpu().clone()
        pre_m, pre_v = opt._m.cpu().clone() if opt._m is not None else None, opt._v.cpu().clone() if opt._v is not None else None
        pre_ema = opt._ema.cpu().clone() if opt._ema is not None and opt.n_averaged > 0 else None
        del log[:]
        if mode == "step_ranges":
            opt.step_ranges(ranges, before_each=lambda j: log.append(("before", j)), grads=used[0])
            opt_twin.step_ranges(ranges, grads=used[1])
        else:
            opt.step()
            opt_twin.step()
        torch.cuda.synchronize()
        post = m.engine().flat.detach().cpu().clone()
        due = i % 2 == 0
        assert w.pending == due
        if mode == "step_ranges":
            befores = [k for k, e in enumerate(log) if e[0] == "before"]
            collects = [k for k, e in enumerate(log) if e[0] == "collect"]
            assert [log[k][1] for k in befores] == [0, 1, 2]
            assert bool(collects) == due
            if due:
                assert max(befores) < min(collects), log      # every range's before_each ran before the first collection
        if not due:
            assert not [e for e in log if e[0] == "collect"]
            continue
        rec = w.read()
        assert not w.pending
        steps_read.append(rec["step"])
        assert rec["step"] == i and set(rec) == {"step", "den"} | set(kinds) - ({"ema"} if pre_ema is None else set())
        assert rec["den"] == den
        _check_kind(f"{mode} step {i} gradients (den {den})", rec["gradients"], grad_host, items, names, bins, den=den)
        _check_kind(f"{mode} step {i} parameters", rec["parameters"], pre, items, names, bins)
        _check_kind(f"{mode} step {i} updates", rec["updates"], post, items, names, bins, other=pre)
        if mode == "groups":
            # the tensor in no group did not move: its update is all zeros ...
            first = rec["updates"][unowned]
            assert first.zeros == first.numel and first.min == first.max == 0.0 and int(first.hist[bins // 2]) == first.numel
            assert rec["gradients"][unowned].l2 > 0.0        # ... and its gradient is watched like any other
        if "exp_avg" in kinds and pre_m is not None and i > 0:
            _check_kind(f"{mode} step {i} exp_avg", rec["exp_avg"], pre_m, items, names, bins)
            _check_kind(f"{mode} step {i} exp_avg_sq", rec["exp_avg_sq"], pre_v, items, names, bins)
        if pre_ema is not None and mode == "fp32":
            _check_kind(f"{mode} step {i} ema", rec["ema"], pre_ema, items, names, bins)
    assert steps_read == [0, 2, 4]
    a, b = _state(m, opt), _state(twin, opt_twin)
    assert a.keys() == b.keys() and (precision == "bf16") == ("sh" in a) and (mode in ("fp32", "groups")) == ("ema" in a)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{mode}: {k} differs with the watch attached"
    assert m.engine().shadows_fresh() == twin.engine().shadows_fresh()
    # detached: the step as it was
    opt.watch = None
    m.train_step(*_batch(seed=99))
    opt.step() if mode != "step_ranges" else opt.step_ranges(ranges)
    assert not w.pending


@pytest.mark.parametrize("mode", ["fp32", "bf16_grads"])
def test_watched_norm_equals_the_clip_norm(mode):
    m = _model(CFG, "fp32" if mode == "fp32" else "bf16")
    if mode == "bf16_grads":
        assert m.set_grad_bf16(True)
    w = ModelWatch(m, log="gradients", log_freq=1)
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, max_grad_norm=1e-3, watch=w)
    for i, with_den in enumerate((False, mode == "fp32")):
        m.train_step(*_batch(seed=3 + i), normalise=not with_den)
        opt.grad_scale = m.loss_terms()[1:2] if with_den else None
        opt.step()
        rec = w.read()
        den = rec["den"]
        assert (den > 1.0) == with_den
        total = math.sqrt(sum((st.l2 * den) ** 2 for st in rec["gradients"].values())) / den
        norm = float(opt.grad_norm())
        rel = abs(total - norm) / norm
        print(f"{mode} den {den}: sqrt(sum of the watched sumsq) / den {total!r}, optimizer.grad_norm() {norm!r}, relative difference {rel:.3e}")
        assert rel <= 2.0 ** -23 and float(opt.clip_coef()) < 1.0


def test_prepare_fused_is_refused_by_a_gradient_watch_only():
    cfg, B, L, lengths, kind = synth.CASES["tiny_ragged"]
    batch = [t.cuda() for t in synth.make_inputs(cfg, B, L, lengths, kind)]
    runs = {}
    for log in ("gradients", "all", ["updates"], "parameters", None):
        m = _model(cfg, "bf16")
        w = None if log is None else ModelWatch(m, log=log, log_freq=2)
        opt = FusedAdam(m, lr=1e-3, weight_decay=0.01, watch=w)
        losses = [float(m.train_step(*batch, use_graph=i > 0, optimizer=opt)) for i in range(3)]
        plan = next(p for p in m.engine().plans.values() if p.train)
        armed = getattr(plan, "_fused_key", None) is not None
        assert armed == (log in ("parameters", None)), (log, getattr(plan, "_fused_err", None))
        if armed:
            assert opt.prepare_fused(plan) is True
            opt.finish_fused(plan)
        else:
            assert opt.prepare_fused(plan) is False
        runs[str(log)] = (losses, _state(m, opt))
        if log == "parameters":
            rec = w.read()                                   # the in-launch steps are counted; step 2 was due
            assert rec["step"] == 2 and set(rec) == {"step", "den", "parameters"}
    for k, (losses, state) in runs.items():
        assert losses == runs["None"][0], k
        for f in state:
            assert torch.equal(state[f], runs["None"][1][f]), (k, f)


def test_collect_by_hand_for_a_loop_with_a_torch_optimizer():
    m = _model()
    w = ModelWatch(m, log="all", bins=16)
    loss = m.train_step(*_batch())
    assert float(loss) > 0
    w.begin(7)
    w.collect("gradients", m.flat_gradients())
    w.collect("parameters", m.engine().flat)
    assert w.pending
    rec = w.read()
    assert rec["step"] == 7 and rec["den"] == 1.0
    _check_kind("by hand, gradients", rec["gradients"], m.flat_gradients().cpu(), _items(m), _names(m), 16)
    _check_kind("by hand, parameters", rec["parameters"], m.engine().flat.detach().cpu(), _items(m), _names(m), 16)
    for name, p in m.named_parameters():
        assert rec["gradients"][name].numel == p.numel()
    with pytest.raises(ValueError, match="flat device tensor"):
        w.collect("gradients", m.flat_gradients()[:-64])
    with pytest.raises(ValueError, match="fp32 or bf16"):
        w.collect("gradients", m.flat_gradients().double())
    with pytest.raises(ValueError, match="one-element"):
        w.collect("gradients", m.flat_gradients(), den=torch.ones(2, device="cuda"))


# ---- 8. the loop --------------------------------------------------------------------------------------------------------------------------
def _dataset(n_dia, d_t, d_a, seed):
    import pandas as pd
    import dataset as ds
    g = np.random.default_rng(seed)
    rows = [(f"utt {d}-{u}", list(ds.EMOTIONS)[int(g.integers(0, 7))], d, u) for d in range(n_dia) for u in range(int(g.integers(1, 10)))]
    table = pd.DataFrame(rows, columns=["Utterance", "Emotion", "Dialogue_ID", "Utterance_ID"])
    text = torch.from_numpy(g.standard_normal((len(rows), d_t)).astype(np.float32))
    audio = torch.from_numpy(g.standard_normal((len(rows), d_a)).astype(np.float32))
    return ds.Dataset("train", text_embeddings=text, audio_embeddings=audio, table=table)


def _config(tmp_path, **rt):
    from utils import AttrDict, get_config
    cfg = AttrDict(dict(get_config()))
    cfg.model = AttrDict(synth._cfg(40, 48, 64, 4, 4, 4, 1, 1, 1, dropout=0.0))
    cfg.runtime = AttrDict(dict(cfg.runtime, **rt))
    cfg.solver = AttrDict(dict(cfg.solver, epochs=2, lr=2e-3, weight_decay=0.01, balance_classes=False,
                               early_stopping=AttrDict(enabled=False, patience=5, restore_best_weights=False),
                               scheduler=AttrDict(enabled=False, scheduler_fn="ExponentialLR", gamma=0.9)))
    cfg.checkpoint = AttrDict(save_path=str(tmp_path / "ck" / "m2fnet.pth"), load_path=str(tmp_path / "ck" / "m2fnet.pth"),
                              save_checkpoint=False, load_checkpoint=False)
    cfg.wandb = AttrDict(dict(cfg.wandb, enabled=False))
    cfg.train = AttrDict(data_loader=AttrDict(batch_size=8, shuffle=True, num_workers=0))
    cfg.val = AttrDict(data_loader=AttrDict(batch_size=8, shuffle=False, num_workers=0))
    return cfg


@pytest.mark.parametrize("accumulation", [1, 2])
def test_train_main_writes_one_json_line_per_due_step(tmp_path, monkeypatch, accumulation):
    monkeypatch.chdir(ROOT)
    import train as tr
    path = tmp_path / "watch" / "watch.jsonl"
    cfg = _config(tmp_path, watch={"enabled": True, "log": "all", "log_freq": 2, "bins": 16, "file": str(path)},
                  grad_accumulation=accumulation)
    sets = {"train": _dataset(40, 48, 40, 1), "val": _dataset(12, 48, 40, 2)}      # 5 batches of 8 dialogues per epoch
    monkeypatch.setattr(tr, "get_config", lambda: cfg)
    monkeypatch.setattr(tr, "Dataset", lambda mode, **kw: sets[mode])
    tr.main()
    lines = [json.loads(x) for x in path.read_text().splitlines()]
    per_epoch = 5 if accumulation == 1 else 3                # optimizer steps: one per batch, or one per group of two (the last one short)
    assert [x["step"] for x in lines] == [n for n in range(2 * per_epoch) if n % 2 == 0]
    names = [n for n, _ in tr.M2FNet(cfg.model).named_parameters()]
    for x in lines:
        assert set(x) == {"step", "den", "gradients", "parameters"}
        assert (x["den"] > 1.0) == (accumulation > 1)        # the group's denominator; 1 when the step normalises itself
        for kind in ("gradients", "parameters"):
            assert sorted(x[kind]) == sorted(names)
            for name, st in x[kind].items():
                assert len(st["hist"]) == 16 and sum(st["hist"]) == st["finite"] == st["numel"] > 0, (kind, name)
                assert st["min"] <= st["mean"] <= st["max"] and st["rms"] >= 0.0
        assert any(st["l2"] > 0.0 for st in x["gradients"].values())


def test_train_logs_histograms_beside_the_running_loss(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(ROOT)
    import dataset as ds
    import train as tr
    logged = []

    class Histogram:
        def __init__(self, np_histogram=None):
            self.counts, self.edges = np_histogram

    stub = types.SimpleNamespace(log=logged.append, Histogram=Histogram, watch=lambda *a, **k: logged.append("wandb.watch"),
                                 finish=lambda: None)
    monkeypatch.setattr(tr, "wandb", stub)
    cfg = _config(tmp_path, watch={"enabled": True, "log": "all", "log_freq": 2, "bins": 16, "file": None})
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = tr.M2FNet(cfg.model).to(device)
    crit = tr.M2FCrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    opt = tr.build_optimizer(cfg, model)
    w = tr.attach_watch(cfg, model, opt, 0, 1)
    assert opt.watch is w and w.log_freq == 2 and w.bins == 16
    assert tr.attach_watch(cfg, model, tr.build_optimizer(cfg, model), 1, 2) is None      # the other ranks do not watch
    dl = torch.utils.data.DataLoader(_dataset(40, 48, 40, 1), collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    tr.train(model, dl, crit, opt, 0, True, device)
    assert len(logged) == 5
    names = [n for n, _ in model.named_parameters()]
    keys = {f"{k}/{n}" for k in ("gradients", "parameters") for n in names}
    for step, entry in enumerate(logged):
        assert "Train/Running_loss" in entry
        watched = {k for k in entry if k not in ("Train/Running_loss", "Params/Global_step")}
        assert watched == (keys if step % 2 == 0 else set()), step
        for k in watched:
            assert isinstance(entry[k], Histogram) and len(entry[k].counts) == 16 and len(entry[k].edges) == 17
    # wandb.watch_model: the reference's call stays, and rank 0 is pointed to runtime.watch when that block is off
    cfg_off = _config(tmp_path)
    cfg_off.wandb = type(cfg_off.wandb)(dict(cfg_off.wandb, enabled=True, watch_model=True))
    cfg_off.solver.epochs = 0
    del logged[:]
    capsys.readouterr()
    tr.training_loop(model, dl, dl, crit, tr.build_optimizer(cfg_off, model), None, 0, cfg_off, device)
    assert logged == ["wandb.watch"] and "runtime.watch" in capsys.readouterr().out
