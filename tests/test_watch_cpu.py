"""Host side of the model watch (mer_amd.watch.ModelWatch, csrc/tensor_stats.hip): the restatement of its per-tensor rules
(tests/golden/watch_ref.py) against torch.histc count for count, the C entry points and their size functions, the `runtime.watch` block
and src/train.py's check of it (raised before any GPU use), the due schedule and the host-side record handling."""
import ctypes
import inspect
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import synth  # noqa: E402
import watch_ref as ref  # noqa: E402
from mer_amd import layout, runtime  # noqa: E402
from mer_amd import watch as W  # noqa: E402

SYMBOLS = ("m2f_tensor_stats_scratch_bytes", "m2f_tensor_stats_record_bytes", "m2f_tensor_stats")


# ---- the restatement against torch.histc ------------------------------------------------------------------------------------------
def _randn(n, scale, seed, bf16=False):
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale
    return x.bfloat16().float() if bf16 else x


def _case(name):
    g = torch.Generator().manual_seed(99)
    return {
        "2M_0.02": lambda: _randn(2_097_152, 0.02, 1),
        "589k_0.05": lambda: _randn(589_824, 0.05, 2),
        "2304_1e-4": lambda: _randn(2_304, 1e-4, 3),
        "7": lambda: _randn(7, 1.0, 4),
        "1": lambda: _randn(1, 1.0, 5),
        "230k_3_bf16": lambda: _randn(230_400, 3.0, 6, bf16=True),
        "1.7M_1e-6": lambda: _randn(1_769_472, 1e-6, 7),
        "uniform": lambda: torch.rand(1_000_003, generator=g) * 2.0 - 1.0,
        "dyadic": lambda: torch.randint(-512, 513, (300_000,), generator=g).float() / 64.0,
    }[name]()


CASES = ["2M_0.02", "589k_0.05", "2304_1e-4", "7", "1", "230k_3_bf16", "1.7M_1e-6", "uniform", "dyadic"]


@pytest.mark.parametrize("bins", [2, 64, 256])
@pytest.mark.parametrize("name", CASES)
def test_restated_histogram_equals_torch_histc_count_for_count(name, bins):
    x = _case(name)
    want = torch.histc(x, bins, min=float(x.min()), max=float(x.max())).to(torch.int64)
    got = ref.tensor_stats(x, bins)["hist"]
    differing = int((got != want).sum())
    print(f"{name} bins {bins}: {differing} differing counts of {bins}")
    assert differing == 0
    assert int(got.sum()) == x.numel()


def test_constant_tensor_goes_to_the_middle_bin():
    x = torch.full((100,), 0.5)
    want = torch.histc(x, 64, min=0.5, max=0.5).to(torch.int64)
    st = ref.tensor_stats(x, 64)
    assert int(want[32]) == 100 and torch.equal(st["hist"], want)
    assert (st["lo"], st["hi"], st["min"], st["max"]) == (-0.5, 1.5, 0.5, 0.5)
    for bins in (2, 7, 256):
        h = ref.tensor_stats(x, bins)["hist"]
        assert int(h[bins // 2]) == 100 and int(h.sum()) == 100


def test_non_finite_values_are_counted_and_left_out():
    x = _randn(1000, 1.0, 11)
    x[3], x[500], x[501], x[7], x[8] = float("nan"), float("inf"), float("-inf"), 0.0, -0.0
    st = ref.tensor_stats(x, 64)
    fin = x[torch.isfinite(x)]
    assert (st["numel"], st["finite"], st["nan"], st["inf"], st["zeros"]) == (1000, 997, 1, 2, 2)
    assert st["min"] == float(fin.min()) and st["max"] == float(fin.max())
    assert st["sum"] == float(fin.double().sum()) and math.isfinite(st["sumsq"])
    assert torch.equal(st["hist"], torch.histc(fin, 64, min=float(fin.min()), max=float(fin.max())).to(torch.int64))
    assert int(st["hist"].sum()) == 997


def test_a_tensor_with_no_finite_value_gives_nan_fields_and_zero_counts():
    st = ref.tensor_stats(torch.tensor([float("nan"), float("inf"), float("-inf"), float("nan")]), 16)
    assert (st["numel"], st["finite"], st["nan"], st["inf"], st["zeros"]) == (4, 0, 2, 2, 0)
    assert all(math.isnan(st[k]) for k in ("min", "max", "sum", "sumsq", "mean", "l2", "rms"))
    assert int(st["hist"].sum()) == 0 and st["hist"].numel() == 16


def test_buffer_stats_skips_the_pads_and_takes_the_difference_in_fp32():
    flat = torch.full((256,), float("nan"))
    items = [(0, 7), (64, 50), (128, 100)]
    g = torch.Generator().manual_seed(3)
    for o, n in items:
        flat[o: o + n] = torch.randn(n, generator=g)
    rows = ref.buffer_stats(flat, items, 8)
    assert [r["nan"] for r in rows] == [0, 0, 0] and [r["numel"] for r in rows] == [7, 50, 100]
    other = torch.randn(256, generator=g)
    rows = ref.buffer_stats(flat, items, 8, other=other)
    assert rows[1]["min"] == float((flat[64:114] - other[64:114]).min())


# ---- the C entry points -------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    header = open(runtime.HEADER_PATH).read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in runtime.SIGNATURES, name
        assert getattr(runtime.lib(), name) is not None
    lib = runtime.lib()
    assert lib.m2f_tensor_stats_scratch_bytes(None, 64) == -1
    assert "NULL configuration" in lib.m2f_last_error().decode()
    assert lib.m2f_tensor_stats_record_bytes(None, 64) == -1
    assert "NULL configuration" in lib.m2f_last_error().decode()
    # argument errors come back through m2f_last_error without a GPU call
    assert lib.m2f_tensor_stats(None, None, 0, None, 64, None, None, None, 0, 0, None) != 0
    assert "NULL" in lib.m2f_last_error().decode()
    cc = runtime.config_to_c(layout.M2FConfig.from_model_config(synth.CASES["tiny_ragged"][0]))
    buf = (ctypes.c_double * 64)()
    addr = ctypes.addressof(buf)
    for bins in (1, 0, -3, 257):
        assert lib.m2f_tensor_stats_scratch_bytes(ctypes.byref(cc), bins) == -1
        assert "bins" in lib.m2f_last_error().decode()
        assert lib.m2f_tensor_stats_record_bytes(ctypes.byref(cc), bins) == -1
        assert lib.m2f_tensor_stats(ctypes.byref(cc), addr, 0, None, bins, None, addr, addr, 0, 0, None) != 0
        assert "bins" in lib.m2f_last_error().decode()
    assert lib.m2f_tensor_stats(ctypes.byref(cc), addr, 1, addr, 64, None, addr, addr, 0, 0, None) != 0
    assert "fp32" in lib.m2f_last_error().decode()
    assert lib.m2f_tensor_stats(ctypes.byref(cc), addr + 4, 0, None, 64, None, addr, addr, 0, 0, None) != 0
    assert "aligned" in lib.m2f_last_error().decode()


def test_sizes_are_what_the_slice_count_and_bins_predict():
    for name in ("tiny_ragged", "c2_slice"):
        c = layout.M2FConfig.from_model_config(synth.CASES[name][0])
        specs, _ = layout.param_specs(c)
        uniq = [s for s in specs if not s.alias_of]
        slices = sum((s.numel + 8191) // 8192 for s in uniq)
        cc = runtime.config_to_c(c)
        for bins in (2, 64, 256):
            assert runtime.lib().m2f_tensor_stats_scratch_bytes(ctypes.byref(cc), bins) == 40 * slices
            assert runtime.lib().m2f_tensor_stats_record_bytes(ctypes.byref(cc), bins) == 8 * (runtime.TSTATS_HEADER + len(uniq) * (runtime.TSTATS_FIELDS + bins))


# ---- runtime.watch ------------------------------------------------------------------------------------------------------------------
def _cfg(**rt):
    return {"runtime": dict(rt)}


def test_config_has_the_watch_block_disabled():
    from utils import get_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        cfg = get_config()
    finally:
        os.chdir(cwd)
    assert dict(cfg.runtime.watch) == {"enabled": False, "log": "all", "log_freq": 100, "bins": 64, "file": None}
    assert "watch_model" in cfg.wandb                        # the reference's key stays


def test_watch_settings_are_checked_before_gpu_use(monkeypatch):
    import train as tr
    calls = []
    monkeypatch.setattr(runtime, "require_gpu", lambda: calls.append("require_gpu"))
    monkeypatch.setattr(runtime, "lib", lambda: calls.append("lib"))
    assert tr.watch_settings(_cfg()) is None
    assert tr.watch_settings(_cfg(watch={"enabled": False, "log": "all"})) is None
    assert tr.watch_settings(_cfg(watch={"enabled": True})) == {"log": ("gradients", "parameters"), "log_freq": 100, "bins": 64, "file": None}
    got = tr.watch_settings(_cfg(watch={"enabled": True, "log": ["ema", "updates", "gradients"], "log_freq": 1, "bins": 256, "file": "w.jsonl"}))
    assert got == {"log": ("gradients", "updates", "ema"), "log_freq": 1, "bins": 256, "file": "w.jsonl"}
    assert tr.watch_settings(_cfg(watch={"enabled": True, "log": "parameters"}))["log"] == ("parameters",)
    bad_blocks = [
        ("unknown key", {"enabled": True, "every": 3}),
        ("log must be", {"enabled": True, "log": "weights"}),
        ("log must be", {"enabled": True, "log": ["gradients", "activations"]}),
        ("log must be", {"enabled": True, "log": []}),
        ("log must be", {"enabled": True, "log": 3}),
        ("twice", {"enabled": True, "log": ["ema", "ema"]}),
        ("log_freq", {"enabled": True, "log_freq": 0}),
        ("log_freq", {"enabled": True, "log_freq": 2.5}),
        ("log_freq", {"enabled": True, "log_freq": True}),
        ("bins", {"enabled": True, "bins": 1}),
        ("bins", {"enabled": True, "bins": 257}),
        ("bins", {"enabled": True, "bins": "64"}),
        ("enabled", {"enabled": "yes"}),
        ("file", {"enabled": True, "file": 3}),
        ("bins", {"enabled": False, "bins": 1}),             # a disabled block is still checked, as runtime.ema is
    ]
    for match, block in bad_blocks:
        with pytest.raises(ValueError, match=match):
            tr.watch_settings(_cfg(watch=block))
    with pytest.raises(ValueError, match="mapping"):
        tr.watch_settings(_cfg(watch=True))
    with pytest.raises(ValueError, match="fused_optimizer"):
        tr.watch_settings(_cfg(watch={"enabled": True}, fused_optimizer=True))
    for log in ("all", "gradients", ["updates"]):
        with pytest.raises(ValueError, match="grad_overlap"):
            tr.watch_settings(_cfg(watch={"enabled": True, "log": log}, grad_overlap=True), world=2)
    assert tr.watch_settings(_cfg(watch={"enabled": True, "log": "parameters"}, grad_overlap=True), world=2) is not None
    assert tr.watch_settings(_cfg(watch={"enabled": True}, grad_overlap=True), world=1) is not None      # one rank ignores grad_overlap
    assert tr.watch_settings(_cfg(watch={"enabled": False}, fused_optimizer=True)) is None               # off: nothing is refused
    # another optimizer is refused, again without a device call
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match="FusedAdam"):
        tr.attach_watch(_cfg(watch={"enabled": True}), None, torch.optim.SGD([p], lr=0.1))
    assert tr.attach_watch(_cfg(), None, torch.optim.SGD([p], lr=0.1)) is None
    assert calls == []
    # main() runs the check with the other refusals, ahead of init_distributed / the device, and attaches after the optimizer is built
    src = inspect.getsource(tr.main)
    assert src.index("watch_settings(config") < src.index("init_distributed")
    assert src.index("build_optimizer(config, model)") < src.index("attach_watch(config, model, optimizer, rank, world)")


class _FakeModel:
    def engine(self):
        raise AssertionError("no device call expected")

    def named_parameters(self):
        return iter(())


def test_model_watch_arguments_and_due_schedule():
    w = W.ModelWatch(_FakeModel())
    assert (w.kinds, w.log_freq, w.bins, w.pending, w.file) == (("gradients", "parameters"), 100, 64, False, None)
    assert [n for n in range(301) if w.due(n)] == [0, 100, 200, 300]
    w = W.ModelWatch(_FakeModel(), log=("exp_avg_sq", "parameters", "exp_avg"), log_freq=2, bins=2)
    assert w.kinds == ("parameters", "exp_avg", "exp_avg_sq")
    assert [n for n in range(6) if w.due(n)] == [0, 2, 4]
    assert W.ModelWatch(_FakeModel(), log="gradients").kinds == ("gradients",)
    assert W.ModelWatch(_FakeModel(), log=W.KINDS).kinds == W.KINDS
    for kw in ({"log": "weights"}, {"log": ["grads"]}, {"log": []}, {"log": None}, {"log_freq": 0}, {"log_freq": -1}, {"log_freq": 1.5},
               {"log_freq": True}, {"bins": 1}, {"bins": 257}, {"bins": 64.0}, {"bins": False}):
        with pytest.raises(ValueError):
            W.ModelWatch(_FakeModel(), **kw)
    with pytest.raises(TypeError, match="M2FNet"):
        W.ModelWatch(torch.nn.Linear(2, 2))
    with pytest.raises(RuntimeError, match="nothing has been collected"):
        W.ModelWatch(_FakeModel()).read()
    with pytest.raises(ValueError, match="not one of the watched kinds"):
        W.ModelWatch(_FakeModel(), log="parameters").collect("gradients", torch.zeros(4))


def test_optimizer_surface():
    from mer_amd.optim import FusedAdam, FusedAdamW
    for cls in (FusedAdam, FusedAdamW):
        p = inspect.signature(cls.__init__).parameters["watch"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY


def _record(bins=8):
    """A host record as read() builds it, from hand-made rows."""
    g = torch.Generator().manual_seed(0)
    rec = {"step": 4, "den": 2.0}
    for kind, den in (("gradients", 2.0), ("parameters", 1.0)):
        rec[kind] = {}
        for name, n in (("a.weight", 100), ("a.bias", 5), ("dead", 3)):
            x = torch.randn(n, generator=g) if name != "dead" else torch.full((n,), float("nan"))
            st = ref.tensor_stats(x, bins)
            row = np.array([st[k] for k in ("numel", "finite", "nan", "inf", "zeros", "min", "max", "sum", "sumsq")], dtype=np.float64)
            rec[kind][name] = W.stats_from_row(row, st["hist"].numpy(), den)
    return rec


def test_stats_from_row_divides_the_value_fields_by_den():
    x = torch.randn(1000, generator=torch.Generator().manual_seed(2))
    st = ref.tensor_stats(x, 16)
    row = np.array([st[k] for k in ("numel", "finite", "nan", "inf", "zeros", "min", "max", "sum", "sumsq")], dtype=np.float64)
    one, half = W.stats_from_row(row, st["hist"].numpy()), W.stats_from_row(row, st["hist"].numpy(), den=2.0)
    assert (one.numel, one.finite, one.nan, one.inf, one.zeros) == (1000, 1000, 0, 0, st["zeros"])
    assert (one.min, one.max, one.mean, one.l2, one.rms) == (st["min"], st["max"], st["mean"], st["l2"], st["rms"])
    assert one.edges.shape == (17,) and one.edges[0] == st["min"] and abs(one.edges[-1] - st["max"]) <= 1e-15
    for f in ("min", "max", "mean", "l2", "rms"):
        assert getattr(half, f) == getattr(one, f) / 2.0
    assert np.array_equal(half.edges, one.edges / 2.0) and np.array_equal(half.hist, one.hist) and half.hist.dtype == np.int64
    const = W.stats_from_row(np.array([4, 4, 0, 0, 0, 0.5, 0.5, 2.0, 1.0]), np.array([0, 4], dtype=np.int64))
    assert (const.edges[0], const.edges[-1]) == (-0.5, 1.5)


def test_wandb_payload_summary_and_json_line():
    w = W.ModelWatch(_FakeModel(), bins=8)
    rec = _record(8)
    pay = w.wandb_payload(rec)
    assert list(pay) == [f"{k}/{n}" for k in ("gradients", "parameters") for n in ("a.weight", "a.bias", "dead")]
    for counts, edges in pay.values():
        assert isinstance(counts, list) and isinstance(edges, list) and len(counts) == 8 and len(edges) == 9
        assert all(isinstance(c, int) for c in counts)
    assert sum(pay["gradients/a.weight"][0]) == 100 and sum(pay["parameters/dead"][0]) == 0
    lines = w.summary(rec)
    assert len(lines) == 6 and lines[0].startswith("step 4 gradients/a.weight: numel 100 finite 100 nan 0")
    line = w.json_line(rec)
    assert "\n" not in line
    back = json.loads(line)
    assert back["step"] == 4 and back["den"] == 2.0 and set(back) == {"step", "den", "gradients", "parameters"}
    for kind in ("gradients", "parameters"):
        for name, st in rec[kind].items():
            got = back[kind][name]
            assert got["hist"] == st.hist.tolist()
            for f in W.SCALARS:
                a, b = got[f], getattr(st, f)
                assert a == b or (math.isnan(a) and math.isnan(b)), (kind, name, f)
