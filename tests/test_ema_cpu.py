"""Host side of the weight average inside the optimizer kernels (FusedAdam.ema_decay): the float64 restatement the GPU tests take
their reference values from (tests/golden/ema_ref.py) against torch's own AveragedModel, the warm-up sequence, the runtime.ema
block of the config and src/train.py's check of it (raised before any GPU use), the optimizer's argument checks, the new C entry
points, and that an optimizer without ema_decay is the one it was."""
import inspect
import os
import re
import sys

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import ema_ref as ref  # noqa: E402
import synth  # noqa: E402
from mer_amd import runtime  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam, FusedAdamW, check_ema_decay, ema_decay_at  # noqa: E402

SYMBOLS = ("m2f_adam_step_ema", "m2f_adam_step_g16_ema", "m2f_adam_step_shadowed_range_ema", "m2f_adam_step_grouped_ema",
           "m2f_ema_exchange")


# ---- the rule, pinned to torch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.5, 0.9, 0.99, 0.999])
def test_float64_restatement_agrees_with_torch_averaged_model(decay):
    """12 updates of torch's fp32 AveragedModel + get_ema_multi_avg_fn(decay) against ema_ref in float64, element by element, within the
    bound the GPU kernels are held to (8 k 2^-24 M); the first update is a copy, bit for bit."""
    g = torch.Generator().manual_seed(int(decay * 1000))
    model = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.Linear(17, 5))
    with torch.no_grad():
        for i, p in enumerate(model.parameters()):
            p.copy_(torch.randn(p.shape, generator=g) * 10.0 ** (i - 2))     # magnitudes spread over decades
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))
    mine = [ref.Average(decay) for _ in model.parameters()]
    worst = 0.0
    for k in range(12):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn(p.shape, generator=g) * 0.05 * p.abs().mean())
        avg.update_parameters(model)
        for a, p, e in zip(mine, model.parameters(), avg.module.parameters()):
            a.step(p)
            if k == 0:
                assert torch.equal(e, p)
            worst = max(worst, a.error_ratio(e))
    print(f"decay {decay}: torch's fp32 AveragedModel differs from the float64 restatement by at most {worst:.3f} of 8 k 2^-24 M over 12 updates")
    assert worst <= 1.0
    assert all(a.n == 12 for a in mine) and int(avg.n_averaged) == 12


def test_warmup_sequence_in_closed_form():
    for decay in (0.5, 0.9, 0.999):
        for n in range(0, 2000, 7):
            want = min(decay, (1.0 + n) / (10.0 + n))
            assert ref.decay_at(decay, n, True) == want == ema_decay_at(decay, n, True)
            assert ref.decay_at(decay, n, False) == decay == ema_decay_at(decay, n, False)
    assert ref.decay_at(0.999, 0, True) == 0.1 and ref.decay_at(0.999, 8, True) == 0.5
    # the warm-up ends where (1 + n) / (10 + n) reaches the decay: n = (10 d - 1) / (1 - d)
    assert ref.decay_at(0.9, 79, True) < 0.9 and ref.decay_at(0.9, 80, True) == 0.9
    assert ref.weight_at(0.9, 0) == 1.0 and ref.weight_at(0.9, 0, True) == 1.0             # update 0 always copies
    assert ref.weight_at(0.9, 3) == 1.0 - 0.9
    # a float64 run of the sequence: constant parameters stay put, a step input follows the closed form
    a = ref.Average(0.9, True)
    p = torch.tensor([2.0, -3.0])
    for _ in range(5):
        a.step(p)
    assert torch.equal(a.value, p.double())
    b = ref.Average(0.5)
    b.step(torch.zeros(1))
    for k in range(1, 6):
        b.step(torch.ones(1))
        assert abs(float(b.value) - (1.0 - 0.5 ** k)) < 1e-15


# ---- config ------------------------------------------------------------------------------------------------------------------------
def _cfg(**rt):
    return {"runtime": dict(rt)}


def test_config_has_the_ema_block_disabled():
    from utils import get_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        cfg = get_config()
    finally:
        os.chdir(cwd)
    assert dict(cfg.runtime["ema"]) == {"enabled": False, "decay": 0.999, "warmup": False, "evaluate": True}


def test_ema_settings_check_before_gpu_use():
    import train as tr
    assert tr.ema_settings(_cfg()) is None
    assert tr.ema_settings(_cfg(ema=None)) is None
    assert tr.ema_settings(_cfg(ema={})) is None
    assert tr.ema_settings(_cfg(ema={"enabled": False, "decay": 0.5})) is None
    assert tr.ema_settings(_cfg(ema={"enabled": True})) == (0.999, False, True)
    assert tr.ema_settings(_cfg(ema={"enabled": True, "decay": 0.9, "warmup": True, "evaluate": False})) == (0.9, True, False)
    assert tr.ema_settings(_cfg(ema={"enabled": True, "decay": 0})) == (0.0, False, True)
    assert tr.ema_settings(_cfg(ema={"enabled": True, "decay": 1})) == (1.0, False, True)
    for bad in (-0.1, 1.5, True, "0.9", None, [0.9], float("nan")):
        with pytest.raises(ValueError, match=r"runtime\.ema\.decay"):
            tr.ema_settings(_cfg(ema={"enabled": True, "decay": bad}))
    with pytest.raises(ValueError, match=r"runtime\.ema\.decay"):           # a bad value is refused even while disabled
        tr.ema_settings(_cfg(ema={"enabled": False, "decay": 2}))
    for key in ("enabled", "warmup", "evaluate"):
        for bad in (1, 0, "yes", None):
            with pytest.raises(ValueError, match=rf"runtime\.ema\.{key}"):
                tr.ema_settings(_cfg(ema={"enabled": True, key: bad}))
    with pytest.raises(ValueError, match="unknown key"):
        tr.ema_settings(_cfg(ema={"enabled": True, "decays": 0.9}))
    with pytest.raises(ValueError, match="mapping"):
        tr.ema_settings(_cfg(ema=0.999))
    with pytest.raises(ValueError, match="fused_optimizer"):
        tr.ema_settings(_cfg(ema={"enabled": True}, fused_optimizer=True))
    assert tr.ema_settings(_cfg(ema={"enabled": False}, fused_optimizer=True)) is None
    # everything else combines
    ok = _cfg(ema={"enabled": True}, grad_accumulation=4, clip_grad_norm=1.0, grad_bf16=True, precision="bf16", grad_overlap=True,
              grad_exchange="bf16", optimizer={"name": "adamw"})
    assert tr.ema_settings(ok) == (0.999, False, True)
    # main() runs the check beside the others, ahead of init_distributed / the device
    src = inspect.getsource(tr.main)
    assert src.index("clip_grad_norm(config") < src.index("ema_settings(config)") < src.index("init_distributed")
    assert set(tr.CHECKPOINT_KEYS) == {"epoch", "model_state_dict", "optimizer_state_dict"} and tr.EMA_KEY == "ema_state_dict"


# ---- the optimizer's surface -----------------------------------------------------------------------------------------------------
def _cpu_model():
    cfg = synth.CASES["tiny_ragged"][0]
    m = M2FNet(cfg)
    m.load_state_dict(synth.make_state_dict(cfg))
    return m


def test_ema_decay_range_errors():
    m = _cpu_model()
    for bad in (-1e-9, 1.0000001, 2, -1, True, "0.9", float("nan"), [0.5]):
        with pytest.raises(ValueError, match="ema_decay"):
            FusedAdam(m, ema_decay=bad)
        with pytest.raises(ValueError, match="ema_decay"):
            FusedAdamW(m, ema_decay=bad)
        with pytest.raises(ValueError, match="ema_decay"):
            check_ema_decay(bad)
    for ok in (0, 0.0, 0.5, 1, 1.0):
        opt = FusedAdam(m, ema_decay=ok)
        assert opt.ema_decay == float(ok) and isinstance(opt.ema_decay, float) and opt.ema_warmup is False
    assert FusedAdamW(m, ema_decay=0.99, ema_warmup=True).ema_warmup is True
    assert FusedAdam(m).ema_decay is None and check_ema_decay(None) is None
    with pytest.raises(TypeError):
        FusedAdam(m, 1e-3, (0.9, 0.999), 1e-8, 0.0, None, 0.9)              # keyword-only
    sig = inspect.signature(FusedAdam.__init__)
    assert sig.parameters["ema_decay"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["ema_decay"].default is None
    assert sig.parameters["ema_warmup"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["ema_warmup"].default is False
    for name in ("ema_parameters", "ema_state_dict", "load_ema_state_dict", "averaged_parameters"):
        assert callable(getattr(FusedAdam, name))
    opt = FusedAdam(m, ema_decay=0.9)
    assert opt.n_averaged == 0
    with pytest.raises(RuntimeError, match="no EMA step"):
        opt.ema_parameters()
    with pytest.raises(RuntimeError, match="no EMA step"):
        opt.ema_state_dict()
    with pytest.raises(RuntimeError, match="no average yet"):
        with opt.averaged_parameters():
            pass


def test_state_dict_without_ema_is_unchanged():
    """ema_decay=None: state_dict() has the keys and values it has always had; and with ema_decay set it still is torch's format,
    with nothing of the average in it."""
    m = _cpu_model()
    plain, none, ema = FusedAdam(m, lr=1e-3, weight_decay=0.01), FusedAdam(m, lr=1e-3, weight_decay=0.01, ema_decay=None), \
        FusedAdam(m, lr=1e-3, weight_decay=0.01, ema_decay=0.9, ema_warmup=True)
    want = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=0.01).state_dict()
    for opt in (plain, none, ema):
        sd = opt.state_dict()
        assert set(sd) == {"state", "param_groups"} and sd["state"] == {}
        assert len(sd["param_groups"]) == 1
        g = sd["param_groups"][0]
        assert g["params"] == want["param_groups"][0]["params"]
        assert not any("ema" in k for k in g)
        for k in ("lr", "betas", "eps", "weight_decay"):
            assert g[k] == want["param_groups"][0][k]
    assert plain.state_dict() == none.state_dict() == ema.state_dict()
    ga, gb = FusedAdamW(m, lr=1e-3).state_dict(), FusedAdamW(m, lr=1e-3, ema_decay=0.5).state_dict()
    assert ga == gb
    torch.optim.AdamW(m.parameters()).load_state_dict(gb)                    # still interchanges with torch


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_ema_entry_points():
    header = open(runtime.HEADER_PATH).read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in runtime.SIGNATURES, name
        assert getattr(runtime.lib(), name) is not None
    assert "AveragedModel.update_parameters" in header and "get_ema_multi_avg_fn" in header
    # argument errors come back through m2f_last_error without a GPU call
    lib = runtime.lib()
    assert lib.m2f_adam_step_ema(None, None, None, None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0.1, None, None) != 0
    assert "EMA buffer" in lib.m2f_last_error().decode()
    assert lib.m2f_adam_step_g16_ema(None, None, None, None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0.1, None, None) != 0
    assert lib.m2f_adam_step_shadowed_range_ema(None, None, None, 0, None, None, None, None, 0.1, 0, -1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1,
                                                None, None) != 0
    assert lib.m2f_adam_step_grouped_ema(None, None, None, 0, None, None, None, None, 0.1, None, 0, None, 0, -1, None, None) != 0
    assert lib.m2f_ema_exchange(None, None, None, None, 0, None) != 0
    assert "NULL" in lib.m2f_last_error().decode()
    import ctypes
    buf = (ctypes.c_float * 8)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    assert lib.m2f_adam_step_ema(None, None, None, None, addr, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.5, None, None) != 0
    assert "[0, 1]" in lib.m2f_last_error().decode()
