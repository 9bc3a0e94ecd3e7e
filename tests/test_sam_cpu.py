"""Host side of sharpness-aware minimisation (FusedAdam.sam_rho, M2FNet.sam_step): the optimizer's argument checks, the state errors
and refusals that need no device, the runtime.sam block of the config and src/train.py's check of it, the new C entry points and the
Makefile gate, and the power of the float64 reference (tests/sam_ref.py) the GPU tests compare with: on the test configuration the
plain gradient must miss the SAM gradient by well over the bound the GPU step is held to, or that bound would show nothing."""
import inspect
import os
import re
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import sam_ref as ref  # noqa: E402
import synth  # noqa: E402
from mer_amd import dp, runtime  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam, FusedAdamW  # noqa: E402

CFG = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2, ncls=7)
# the four plan kinds of tests/test_aux_head_model_gpu.py: (B, L, seed, lengths) and the rho the power check runs at
KINDS = {"padded_4x6": (4, 6, 1, [6, 6, 5, 6], 0.5), "bucketed_3x5": (3, 5, 4, [5, 2, 4], 0.5),
         "packed_5x9": (5, 9, 2, [9, 1, 5, 3, 2], 0.5), "long_2x70": (2, 70, 3, [70, 5], 0.5)}
SYMBOLS = ("m2f_sam_perturb", "m2f_sam_restore")


def last_classifier_weight(sd):
    return [k for k in sd if k.startswith("output_layer.") and k.endswith(".weight")][-1]


def _cpu_model():
    m = M2FNet(CFG)
    m.load_state_dict(synth.make_state_dict(CFG))
    return m


# ---- the reference's own power ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_plain_gradient_misses_the_sam_gradient_by_twenty_bounds(kind):
    """The GPU step's gradients are held to 3e-5 + 1e-3 x max |g| of the reference's SAM gradient.  On the LAST classifier weight the
    plain gradient (no perturbation) must lie at >= 20 x that bound, so a step that skipped the perturbation cannot pass.  Most
    encoder tensors move by less than the bound: the assertion is on that tensor, the count over all is printed."""
    B, L, seed, lengths, rho = KINDS[kind]
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    sd = ref.as_float64(synth.make_state_dict(CFG))
    t, a, kp, em = synth.make_inputs(CFG, B, L, lengths, "randn", seed=seed)
    r = ref.sam_gradient(sd, CFG, (t.double(), a.double(), kp, em), rho)
    name = last_classifier_weight(sd)
    outside, factors = 0, {}
    for k in ref.unique_names(sd):
        bound = 3e-5 + 1e-3 * r["sam"][k].abs().max().item()
        factors[k] = (r["plain"][k] - r["sam"][k]).abs().max().item() / bound
        outside += factors[k] > 1.0
    e, n = ref.perturbation(sd, r["plain"], rho)
    size = float(torch.sqrt(sum((d ** 2).sum() for d in e.values())))
    print(f"{kind} rho {rho}: ||g|| {n:.6f}, ||e|| {size:.6f}, loss {float(r['loss']):.6f} -> {float(r['loss_at']):.6f} at w + e; plain "
          f"misses on {name} by {factors[name]:.0f} x the bound; {outside} of {len(factors)} tensors outside it")
    assert abs(size - rho) <= 1e-9 * rho and float(r["loss_at"]) > float(r["loss"])
    assert factors[name] >= 20.0, (kind, factors[name])


def test_reference_counts_a_shared_tensor_once_and_rho_scales_e():
    cfg = synth.CASES["tiny_shared_norm"][0]
    sd = synth.make_state_dict(cfg)
    names = ref.unique_names(sd)
    assert len(names) < len(sd)                                     # shared LayerNorms: several names, one tensor
    g = {k: torch.full_like(v, 2.0, dtype=torch.float64) for k, v in sd.items()}
    n = ref.grad_norm(sd, g)
    assert abs(n - 2.0 * sum(sd[k].numel() for k in names) ** 0.5) <= 1e-12 * n
    at, _ = ref.perturbed(sd, g, 0.25)
    assert [k for k in ref.unique_names(at)] == names               # the aliasing survives
    moved = torch.sqrt(sum(((at[k] - sd[k].double()) ** 2).sum() for k in names))
    assert abs(float(moved) - 0.25) <= 1e-12
    zero = {k: torch.zeros_like(v, dtype=torch.float64) for k, v in sd.items()}
    at0, n0 = ref.perturbed(sd, zero, 0.25)
    assert n0 == 0.0 and all(torch.equal(at0[k], sd[k].double()) for k in names)


# ---- the optimizer's surface -----------------------------------------------------------------------------------------------------
def test_sam_rho_argument_errors():
    m = _cpu_model()
    for bad in (0, 0.0, -0.05, True, "0.05", float("nan"), float("inf"), [0.05]):
        with pytest.raises(ValueError, match="sam_rho"):
            FusedAdam(m, sam_rho=bad)
        with pytest.raises(ValueError, match="sam_rho"):
            FusedAdamW(m, sam_rho=bad)
        with pytest.raises(ValueError, match="sam_rho"):
            runtime.check_sam_rho(bad)
    for ok in (0.05, 1, 2.5):
        opt = FusedAdam(m, sam_rho=ok)
        assert opt.sam_rho == float(ok) and isinstance(opt.sam_rho, float) and opt.sam_pending is False
    assert FusedAdamW(m, sam_rho=0.1).sam_rho == 0.1
    assert FusedAdam(m).sam_rho is None and runtime.check_sam_rho(None) is None
    with pytest.raises(TypeError):
        FusedAdam(m, 1e-3, (0.9, 0.999), 1e-8, 0.0, None, 0.05)             # keyword-only
    for cls in (FusedAdam, FusedAdamW):
        par = inspect.signature(cls.__init__).parameters["sam_rho"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    for name in ("first_step", "restore", "sam_norm"):
        assert callable(getattr(FusedAdam, name))
    assert callable(M2FNet.sam_step)


def test_state_errors_that_need_no_device():
    m = _cpu_model()
    opt = FusedAdam(m, sam_rho=0.05)
    with pytest.raises(RuntimeError, match=r"FusedAdam\.step\(\): sam_rho is set and no perturbation is pending"):
        opt.step()
    with pytest.raises(RuntimeError, match=r"FusedAdam\.step_ranges\(\): sharpness-aware"):
        opt.step_ranges([(0, 64)])
    with pytest.raises(RuntimeError, match=r"FusedAdam\.sam_norm: first_step\(\) has not run"):
        opt.sam_norm()
    with pytest.raises(RuntimeError, match=r"FusedAdam\.first_step\(\): sam_rho is None"):
        FusedAdam(m).first_step()
    opt.sam_rho = -1.0                                              # the attribute is checked where it is read
    with pytest.raises(ValueError, match="sam_rho"):
        opt.first_step()
    with pytest.raises(ValueError, match="sam_rho"):
        opt.step()
    opt.sam_rho = 0.05
    assert opt.restore() is False                                  # nothing pending: nothing to do
    assert opt.prepare_fused(None) is False                        # the in-launch optimizer cannot wait for a second pass
    # a pending perturbation (the flag alone: no device here)
    opt._sam_pending = True
    for call, name in ((opt.first_step, r"first_step\(\)"), (lambda: opt.prepare_fused(None), r"prepare_fused\(\)"),
                       (opt.ema_state_dict, r"ema_state_dict\(\)"), (lambda: opt.averaged_parameters().__enter__(), r"averaged_parameters\(\)"),
                       (lambda: opt.step_ranges([(0, 64)]), r"step_ranges\(\)")):
        with pytest.raises(RuntimeError, match=r"FusedAdam\." + name + ".*pending"):
            call()
    opt._sam_pending = False
    # a grouped optimizer that leaves a tensor in no group
    some = [p for n, p in m.named_parameters() if n.startswith("output_layer.")]
    part = FusedAdamW(m, params=[{"params": some}], sam_rho=0.05)
    with pytest.raises(RuntimeError, match=r"FusedAdam\.first_step\(\): .*cover every tensor"):
        part.first_step()


def test_refusals_that_need_no_device():
    m = _cpu_model()
    opt = FusedAdam(m, sam_rho=0.05)
    t, a, kp, em = synth.make_inputs(CFG, 4, 6, [6, 6, 5, 6], "randn", seed=1)
    with pytest.raises(RuntimeError, match=r"M2FNet\.train_step: optimizer= .*sharpness-aware minimisation \(optimizer\.sam_rho\)"):
        m.train_step(t, a, kp, em, optimizer=opt)
    with pytest.raises(RuntimeError, match=r"M2FNet\.sam_step: optimizer\.sam_rho is None"):
        m.sam_step(t, a, kp, em, FusedAdam(m))
    opt._sam_pending = True
    with pytest.raises(RuntimeError, match="M2FNet.sam_step: a perturbation is already pending"):
        m.sam_step(t, a, kp, em, opt)
    opt._sam_pending = False
    m._grad_accumulation = True
    with pytest.raises(RuntimeError, match="M2FNet.sam_step: under gradient accumulation"):
        m.sam_step(t, a, kp, em, opt)
    m._grad_accumulation = False
    with pytest.raises(RuntimeError, match="DataParallelStep: sharpness-aware minimisation"):
        dp.DataParallelStep(m, opt)
    assert m._engine is None, "refused before an engine was built"


def test_state_dict_without_and_with_sam_rho_is_the_same():
    m = _cpu_model()
    plain, sam = FusedAdam(m, lr=1e-3, weight_decay=0.01), FusedAdam(m, lr=1e-3, weight_decay=0.01, sam_rho=0.05)
    assert plain.state_dict() == sam.state_dict()
    assert not any("sam" in k for k in sam.state_dict()["param_groups"][0])
    assert FusedAdamW(m, lr=1e-3).state_dict() == FusedAdamW(m, lr=1e-3, sam_rho=0.1).state_dict()


# ---- config ------------------------------------------------------------------------------------------------------------------------
def _cfg(**rt):
    return {"runtime": dict(rt)}


def test_config_has_the_sam_block_disabled():
    from utils import get_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        cfg = get_config()
    finally:
        os.chdir(cwd)
    assert dict(cfg.runtime["sam"]) == {"enabled": False, "rho": 0.05}


def test_sam_settings_check_before_gpu_use():
    import train as tr
    assert tr.sam_settings(_cfg()) is None and tr.sam_settings(_cfg(sam=None)) is None and tr.sam_settings(_cfg(sam={})) is None
    assert tr.sam_settings(_cfg(sam={"enabled": False, "rho": 0.1})) is None
    assert tr.sam_settings(_cfg(sam={"enabled": True})) == 0.05
    assert tr.sam_settings(_cfg(sam={"enabled": True, "rho": 2})) == 2.0
    for bad in (0, -0.1, True, "0.05", None, [0.05], float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"runtime\.sam\.rho"):
            tr.sam_settings(_cfg(sam={"enabled": True, "rho": bad}))
    with pytest.raises(ValueError, match=r"runtime\.sam\.rho"):             # a bad value is refused even while disabled
        tr.sam_settings(_cfg(sam={"enabled": False, "rho": 0}))
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match=r"runtime\.sam\.enabled"):
            tr.sam_settings(_cfg(sam={"enabled": bad}))
    with pytest.raises(ValueError, match="unknown key"):
        tr.sam_settings(_cfg(sam={"enabled": True, "radius": 0.05}))
    with pytest.raises(ValueError, match="mapping"):
        tr.sam_settings(_cfg(sam=0.05))
    on = {"enabled": True}
    with pytest.raises(ValueError, match="fused_optimizer"):
        tr.sam_settings(_cfg(sam=on, fused_optimizer=True))
    with pytest.raises(ValueError, match="fused_step"):
        tr.sam_settings(_cfg(sam=on, fused_step=False))
    with pytest.raises(ValueError, match="grad_accumulation"):
        tr.sam_settings(_cfg(sam=on, grad_accumulation=2))
    with pytest.raises(ValueError, match="data-parallel"):
        tr.sam_settings(_cfg(sam=on), world=2)
    assert tr.sam_settings(_cfg(sam={"enabled": False}, fused_optimizer=True), world=2) is None
    ok = _cfg(sam=on, clip_grad_norm=1.0, grad_bf16=True, precision="bf16", ema={"enabled": True}, optimizer={"name": "adamw"})
    assert tr.sam_settings(ok) == 0.05
    src = inspect.getsource(tr.main)
    assert src.index("ema_settings(config)") < src.index("sam_settings(config") < src.index("init_distributed")
    assert "Train/SAM_grad_norm" in inspect.getsource(tr._sam_log) and "sam_step" in inspect.getsource(tr.train)


# ---- C ABI and the build's gate ------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_sam_entry_points():
    header = open(runtime.HEADER_PATH).read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in runtime.SIGNATURES, name
        assert getattr(runtime.lib(), name) is not None
    assert len(runtime.SIGNATURES["m2f_sam_perturb"][1]) == 11 and len(runtime.SIGNATURES["m2f_sam_restore"][1]) == 4


def test_makefile_holds_sam_to_the_spill_gate():
    mk = open(os.path.join(runtime.CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    gated = re.search(r"^GATED = (.*)$", mk, re.M).group(1).split()
    assert "sam.hip" in srcs and "sam" in gated
    assert re.search(r"^sam\.o: GATE = check_spills\.py --sam$", mk, re.M) and re.search(r"^#   sam: ", mk, re.M)
    assert '"--sam"' in open(os.path.join(runtime.CSRC, "check_spills.py")).read()
