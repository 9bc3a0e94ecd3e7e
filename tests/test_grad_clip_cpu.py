"""Host side of gradient clipping by global norm: the config key and src/train.py's check of it (raised before any GPU use), the new
C entry points, and the float64 restatement of torch.nn.utils.clip_grad_norm_ (tests/golden/grad_clip_ref.py) that the GPU tests
take their reference values from."""
import inspect
import os
import re
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import grad_clip_ref as ref  # noqa: E402
from mer_amd import runtime  # noqa: E402

SYMBOLS = ("m2f_grad_norm_scratch_bytes", "m2f_grad_sumsq", "m2f_grad_norm_finalize")


def _cfg(**rt):
    return {"runtime": dict(rt)}


def test_config_has_clip_grad_norm_null():
    from utils import get_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        cfg = get_config()
    finally:
        os.chdir(cwd)
    assert "clip_grad_norm" in cfg.runtime and cfg.runtime.clip_grad_norm is None


def test_clip_grad_norm_check_before_gpu_use():
    import train as tr
    assert tr.clip_grad_norm(_cfg()) is None
    assert tr.clip_grad_norm(_cfg(clip_grad_norm=None)) is None
    assert tr.clip_grad_norm(_cfg(clip_grad_norm=1)) == 1.0
    assert tr.clip_grad_norm(_cfg(clip_grad_norm=0.25)) == 0.25
    assert isinstance(tr.clip_grad_norm(_cfg(clip_grad_norm=2)), float)
    for bad in (0, 0.0, -1, -0.5, True, False, "1.0", [1.0], float("nan"), float("inf")):
        with pytest.raises(ValueError, match="positive finite number"):
            tr.clip_grad_norm(_cfg(clip_grad_norm=bad))
    with pytest.raises(ValueError, match="fused_optimizer"):
        tr.clip_grad_norm(_cfg(clip_grad_norm=1.0, fused_optimizer=True))
    with pytest.raises(ValueError, match="grad_overlap"):
        tr.clip_grad_norm(_cfg(clip_grad_norm=1.0, grad_overlap=True), world=2)
    # one rank ignores grad_overlap; the other modes combine: bf16 gradients, accumulation, the bf16 exchange
    assert tr.clip_grad_norm(_cfg(clip_grad_norm=1.0, grad_overlap=True), world=1) == 1.0
    assert tr.clip_grad_norm(_cfg(clip_grad_norm=1.0, grad_bf16=True, precision="bf16")) == 1.0
    assert tr.clip_grad_norm(_cfg(clip_grad_norm=1.0, grad_accumulation=4)) == 1.0
    assert tr.clip_grad_norm(_cfg(clip_grad_norm=1.0, grad_exchange="bf16"), world=8) == 1.0
    # off: nothing is refused
    assert tr.clip_grad_norm(_cfg(fused_optimizer=True, grad_overlap=True), world=2) is None
    # main() runs the check next to grad_accumulation_steps, ahead of init_distributed / the device
    src = inspect.getsource(tr.main)
    assert src.index("clip_grad_norm(config") < src.index("init_distributed")
    assert "optimizer.max_grad_norm = clip_grad_norm(config, world)" in src


def test_header_declares_and_library_exports_the_norm_entry_points():
    header = open(runtime.HEADER_PATH).read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in runtime.SIGNATURES, name
        assert getattr(runtime.lib(), name) is not None
    # argument errors come back through m2f_last_error without a GPU call
    assert runtime.lib().m2f_grad_norm_scratch_bytes(None) == -1
    assert "NULL configuration" in runtime.lib().m2f_last_error().decode()
    assert runtime.lib().m2f_grad_sumsq(None, None, 0, 0, -1, None, 0, 0, None) != 0
    assert "NULL" in runtime.lib().m2f_last_error().decode()
    assert runtime.lib().m2f_grad_norm_finalize(None, None, None, 1.0, None, None) != 0


def test_scratch_holds_one_partial_per_slice_of_a_tensor():
    import ctypes
    import synth
    from mer_amd import layout
    for name in ("tiny_ragged", "c2_slice"):
        c = layout.M2FConfig.from_model_config(synth.CASES[name][0])
        specs, _ = layout.param_specs(c)
        slices = sum((s.numel + 8191) // 8192 for s in specs if not s.alias_of)
        cc = runtime.config_to_c(c)
        assert runtime.lib().m2f_grad_norm_scratch_bytes(ctypes.byref(cc)) == 8 * slices


def test_optimizer_surface():
    from mer_amd.optim import FusedAdam
    sig = inspect.signature(FusedAdam.__init__)
    assert sig.parameters["max_grad_norm"].default is None
    for name in ("grad_norm", "clip_coef"):
        assert callable(getattr(FusedAdam, name))


def _random_grads(seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    shapes = [(7,), (33, 5), (128, 64), (1,), (300, 300)]
    # magnitudes spread over six decades from tensor to tensor
    return [torch.randn(s, generator=g, dtype=torch.float64).mul_(10.0 ** (i - 3)).to(dtype) for i, s in enumerate(shapes)]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("where", ["above", "at", "below"])
def test_float64_restatement_agrees_with_torch(seed, where):
    """norm, coefficient and the clipped gradients of grad_clip_ref against torch.nn.utils.clip_grad_norm_ in float64: both evaluate the
    same formula, torch as a norm of per-tensor norms - they agree to a few float64 ulps (bound 1e-13 relative)."""
    grads = _random_grads(seed)
    n0 = ref.norm(grads)
    max_norm = {"above": 0.37 * n0, "at": n0, "below": 2.5 * n0}[where]
    params = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    assert abs(total - n0) <= 1e-13 * n0
    c = ref.coef(n0, max_norm)
    if where == "below":
        assert c == 1.0 and ref.divisor(3.0, c) == 3.0
    else:
        assert c < 1.0                                    # at max_norm exactly: max_norm / (norm + 1e-6) is just below one, as in torch
        assert ref.divisor(3.0, c) == 3.0 / c
    mine = [g.clone() for g in grads]
    assert ref.clip_(mine, max_norm) == n0
    for p, g in zip(params, mine):
        assert torch.allclose(p.grad, g, rtol=1e-13, atol=0.0)


def test_restatement_skips_the_pads_of_a_flat_buffer():
    flat = torch.full((256,), 1e6, dtype=torch.float32)
    items = [(0, 7), (64, 50), (128, 100)]
    g = torch.Generator().manual_seed(3)
    for o, n in items:
        flat[o: o + n] = torch.randn(n, generator=g)
    want = float(torch.cat([flat[o: o + n] for o, n in items]).double().norm())
    assert abs(ref.norm(ref.tensors_of(flat, items), den=2.0) - want / 2.0) <= 1e-14 * want
