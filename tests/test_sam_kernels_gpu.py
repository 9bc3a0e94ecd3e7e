"""The sharpness-aware minimisation entries (m2f_sam_perturb, m2f_sam_restore; csrc/sam.hip) on caller-owned flat buffers of small
layouts whose tensors hit every path of the kernels: 4-column groups (cols % 4 == 0) and the scalar path (widths 50 and 4,101),
matrices whose rows are no multiple of 64 or of 8 (a padded leading dimension of the W^T shadow), 1-D tensors shorter and longer
than a 4,096-element tile, fp32 and bf16 gradients, with and without shadows.  Every pad between tensors holds a sentinel.  The
coefficient and every element are compared with float64; the shadows with what the forward's own cast path and the Adam kernel write
from the same values, bit for bit.  Every comparison prints its figures before it asserts (-s)."""
import dataclasses
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import param_tables_ref as tables  # noqa: E402
import synth  # noqa: E402
from mer_amd import layout, runtime  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402

DEV = "cuda"
EPS32 = torch.finfo(torch.float32).eps
SENTINEL = 12345.678
# widths 50 / 20 / 36, classifier 50: in_proj 150 x 50 and 60 x 20 (rows % 8 != 0), linear1 2048 x 50 (scalar path over 32 row
# tiles), linear2 50 x 2048 (vector path, rows % 64 != 0, ldt 56), 7 x 50; a model can be built over it (the cast-path comparison)
MODEL_CFG = synth._cfg(50, 20, 36, 2, 2, 2, 1, 1, 1, hid=50, ncls=3)
SMALL = layout.M2FConfig.from_model_config(MODEL_CFG)
# the same with a feed-forward width of 4,101: linear1.bias is a 1-D tensor longer than a tile whose last group is short, and
# linear2.weight a matrix of 4,101 columns (scalar path over 65 column tiles)
WIDE = dataclasses.replace(layout.M2FConfig.from_model_config(synth._cfg(24, 20, 20, 2, 2, 2, 1, 1, 1, hid=20, ncls=2)), dim_ff=4101)
CONFIGS = {"small": SMALL, "wide": WIDE}


def _mask(c):
    """bool [total]: True on parameter elements, False on the alignment pads."""
    ts, total = tables.tensors(c)
    m = torch.zeros(total, dtype=torch.bool)
    for off, n, _ in ts:
        m[off: off + n] = True
    return m.to(DEV)


def _buffers(c, seed, g16=False, shadows=False, zero_grad=False):
    total = tables.tensors(c)[1]
    elem = _mask(c)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    p = torch.randn(total, device=DEV, generator=gen) * 0.1
    g = torch.zeros(total, device=DEV) if zero_grad else torch.randn(total, device=DEV, generator=gen) * 1e-3
    saved = torch.full((total,), -SENTINEL, device=DEV)
    p[~elem] = SENTINEL
    g[~elem] = SENTINEL
    if g16:
        g = g.to(torch.bfloat16)
    s = {"p": p, "g": g, "saved": saved, "elem": elem,
         "scratch": runtime.grad_norm_scratch(c, DEV), "record": torch.zeros(4, device=DEV)}
    s["sh"] = runtime.param_shadow_buffer(c, DEV) if shadows else None
    return s


def _perturb(c, s, rho, den=None):
    runtime.grad_sumsq(c, s["g"], s["scratch"])
    runtime.sam_perturb(c, s["p"], s["g"], s["saved"], s["sh"], s["scratch"], s["record"], rho, den)
    torch.cuda.synchronize()


def _ulp(x32):
    a = x32.abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def test_layouts_have_the_shapes_these_tests_need():
    for name, want in (("small", dict(scalar=True, vec=True, rows64=True, rows8=True, short=True)),
                       ("wide", dict(scalar=True, long=True, tail=True))):
        ts = tables.tensors(CONFIGS[name])[0]
        mats, vecs = [s for _, _, s in ts if len(s) == 2], [n for _, n, s in ts if len(s) == 1]
        have = dict(scalar=any(c % 4 for _, c in mats), vec=any(c % 4 == 0 for _, c in mats), rows64=any(r % 64 for r, _ in mats),
                    rows8=any(r % 8 for r, _ in mats), short=any(n < 4096 for n in vecs), long=any(n > 4096 for n in vecs),
                    tail=any(n > 4096 and n % 4 for n in vecs))
        assert all(have[k] for k in want), (name, have)
        assert any(n % 64 for _, n, _ in ts), "a pad between tensors"
        assert tables.n_slices(CONFIGS[name]) > 1 and tables.items(CONFIGS[name])[1][-1] > 1      # more than one block in both forms


@pytest.mark.parametrize("shadows", [False, True])
@pytest.mark.parametrize("g16", [False, True])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_perturb_and_restore_against_float64(name, g16, shadows):
    c = CONFIGS[name]
    rho = 0.05
    den = torch.tensor([3.0], device=DEV) if g16 else None           # (both divisor forms across the cases)
    s = _buffers(c, 5, g16, shadows)
    before = {k: s[k].clone() for k in ("p", "g", "saved")}
    elem = s["elem"]
    _perturb(c, s, rho, den)
    # the record
    g64 = s["g"].double()[elem]
    d = 3.0 if den is not None else 1.0
    root = float(torch.sqrt((g64 * g64).sum()))
    norm64 = root / d
    c64 = rho / (norm64 + 1e-12) / d
    rec = s["record"].double().cpu().tolist()
    print(f"{name} g16 {g16} shadows {shadows}: norm {rec[0]!r} (float64 {norm64!r}), c {rec[1]!r} (float64 {c64!r}, "
          f"relative error {abs(rec[1] - c64) / c64:.3e}), den {rec[2]}, root {rec[3]!r}")
    assert abs(rec[1] - c64) <= 2 * EPS32 * c64 and abs(rec[0] - norm64) <= EPS32 * norm64 and abs(rec[3] - root) <= EPS32 * root
    assert rec[2] == d
    # every element: within one ulp of float64 w + c g, c the published coefficient
    want = before["p"].double() + rec[1] * s["g"].double()
    err = ((s["p"].double() - want).abs() / _ulp(want.float()))[elem]
    moved = int((s["p"] != before["p"])[elem].sum())
    print(f"  worst element error {err.max().item():.3f} ulp; {moved} of {int(elem.sum())} elements moved")
    assert err.max().item() <= 1.0 and moved > 0.5 * int(elem.sum())
    # the backup and the pads
    assert torch.equal(s["saved"][elem], before["p"][elem])
    for k in ("p", "g", "saved"):
        assert torch.equal(s[k][~elem], before[k][~elem]), f"pads of {k}"
    assert torch.equal(s["g"], before["g"])
    # two runs give the same bits
    s2 = _buffers(c, 5, g16, shadows)
    _perturb(c, s2, rho, den)
    assert torch.equal(s2["p"], s["p"]) and torch.equal(s2["record"], s["record"]) and torch.equal(s2["saved"], s["saved"])
    if shadows:
        assert torch.equal(s2["sh"], s["sh"])
        # the Adam kernel's own shadows of the same values: a step that moves nothing (lr 0, no decay, zero gradient and moments)
        a = _buffers(c, 5, False, True, zero_grad=True)
        a["p"].copy_(s["p"])
        zeros = torch.zeros_like(a["p"])
        runtime.adam_step_shadowed(c, a["p"], a["g"].zero_(), zeros, zeros.clone(), a["sh"], 1, lr=0.0, weight_decay=0.0)
        torch.cuda.synchronize()
        assert torch.equal(a["p"][elem], s["p"][elem])
        diff = int((a["sh"] != s["sh"]).sum())
        print(f"  shadow buffer against the Adam kernel's of the same values: {diff} of {s['sh'].numel()} differ")
        assert diff == 0
    # restore: w's bits, pads untouched
    shadow_before = None if not shadows else s["sh"].clone()
    runtime.sam_restore(c, s["p"], s["saved"])
    torch.cuda.synchronize()
    assert torch.equal(s["p"], before["p"])
    assert shadow_before is None or torch.equal(s["sh"], shadow_before)         # (the restore leaves the shadows to the caller)


@pytest.mark.parametrize("g16", [False, True])
def test_shadows_are_what_the_forwards_cast_path_writes(g16):
    """A twin model in bf16 mode is given w' and runs a forward: its engine's shadow buffer - W, W^T, the zero columns, the table region -
    must equal the buffer the perturbation wrote."""
    s = _buffers(SMALL, 9, g16, True)
    _perturb(SMALL, s, 0.5)
    twin = M2FNet(MODEL_CFG, precision="bf16").to(DEV).train()               # (dropout 0; a train plan casts W and W^T)
    eng = twin.engine()
    assert eng.wshadow is not None and eng.flat.numel() == s["p"].numel()
    with torch.no_grad():
        flat = twin.flat_parameters()                     # (hands the buffer out and invalidates the shadows)
        flat.copy_(torch.where(s["elem"], s["p"], torch.zeros_like(s["p"])))
    assert not eng.shadows_fresh()
    t, a, kp, em = [x.to(DEV) for x in synth.make_inputs(MODEL_CFG, 2, 4, [4, 3], "randn", seed=1)]
    twin.train_step(t, a, kp, em, use_graph=False)
    torch.cuda.synchronize()
    diff = int((eng.wshadow != s["sh"]).sum())
    nz = int((s["sh"] != 0).sum())
    print(f"g16 {g16}: shadow buffer of {s['sh'].numel()} bf16 values ({nz} non-zero) against the forward's casts: {diff} differ")
    assert nz > 0.5 * int(s["elem"].sum()) and diff == 0


@pytest.mark.parametrize("shadows", [False, True])
@pytest.mark.parametrize("g16", [False, True])
def test_zero_gradient_moves_nothing(g16, shadows):
    s = _buffers(SMALL, 3, g16, shadows, zero_grad=True)
    before = s["p"].clone()
    _perturb(SMALL, s, 0.05)
    rec = s["record"].cpu()
    print(f"zero gradient: record {rec.tolist()}")
    assert torch.isfinite(rec).all() and rec[0] == 0.0 and rec[1] > 0.0
    assert torch.equal(s["p"], before) and torch.isfinite(s["p"]).all()
    assert torch.equal(s["saved"][s["elem"]], before[s["elem"]])


def test_entry_points_refuse_bad_arguments():
    s = _buffers(SMALL, 1)
    for rho in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(runtime.HipError, match="m2f_sam_perturb: rho"):
            runtime.sam_perturb(SMALL, s["p"], s["g"], s["saved"], None, s["scratch"], s["record"], rho)
    with pytest.raises(runtime.HipError, match="m2f_sam_perturb: params and saved are the same buffer"):
        runtime.sam_perturb(SMALL, s["p"], s["g"], s["p"], None, s["scratch"], s["record"], 0.05)
    with pytest.raises(runtime.HipError, match="m2f_sam_perturb: the flat buffers must be 16-byte aligned"):
        runtime.sam_perturb(SMALL, s["p"][1:], s["g"], s["saved"], None, s["scratch"], s["record"], 0.05)
    with pytest.raises(runtime.HipError, match="m2f_sam_restore: params and saved are the same buffer"):
        runtime.sam_restore(SMALL, s["p"], s["p"])
    with pytest.raises(runtime.HipError, match="m2f_sam_restore: the flat buffers must be 16-byte aligned"):
        runtime.sam_restore(SMALL, s["p"], s["saved"][1:])
