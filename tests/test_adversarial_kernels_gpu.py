"""The adversarial ascent kernels on the device (functional.adversarial_ascend / adversarial_init, csrc/adversarial.hip) against the
float64 statements of tests/golden/adversarial_ref.py.

Bound, measured here and not chosen: the same statements run as plain fp32 torch on the SAME inputs lie some distance from float64; each
output of the kernel (delta, x) gets 4 times that distance for its case, relative to the output's largest element, floored at 8 fp32 eps
(the project's rule for aux_head and supcon).  Exact properties: rows whose flag is set and the pad columns behind d keep their bits in
x and delta (sentinels; their g and x_clean hold NaN - never read), epsilon = 0 leaves x == x_clean, x == x_clean + delta always, a
row's norm stays inside epsilon * (1 + 4 eps), two runs give the same bits (the launcher has no grid to choose: it follows from T), the
uniform start is the host replica's bit for bit.  Every comparison prints its figures before it asserts (-s)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adversarial_ref as ref  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402

DEV = "cuda"
EPS32 = torch.finfo(torch.float32).eps
# T: one row, a partial workgroup of four rows, whole 16-row slices of the batch norm's partials, a slice boundary, several slices with a
# ragged end.  d: one partial 16-byte piece set (20), pad8(d) != d (20, 100, 301), a last vector that straddles d (301: its buffers hold
# sentinels behind d), the launcher's other register forms (301 -> two pieces per lane, 768 and 1,024 -> four: the shipped widths and the
# register form's limit) and the looping form above it (1,500, d % 8 != 0)
SHAPES = [(1, 20), (5, 100), (64, 301), (65, 768), (130, 1024), (130, 1500), (130, 20), (5, 1500), (65, 100), (130, 301), (64, 1024), (1, 768)]
# (epsilon, step_size): the projection idle (the candidate stays inside the ball) and binding
REGIMES = {"idle": (10.0, 0.125), "bind": (0.5, 1.0)}
_cache = {}


def _case(T, d, inf):
    """x_clean, g, delta as [T, d] views of [T, pad8(d)] device buffers with sentinels, the flags, and CPU copies of the logical parts.
    Row 1 has a zero gradient, row 2 (inf) one with an inf in it, every third row from 3 on is masked and holds NaN in g and x_clean."""
    key = (T, d, inf)
    if key not in _cache:
        gen = torch.Generator().manual_seed(1000 * T + d)
        ld = (d + 7) // 8 * 8
        xc, g = torch.randn(T, d, generator=gen) * 0.6, torch.randn(T, d, generator=gen) * 3e-3
        dl = torch.randn(T, d, generator=gen) * (0.3 / d ** 0.5)
        pad = torch.zeros(T, dtype=torch.bool)
        pad[3::3] = True
        if T > 1:
            g[1] = 0.0
        if T > 2 and inf:
            g[2, d // 2] = float("inf")
        g[pad], xc[pad] = float("nan"), float("nan")
        dl[pad] = 7.25

        def place(t, fill):
            buf = torch.full((T, ld), fill, dtype=torch.float32, device=DEV)
            buf[:, :d] = t.to(DEV)
            return buf

        _cache[key] = (xc, g, dl, pad, ld, place)
    return _cache[key]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(T, d, inf, norm, eps, step):
    xc, g, dl, pad, ld, place = _case(T, d, inf)
    bx, bg, bd, bo = place(xc, float("nan")), place(g, float("nan")), place(dl, -123.5), place(torch.full((T, d), 3.5), -77.0)
    before_d, before_o = bd.clone(), bo.clone()
    out_d, out_x = F.adversarial_ascend(bx[:, :d], bg[:, :d], bd[:, :d], bo[:, :d], pad.to(DEV), eps, step, norm)
    assert out_d.data_ptr() == bd.data_ptr() and out_x.data_ptr() == bo.data_ptr()              # in place: the views were kernel-ready
    # masked rows and pad columns: bit for bit what they were
    keep = torch.zeros(T, ld, dtype=torch.bool, device=DEV)
    keep[:, d:] = True
    keep[pad.to(DEV)] = True
    assert torch.equal(_bits(bd)[keep], _bits(before_d)[keep]) and torch.equal(_bits(bo)[keep], _bits(before_o)[keep])
    return bd[:, :d], bo[:, :d], bx[:, :d]


def _distance(x, r64, live):
    big = r64[live].abs().max().item()
    return (x.double().cpu()[live] - r64[live]).abs().max().item() / (big if big > 0 else 1.0)


@pytest.mark.parametrize("T,d", SHAPES)
def test_ascent_matches_the_float64_reference(T, d):
    for norm in ("utterance", "batch"):
        for regime, (eps, step) in REGIMES.items():
            for inf in (False, True):
                if inf and T < 3:
                    continue
                xc, g, dl, pad, _, _ = _case(T, d, inf)
                live = ~pad
                new, x, xclean_dev = _run(T, d, inf, norm, eps, step)
                r64 = ref.ascend(xc, g, dl, pad, eps, step, norm, torch.float64)
                r32 = ref.ascend(xc, g, dl, pad, eps, step, norm, torch.float32)
                for name, got, k in (("delta", new, 0), ("x", x, 1)):
                    d32, dk = _distance(r32[k], r64[k], live), _distance(got, r64[k], live)
                    bound = max(4 * d32, 8 * EPS32)
                    print(f"{T} x {d} {norm} {regime} inf={inf}: {name}: kernel {dk:.3e}, fp32 torch form {d32:.3e}, bound {bound:.3e}")
                    assert torch.isfinite(got[live.to(DEV)]).all() and dk <= bound, (T, d, norm, regime, inf, name, dk, bound)
                lv = live.to(DEV)
                assert torch.equal(x[lv], xclean_dev[lv] + new[lv])                                # one fp32 add
                # a zero gradient (row 1) and one with an inf (row 2) leave the row's delta where the projection is idle for it: under the
                # utterance norm in both regimes (||delta|| is about 0.3), under the batch norm (where the inf stops every row) in the idle one
                if T > 1 and (norm == "utterance" or regime == "idle"):
                    assert torch.equal(new[1].cpu(), dl[1])
                if inf and norm == "utterance":
                    assert torch.equal(new[2].cpu(), dl[2])
                if inf and norm == "batch" and regime == "idle":
                    assert torch.equal(new[lv].cpu(), dl[live])
                n64 = new[lv].double().norm(dim=-1) if norm == "utterance" else new[lv].double().norm().reshape(1)
                assert bool((n64 <= eps * (1 + 4 * EPS32)).all()), (T, d, norm, regime, n64.max().item())


@pytest.mark.parametrize("T,d", [(5, 100), (130, 301), (65, 768), (130, 1024), (130, 1500)])
def test_epsilon_zero_leaves_the_clean_input(T, d):
    for norm in ("utterance", "batch"):
        xc, _, _, pad, _, _ = _case(T, d, False)
        new, x, xclean_dev = _run(T, d, False, norm, 0.0, 1.0)
        lv = (~pad).to(DEV)
        assert torch.equal(x[lv], xclean_dev[lv]) and not new[lv].any()
        assert torch.equal(_bits(x[lv]), _bits(xclean_dev[lv]))                                    # bit for bit: x_clean + 0


def test_two_runs_give_the_same_bits():
    for T, d in ((130, 301), (130, 1024), (130, 1500), (65, 768), (5, 100)):
        for norm in ("utterance", "batch"):
            a, b = _run(T, d, False, norm, 0.5, 1.0), _run(T, d, False, norm, 0.5, 1.0)
            live = (~_case(T, d, False)[3]).to(DEV)
            assert torch.equal(a[0][live], b[0][live]) and torch.equal(a[1][live], b[1][live]), (T, d, norm)


def test_projection_alone_and_copies_of_unaligned_rows():
    """g None is a zero gradient; [B, L, d] tensors whose rows are not 16-byte aligned travel through a copy and give the same bits as
    the padded buffers the plan uses."""
    T, d = 65, 301
    xc, g, dl, pad, _, _ = _case(T, d, False)
    new, x, _ = _run(T, d, False, "utterance", 0.5, 1.0)
    d2 = dl.to(DEV).clone()
    xc2 = torch.nan_to_num(xc).to(DEV)
    out_d, out_x = F.adversarial_ascend(xc2, torch.nan_to_num(g).to(DEV), d2, None, pad.to(DEV), 0.5, 1.0, "utterance")
    live = (~pad).to(DEV)
    assert out_d is d2 and torch.equal(out_d[live], new[live]) and torch.equal(out_x[live], x[live])
    assert torch.equal(out_d[~live].cpu(), dl[pad]) and torch.equal(out_x[~live], xc2[~live])      # padding rows: delta and x_clean
    # 3-D, and the projection alone
    d3 = (dl.to(DEV) * 40).reshape(5, 13, d).clone()
    p_d, p_x = F.adversarial_ascend(xc2.reshape(5, 13, d), None, d3, None, pad.to(DEV).reshape(5, 13), 0.5, 1.0, "utterance")
    r64 = ref.ascend(torch.nan_to_num(xc), None, dl * 40, pad, 0.5, 1.0, "utterance")
    r32 = ref.ascend(torch.nan_to_num(xc), None, dl * 40, pad, 0.5, 1.0, "utterance", torch.float32)
    assert p_d.shape == (5, 13, d) and p_d is d3
    assert _distance(p_d.reshape(T, d), r64[0], ~pad) <= max(4 * _distance(r32[0], r64[0], ~pad), 8 * EPS32)
    assert bool((p_d.reshape(T, d)[live].double().norm(dim=-1) <= 0.5 * (1 + 4 * EPS32)).all())


@pytest.mark.parametrize("T,d", [(1, 20), (5, 100), (65, 301), (130, 768), (64, 1500)])
def test_uniform_start_is_the_host_replica_bit_for_bit(T, d):
    state = [0x12345678, 0x9ABCDEF0, 41, 0]
    to_i32 = lambda u: u - (1 << 32) if u >= (1 << 31) else u
    rng = torch.tensor([to_i32(v) for v in state], dtype=torch.int32, device=DEV)
    pad = torch.zeros(T, dtype=torch.bool)
    pad[2::4] = True
    ld = (d + 7) // 8 * 8
    for site, mag in ((ref.SITE_TEXT, 0.5), (ref.SITE_AUDIO, 3.0)):
        buf = torch.full((T, ld), -9.5, dtype=torch.float32, device=DEV)
        F.adversarial_init(buf[:, :d], mag, rng, site, pad.to(DEV))
        want = torch.from_numpy(ref.uniform_start(state, site, np.arange(T), d, mag))
        got = buf.cpu()
        assert torch.equal(_bits(got[:, :d][~pad]), _bits(want[~pad])), (T, d, site)
        assert bool((got[:, d:] == -9.5).all()) and bool((got[pad] == -9.5).all())
        assert got[:, :d][~pad].abs().max().item() <= mag / d ** 0.5 * (1 + 1e-6)
