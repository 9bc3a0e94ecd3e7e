"""The auxiliary label head's kernels on the device (functional.aux_head, csrc/aux_head.hip; the head and the loss module under
autograd) against the float64 reference (tests/golden/aux_head_ref.py).

Bound, measured here and not chosen: the reference's own statements run as plain fp32 torch on the SAME inputs lie some distance from
float64; each output of the kernels (aux_logits, row_terms, dfeatures, dparams) gets 4 times that distance for its case, relative to the
output's largest element, floored at 8 fp32 eps of that element for inputs where fp32 torch happens to be exact.  Exact properties:
ignored rows give exactly 0 in row_terms, dfeatures and their share of dparams whatever their features hold (aux_logits = W h + b is
defined for every row and is not zero), nothing is NaN at logit margins of 120, two calls give the same bits (the launcher has no grid
to choose: it follows from N and D).  Every comparison prints its figures before it asserts (-s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import aux_head_ref as ref  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402
from mer_amd.aux_head import AuxiliaryHead  # noqa: E402
from mer_amd.optim import M2FAuxiliaryLoss  # noqa: E402

DEV = "cuda"
LAM, C = 0.7, 7
EPS32 = torch.finfo(torch.float32).eps
# name: N, D, A, eps_a, class weights, seed - N: one row, a partial block (8-row blocks of the rows and join kernels, 16-row partials and
# 64-row workgroups of the parameter gradient), a block boundary on either side, several blocks;
# D: pad8(D) != D (20, 100), inside one 16-byte piece per lane (20, 64, 100); then the widths at which the launchers take their other
# instantiations: 301 (two pieces per lane, D % 4 != 0: the last vector straddles D - its inputs sit in a row stride of 304 whose pad
# columns hold NaN), 768 (the shipped CLASSIFIER.hidden_size: four pieces per lane, three column blocks of the parameter gradient) and
# 1,024 with 16 classes (the largest block: 65,600 bytes of LDS, past the 64 KB a launch gets without asking); 130 rows give the
# parameter gradient several row blocks AND column blocks.  A: the smallest, an odd one, the largest
CASES = {"1x20x2": (1, 20, 2, 0.0, False, 21), "15x100x3": (15, 100, 3, 0.1, True, 22), "64x64x16": (64, 64, 16, 0.0, True, 23),
         "65x20x3": (65, 20, 3, 0.1, False, 24), "130x100x16": (130, 100, 16, 0.1, True, 25), "130x64x2": (130, 64, 2, 0.0, False, 26),
         "130x301x16": (130, 301, 16, 0.1, True, 27), "65x768x3": (65, 768, 3, 0.0, False, 28), "130x768x16": (130, 768, 16, 0.1, True, 29),
         "130x1024x16": (130, 1024, 16, 0.0, True, 30)}
OUTPUTS = ("logits", "rows", "dfeat", "dparams")
_cache = {}


def _ref(h, y, s, params, w, A, eps, dtype):
    D = h.shape[1]
    r = ref.aux_head(h.cpu(), y.cpu(), s.cpu(), params[: A * D].view(A, D).cpu(), params[A * D:].cpu(), C, None if w is None else w.cpu(),
                     LAM, eps, dtype)
    r["dparams"] = ref.dparams(r)
    return r


def _case(name):
    """inputs (on the device), the float64 reference and the fp32-torch run of the same statements (both on the CPU), computed once."""
    if name not in _cache:
        N, D, A, eps, cw, seed = CASES[name]
        h, y, s, params, w = ref.random_case(N, D, A, C, seed)
        w = w if cw else None
        hd = h.to(DEV)
        if D % 4:                                          # (read in place: the row stride travels, the pad columns hold NaN)
            buf = torch.full((N, (D + 3) // 4 * 4), float("nan"), device=DEV)
            buf[:, :D] = hd
            hd = buf[:, :D]
        _cache[name] = (hd, y.to(DEV), s.to(DEV), params.to(DEV), None if w is None else w.to(DEV),
                        _ref(h, y, s, params, w, A, eps, torch.float64), _ref(h, y, s, params, w, A, eps, torch.float32))
    return _cache[name]


def _distance(x, r64, key):
    big = r64[key].abs().max().item()
    return (x.double().cpu() - r64[key]).abs().max().item() / (big if big > 0 else 1.0)


def _check(name, got, r64, r32):
    for key, x in zip(OUTPUTS, got):
        d32, dk = _distance(r32[key], r64, key), _distance(x, r64, key)
        bound = max(4 * d32, 8 * EPS32)
        print(f"{name}: {key}: kernels {dk:.3e}, fp32 torch form {d32:.3e}, bound {bound:.3e}")
        assert torch.isfinite(x).all() and dk <= bound, (name, key, dk, bound)


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_match_the_float64_reference(name):
    N, D, A, eps, _, _ = CASES[name]
    h, y, s, params, w, r64, r32 = _case(name)
    print(f"{name}: {int(r64['live'].sum())} live rows of {N}")
    got = F.aux_head(h, y, s, params, (LAM, eps), w, n_classes=C)
    assert got[0].shape == (N, A) and got[1].shape == (N,) and got[2].shape == (N, D) and got[3].shape == (A * D + A,)
    _check(name, got, r64, r32)
    dead = ~r64["live"].to(DEV)
    assert not got[1][dead].any() and not got[2][dead].any()                  # ignored rows: exact zeros
    if N >= 8:
        assert bool(dead.any()) and bool((~dead).any())
        assert not got[1][1].any() and not got[2][1].any()                    # emotion label -1 with a valid auxiliary label


def test_two_calls_give_the_same_bits():
    for name in ("15x100x3", "130x100x16", "130x64x2", "130x301x16", "130x768x16", "130x1024x16"):
        h, y, s, params, w, _, _ = _case(name)
        eps = CASES[name][3]
        a, b = F.aux_head(h, y, s, params, (LAM, eps), w, n_classes=C), F.aux_head(h, y, s, params, (LAM, eps), w, n_classes=C)
        assert all(torch.equal(p, q) for p, q in zip(a, b)), name


def test_all_auxiliary_labels_ignored_cost_exactly_nothing():
    h, y, s, params, w, _, _ = _case("65x20x3")
    logits, rows, dfeat, dparams = F.aux_head(h, y, torch.full_like(s, -1), params, (LAM, 0.1), w, n_classes=C)
    assert not rows.any() and not dfeat.any() and not dparams.any() and torch.isfinite(logits).all()
    # weight 0: the terms and the logits as they are, no gradient
    on = F.aux_head(h, y, s, params, (LAM, 0.1), w, n_classes=C)
    off = F.aux_head(h, y, s, params, (0.0, 0.1), w, n_classes=C)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]) and not off[2].any() and not off[3].any()


@pytest.mark.parametrize("name", ["65x20x3", "130x100x16", "130x301x16", "130x768x16"])
def test_nan_and_inf_in_ignored_rows_do_not_leak(name):
    N, D, A, eps, _, _ = CASES[name]
    h, y, s, params, w, r64, _ = _case(name)
    dead = ~r64["live"].to(DEV)
    bad = h.clone()
    bad[dead] = float("nan")
    bad[torch.nonzero(dead)[0, 0]] = float("inf")
    clean = F.aux_head(h, y, s, params, (LAM, eps), w, n_classes=C)
    got = F.aux_head(bad, y, s, params, (LAM, eps), w, n_classes=C)
    assert torch.isfinite(got[3]).all() and torch.equal(got[3], clean[3])     # a select, not a product with 0
    assert not got[1][dead].any() and not got[2][dead].any()
    assert torch.equal(got[1], clean[1]) and torch.equal(got[2], clean[2]) and torch.equal(got[0][~dead], clean[0][~dead])


@pytest.mark.parametrize("margin", [120.0, -120.0])
def test_logit_margins_of_120_stay_finite(margin):
    N, D, A = 65, 64, 3
    h, y, s, params, w = ref.random_case(N, D, A, C, 31, margin=abs(margin))
    if margin < 0:
        params = torch.cat([-params[: A * D], params[A * D:]])
    for eps in (0.0, 0.1):
        got = F.aux_head(h.to(DEV), y.to(DEV), s.to(DEV), params.to(DEV), (LAM, eps), w.to(DEV), n_classes=C)
        spread = (got[0].max(1).values - got[0].min(1).values).max().item()
        print(f"margin {margin}: largest spread of a row's logits {spread:.1f}")
        assert spread > 100.0
        assert all(torch.isfinite(x).all() for x in got)
        r64 = _ref(h, y, s, params, w, A, eps, torch.float64)
        r32 = _ref(h, y, s, params, w, A, eps, torch.float32)
        _check(f"margin {margin} eps {eps}", got, r64, r32)


@pytest.mark.parametrize("name", ["15x100x3", "130x100x16", "130x301x16", "130x768x16"])
def test_head_under_autograd_is_the_linear_layer(name):
    """head(features) and its backward (the join and parameter-gradient kernels with the upstream gradient as g) against nn.Linear in
    float64, by the same rule."""
    N, D, A, _, _, seed = CASES[name]
    h = _case(name)[0]
    torch.manual_seed(seed)
    head = AuxiliaryHead(D, A).to(DEV)
    up = torch.randn(N, A, generator=torch.Generator().manual_seed(seed))
    res = {}
    for dtype in (torch.float64, torch.float32):
        lin = torch.nn.Linear(D, A).to(dtype)
        lin.load_state_dict({k: v.cpu().to(dtype) for k, v in head.state_dict().items()})
        x = h.cpu().to(dtype).requires_grad_(True)
        out = lin(x)
        out.backward(up.to(dtype))
        res[dtype] = {"logits": out.detach(), "dfeat": x.grad, "dparams": torch.cat([lin.weight.grad.reshape(-1), lin.bias.grad])}
    x = h.clone().contiguous().requires_grad_(True)
    out = head(x.view(1, N, D))
    assert out.shape == (1, N, A)
    out.backward(up.to(DEV).view(1, N, A))
    got = {"logits": out.detach().view(N, A), "dfeat": x.grad, "dparams": head.params.grad}
    for key in ("logits", "dfeat", "dparams"):
        d32, dk = _distance(res[torch.float32][key], res[torch.float64], key), _distance(got[key], res[torch.float64], key)
        bound = max(4 * d32, 8 * EPS32)
        print(f"{name}: head under autograd: {key}: kernels {dk:.3e}, fp32 torch {d32:.3e}, bound {bound:.3e}")
        assert dk <= bound
    assert torch.equal(head.weight, head.params[: A * D].view(A, D)) and list(head.state_dict()) == ["weight", "bias"]


def test_loss_module_matches_the_reference_and_differentiates():
    name = "130x100x16"
    N, D, A, eps, _, seed = CASES[name]
    h, y, s, params, w, _, _ = _case(name)
    head = AuxiliaryHead(D, A).to(DEV)
    with torch.no_grad():
        head.params.copy_(params)
    crit = M2FAuxiliaryLoss(weight=w, label_smoothing=eps)
    x = h.clone().requires_grad_(True)
    loss = crit(x, head, y, s)
    loss.backward()
    r64 = ref.aux_head(h.cpu(), y.cpu(), s.cpu(), head.weight.detach().cpu(), head.bias.detach().cpu(), C, w.cpu(), 1.0, eps)
    r32 = ref.aux_head(h.cpu(), y.cpu(), s.cpu(), head.weight.detach().cpu(), head.bias.detach().cpu(), C, w.cpu(), 1.0, eps, torch.float32)
    want = (r64["aux"] / r64["den"]).item()
    d32 = abs((r32["aux"] / r32["den"]).item() - want) / abs(want)
    dk = abs(loss.item() - want) / abs(want)
    print(f"loss module: {loss.item()!r} against {want!r}: {dk:.3e}, fp32 torch form {d32:.3e}")
    assert dk <= max(4 * d32, 8 * EPS32)
    for key, g in (("dfeat", x.grad), ("dparams", head.params.grad)):
        r = {"dfeat": r64["dfeat"] / r64["den"], "dparams": ref.dparams(r64) / r64["den"]}
        q = {"dfeat": r32["dfeat"] / r32["den"], "dparams": ref.dparams(r32) / r32["den"]}
        d32, dk = _distance(q[key], r, key), _distance(g, r, key)
        print(f"loss module: {key}: kernels {dk:.3e}, fp32 torch form {d32:.3e}")
        assert dk <= max(4 * d32, 8 * EPS32)
    assert crit.last_logits.shape == (N, A) and crit.last_terms.shape == (N,)


def test_the_entry_refuses_what_it_cannot_run():
    h, y, s, params, w, _, _ = _case("15x100x3")
    with pytest.raises(ValueError, match="aux_head: params holds"):
        F.aux_head(h, y, s, params[:-1].clone(), (LAM, 0.0), w, n_classes=C)
    with pytest.raises(ValueError, match="aux_head: params holds"):
        F.aux_head(h, y, s, torch.zeros(17 * 101, device=DEV), (LAM, 0.0), w, n_classes=C)          # A = 17
    with pytest.raises(ValueError, match="aux_head: aux_labels must be int64"):
        F.aux_head(h, y, s[:-1], params, (LAM, 0.0), w, n_classes=C)
    with pytest.raises(ValueError, match="aux weight must be >= 0"):
        F.aux_head(h, y, s, params, (-1.0, 0.0), w, n_classes=C)
    with pytest.raises(ValueError, match="1 <= D <= 1024"):
        F.aux_head(torch.zeros(4, 1028, device=DEV), y[:4], s[:4], torch.zeros(2 * 1029, device=DEV), (LAM, 0.0), None, n_classes=C)
    assert torch.isfinite(F.aux_head(h, y, s, params, (LAM, 0.0), w, n_classes=C)[3]).all()          # ... and still runs


# ---- the join launch on caller-owned buffers: the gate, the accumulation and the bf16 shadow ------------------------------------------------
@pytest.mark.parametrize("add", [True, False])
@pytest.mark.parametrize("N,D,A", [(37, 100, 3), (37, 301, 16), (70, 768, 3), (37, 1024, 16)])
def test_join_writes_the_bf16_rounding_of_what_it_leaves_in_dh(N, D, A, add):
    """The step's join launch (m2f_aux_head_join: the same kernel, a caller-owned dh and shadow) at one, two and four 16-byte pieces per
    lane.  The shadow holds EXACTLY the bf16 rounding (nearest even: torch's cast) of every dh element the launch wrote - bit equality,
    with the gate, its scale and the accumulation in; the columns behind D keep what they held in both buffers (the row stride is D
    rounded up to 8, as the plan pads, plus NaN in h's pad columns); dh itself against float64 by the kernel tests' rule."""
    g = torch.Generator().manual_seed(1000 * N + D + A)
    ld = (D + 7) // 8 * 8
    hbuf = torch.full((N, ld), float("nan"))
    hbuf[:, :D] = torch.randn(N, D, generator=g) * (torch.rand(N, D, generator=g) >= 0.4)           # <= 0 where the gate is shut
    dh0 = torch.randn(N, ld, generator=g)
    gr = torch.randn(N, A, generator=g) * (torch.rand(N, 1, generator=g) >= 0.2)                     # some rows carry no gradient
    params = torch.cat([(torch.randn(A, D, generator=g) / D ** 0.5).reshape(-1), torch.randn(A, generator=g)])
    scale, lam, gate = 0.37, 0.8, 1.0 / 0.6
    dh = dh0.to(DEV)
    SENTINEL = 0x1234
    shadow = torch.full((N * ld,), SENTINEL, dtype=torch.int16, device=DEV)
    out = F.aux_head_join(dh[:, :D], gr.to(DEV), params.to(DEV), h=hbuf.to(DEV)[:, :D], scale=scale, weight=lam, gate_scale=gate, add=add,
                          shadow=shadow)
    assert out.data_ptr() == dh.data_ptr()
    got, sh = dh.cpu(), shadow.cpu().view(N, ld)
    assert torch.isfinite(got).all()
    # the shadow: the bf16 bits of dh as it now stands, element for element
    want_bits = got[:, :D].contiguous().to(torch.bfloat16).view(torch.int16)
    wrong = int((sh[:, :D] != want_bits).sum())
    print(f"{N} x {D} x {A} add {add}: {wrong} of {N * D} shadow elements differ from the bf16 rounding of dh")
    assert wrong == 0 and torch.equal(sh[:, :D], want_bits)
    truncated = (got[:, :D].contiguous().view(torch.int32) >> 16).to(torch.int16)
    assert bool((want_bits != truncated).any())                                                    # (rounding, not truncation, is what was checked)
    assert bool((sh[:, D:] == SENTINEL).all()) and torch.equal(got[:, D:], dh0[:, D:])             # the pad columns: untouched
    # dh: float64 and the same statements in fp32
    res = {}
    for dtype in (torch.float64, torch.float32):
        W = params[: A * D].view(A, D).to(dtype)
        gatev = torch.where(hbuf[:, :D] > 0, torch.tensor(gate, dtype=dtype), torch.tensor(0.0, dtype=dtype))
        term = gatev * ((torch.tensor(scale, dtype=dtype) * torch.tensor(lam, dtype=dtype)) * (gr.to(dtype) @ W))
        res[dtype] = (dh0[:, :D].to(dtype) if add else 0) + term
    big = res[torch.float64].abs().max().item()
    d32 = (res[torch.float32].double() - res[torch.float64]).abs().max().item() / big
    dk = (got[:, :D].double() - res[torch.float64]).abs().max().item() / big
    print(f"{N} x {D} x {A} add {add}: dh: kernel {dk:.3e}, fp32 torch form {d32:.3e}, bound {max(4 * d32, 8 * EPS32):.3e}")
    assert dk <= max(4 * d32, 8 * EPS32)
    shut = hbuf[:, :D] <= 0
    assert torch.equal(got[:, :D][shut], dh0[:, :D][shut] if add else torch.zeros(int(shut.sum())))  # a shut gate: exactly nothing joins


def test_loss_module_without_an_emotion_label_is_zero():
    h, y, s, params, w, _, _ = _case("15x100x3")
    head = AuxiliaryHead(100, 3).to(DEV)
    x = h.clone().requires_grad_(True)
    loss = M2FAuxiliaryLoss(weight=w)(x, head, torch.full_like(y, -1), s)
    loss.backward()
    assert loss.item() == 0.0 and not x.grad.any() and not head.params.grad.any()
