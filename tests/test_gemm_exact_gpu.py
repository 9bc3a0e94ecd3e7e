"""Every GEMM form m2f_gemm / m2f_gemm_fp8 / m2f_gemm_p8 dispatches to, held to EXACT results.

Operands are small integers (tests/golden/exact_gemm.py; tests/test_gemm_exact_cpu.py checks the premises): exact in fp32, bf16 and
e4m3, with every partial sum below 2^24, so a correct kernel's fp32 result equals the float64 reference bit for bit whatever its
summation order.  Epilogue terms are integers up to 2^12 (exact in fp32, not in bf16).  Each case
  * asserts the kernel form it covers (m2f_gemm_last_form, set by the host dispatch code);
  * writes into a view of a NaN-filled buffer with guard rows and columns, and asserts the guard is still NaN afterwards;
  * compares with torch.equal against the float64 reference cast to fp32.
Rounding probes (fp32 values below, at and above bf16 / e4m3 ties) with a one-hot operand turn the GEMM into a copy of the ROUNDED
other operand: every fp32-source bf16 staging path (A and B side, both segments, 16-byte and element-wise, k-contiguous and
row-major) and the skinny bf16 path must round exactly as torch's .to(torch.bfloat16) does; fp32 mode must pass full 24-bit
mantissas through unchanged.  Output rounding (bf16 shadows, e4m3 results, the e4m3 quantiser) is compared bit for bit with torch.

Not exact, stated bounds: GELU, against float64 GELU of the exact pre-activation - the erf of common.h is Abramowitz-Stegun 7.1.26
(1.5e-7) in the fp32-source kernels and a degree-13 polynomial (4.33e-4) in the bf16 / fp8 kernels; the bound is 0.5 |x| erf_err
plus 4 fp32 ulps of |x|.

The same integer treatment covers the parameter-shadow cast of the fused optimizer (ties, subnormals, overflow to inf) and the
implicit-GEMM convolutions: mel_resnet.conv exactly (fp32 result bit for bit against float64 conv2d, bf16 result as torch rounds
it); functional.w2v_conv_layer and functional.w2v_pos_conv end in GELU, so they are held to the erf bound above around the exact
integer pre-activation - a bound below half an integer step, so a dropped or misplaced product still shows.

Not reachable here: the NN form through TRANSPOSED bf16 shadows (m2f_gemm passes no transposed shadows; only plans do) and
grouped multi-problem launches (plans only; the model tests cover them).
The dispatch itself - which form a launch takes at each threshold - is pinned by tests/golden/gemm_dispatch_forms.json: one case per
form is launched here and must take the recorded form, which m2f_gemm_form (the chooser without a launch) must name too; at a threshold
the two neighbours and the register-staged form agree bit for bit.
The module prints a coverage table: form -> cases -> elements compared.
"""
import ctypes
import math
import os
import sys
from collections import defaultdict

import pytest
import torch

import exact_gemm as X

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAN = float("nan")

FORMS = {1: "fp32-source 64x64", 2: "fp32-source 128x128", 3: "fp32-source split-K", 4: "bf16-source 64x64",
         5: "bf16-source 128x128", 6: "bf16-source 256x128", 7: "ring 64x64", 8: "ring 128x64", 9: "ring 128x128",
         10: "ring 256x128", 11: "p8 KC", 12: "p8 RC", 13: "skinny NT", 14: "skinny NN", 15: "fp8 128x128",
         16: "fp8 256x128", 17: "fp8 ring 256x128", 18: "fp8 p8"}
VEC, SRC16 = 0x100, 0x200
COVERAGE = defaultdict(lambda: [0, 0])
NOT_REACHED = {"NN through transposed shadows": "m2f_gemm passes no transposed shadows (only plans do)",
               "grouped multi-problem launches": "plans only"}


@pytest.fixture(scope="module", autouse=True)
def _coverage_table():
    yield
    print("\n\nexact GEMM coverage: form -> cases -> elements compared")
    for key in sorted(COVERAGE):
        c, e = COVERAGE[key]
        print(f"  {key:<44s} {c:6d} {e:14,d}")
    for k, why in NOT_REACHED.items():
        print(f"  {k:<44s} not reached: {why}")


def _lib():
    import mer_amd  # noqa: F401
    from mer_amd import runtime
    return runtime.lib()


def _form():
    return _lib().m2f_gemm_last_form()


def _record(key, n):
    COVERAGE[key][0] += 1
    COVERAGE[key][1] += int(n)


def _assert_form(want, vec=None, what=""):
    got = _form()
    assert got & 0xFF == want, f"{what}: dispatched to {FORMS.get(got & 0xFF, got & 0xFF)} (0x{got:x}), not {FORMS[want]}"
    if vec is not None:
        assert bool(got & VEC) == vec, f"{what}: 16-byte staging {bool(got & VEC)}, expected {vec}"
    return FORMS[want] + ("" if vec is None else (" vec" if vec else " element-wise"))


def _operand(t, unaligned):
    """a CUDA copy of 2-D t; unaligned: a view with a leading dimension % 4 != 0 (element-wise staging)"""
    r, c = t.shape
    if not unaligned:
        return t.to(DEV).contiguous()
    ld = c + 1 if (c + 1) % 4 else c + 2
    buf = torch.zeros(r, ld, device=DEV)
    buf[:, :c] = t.to(DEV)
    return buf[:, :c]


def _guarded(M, N, unaligned=False, fill=None):
    """(buffer, output view, guard mask): guard rows above and below, guard columns; unaligned: ldc % 4 != 0 and a base that is
    not 16-byte aligned"""
    if unaligned:
        col0, ld = 1, N + 2 if (N + 2) % 4 else N + 3
    else:
        col0, ld = 0, (N + 3) // 4 * 4 + 8
    buf = torch.full((M + 2, ld), NAN, device=DEV)
    out = buf[1:M + 1, col0:col0 + N]
    if fill is not None:
        out.copy_(fill)
    mask = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    mask[1:M + 1, col0:col0 + N] = False
    return buf, out, mask


def _guard_ok(buf, mask, what):
    g = buf[mask]
    assert torch.isnan(g).all(), f"{what}: {int((~torch.isnan(g)).sum())} guard elements written"


def _equal(got, ref, what):
    ref32 = ref.float()
    assert torch.equal(ref32.double(), ref), f"{what}: reference not exact in fp32"
    if not torch.equal(got, ref32):
        d = got != ref32
        i = d.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(d.sum())} of {got.numel()} differ; first at {i}: {got[tuple(i)].item()!r} "
                             f"vs {ref32[tuple(i)].item()!r}")


def _layout_operands(A, B, layout, unaligned):
    """logical A [M, K], B [N, K] -> the physical operands of NT / NN / TN"""
    from mer_amd import functional as F
    if layout == F.NT:
        return _operand(A, unaligned), _operand(B, unaligned)
    if layout == F.NN:
        return _operand(A, unaligned), _operand(B.t().contiguous(), unaligned)
    return _operand(A.t().contiguous(), unaligned), _operand(B.t().contiguous(), unaligned)


def _gemm_case(form, M, N, K, layout, prec, *, K1=0, tile=0, src16=False, split_k=False, terms=(), unaligned=False,
               unaligned_out=None, scaled=False, seed=0, vec=None, key=None):
    """one integer GEMM through functional.gemm: exact result, untouched guard, dispatched form"""
    from mer_amd import functional as F
    unaligned_out = unaligned if unaligned_out is None else unaligned_out
    Kt = K + K1
    A, B = X.ints((M, Kt), seed), X.ints((N, Kt), seed + 1)
    if scaled:
        A, B = A * X.pow2(M, seed + 2)[:, None], B * X.pow2(N, seed + 3)[:, None]
    kw = {}
    a, b = _layout_operands(A[:, :K], B[:, :K], layout, unaligned)
    if K1:
        kw["a1"], kw["b1"] = _layout_operands(A[:, K:], B[:, K:], layout, unaligned)
    Ad, Bd = A.double().to(DEV), B.double().to(DEV)
    if "relu_a" in terms:
        kw["relu_a"] = True
        Ad = Ad.clamp_min(0)
    if "relu_b" in terms:
        kw["relu_b"] = True
        Bd = Bd.clamp_min(0)
    pre = Ad @ Bd.t()
    if "bias" in terms:
        bias = X.terms((N,), seed + 4).to(DEV)
        kw["bias"] = bias
        pre = pre + bias.double()
    if "relu" in terms:
        kw["relu_out"] = True
        pre = pre.clamp_min(0)
    ref = pre
    drop = "drop" in terms
    if drop:
        kw.update(drop_site=7, drop_p=0.5, rng=torch.tensor([11, 22, 3, 0], dtype=torch.int32, device=DEV))
    res = gate = c0 = None
    if "res" in terms:
        res = X.terms((M, N), seed + 5).to(DEV)
        kw["res"] = res
    if "gate" in terms:
        gate = X.ints((M, N), seed + 6).to(DEV)
        kw.update(gate=gate, gate_scale=1.25)
    if "acc" in terms:
        c0 = X.terms((M, N), seed + 7).to(DEV)
        kw["accumulate"] = True
    bias_grad = "bias_grad" in terms
    buf, out, mask = _guarded(M, N, unaligned_out, fill=c0)
    r = F.gemm(a, b, layout, prec, tile=tile, split_k=split_k, src16=src16, out=out, bias_grad=bias_grad, **kw)
    torch.cuda.synchronize()
    what = f"{FORMS[form]} {['NT', 'NN', 'TN'][layout]} prec={prec} {M}x{N}x{K}+{K1} {sorted(terms)} unaligned={unaligned}"
    name = _assert_form(form, vec, what)
    _guard_ok(buf, mask, what)
    if drop:
        keep = out == (2 * pre).float() if res is None and gate is None and c0 is None else None
        if keep is None:                                     # the mask depends on (site, rng, row, col, N) only: take it from a run without the other terms
            kw2 = {k: v for k, v in kw.items() if k not in ("res", "gate", "gate_scale", "accumulate")}
            plain = F.gemm(a, b, layout, prec, tile=tile, split_k=split_k, src16=src16, **kw2)
            keep = plain == (2 * pre).float()
        nz = pre != 0                                        # (where the product is 0, kept and dropped look alike)
        assert nz.sum().item() > 1000, f"{what}: too few nonzero results to see the dropout rate"
        frac = (keep & nz).sum().item() / nz.sum().item()
        assert 0.45 < frac < 0.55, f"{what}: kept fraction {frac}"
        keep = keep | ~nz
        ref = torch.where(keep, 2 * pre, torch.zeros_like(pre))
    if res is not None:
        ref = ref + res.double()
    if gate is not None:
        ref = torch.where(gate > 0, ref * 1.25, torch.zeros_like(ref))
    if c0 is not None:
        ref = ref + c0.double()
    _equal(out, ref, what)
    n = out.numel()
    if bias_grad:
        _, bg = r
        _equal(bg, Ad.sum(1), what + " bias_grad")
        n += bg.numel()
    _record(key or name, n)


# ---- fp32-source (fp32 mode; bf16 mode staged from fp32 originals) ----------------------------------------------------------

def _bk(prec, tile, src16=False):
    from mer_amd import runtime
    if src16 or prec == runtime.BF16:
        return 128 if tile == 64 else 64
    return 64 if tile == 64 else 32


def _edge_shapes(T, BK):
    return [(T - 1, T + 1, T), (T, T - 1, T + 1), (T + 1, T, T - 1), (3 * T + 5, 2 * T + 3, 5 * BK + 7), (T + 3, T + 5, 12),
            (2 * T + 7, T + 9, BK - 1), (T + 2, 2 * T + 1, BK + 1)]


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("prec", [0, 1])
def test_fp32_source_forms_are_exact(prec, tile, layout):
    form = 1 if tile == 64 else 2
    BK = _bk(prec, tile)
    for i, (M, N, K) in enumerate(_edge_shapes(tile, BK)):
        _gemm_case(form, M, N, K, layout, prec, tile=tile, seed=10 * i, unaligned=i % 2 == 1, vec=False if i % 2 else None)
    # 16-byte staging on every operand (k, rows, leading dimensions multiples of 4), and its element-wise twin
    _gemm_case(form, 2 * tile, tile + 4, 4 * BK, layout, prec, tile=tile, seed=91, vec=True)
    _gemm_case(form, 2 * tile, tile + 4, 4 * BK, layout, prec, tile=tile, seed=91, unaligned=True, vec=False)
    # two segments, K0 ending inside a k-tile; scaled operands
    _gemm_case(form, tile + 5, tile + 3, 40, layout, prec, K1=BK + 3, tile=tile, seed=92)
    _gemm_case(form, tile + 5, tile + 3, 40, layout, prec, K1=BK + 3, tile=tile, seed=93, unaligned=True, vec=False)
    _gemm_case(form, 2 * tile + 1, tile, 3 * BK, layout, prec, tile=tile, seed=94, scaled=True)


EPI_TERMS = [("bias",), ("bias", "relu"), ("res",), ("gate",), ("acc",), ("relu_a",), ("relu_b",), ("drop",),
             ("bias", "relu", "drop", "res", "gate", "acc", "relu_a")]


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("prec", [0, 1])
def test_fp32_source_epilogue_terms_are_exact(prec, layout):
    for i, terms in enumerate(EPI_TERMS):
        _gemm_case(1, 130, 97, 200, layout, prec, tile=64, terms=terms, seed=200 + i)
        _gemm_case(2, 130, 131, 100, layout, prec, tile=128, terms=terms, seed=300 + i, unaligned_out=True)
    if layout == 2:
        _gemm_case(1, 100, 70, 150, layout, prec, tile=64, terms=("bias_grad",), seed=399)
        _gemm_case(2, 130, 70, 150, layout, prec, tile=128, terms=("bias_grad", "relu_b"), seed=398)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("prec", [0, 1])
def test_split_k_is_exact(prec, layout):
    for i, (M, N, K, K1, terms) in enumerate([(130, 200, 1000, 0, ()), (63, 65, 515, 0, ()), (130, 70, 300, 229, ()),
                                              (100, 129, 600, 0, ("bias", "relu", "res", "gate", "acc", "drop")),
                                              (64, 64, 256, 200, ("bias", "relu_a", "acc")), (130, 97, 600, 0, ("drop",))]):
        _gemm_case(3, M, N, K, layout, prec, K1=K1, tile=64, split_k=True, terms=terms, seed=400 + i, unaligned_out=i % 2 == 1)


# ---- bf16-source register-staged forms ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("tile", [64, 128])
def test_bf16_source_forms_are_exact(tile, layout):
    form = 4 if tile == 64 else 5
    BK = _bk(1, tile, True)
    for i, (M, N, K) in enumerate(_edge_shapes(tile, BK)):
        _gemm_case(form, M, N, K, layout, 1, tile=tile, src16=True, seed=500 + 10 * i, unaligned_out=i % 2 == 1)
    _gemm_case(form, tile + 5, tile + 3, 40, layout, 1, K1=BK + 3, tile=tile, src16=True, seed=590)
    _gemm_case(form, 2 * tile + 1, tile, 3 * BK, layout, 1, tile=tile, src16=True, seed=591, scaled=True)
    for i, terms in enumerate(EPI_TERMS):
        _gemm_case(form, 2 * tile + 3, tile + 7, 2 * BK + 9, layout, 1, tile=tile, src16=True, terms=terms, seed=600 + i)
    if layout == 2:
        _gemm_case(form, 100, 70, 150, layout, 1, tile=tile, src16=True, terms=("bias_grad", "relu_b"), seed=699)


def test_bf16_source_256x128_is_exact():
    """>= 1,024 tiles of 256x128 with a pinned tile (no ring / p8): the register-staged 256x128 build"""
    _gemm_case(6, 8192 - 3, 4096 - 5, 72, 0, 1, tile=128, src16=True, seed=700, terms=("bias", "res"))
    _gemm_case(6, 8192, 4096, 136, 0, 1, tile=128, src16=True, seed=701, terms=("gate", "acc"))


# ---- ring forms (tile = 0: automatic) ----------------------------------------------------------------------------------------

WIDTH = {7: 512, 8: 1344, 9: 3328, 10: 4096}
ROWS = {10: 4001}


@pytest.mark.parametrize("form", [7, 8, 9, 10])
def test_ring_forms_are_exact(form):
    W, R = WIDTH[form], ROWS.get(form, 1001)
    full = ("bias", "relu", "res") if form == 10 else ("bias", "relu", "res", "gate", "acc", "drop", "relu_a")
    cases = [(R, W + 2, 200, 0, ("bias", "relu")), (R, W + 8, 1000, 0, ("res",)), (R, W, 40, 0, ()),   # ragged; short k
             (R, W, 63, 0, ()), (R, W, 65, 0, ()), (R, W, 129, 0, ()), (R, W, 191, 0, ()),              # ring depth +- 1 k-tiles
             (R, W, 1000, 72, full), (R, W + 1, 520, 0, full)]
    for i, (M, N, K, K1, terms) in enumerate(cases):
        _gemm_case(form, M, N, K, 0, 1, K1=K1, src16=True, terms=terms, seed=800 + 10 * form + i, unaligned_out=N % 4 != 0)


# ---- the dispatch thresholds (tests/golden/gemm_dispatch_forms.json, recorded from the build in front of csrc/gemm_dispatch.hip) --------

def _dispatch_cases():
    import json
    import make_gemm_dispatch_forms as D
    return D, {c["name"]: c for c in json.load(open(D.FIXTURE))["cases"]}


def _one_case_per_form():
    """the cheapest fixture case of every form"""
    _, cases = _dispatch_cases()
    best = {}
    for c in cases.values():
        cost = c["M"] * c["N"] * (c["K0"] + c["K1"])
        if c["form"] & 0xFF not in best or cost < best[c["form"] & 0xFF][0]:
            best[c["form"] & 0xFF] = (cost, c["name"])
    return [name for _, (_, name) in sorted(best.items())]


@pytest.mark.parametrize("name", _one_case_per_form())
def test_a_launch_takes_the_form_the_fixture_and_the_dry_entry_name(name):
    """m2f_gemm / m2f_gemm_fp8 dispatch to the recorded form, and m2f_gemm_form - the same chooser, nothing launched - names it too"""
    D, cases = _dispatch_cases()
    c = cases[name]
    got, _ = D.run_case(c)
    dry = _lib().m2f_gemm_form(*D.dry_args(c), None)
    assert got == c["form"] == dry, f"{name}: launched 0x{got:03x}, recorded 0x{c['form']:03x}, m2f_gemm_form 0x{dry:03x}"
    _record("dispatch: " + FORMS[got & 0xFF], 0)


@pytest.mark.parametrize("below,at", [("ring64x64_79_tiles", "ring64x64_80_tiles"), ("ring128x64_149_tiles", "ring128x64_150_tiles"),
                                      ("ring128x128_199_tiles", "ring128x128_200_tiles"), ("p8_255_tiles", "p8_256_tiles")])
def test_results_do_not_move_at_a_threshold(below, at):
    """the first launch at a threshold, its neighbour below it and the register-staged form of the same problem (a forced tile takes no
    LDS-DMA form), on the same integer data: the rows they share agree bit for bit"""
    D, cases = _dispatch_cases()
    lo, hi = cases[below], cases[at]
    assert (lo["N"], lo["K0"], lo["K1"], lo["bits"]) == (hi["N"], hi["K0"], hi["K1"], hi["bits"]) and lo["M"] < hi["M"]
    A, B = X.ints((hi["M"], hi["K0"]), 21).to(DEV), X.ints((hi["N"], hi["K0"]), 22).to(DEV)
    f_hi, c_hi = D.run_case(hi, A, B)
    f_lo, c_lo = D.run_case(lo, A[:lo["M"]].contiguous(), B)
    f_st, c_st = D.run_case(dict(hi, tile=64), A, B)
    assert (f_hi, f_lo) == (hi["form"], lo["form"]) and f_hi != f_lo and f_st & 0xFF == 4, (hex(f_hi), hex(f_lo), hex(f_st))
    _equal(c_st, A.double() @ B.double().t(), f"{at}: register-staged")
    assert torch.equal(c_hi, c_st), f"{at}: {FORMS[f_hi & 0xFF]} differs from the register-staged form"
    assert torch.equal(c_lo, c_st[:lo["M"]]), f"{below}: {FORMS[f_lo & 0xFF]} differs from the register-staged form"
    _record("dispatch: across " + FORMS[f_hi & 0xFF] + " threshold", c_hi.numel() + c_lo.numel())


# ---- eight-phase form --------------------------------------------------------------------------------------------------------

def test_p8_kc_through_the_dispatcher_is_exact():
    _gemm_case(11, 8192, 2048, 512, 0, 1, src16=True, terms=("bias", "relu", "res"), seed=900)
    _gemm_case(11, 8192, 2048, 1024, 0, 1, src16=True, terms=(), seed=901, scaled=True)


def _p8_tool():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import p8_bench
    return p8_bench


def _p8(rc, M, N, K, a16, b16, out, bias=None, res=None, act=0, relu_b=0, bias_grad=None):
    p8_bench = _p8_tool()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    r = _lib().m2f_gemm_p8(rc, M, N, K, p(a16), a16.stride(0), p(b16), b16.stride(0), p(out), out.stride(0), p(bias), p(res),
                           res.stride(0) if res is not None else 0, act, 0, relu_b, p(bias_grad), p(p8_bench.SCRATCH),
                           p8_bench.SCRATCH.numel(), 0, None)
    assert r == 0, f"m2f_gemm_p8 -> {r}"


@pytest.mark.parametrize("M,N,K", [(300, 768, 1000), (512, 256, 64), (7, 300, 48), (768, 300, 1024)])
def test_p8_rc_direct_is_exact(M, N, K):
    """weight-gradient form: C = A^T relu(B), bias_grad = row sums of A^T, over row-major bf16 operands"""
    A, B = X.ints((K, M), M + N), X.ints((K, N), K)
    a16 = torch.zeros(K, (M + 7) // 8 * 8, dtype=torch.bfloat16, device=DEV)
    b16 = torch.zeros(K, (N + 7) // 8 * 8, dtype=torch.bfloat16, device=DEV)
    a16[:, :M], b16[:, :N] = A.to(DEV), B.to(DEV)
    buf, out, mask = _guarded(M, N)
    bg = torch.full((M + 8,), NAN, device=DEV)
    _p8(1, M, N, K, a16, b16, out, relu_b=1, bias_grad=bg[:M])
    torch.cuda.synchronize()
    _assert_form(12, what="p8 RC")
    _guard_ok(buf, mask, "p8 RC")
    assert torch.isnan(bg[M:]).all()
    Ad, Bd = A.double().to(DEV), B.double().to(DEV)
    _equal(out, Ad.t() @ Bd.clamp_min(0), f"p8 RC {M}x{N}x{K}")
    _equal(bg[:M], Ad.sum(0), f"p8 RC bias_grad {M}x{N}x{K}")
    _record(FORMS[12], out.numel() + M)


@pytest.mark.parametrize("M,N,K,act", [(512, 768, 1024, 1), (300, 252, 64, 0), (256, 256, 128, 1)])
def test_p8_kc_direct_is_exact(M, N, K, act):
    A, B = X.ints((M, K), M), X.ints((N, K), N + 1)
    bias, res = X.terms((N,), 3).to(DEV), X.terms((M, N), 4).to(DEV)
    buf, out, mask = _guarded(M, N)
    _p8(0, M, N, K, A.to(DEV).to(torch.bfloat16), B.to(DEV).to(torch.bfloat16), out, bias=bias, res=res, act=act)
    torch.cuda.synchronize()
    _assert_form(11, what="p8 KC direct")
    _guard_ok(buf, mask, "p8 KC direct")
    pre = A.double().to(DEV) @ B.double().to(DEV).t() + bias.double()
    _equal(out, (pre.clamp_min(0) if act else pre) + res.double(), f"p8 KC {M}x{N}x{K}")
    _record(FORMS[11] + " direct", out.numel())


# ---- skinny ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16_src16"])
def test_skinny_forms_are_exact(mode):
    from mer_amd import functional as F, runtime
    prec = runtime.F32 if mode == "f32" else runtime.BF16
    src16 = mode == "bf16_src16"
    for (T, K, ncls, vec) in [(300, 768, 7, True), (37, 50, 3, False), (1024, 1024, 8, True)]:
        h, w, bias = X.ints((T, K), T).to(DEV), X.ints((ncls, K), K).to(DEV), X.terms((ncls,), 1).to(DEV)
        buf, out, mask = _guarded(T, ncls, unaligned=not vec)
        F.gemm(h, w, F.NT, prec, bias=bias, src16=src16, out=out)
        torch.cuda.synchronize()
        name = _assert_form(13, vec=vec, what=f"skinny NT {mode}")
        assert bool(_form() & SRC16) == src16
        _guard_ok(buf, mask, "skinny NT")
        _equal(out, h.double() @ w.double().t() + bias.double(), f"skinny NT {T}x{ncls}x{K}")
        _record(name, out.numel())
        dl, gate = X.ints((T, ncls), T + 1).to(DEV), X.ints((T, K), T + 2).to(DEV)
        buf, out, mask = _guarded(T, K, unaligned=not vec)
        F.gemm(dl, w, F.NN, prec, gate=gate, gate_scale=1.25, src16=src16, out=out)
        torch.cuda.synchronize()
        name = _assert_form(14, vec=vec, what=f"skinny NN {mode}")
        _guard_ok(buf, mask, "skinny NN")
        ref = dl.double() @ w.double()
        _equal(out, torch.where(gate > 0, ref * 1.25, torch.zeros_like(ref)), f"skinny NN {T}x{K}x{ncls}")
        _record(name, out.numel())


# ---- rounding probes ---------------------------------------------------------------------------------------------------------

def _probe_matrix(rows, cols, seed, values):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, values.numel(), (rows, cols), generator=g)
    return values[idx]


def _probe_case(form, layout, prec, side, unaligned, K1, tile, values, expect, seed):
    """C = P B^T with B one-hot (side 'a'), or A P^T with A one-hot (side 'b'): a copy of `expect`(P)."""
    from mer_amd import functional as F
    M, N, K = (68, 64, 96) if tile == 64 else (132, 128, 160)        # rows, k and leading dimensions % 4 == 0: 16-byte staging
    Kt = K + K1
    P = _probe_matrix(M if side == "a" else N, Kt, seed, values)
    H, _ = X.one_hot(N if side == "a" else M, Kt, seed + 1)
    A, B = (P, H) if side == "a" else (H, P)
    kw = {}
    a, b = _layout_operands(A[:, :K], B[:, :K], layout, unaligned)
    if K1:
        kw["a1"], kw["b1"] = _layout_operands(A[:, K:], B[:, K:], layout, unaligned)
    buf, out, mask = _guarded(M, N, unaligned)
    F.gemm(a, b, layout, prec, tile=tile, out=out, **kw)
    torch.cuda.synchronize()
    what = f"probes side {side} layout {layout} prec {prec} K1={K1} unaligned={unaligned}"
    name = _assert_form(form, vec=not unaligned, what=what)
    _guard_ok(buf, mask, what)
    Ae, Be = (expect(A), B) if side == "a" else (A, expect(B))
    ref = Ae.double().to(DEV) @ Be.double().to(DEV).t()
    _equal(out, ref, what)
    _record(name + " (probes)", out.numel())
    return out


def _rne(t):
    return t.to(torch.bfloat16).float()


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("tile", [64, 128])
def test_bf16_staging_rounds_to_nearest_even(tile, layout):
    """every fp32-source bf16 staging path rounds exactly as torch: A and B side, both segments, 16-byte and element-wise"""
    values, _ = X.bf16_probes()
    form = 1 if tile == 64 else 2
    for side in "ab":
        for unaligned in (False, True):
            for K1 in (0, 40):
                _probe_case(form, layout, 1, side, unaligned, K1, tile, values, _rne, seed=1000 + 7 * layout + tile + K1)


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("tile", [64, 128])
def test_fp32_mode_passes_24_bit_mantissas_through(tile, layout):
    values = X.fp24_probes(4096, 3)
    form = 1 if tile == 64 else 2
    for side in "ab":
        for unaligned in (False, True):
            _probe_case(form, layout, 0, side, unaligned, 40, tile, values, lambda t: t, seed=1100 + layout + tile)


def test_bf16_staging_of_subnormals():
    """fp32 subnormals through bf16 staging and the bf16 MFMA: neither the conversion nor the MFMA flushes them - every path gives
    torch's rounding, bit for bit (measured on MI355X: all 4,087 elements per path)."""
    from mer_amd import functional as F
    values = X.bf16_subnormal_probes()
    P = _probe_matrix(67, 96, 5, values)
    H, _ = X.one_hot(61, 96, 6)
    want = (_rne(P).double().to(DEV) @ H.double().to(DEV).t()).float()
    for layout in (0, 1, 2):
        for unaligned in (False, True):
            a, b = _layout_operands(P, H, layout, unaligned)
            got = F.gemm(a, b, layout, 1, tile=64)
            torch.cuda.synchronize()
            _assert_form(1, vec=False if unaligned else None, what="subnormal probes")
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"subnormals, layout {layout} unaligned {unaligned}"
            _record(FORMS[1] + " (subnormal probes)", got.numel())


@pytest.mark.parametrize("src16", [False, True], ids=["rounds_fp32_operands", "copies_bf16_shadows"])
def test_skinny_bf16_on_probes(src16):
    """src16 = False: the skinny kernel rounds fp32 operands itself - its rounding against torch's.  src16 = True: the shadows come
    from torch's own cast (functional._shadow16), so this half checks only that the kernel reads the shadows faithfully."""
    from mer_amd import functional as F
    values, _ = X.bf16_probes()
    for side in "ab":
        for (T, K, ncls) in [(300, 768, 7), (37, 50, 3)]:
            P = _probe_matrix(T if side == "a" else ncls, K, 9, values)
            H, _ = X.one_hot(ncls if side == "a" else T, K, 10)
            h, w = (P, H) if side == "a" else (H, P)
            got = F.gemm(h.to(DEV), w.to(DEV), F.NT, 1, src16=src16)
            torch.cuda.synchronize()
            _assert_form(13, what="skinny probes")
            assert bool(_form() & SRC16) == src16
            ref = _rne(h).double().to(DEV) @ _rne(w).double().to(DEV).t()
            _equal(got, ref, f"skinny probes side {side} {T}x{ncls}x{K}")
            _record(FORMS[13] + " (probes)", got.numel())


# ---- output rounding ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form,M,N,K,kw", [(1, 300, 200, 1000, {"tile": 64}), (4, 300, 200, 1000, {"tile": 64, "src16": True}),
                                           (5, 300, 260, 1000, {"tile": 128, "src16": True}), (9, 1024, 3328, 1024, {"src16": True}),
                                           (7, 1001, 514, 1000, {"src16": True}), (11, 8192, 2048, 1024, {"src16": True})])
def test_bf16_shadow_of_the_result_rounds_to_nearest_even(form, M, N, K, kw):
    """integer results above 256 land on bf16 ties: the shadow each form writes under m2f_set_shadow_map must be torch's rounding"""
    from mer_amd import functional as F, runtime
    lib = _lib()
    A, B = X.ints((M, K), M), X.ints((N, K), N)
    bias = X.terms((N,), 1).to(DEV)
    ws = torch.full((M * N,), NAN, device=DEV)
    sh = torch.zeros(M * N, dtype=torch.bfloat16, device=DEV)
    out = ws.view(M, N)
    runtime.check(lib.m2f_set_shadow_map(ws.data_ptr(), sh.data_ptr(), ws.numel()), "m2f_set_shadow_map")
    try:
        F.gemm(A.to(DEV), B.to(DEV), F.NT, runtime.BF16, bias=bias, out=out, **kw)
        torch.cuda.synchronize()
    finally:
        runtime.check(lib.m2f_set_shadow_map(None, None, 0), "m2f_set_shadow_map")
    name = _assert_form(form, what="shadow output")
    ref = A.double().to(DEV) @ B.double().to(DEV).t() + bias.double()
    _equal(out, ref, f"{name} shadow case")
    ties = ((out.view(torch.int32) & 0xFFFF) == 0x8000).sum().item()
    assert ties > 100, ties
    assert torch.equal(sh.view(M, N).view(torch.int16), out.to(torch.bfloat16).view(torch.int16)), f"{name}: bf16 shadow"
    _record(name + " (bf16 result)", out.numel())


def test_quantize_fp8_rounds_ties_to_even_and_saturates():
    from mer_amd import functional as F
    v = X.e4m3_probes()
    v = torch.cat([v, torch.zeros((-v.numel()) % 4)])
    for scale in (1.0, 0.5, 2.0):
        got = F.quantize_fp8(v.to(DEV), scale)
        torch.cuda.synchronize()
        want = (v * scale).clamp(-448, 448).to(torch.float8_e4m3fn)
        assert torch.equal(got.cpu().float(), want.float()), (v[got.cpu().float() != want.float()][:8], scale)
    _record("e4m3 quantiser (probes)", 3 * v.numel())


# ---- fp8 ---------------------------------------------------------------------------------------------------------------------

FP8_CASES = [((300, 200, 64), 0, 15), ((1024, 768, 768), 0, 15), ((4096 * 9 + 5, 1024 + 40, 256 + 48), 0, 17),
             ((8192, 1024, 512), 0, 17), ((8192, 1024, 512), 1, 15), ((4096, 4096, 256), 0, 18), ((4000, 4096, 384), 1, 18),
             ((16384, 1024, 1024), 0, 18), ((8448, 4096, 64), 1, 16)]


@pytest.mark.parametrize("shape,act,form", FP8_CASES)
def test_fp8_forms_are_exact(shape, act, form):
    from mer_amd import functional as F
    M, N, K = shape
    A, B = X.ints((M, K), M + 1), X.ints((N, K), N + 2)
    a8, b8 = A.to(DEV).to(torch.float8_e4m3fn), B.to(DEV).to(torch.float8_e4m3fn)
    bias, res = X.terms((N,), 3).to(DEV), X.terms((M, N), 4).to(DEV)
    acc = 0.25
    buf, out, mask = _guarded(M, N)
    F.gemm_fp8(a8, b8, acc, bias=bias, res=res, activation=act, out=out)
    torch.cuda.synchronize()
    name = _assert_form(form, what=f"fp8 {shape} act {act}")
    _guard_ok(buf, mask, f"fp8 {shape}")
    pre = (A.double().to(DEV) @ B.double().to(DEV).t()) * acc + bias.double()
    _equal(out, (pre.clamp_min(0) if act else pre) + res.double(), f"fp8 {shape} act {act}")
    _record(name, out.numel())
    del buf, out, res
    # e4m3 result: quantised exactly as torch quantises the exact fp32 result
    ld = N + 8
    b8buf = torch.full((M + 2, ld), 0x7F, dtype=torch.uint8, device=DEV)
    out8 = b8buf[1:M + 1, :N].view(torch.float8_e4m3fn)
    F.gemm_fp8(a8, b8, acc, bias=bias, activation=act, out8=out8, out8_scale=1.0 / 16)
    torch.cuda.synchronize()
    name8 = FORMS[_form() & 0xFF]
    guard = torch.ones(b8buf.shape, dtype=torch.bool, device=DEV)
    guard[1:M + 1, :N] = False
    assert (b8buf[guard] == 0x7F).all(), f"fp8 e4m3 result {shape}: guard written"
    v = (pre.clamp_min(0) if act else pre).float()
    want = (v * (1.0 / 16)).clamp(-448, 448).to(torch.float8_e4m3fn)
    assert torch.equal(out8.float(), want.float()), f"{name8} e4m3 result {shape}: {int((out8.float() != want.float()).sum())} differ"
    _record(name8 + " (e4m3 result)", out8.numel())


# ---- GELU (the one epilogue term that cannot be exact) -----------------------------------------------------------------------

# (the polynomial's largest error, evaluated in float64 on |z| <= 3 and at the clamp beyond: 4.325e-4 at z = 0.301; measured
#  worst kernel GELU error 0.997 of this bound in the bf16-source, ring and p8 forms, 0.32 of the A-S bound in the fp32-source ones)
ERF_AS, ERF_POLY = 1.5e-7, 4.33e-4


def _gelu_bound(pre, erf_err):
    return 0.5 * pre.abs() * erf_err + 4 * pre.abs() * 2.0 ** -23 + 1e-30


@pytest.mark.parametrize("form,M,N,K,kw,erf_err", [
    (1, 300, 200, 136, {"precision": 0, "tile": 64}, ERF_AS), (2, 300, 260, 136, {"precision": 1, "tile": 128}, ERF_AS),
    (4, 300, 200, 136, {"precision": 1, "tile": 64, "src16": True}, ERF_POLY),
    (6, 8192 - 3, 4096 - 5, 72, {"precision": 1, "tile": 128, "src16": True}, ERF_POLY),
    (10, 4001, 4098, 200, {"precision": 1, "src16": True}, ERF_POLY), (11, 8192, 2048, 512, {"precision": 1, "src16": True}, ERF_POLY)])
def test_gelu_epilogue_within_the_stated_erf_bound(form, M, N, K, kw, erf_err):
    from mer_amd import functional as F
    A, B = X.ints((M, K), 5), X.ints((N, K), 6)
    bias = (X.ints((N,), 7) / 4).to(DEV)
    A, B = A / 16, B / 16                                     # pre-activations within a few units: where erf bends
    buf, out, mask = _guarded(M, N)
    F.gemm(A.to(DEV), B.to(DEV), F.NT, bias=bias, relu_out=2, out=out, **kw)
    torch.cuda.synchronize()
    name = _assert_form(form, what="GELU")
    _guard_ok(buf, mask, "GELU")
    pre = A.double().to(DEV) @ B.double().to(DEV).t() + bias.double()
    ref = 0.5 * pre * (1 + torch.special.erf(pre / math.sqrt(2)))
    err = (out.double() - ref).abs()
    worst = (err / _gelu_bound(pre, erf_err)).max().item()
    print(f"\nGELU {name}: max |err| {err.max().item():.3e}, {worst:.3f} of the bound")
    assert worst <= 1.0
    _record(name + " (GELU, bounded)", out.numel())


# ---- the parameter-shadow cast (fused-optimizer shadows) ---------------------------------------------------------------------

def test_parameter_shadow_cast_rounds_ties_to_even_and_overflows_to_inf():
    """runtime.adam_step_shadowed with lr = 0 and zero gradients leaves every parameter as it is and writes its bf16 shadows (W and
    W^T of every 2-D parameter): crafted parameters at bf16 ties, subnormals and values that round to +-inf must come out as torch's
    cast, bit for bit.  (Parameters that ARE inf are left out: the update's 0 x p would be NaN in any formula with a decay term.)"""
    import synth
    from mer_amd import layout, runtime
    cfg = synth.CASES["tiny_odd_heads"][0]
    c = layout.M2FConfig.from_model_config(cfg)
    total = runtime.verify_layout(c)
    ovf = X.bf16_overflow_probes()
    values = torch.cat([X.bf16_probes()[0], X.bf16_subnormal_probes(), ovf[torch.isfinite(ovf)]])
    real = torch.zeros(total, dtype=torch.bool)
    specs = layout.param_specs(c)[0]
    for sp in specs:
        if not sp.alias_of:
            real[sp.offset: sp.offset + sp.numel] = True
    p = torch.where(real, _probe_matrix(1, total, 17, values)[0], torch.zeros(total)).to(DEV)
    assert torch.isinf(p.cpu().to(torch.bfloat16).float()).any()
    zeros = lambda: torch.zeros(total, device=DEV)
    got = p.clone()
    sh = runtime.param_shadow_buffer(c, torch.device(DEV))
    runtime.adam_step_shadowed(c, got, zeros(), zeros(), zeros(), sh, 1, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), p.view(torch.int32))
    r64, p8 = (lambda n: (n + 63) // 64 * 64), (lambda n: (n + 7) // 8 * 8)
    run, n = 0, 0                                              # the shadow layout of csrc/param_tables.hip::pm_add (tests/test_shared_shadows_gpu.py)
    for sp in specs:
        if sp.alias_of or len(sp.shape) != 2:
            continue
        rows, cols = sp.shape
        w = p[sp.offset: sp.offset + rows * cols].view(rows, cols)
        plain = sh[run: run + rows * p8(cols)].view(rows, p8(cols))[:, :cols]
        run += r64(rows * p8(cols))
        trans = sh[run: run + cols * p8(rows)].view(cols, p8(rows))[:, :rows]
        run += r64(cols * p8(rows))
        assert torch.equal(plain, w.to(torch.bfloat16).view(torch.int16)), sp.name
        assert torch.equal(trans, w.t().to(torch.bfloat16).view(torch.int16)), sp.name
        n += 2 * rows * cols
    assert n > 10000
    _record("parameter-shadow cast (probes)", n)


# ---- implicit-GEMM convolutions ----------------------------------------------------------------------------------------------

def _flat_guarded(shape, dtype=torch.float32, margin=64):
    """a contiguous output inside a NaN-filled buffer with `margin` guard elements before and after it"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * margin,), NAN, dtype=dtype, device=DEV)
    return buf, buf[margin: margin + n].view(*shape), margin


def _flat_guard_ok(buf, margin, what):
    assert torch.isnan(buf[:margin]).all() and torch.isnan(buf[-margin:]).all(), f"{what}: guard written"


# the convolutions of ResNet18's four stages, as tests/test_mel_resnet_gpu.py runs them: (B, H, W, Cin, Cout, ks, stride)
MEL_CONVS = [(1, 251, 32, 64, 64, 3, 1), (2, 251, 32, 64, 128, 3, 2), (2, 251, 32, 64, 128, 1, 2), (1, 126, 16, 128, 128, 3, 1),
             (3, 126, 16, 128, 256, 3, 2), (3, 126, 16, 128, 256, 1, 2), (3, 63, 8, 256, 256, 3, 1), (3, 63, 8, 256, 512, 3, 2),
             (3, 63, 8, 256, 512, 1, 2), (1, 32, 4, 512, 512, 3, 1), (3, 61, 8, 256, 512, 3, 2), (3, 61, 8, 256, 512, 1, 2),
             (3, 31, 4, 512, 512, 3, 1)]


@pytest.mark.parametrize("shape", MEL_CONVS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_mel_conv_is_exact(shape, bf16, with_res):
    """mel_resnet.conv on integers: the fp32 result equals float64 conv2d (+ bias, + residual, ReLU or not) bit for bit; the bf16
    result is torch's rounding of it.  (A bf16-mode residual is an integer in [-128, 128]: it arrives in bf16.)"""
    import torch.nn.functional as TF
    from mer_amd import mel_resnet as MR
    B, H, W, Cin, Cout, ks, s = shape
    seed = H * Cin + ks + s + 2 * bf16
    x, w, b = X.ints((B, H, W, Cin), seed), X.ints((Cout, Cin, ks, ks), seed + 1), X.terms((Cout,), seed + 2)
    Ho, Wo = (H + 2 * (ks // 2) - ks) // s + 1, (W + 2 * (ks // 2) - ks) // s + 1
    res = (X.ints((B, Ho, Wo, Cout), seed + 3, -128, 128) if bf16 else X.terms((B, Ho, Wo, Cout), seed + 3)) if with_res else None
    dt = torch.bfloat16 if bf16 else torch.float32
    pre = TF.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), stride=s, padding=ks // 2).permute(0, 2, 3, 1)
    if with_res:
        pre = pre + res.double()
    pre = pre.to(DEV)                                          # (float64 references on the CPU: the GPU library has no fp64 conv)
    xq, wq = x.to(DEV).to(dt), MR.pack_conv(w).to(DEV).to(dt)
    rq = res.to(DEV).to(dt) if with_res else None
    what = f"mel conv {shape} bf16={bf16} res={with_res}"
    for relu in (True, False):
        ref = pre.clamp_min(0) if relu else pre
        buf, out, mg = _flat_guarded((B, Ho, Wo, Cout))
        MR.conv(xq, wq, b.to(DEV), ks, s, res=rq, relu=relu, out_fp32=True, out=out)
        torch.cuda.synchronize()
        _flat_guard_ok(buf, mg, what)
        _equal(out, ref, f"{what} relu={relu}")
        _record("mel conv " + ("bf16" if bf16 else "fp32"), out.numel())
        if bf16:                                               # the bf16 result: torch's rounding of the exact fp32 one
            buf16, o16, mg = _flat_guarded((B, Ho, Wo, Cout), torch.bfloat16)
            MR.conv(xq, wq, b.to(DEV), ks, s, res=rq, relu=relu, out=o16)
            torch.cuda.synchronize()
            _flat_guard_ok(buf16, mg, what + " bf16 result")
            assert torch.equal(o16.view(torch.int16), ref.float().to(torch.bfloat16).view(torch.int16)), f"{what}: bf16 result"
            _record("mel conv bf16 (bf16 result)", o16.numel())


def _gelu_err_ratio(got, pre, erf_err, extra=0.0):
    """max |got - GELU(pre)| as a fraction of the stated bound 0.5 |pre| erf_err + 4 fp32 ulps of |pre| (+ extra)"""
    ref = 0.5 * pre * (1 + torch.special.erf(pre / math.sqrt(2)))
    bound = _gelu_bound(pre, erf_err) + extra
    return ((got.double() - ref).abs() / bound).max().item(), bound


@pytest.mark.parametrize("k,T_in", [(3, 63), (2, 64), (3, 40), (2, 41)])
@pytest.mark.parametrize("prec", [0, 1])
def test_w2v_conv_layer_on_integers(k, T_in, prec):
    """functional.w2v_conv_layer (Conv1d + GELU on the GEMM, overlapping windows, the last window ending at the last row): GELU of
    the exact integer pre-activation within the erf bound of the form that ran (Abramowitz-Stegun for the fp32-source kernels, the
    polynomial for the bf16-source ones).  That bound stays below half an integer step here, so any product dropped, repeated or
    misplaced shows.  (Measured on MI355X: 0.105 of the bound in fp32 mode, 0.842 in bf16 mode.)"""
    import torch.nn.functional as TF
    from mer_amd import functional as F
    C, s, P_in, B = 64, 2, 64, 3
    x, w = X.ints((B * P_in + 1, C), k * 100 + T_in), X.ints((C, C, k), k)
    T_out = (T_in - k) // s + 1
    xr = x[: B * P_in].view(B, P_in, C)[:, :T_in].double().transpose(1, 2)
    pre = TF.conv1d(xr, w.double(), stride=s).transpose(1, 2).to(DEV)            # [B, T_out, C]
    buf, out, mg = _flat_guarded((B * P_in // s, C))
    F.w2v_conv_layer(x.to(DEV), w.to(DEV), s, P_in, precision=prec, out=out)
    torch.cuda.synchronize()
    form = _form() & 0xFF
    assert (form in (1, 2, 3)) == (prec == 0), FORMS.get(form, form)
    _flat_guard_ok(buf, mg, "w2v conv layer")
    got = out.view(B, P_in // s, C)[:, :T_out]
    ratio, bound = _gelu_err_ratio(got, pre, ERF_AS if form in (1, 2, 3) else ERF_POLY)
    print(f"\nw2v conv layer k={k} T_in={T_in} ({FORMS[form]}): {ratio:.3f} of the GELU bound, bound <= {bound.max().item():.3f}")
    assert ratio <= 1.0 and bound.max().item() < 0.5
    _record(f"w2v conv layer ({FORMS[form]}, GELU, bounded)", got.numel())


@pytest.mark.parametrize("d,G,K,S,lengths", [(64, 4, 16, 70, [70, 45, 3]), (768, 16, 128, 130, [130, 64, 129]), (128, 4, 15, 9, [9, 5])])
@pytest.mark.parametrize("bf16", [False, True])
def test_w2v_pos_conv_on_integers(d, G, K, S, lengths, bf16):
    """functional.w2v_pos_conv (grouped conv + bias, GELU, + residual; rows at or past an utterance's length read as zero): within the
    Abramowitz-Stegun erf bound (the kernel's erf in both modes) of GELU of the exact integer pre-activation, plus the rounding of the
    residual add - far below one integer step.  (Measured on MI355X: at most 0.107 of the bound, both modes.)"""
    import torch.nn.functional as TF
    from mer_amd import functional as F
    B = len(lengths)
    x, w, bias = X.ints((B * S, d), d + K), X.ints((d, d // G, K), K), X.terms((d,), G)
    lens = torch.tensor(lengths)
    keep = (torch.arange(S)[None, :] < lens[:, None]).double()[..., None]
    xm = x.view(B, S, d).double() * keep
    y = TF.conv1d(xm.transpose(1, 2), w.double(), bias.double(), padding=K // 2, groups=G)[..., :S].transpose(1, 2).to(DEV)
    xm = xm.to(DEV)
    buf, out, mg = _flat_guarded((B * S, d))
    F.w2v_pos_conv(x.to(DEV), lens.to(DEV), w.to(DEV), bias.to(DEV), G, B, S, bf16=bf16, out=out)
    torch.cuda.synchronize()
    _flat_guard_ok(buf, mg, "w2v pos conv")
    got = out.view(B, S, d).double() - xm                     # (exact: |x| <= 4 and the result's ulp is well above the GELU error)
    want_sum = 0.5 * y * (1 + torch.special.erf(y / math.sqrt(2))) + xm
    add_ulp = want_sum.abs() * 2.0 ** -23                     # the residual add rounds once
    ratio, bound = _gelu_err_ratio(got, y, ERF_AS, extra=2 * add_ulp)
    print(f"\nw2v pos conv d={d} G={G} K={K} bf16={bf16}: {ratio:.3f} of the GELU bound, bound <= {bound.max().item():.2e}")
    assert ratio <= 1.0 and bound.max().item() < 0.5
    _record("w2v pos conv (GELU, bounded)", out.numel())
