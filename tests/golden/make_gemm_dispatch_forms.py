"""Which kernel form every GEMM dispatch rule picks, recorded from a build on an MI355X:
    python3 tests/golden/make_gemm_dispatch_forms.py  ->  tests/golden/gemm_dispatch_forms.json

Each case is launched through m2f_gemm / m2f_gemm_fp8 on seeded tensors and m2f_gemm_last_form() is recorded beside its description.
The file was recorded from the build in front of the change that moved the dispatch policy into csrc/gemm_dispatch.hip (no threshold
moved, so no form may); re-record it only with a change that is meant to move a threshold or a rule.

tests/test_gemm_dispatch_cpu.py asks m2f_gemm_form (the dry entry, no GPU) for the same forms; tests/test_gemm_exact_gpu.py launches a
subset again.  A case: mode f32 / bf16 / fp8, layout 0 NT / 1 NN / 2 TN, the forced tile, M, N, K0, K1 and the names of the BITS that
are set.  Every leading dimension is pad8(extent) of the contiguous extent (+ 1 under "odd_ld"), the convention of m2f_gemm_form.

Cases sit at the last tile count below each threshold and the first at it (default knobs, tile = 0); K is the smallest each rule
admits: 64, 72 where the eight-phase form must be refused (k % 64), 256 where split-K needs two k-tiles per slice.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIXTURE = os.path.join(HERE, "gemm_dispatch_forms.json")
DEV = "cuda"
NT, NN, TN = 0, 1, 2
MODES = {"f32": 0, "bf16": 1, "fp8": 2}
# the bits of m2f_gemm_form (include/m2fnet_hip.h, M2F_GEMM_FORM_*)
BITS = {"shadows": 1, "bt_shadow": 2, "odd_ld": 4, "bias_grad": 8, "gelu": 16, "relu_b": 32, "acc": 64, "gate": 128, "drop": 256,
        "c8": 512, "splitk": 1024, "relu_a": 2048, "relu_out": 4096, "res": 8192}
VEC, SRC16, NN_T = 0x100, 0x200, 0x400
P8_RC = 12                                      # the table form: no dispatched launch reaches it


def case(name, mode, M, N, K0=64, *bits, layout=NT, tile=0, K1=0):
    assert all(b in BITS for b in bits), bits
    return dict(name=name, mode=mode, layout=layout, tile=tile, M=M, N=N, K0=K0, K1=K1, bits=sorted(bits))


def _cases():
    S = "shadows"
    c = []
    # ---- bf16 from shadows, NT, tile = 0: the ring ladder --------------------------------------------------------------------
    c += [case("ring64x64_79_tiles", "bf16", 5056, 64, 64, S), case("ring64x64_80_tiles", "bf16", 5120, 64, 64, S),
          case("ring128x64_149_tiles", "bf16", 19072, 64, 64, S), case("ring128x64_150_tiles", "bf16", 19200, 64, 64, S),
          case("ring128x128_199_tiles", "bf16", 25472, 128, 64, S), case("ring128x128_200_tiles", "bf16", 25600, 128, 64, S)]
    # two rounds of 128x128 tiles -> one of 256x128 (k = 72: the eight-phase form would take the upper end at k = 64)
    c += [case("two_rounds_256_tiles", "bf16", 32768, 128, 72, S), case("two_rounds_257_tiles", "bf16", 32896, 128, 72, S),
          case("two_rounds_511_tiles", "bf16", 65408, 128, 72, S), case("two_rounds_512_tiles", "bf16", 65536, 128, 72, S),
          case("two_rounds_384_as_256", "bf16", 384, 16384, 72, S), case("two_rounds_387_as_258", "bf16", 384, 16512, 72, S)]
    c += [case("ring256_511_tiles", "bf16", 130816, 128, 72, S), case("ring256_512_tiles", "bf16", 131072, 128, 72, S)]
    # the eight-phase form: 256 tiles of 256x256, and whole rounds only (85 % fill)
    c += [case("p8_255_tiles", "bf16", 65280, 256, 64, S), case("p8_256_tiles", "bf16", 65536, 256, 64, S),
          case("p8_336_tiles_underfilled", "bf16", 86016, 256, 64, S), case("p8_435_tiles_underfilled", "bf16", 111360, 256, 64, S),
          case("p8_436_tiles", "bf16", 111616, 256, 64, S), case("p8_k_not_64", "bf16", 65536, 256, 72, S),
          case("p8_two_segments", "bf16", 65536, 256, 64, S, K1=64), case("p8_relu_a", "bf16", 65536, 256, 64, S, "relu_a")]
    # what no ring form takes: the register-staged 256x128 build from 1,024 tiles of 256x128
    c += [case("staged256_1023_tiles_relu_b", "bf16", 261888, 128, 64, S, "relu_b"), case("staged256_1024_tiles_relu_b", "bf16", 262144, 128, 64, S, "relu_b"),
          case("staged256_1023_tiles_gate", "bf16", 261888, 128, 64, S, "gate"), case("staged256_1024_tiles_gate", "bf16", 262144, 128, 64, S, "gate")]
    # the automatic tile of the register-staged forms: 128x128 from 256 (TN) / 512 (otherwise) such tiles
    c += [case("auto_tile_tn_255", "bf16", 32640, 128, 64, S, layout=TN), case("auto_tile_tn_256", "bf16", 32768, 128, 64, S, layout=TN),
          case("auto_tile_nn_511", "bf16", 65408, 128, 64, S, layout=NN), case("auto_tile_nn_512", "bf16", 65536, 128, 64, S, layout=NN),
          case("auto_tile_nt_511_relu_b", "bf16", 65408, 128, 64, S, "relu_b"), case("auto_tile_nt_512_relu_b", "bf16", 65536, 128, 64, S, "relu_b")]
    # the epilogue terms the eligibility predicates test, each at a size whose plain launch takes a ring form
    for b in ("gelu", "relu_b", "bias_grad"):
        c.append(case("ring_refuses_" + b, "bf16", 5120, 64, 64, S, b))
    for b in ("acc", "gate", "drop", "gelu", "res", "relu_out"):
        c.append(case("ring256_with_" + b, "bf16", 131072, 128, 72, S, b))
    # the 2 GiB operand limit of the LDS-DMA forms (32-bit byte offsets): M * ldq * 2 bytes
    c += [case("operand_below_2gib", "bf16", (1 << 20) - 1, 64, 1024, S), case("operand_at_2gib", "bf16", 1 << 20, 64, 1024, S)]
    # forced tiles (no ring form), every layout in both precisions, operands without shadows / with an odd leading dimension
    c += [case("forced_64_large", "bf16", 25600, 128, 64, S, tile=64), case("forced_128_large", "bf16", 25600, 128, 64, S, tile=128),
          case("forced_128_as_256x128", "bf16", 262144, 128, 64, S, tile=128), case("forced_64_f32", "f32", 65536, 128, 64, tile=64),
          case("forced_128_f32", "f32", 96, 72, 64, tile=128)]
    for lay, ln in ((NT, "nt"), (NN, "nn"), (TN, "tn")):
        c += [case("small_f32_" + ln, "f32", 96, 72, 64, layout=lay), case("small_bf16_" + ln, "bf16", 96, 72, 64, S, layout=lay),
              case("small_bf16_no_shadows_" + ln, "bf16", 96, 72, 64, layout=lay), case("small_f32_odd_ld_" + ln, "f32", 96, 72, 64, "odd_ld", layout=lay),
              case("small_bf16_odd_ld_" + ln, "bf16", 96, 72, 64, S, "odd_ld", layout=lay)]
    c.append(case("ring_size_odd_ld", "bf16", 5120, 64, 64, S, "odd_ld"))
    # fp32-source forms: 128x128 tiles from 512 of them; split-K below 224 tiles of 64x64 (forward / input-gradient form, scratch present,
    # two k-tiles per slice: K = 256 at BK = 64, 512 at BK = 128)
    c += [case("f32_tile_511", "f32", 65408, 128, 64), case("f32_tile_512", "f32", 65536, 128, 64),
          case("bf16_from_f32_tile_511", "bf16", 65408, 128, 64), case("bf16_from_f32_tile_512", "bf16", 65536, 128, 64),
          case("splitk_223_tiles", "f32", 14272, 64, 256, "splitk"), case("splitk_224_tiles", "f32", 14336, 64, 256, "splitk"),
          case("splitk_no_scratch", "f32", 14272, 64, 256), case("splitk_short_k", "f32", 14272, 64, 64, "splitk"),
          case("splitk_nn", "f32", 14272, 64, 256, "splitk", layout=NN), case("splitk_tn_never", "f32", 14272, 64, 256, "splitk", layout=TN),
          case("splitk_bf16_from_f32", "bf16", 14272, 64, 512, "splitk"), case("splitk_bf16_short_k", "bf16", 14272, 64, 256, "splitk"),
          case("splitk_forced_64", "f32", 96, 72, 256, "splitk", tile=64), case("splitk_forced_128_never", "f32", 96, 72, 256, "splitk", tile=128)]
    # the classifier head's skinny kernels
    c += [case("skinny_nt_f32", "f32", 300, 7, 64), case("skinny_nt_bf16_rounding", "bf16", 300, 7, 64), case("skinny_nt_bf16_shadows", "bf16", 300, 7, 64, S),
          case("skinny_nt_odd_ld", "bf16", 300, 7, 64, S, "odd_ld"), case("skinny_nt_f32_odd_ld", "f32", 300, 7, 64, "odd_ld"),
          case("skinny_nt_relu_out", "f32", 300, 8, 64, "relu_out"), case("skinny_nt_nine_columns", "f32", 300, 9, 64),
          case("skinny_nt_gate_refused", "f32", 300, 7, 64, "gate"), case("skinny_nt_res_refused", "f32", 300, 7, 64, "res"),
          case("skinny_nn_f32", "f32", 300, 64, 7, layout=NN), case("skinny_nn_bf16_shadows_gate", "bf16", 300, 64, 7, S, "gate", layout=NN),
          case("skinny_nn_bf16_rounding", "bf16", 300, 64, 7, layout=NN), case("skinny_nn_odd_ld", "bf16", 300, 64, 7, S, "odd_ld", layout=NN),
          case("skinny_nn_k_nine", "f32", 300, 64, 9, layout=NN), case("skinny_nn_acc_refused", "f32", 300, 64, 7, "acc", layout=NN)]
    # fp8 (e4m3 operands): the four outcomes and their boundaries
    c += [case("fp8_small", "fp8", 300, 200, 64), case("fp8_ring_255_tiles", "fp8", 65280, 128, 64), case("fp8_ring_256_tiles", "fp8", 65536, 128, 64),
          case("fp8_ring_refuses_relu", "fp8", 65536, 128, 64, "relu_out"), case("fp8_ring_gelu", "fp8", 65536, 128, 64, "gelu"),
          case("fp8_ring_c8_whole_tiles", "fp8", 8192, 1024, 64, "c8"), case("fp8_ring_c8_ragged", "fp8", 8191, 1024, 64, "c8"),
          case("fp8_staged_256x128", "fp8", 8448, 4096, 64, "relu_out"), case("fp8_staged_1023_tiles", "fp8", 261888, 128, 64, "relu_out"),
          case("fp8_staged_1024_tiles", "fp8", 262144, 128, 64, "relu_out"),
          case("fp8_p8_256_tiles", "fp8", 4096, 4096, 128), case("fp8_p8_255_tiles", "fp8", 65280, 256, 128), case("fp8_p8_k_not_128", "fp8", 4096, 4096, 192),
          case("fp8_p8_underfilled", "fp8", 86016, 256, 128), case("fp8_p8_c8", "fp8", 4096, 4096, 128, "c8")]
    names = [x["name"] for x in c]
    assert len(set(names)) == len(names), "case names must be unique"
    return c


CASES = _cases()


def pad8(n):
    return (n + 7) // 8 * 8


def bits_value(c):
    return sum(BITS[b] for b in c["bits"])


def dry_args(c, count=1):
    """the arguments of m2f_gemm_form for a case (without the trailing stages_bf16 pointer)"""
    return (MODES[c["mode"]], c["layout"], c["tile"], count, c["M"], c["N"], c["K0"], c["K1"], bits_value(c))


def check_coverage(forms):
    """every M2F_FORM_* value from 1 to 18 except the table form appears at least once"""
    have = {f & 0xFF for f in forms}
    missing = [f for f in range(1, 19) if f != P8_RC and f not in have]
    assert not missing, f"the fixture covers no case of form(s) {missing}"


def _mat(rows, cols, odd, gen, dtype=torch.float32):
    """[rows, cols] seeded values as a view of a buffer with leading dimension pad8(cols) (+ 1: odd)"""
    buf = torch.zeros(rows, pad8(cols) + (1 if odd else 0), dtype=dtype, device=DEV)
    buf[:, :cols] = torch.randn(rows, cols, generator=gen, device=DEV).to(dtype)
    return buf[:, :cols]


def _shadow(t, odd):
    buf = torch.zeros(t.shape[0], pad8(t.shape[1]) + (1 if odd else 0), dtype=torch.bfloat16, device=DEV)
    buf[:, :t.shape[1]] = t.to(torch.bfloat16)
    return buf[:, :t.shape[1]]


_SCRATCH = {}


def _splitk_scratch():
    if not _SCRATCH:
        n = 512
        _SCRATCH["s"] = (torch.empty(n * 4 * 64 * 64, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV), n)
    return _SCRATCH["s"]


def run_case(c, A=None, B=None):
    """launch the case on the build mer_amd loads -> (m2f_gemm_last_form(), C).  A [M, K0 + K1], B [N, K0 + K1] (logical, device):
    given operands instead of seeded ones."""
    from mer_amd.runtime import check, lib, ptr, stream_ptr
    bits = set(c["bits"])
    M, N, K0, K1, layout = c["M"], c["N"], c["K0"], c["K1"], c["layout"]
    odd = "odd_ld" in bits
    gen = torch.Generator(device=DEV).manual_seed(20261020)
    if A is None:
        A = torch.randn(M, K0 + K1, generator=gen, device=DEV)
        B = torch.randn(N, K0 + K1, generator=gen, device=DEV)
    if c["mode"] == "fp8":
        a8, b8 = A.to(torch.float8_e4m3fn).contiguous(), B.to(torch.float8_e4m3fn).contiguous()
        act = 1 if "relu_out" in bits else 2 if "gelu" in bits else 0
        ldc = pad8(N)
        if "c8" in bits:
            out = torch.zeros(M, ldc, dtype=torch.uint8, device=DEV)
            check(lib().m2f_gemm_fp8(M, N, K0, ptr(a8), K0, ptr(b8), K0, 0.25, None, ldc, None, None, 0, act, ptr(out), 1.0 / 16, stream_ptr()), "m2f_gemm_fp8")
        else:
            out = torch.zeros(M, ldc, device=DEV)
            check(lib().m2f_gemm_fp8(M, N, K0, ptr(a8), K0, ptr(b8), K0, 0.25, ptr(out), ldc, None, None, 0, act, None, 1.0, stream_ptr()), "m2f_gemm_fp8")
        torch.cuda.synchronize()
        return lib().m2f_gemm_last_form(), out[:, :N]

    def operand(X, rows_are_k, k0, k1):
        """segment [k0, k1) of logical X [rows, K] in its physical layout (+ shadow)"""
        if k1 <= k0:
            return None, None
        seg = X[:, k0:k1]
        seg = seg.t() if rows_are_k else seg
        buf = torch.zeros(seg.shape[0], pad8(seg.shape[1]) + (1 if odd else 0), device=DEV)
        buf[:, :seg.shape[1]] = seg
        v = buf[:, :seg.shape[1]]
        return v, (_shadow(v, odd) if "shadows" in bits else None)

    a0, a0q = operand(A, layout == TN, 0, K0)
    a1, a1q = operand(A, layout == TN, K0, K0 + K1)
    b0, b0q = operand(B, layout != NT, 0, K0)
    b1, b1q = operand(B, layout != NT, K0, K0 + K1)
    ld = lambda t: t.stride(0) if t is not None else 0          # noqa: E731
    mn = lambda: _mat(M, N, odd, gen)                            # noqa: E731
    out = mn()
    res, gate = (mn() if "res" in bits else None), (mn() if "gate" in bits else None)
    bg = torch.zeros(M, device=DEV) if "bias_grad" in bits else None
    rng = torch.tensor([11, 22, 3, 0], dtype=torch.int32, device=DEV) if "drop" in bits else None
    ws, tickets, nmax = _splitk_scratch() if "splitk" in bits else (None, None, 0)
    relu_out = 1 if "relu_out" in bits else 2 if "gelu" in bits else 0
    check(lib().m2f_gemm(MODES[c["mode"]], layout, M, N, K0, K1, ptr(a0), ld(a0), ptr(a1), ld(a1), ptr(b0), ld(b0), ptr(b1), ld(b1),
                         ptr(out), ld(out), None, ptr(res), ld(res), ptr(gate), ld(gate), 1.25, ptr(bg), int("relu_a" in bits),
                         int("relu_b" in bits), relu_out, int("acc" in bits), 7 if "drop" in bits else 0, 0.5 if "drop" in bits else 0.0,
                         ptr(rng), c["tile"], ptr(ws), ptr(tickets), nmax, ptr(a0q), ld(a0q), ptr(a1q), ld(a1q), ptr(b0q), ld(b0q),
                         ptr(b1q), ld(b1q), stream_ptr()), "m2f_gemm")
    torch.cuda.synchronize()
    return lib().m2f_gemm_last_form(), out


if __name__ == "__main__":
    import mer_amd  # noqa: F401
    rec = []
    for c in CASES:
        form, _ = run_case(c)
        torch.cuda.empty_cache()
        rec.append(dict(c, form=form))
        print(f"{c['name']:<34s} {c['mode']:<5s} layout {c['layout']} tile {c['tile']:3d} {c['M']:7d} x {c['N']:5d} x {c['K0']}+{c['K1']} "
              f"{','.join(c['bits']):<24s} -> 0x{form:03x}", flush=True)
    check_coverage([r["form"] for r in rec])
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(out, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(r) for r in rec) + "\n]}\n")
    print(f"{len(rec)} cases -> {out}")
