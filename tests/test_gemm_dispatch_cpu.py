"""The GEMM dispatch policy (csrc/gemm_dispatch.hip) on the host alone: m2f_gemm_form asks the chooser that m2f_gemm / m2f_gemm_fp8 ask,
on a synthetic batch whose operands are never dereferenced, and launches nothing.

  * every case of tests/golden/gemm_dispatch_forms.json - recorded from m2f_gemm_last_form() of real launches on an MI355X, at the last
    tile count below each threshold and the first at it - gets the recorded form;
  * grouping: every threshold is a sum of per-problem tile counts, so c problems of M x N take the form of one problem of cM x N;
  * an NN launch reports M2F_FORM_NN_T exactly when B has transposed shadows;
  * m2f_gemm_stages_bf16 (what the plan's unread-copy analysis asks) says "shadows only" exactly for the forms that read shadows only;
  * the chooser has no memory: a choice does not depend on the choices before it.
"""
import ctypes
import json
import re

import pytest

import make_gemm_dispatch_forms as G
from mer_amd import runtime

FIXTURE = json.load(open(G.FIXTURE))["cases"]
SHADOW_FORMS = {4, 5, 6, 7, 8, 9, 10, 11}          # bf16-source register-staged, ring, eight-phase
SKINNY = {13, 14}


def form_of(c, count=1, M=None, want_stages=False):
    args = list(G.dry_args(c, count))
    if M is not None:
        args[4] = M
    st = ctypes.c_int(-1)
    f = runtime.lib().m2f_gemm_form(*args, ctypes.byref(st) if want_stages else None)
    return (f, st.value) if want_stages else f


def test_the_fixture_is_the_case_list_and_covers_every_form():
    assert [{k: v for k, v in c.items() if k != "form"} for c in FIXTURE] == G.CASES, "re-record tests/golden/gemm_dispatch_forms.json"
    G.check_coverage([c["form"] for c in FIXTURE])


def test_the_bits_are_the_header_s():
    header = open(runtime.HEADER_PATH).read()
    got = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"M2F_GEMM_FORM_(\w+) = (\d+)", header)}
    assert got == G.BITS


@pytest.mark.parametrize("c", FIXTURE, ids=[c["name"] for c in FIXTURE])
def test_the_dry_entry_gives_the_recorded_form(c):
    got = form_of(c)
    assert got == c["form"], f"{c['name']}: m2f_gemm_form 0x{got:03x}, recorded 0x{c['form']:03x}"


def _group_counts(c):
    """the problem counts that split the case's rows into equal problems of whole 256-row tiles"""
    return [n for n in range(2, 9) if c["M"] % (256 * n) == 0]


GROUPABLE = [c for c in FIXTURE if c["mode"] != "fp8" and c["form"] & 0xFF not in SKINNY and not c["name"].startswith("operand_")
             and _group_counts(c)]


@pytest.mark.parametrize("c", GROUPABLE, ids=[c["name"] for c in GROUPABLE])
def test_grouped_problems_take_the_form_of_their_sum(c):
    for count in _group_counts(c):
        got = form_of(c, count=count, M=c["M"] // count)
        assert got == c["form"], f"{c['name']}: {count} x {c['M'] // count} rows -> 0x{got:03x}, one problem 0x{c['form']:03x}"


def test_enough_cases_are_grouped():
    assert {c["form"] & 0xFF for c in GROUPABLE} >= {1, 2, 4, 5, 6, 7, 8, 9, 10, 11}, sorted({c["form"] & 0xFF for c in GROUPABLE})


@pytest.mark.parametrize("M,N,K,count,base", [(5120, 64, 64, 1, 7), (2560, 64, 64, 2, 7), (96, 72, 64, 1, 4), (25600, 128, 64, 1, 9),
                                              (65536, 256, 64, 1, 11), (131072, 128, 72, 1, 10)])
def test_nn_through_transposed_shadows(M, N, K, count, base):
    c = G.case("nn_t", "bf16", M, N, K, "shadows", "bt_shadow", layout=G.NN)
    assert form_of(c, count=count) == base | G.NN_T                                     # runs as the k-contiguous form: the NT ladder
    assert form_of(dict(c, layout=G.NT), count=count) == base                            # ... the one an NT launch of the shape takes
    plain = form_of(G.case("nn", "bf16", M, N, K, "shadows", layout=G.NN), count=count)
    assert not plain & G.NN_T and plain & 0xFF in (4, 5)                                # no transposed shadow: the row-major NN form
    assert not form_of(dict(c, mode="f32"), count=count) & G.NN_T                        # fp32 mode reads no shadow
    assert form_of(G.case("nn_t_only", "bf16", M, N, K, "bt_shadow", layout=G.NN), count=count) & 0xFF in (1, 2)   # A has none: fp32 staging


GRID = [G.case("grid", "bf16", M, N, K, *bits, layout=lay, tile=tile, K1=K1)
        for (M, N, K, K1) in [(96, 72, 64, 0), (300, 7, 64, 0), (300, 64, 7, 0), (5120, 64, 64, 0), (19200, 64, 64, 0), (25600, 128, 64, 40), (65536, 256, 64, 0),
                              (65536, 256, 72, 0), (262144, 128, 64, 0), (1 << 20, 64, 1024, 0)]
        for lay in (G.NT, G.NN, G.TN) for tile in (0, 64, 128)
        for bits in [(), ("shadows",), ("shadows", "odd_ld"), ("shadows", "bt_shadow"), ("bt_shadow",), ("shadows", "gate"), ("shadows", "relu_b"),
                     ("shadows", "res"), ("shadows", "gelu"), ("shadows", "bias_grad"), ("shadows", "acc", "splitk"), ("splitk",)]]


def test_stages_bf16_agrees_with_the_chosen_form():
    """plan_build.hip::mark_unread_fp32 leaves an fp32 buffer unwritten when no launch stages it: m2f_gemm_stages_bf16 must say "shadows
    only" exactly when the chosen kernel reads shadows only"""
    seen = set()
    for c in GRID:
        for count in (1, 3):
            f, st = form_of(c, count=count, want_stages=True)
            base = f & 0xFF
            # (the answer is for a launch with the automatic tile, as the plans launch; a forced tile moves the form inside its family only)
            reads_shadows_only = base in SHADOW_FORMS or (base in SKINNY and bool(f & G.SRC16))
            assert st == int(reads_shadows_only), (c, count, hex(f), st)
            seen.add((base, st))
    assert {b for b, _ in seen} >= SHADOW_FORMS | SKINNY | {1, 2}, sorted(seen)
    assert {(13, 0), (13, 1), (14, 0), (14, 1)} <= seen


def test_a_choice_does_not_depend_on_the_choices_before_it():
    first = [form_of(c) for c in FIXTURE]
    assert [form_of(c) for c in FIXTURE] == first
    assert [form_of(c) for c in reversed(FIXTURE)] == first[::-1]
    for a, fa in zip(FIXTURE[::7], first[::7]):
        for b in FIXTURE[::5]:
            form_of(b)
            assert form_of(a) == fa, (a["name"], b["name"])


def test_a_refused_launch_has_no_form():
    assert form_of(G.case("k0", "f32", 96, 72, 0)) == 0
    assert form_of(G.case("fp8_k", "fp8", 300, 200, 72)) == 0                         # K % 16
    assert form_of(G.case("count", "f32", 96, 72, 64), count=9) == 0
