"""Host side of csrc/param_tables.hip: the size queries against layout.param_specs, and the argument rules of the entry points that
take a range of parameter tensors or a tensor -> group map - refused on the host table, before any device call, so all of it runs
without a GPU (the pointers are aligned dummies the host never dereferences)."""
import ctypes

import pytest

import param_tables_ref as ref
import synth
from mer_amd import layout, runtime

CASES = ("tiny_ragged", "c2_slice")
SHADOW_ELEMS = {"tiny_ragged": 2100224, "c2_slice": 46625536}      # m2f_param_shadow_elems of the build before param_tables.hip
P = 0x10000                                                        # a 256-byte aligned non-NULL "device pointer"


def _cfg(name):
    return layout.M2FConfig.from_model_config(synth.CASES[name][0])


def _err():
    return runtime.lib().m2f_last_error().decode()


@pytest.mark.parametrize("name", CASES)
def test_size_queries(name):
    c = _cfg(name)
    cc, L = ctypes.byref(runtime.config_to_c(c)), runtime.lib()
    n_tensors, slices, bins = len(ref.tensors(c)[0]), ref.n_slices(c), 64
    want = {
        "norm scratch": (lambda: L.m2f_grad_norm_scratch_bytes(cc), 8 * slices),
        "stats scratch": (lambda: L.m2f_tensor_stats_scratch_bytes(cc, bins), 40 * slices),          # sizeof(StatPartial)
        "stats record": (lambda: L.m2f_tensor_stats_record_bytes(cc, bins),
                         8 * (runtime.TSTATS_HEADER + n_tensors * (runtime.TSTATS_FIELDS + bins))),
        "shadow elems": (lambda: L.m2f_param_shadow_elems(cc), SHADOW_ELEMS[name]),
    }
    for what, (query, value) in want.items():
        assert {query() for _ in range(1000)} == {value}, what                                       # (the cached host table)


def _range_calls(c, tg):
    """{entry point: call(first, end)} with dummy buffers."""
    cc, L = ctypes.byref(runtime.config_to_c(c)), runtime.lib()
    return {
        "m2f_adam_step_shadowed_range": lambda f, e: L.m2f_adam_step_shadowed_range(cc, P, P, 0, P, P, P, f, e, 1e-3, 0.9, 0.999, 1e-8, 0.0,
                                                                                    1, None, None),
        "m2f_adam_step_grouped": lambda f, e: L.m2f_adam_step_grouped(cc, P, P, 0, P, P, None, tg, len(tg), P, f, e, None, None),
        "m2f_adam_step_grouped (shadows)": lambda f, e: L.m2f_adam_step_grouped(cc, P, P, 0, P, P, P, tg, len(tg), P, f, e, None, None),
        "m2f_grad_sumsq": lambda f, e: L.m2f_grad_sumsq(cc, P, 0, f, e, P, 0, 0, None),
    }


@pytest.mark.parametrize("name", CASES)
def test_bad_ranges_are_refused_by_every_range_entry_point(name):
    c = _cfg(name)
    n = len(ref.tensors(c)[0])
    tg = (ctypes.c_int * n)(*([0] * n))
    for entry, call in _range_calls(c, tg).items():
        for why, (first, end) in ref.bad_ranges(c).items():
            assert call(first, end) != 0, (entry, why)
            msg = _err()
            assert msg.startswith(entry.split(" ")[0] + ": ") and any(w in msg for w in ref.RANGE_WORDING), (entry, why, msg)


@pytest.mark.parametrize("name", CASES)
def test_tensor_group_rules_come_before_the_device(name):
    c = _cfg(name)
    cc, L = ctypes.byref(runtime.config_to_c(c)), runtime.lib()
    n = len(ref.tensors(c)[0])

    def grouped(tg, count, shadow):
        return L.m2f_adam_step_grouped(cc, P, P, 0, P, P, shadow, tg, count, P, 0, -1, None, None)

    def exchange(tg, count, shadow):
        return L.m2f_ema_exchange(cc, P, 2 * P, tg, count, None)

    for entry, call in (("m2f_adam_step_grouped", grouped), ("m2f_ema_exchange", exchange)):
        for shadow in (None, P):
            ok = (ctypes.c_int * n)(*([0] * n))
            assert call(ok, n - 1, shadow) != 0
            assert _err() == entry + ": tensor_group must hold one entry per parameter tensor"
            for bad in (16, -2):
                tg = (ctypes.c_int * n)(*([0] * (n - 1) + [bad]))
                assert call(tg, n, shadow) != 0
                assert _err() == entry + ": group index out of range", bad
