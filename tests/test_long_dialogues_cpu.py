"""Host-side surface of long-dialogue support (no GPU): plan sizing accepts L up to 512 for packed plans only, refusals name L,
and the engine's shape buckets (unchanged up to 64, multiples of 64 above)."""
import ctypes
import os

import pytest
import yaml

import mer_amd  # noqa: F401
from mer_amd import layout, runtime
from mer_amd.model import _Engine

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _cc():
    with open(os.path.join(ROOT, "src", "config.yaml")) as f:
        cfg = yaml.safe_load(f)["model"]
    return runtime.config_to_c(layout.M2FConfig.from_model_config(cfg))


def test_packed_workspace_accepts_long_dialogues():
    cc = _cc()
    lib = runtime.lib()
    T = 3 * 110 + 40
    n110 = lib.m2f_workspace_bytes_packed(ctypes.byref(cc), 4, 110, T, 1)
    assert n110 > 0, lib.m2f_last_error()
    n512 = lib.m2f_workspace_bytes_packed(ctypes.byref(cc), 4, 512, T, 1)
    assert n512 > n110                                   # the probabilities buffers grow with L^2
    assert lib.m2f_workspace_bytes_shared(ctypes.byref(cc), 4, 110, T, 1) > 0
    assert lib.m2f_workspace_bytes_packed(ctypes.byref(cc), 4, 110, T, 0) > 0          # eval plan


def test_packed_plan_rejects_L_above_512_naming_it():
    cc = _cc()
    lib = runtime.lib()
    assert lib.m2f_workspace_bytes_packed(ctypes.byref(cc), 2, 513, 600, 1) < 0
    assert b"L = 513" in lib.m2f_last_error()
    assert lib.m2f_workspace_bytes_shared(ctypes.byref(cc), 2, 513, 600, 1) < 0
    assert b"513" in lib.m2f_last_error()


def test_padded_plan_still_rejects_L_above_64():
    cc = _cc()
    lib = runtime.lib()
    assert lib.m2f_workspace_bytes(ctypes.byref(cc), 4, 65, 1) < 0
    assert b"L = 65" in lib.m2f_last_error()
    assert lib.m2f_workspace_bytes_shared(ctypes.byref(cc), 4, 65, 0, 1) < 0           # T = 0: padded
    assert lib.m2f_workspace_bytes(ctypes.byref(cc), 4, 64, 1) > 0


def test_dropout_index_bound_is_refused():
    cc = _cc()                          # shipped config: 8 heads at most -> B * 8 * 512^2 >= 2^32 from B = 2,048 on
    lib = runtime.lib()
    assert lib.m2f_workspace_bytes_packed(ctypes.byref(cc), 2048, 512, 2048 * 2, 0) < 0
    assert b"2^32" in lib.m2f_last_error()


def test_varlen_entries_are_exported_and_bound():
    lib = runtime.lib()
    for name in ("m2f_attention_varlen_fwd", "m2f_attention_varlen_bwd"):
        assert name in runtime.SIGNATURES
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("L", range(1, 65))
def test_bucket_unchanged_up_to_64(L):
    assert _Engine.bucket(5, L) == (8, (L + 15) // 16 * 16)


@pytest.mark.parametrize("L,Lb", [(65, 128), (100, 128), (110, 128), (128, 128), (129, 192), (300, 320), (512, 512)])
def test_bucket_rounds_to_64_above(L, Lb):
    assert _Engine.bucket(16, L) == (16, Lb)
