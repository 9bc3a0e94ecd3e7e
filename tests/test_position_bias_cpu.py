"""Host side of the distance-decay attention bias (M2FNet(position_bias=gain)): the restatement the GPU tests take their reference
values from (tests/golden/position_bias_ref.py) against torch's own float attn_mask= / src_mask= arguments, the slopes against the
literal values of the recipe, gain validation and rounding, the plan keys, and the runtime.position_bias entry of the config with
src/train.py's check of it (raised before any GPU use)."""
import math
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import band_ref as BR  # noqa: E402
import position_bias_ref as R  # noqa: E402
import synth  # noqa: E402
from oracle import m2fnet_oracle as O  # noqa: E402
from mer_amd import functional as F  # noqa: E402
from mer_amd import runtime  # noqa: E402
from mer_amd.model import FusionAttentionModule, M2FNet, _Engine  # noqa: E402

TOL = 1e-12
BANDS = [(None, None), (None, 0), (2, 0)]
HEADS = [3, 4, 5, 12]


def _case(B, L, E, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    text = torch.randn(B, L, E, generator=g, dtype=torch.float64)
    audio = torch.randn(B, L, E, generator=g, dtype=torch.float64)
    key_pad = torch.zeros(B, L, dtype=torch.bool)
    for b, n in enumerate(lengths):
        key_pad[b, n:] = True
    return text, audio, key_pad


def _float_mask(L, H, B, band, gain):
    """the float attn_mask torch's modules take: [B*H, L, L], -inf where the band hides a key, the distance term elsewhere"""
    m = R.bias_term(L, H, gain).masked_fill(BR.band_mask(L, *band)[None], float("-inf"))
    return m[None].expand(B, H, L, L).reshape(B * H, L, L)


# ---- the slopes ----------------------------------------------------------------------------------------------------------------------
LITERAL = {1: [2.0 ** -8],
           2: [2.0 ** -4, 2.0 ** -8],
           3: [1 / 16, 1 / 256, 1 / 4],
           4: [1 / 4, 1 / 16, 1 / 64, 1 / 256],
           5: [1 / 4, 1 / 16, 1 / 64, 1 / 256, 1 / 2],
           8: [2.0 ** -(h + 1) for h in range(8)],
           12: [2.0 ** -(h + 1) for h in range(8)] + [2.0 ** -0.5, 2.0 ** -1.5, 2.0 ** -2.5, 2.0 ** -3.5]}


@pytest.mark.parametrize("H", sorted(LITERAL))
def test_slopes_are_the_recipe(H):
    want = torch.tensor(LITERAL[H], dtype=torch.float64)
    assert (R.slopes(H, 1.0) - want).abs().max().item() <= 1e-15
    assert (R.slopes(H, 0.5) - 0.5 * want).abs().max().item() <= 1e-15
    got = F.position_bias_slopes(H, 1.0)
    assert got.dtype == torch.float32 and got.shape == (H,)
    assert torch.equal(got, want.to(torch.float32))
    assert torch.equal(F.position_bias_slopes(H, 0.75), (0.75 * want).to(torch.float32))
    assert torch.equal(F.position_bias_slopes(H, None), torch.zeros(H))


def test_slopes_use_the_applied_gain():
    g = runtime.position_bias(0.3)
    assert g != 0.3 and torch.equal(F.position_bias_slopes(4, 0.3), (R.slopes(4, g)).to(torch.float32))
    for bad in (0, -1, 2.5, True, "4"):
        with pytest.raises(ValueError):
            F.position_bias_slopes(bad, 1.0)


# ---- the gain ------------------------------------------------------------------------------------------------------------------------
def test_gain_validation_and_rounding():
    assert runtime.position_bias(None) == 0.0 and runtime.position_bias(0) == 0.0 and runtime.position_bias(0.0) == 0.0
    for exact in (1.0, 0.5, 2.0, 0.75, 3, 1e-3 * 0 + 0.25):
        assert runtime.position_bias(exact) == float(exact)
    for g in (0.3, 0.1, 1.2345678, 17.77, 1e-6, 3.0e38, 1.00390625, 1.01171875):      # (the last two: ties, to even)
        got = runtime.position_bias(g)
        assert got == R.applied_gain(g), (g, got)
        assert abs(got - g) <= g * 2.0 ** -8
        assert runtime.position_bias(got) == got                    # (idempotent: the applied value is its own rounding)
    assert runtime.position_bias(1.00390625) == 1.0 and runtime.position_bias(1.01171875) == 1.015625
    for bad in (-1.0, -1e-9, float("inf"), float("nan"), "1.0", True, [1.0], 3.4e38, 1e400):
        with pytest.raises(ValueError, match="position bias"):
            runtime.position_bias(bad)


def test_model_stores_and_reports_the_applied_gain_without_a_device():
    cfg = synth.CASES["tiny_ragged"][0]
    assert M2FNet(cfg).position_bias is None
    assert M2FNet(cfg, position_bias=None).position_bias is None and M2FNet(cfg, position_bias=0.0).position_bias is None
    m = M2FNet(cfg, position_bias=1.0, context=(None, 0))
    assert m.position_bias == 1.0 and m.context == (None, 0)
    m.set_position_bias(0.3)
    assert m.position_bias == R.applied_gain(0.3) == runtime.position_bias(0.3)
    for bad in (-0.5, float("nan"), "1"):
        with pytest.raises(ValueError, match="position bias"):
            m.set_position_bias(bad)
        with pytest.raises(ValueError, match="position bias"):
            M2FNet(cfg, position_bias=bad)
    assert m.position_bias == R.applied_gain(0.3)                    # (a refused setting changes nothing)
    m.set_position_bias()
    assert m.position_bias is None
    assert set(M2FNet(cfg, position_bias=1.0).state_dict()) == set(M2FNet(cfg).state_dict())       # (no parameters)
    assert FusionAttentionModule(16, 4, 0.0).position_bias is None
    assert FusionAttentionModule(16, 4, 0.0, position_bias=1.0).position_bias == 1.0
    with pytest.raises(ValueError, match="position bias"):
        FusionAttentionModule(16, 4, 0.0, position_bias=-1.0)


def test_default_plan_key_is_what_it_was_and_a_gain_has_its_own():
    old = (8, 16, None, True, False, runtime.F32)
    assert _Engine.plan_key(8, 16, None, True, False, runtime.F32) == old
    assert _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (None, None), None) == old
    assert _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (None, None), 0.0) == old
    causal = _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (None, 0))
    assert _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (None, 0), None) == causal
    one = _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (None, None), 1.0)
    half = _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (None, None), 0.5)
    both = _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (None, 0), 1.0)
    assert one[:6] == old and both[:len(causal)] == causal
    assert len({old, causal, one, half, both}) == 5
    assert one[-1] == ("position_bias", 1.0)


def test_new_entries_are_declared_and_exported():
    """The plan-level entries, and the kernel-level entries that CARRY the gain, as the bias_gain field of their options descriptor.
    The per-feature entries (base name + "_bias") are gone from the header, the bindings and the library."""
    header = open(runtime.HEADER_PATH).read()
    carriers = {"m2f_attention_fwd": "m2f_attn_opts", "m2f_attention_varlen_fwd": "m2f_attn_opts",
                "m2f_attention_stream": "m2f_attn_stream_opts", "m2f_attention_stream_chunk": "m2f_attn_stream_opts"}
    mirror = {"m2f_attn_opts": runtime.AttnOptsC, "m2f_attn_stream_opts": runtime.AttnStreamOptsC}
    for sym in tuple(carriers) + ("m2f_plan_attention_bias", "m2f_plan_get_attention_bias"):
        assert sym in runtime.SIGNATURES and ("int " + sym + "(") in header, sym
        assert hasattr(runtime.lib(), sym), sym
    for sym, name in carriers.items():
        struct = header[header.index("typedef struct " + name + " {"):header.index("} " + name + ";")]
        assert "float bias_gain;" in struct and ("bias_gain", ctypes.c_float) in mirror[name]._fields_, name
        assert runtime.SIGNATURES[sym][1][-1] is ctypes.POINTER(mirror[name]), sym
        old = sym + "_bias"
        assert old not in runtime.SIGNATURES and old not in header and not hasattr(runtime.lib(), old), old


# ---- the reference against torch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("H", HEADS)
def test_fusion_form_agrees_with_torch_multihead_attention(H, band):
    """query = text, key = audio, value = text (the fusion module's call) with a float attn_mask [B*H, L, L] = band + distance term and
    key_padding_mask: output and per-head probabilities, on the rows that see a key."""
    B, L, E = 3, 11, 2 * H * 6
    gain = R.applied_gain(1.0)
    text, audio, key_pad = _case(B, L, E, [11, 3, 6], 5 + H)
    mha = torch.nn.MultiheadAttention(E, H, dropout=0.0, batch_first=True).double().train()
    w, bias = mha.in_proj_weight.detach(), mha.in_proj_bias.detach()
    q = text @ w[:E].T + bias[:E]
    k = audio @ w[E:2 * E].T + bias[E:2 * E]
    v = text @ w[2 * E:].T + bias[2 * E:]
    o, p = R.attention(q, k, v, key_pad, H, return_probs=True, band=band, gain=gain)
    mine = o @ mha.out_proj.weight.detach().T + mha.out_proj.bias.detach()
    with torch.no_grad():
        ref, p_ref = mha(text, audio, text, key_padding_mask=key_pad, attn_mask=_float_mask(L, H, B, band, gain), need_weights=True,
                         average_attn_weights=False)
    rows = BR.visible_rows(key_pad, band)
    assert rows[~key_pad].all()
    assert (mine - ref)[rows].abs().max().item() < TOL
    assert (p - p_ref).permute(0, 2, 1, 3)[rows].abs().max().item() < TOL
    assert torch.isfinite(mine).all() and torch.isfinite(p).all()
    hidden = (key_pad[:, None, None, :] | BR.band_mask(L, *band)[None, None]).expand_as(p)
    assert torch.all(p[hidden] == 0)                                # (a hidden key stays hidden: the term goes to visible keys only)
    # the term moves the numbers (the comparison above can fail)
    _, p0 = BR.attention(q, k, v, key_pad, H, return_probs=True, band=band)
    assert (p - p0).abs().max().item() > 1e-3


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("H", HEADS)
def test_encoder_form_agrees_with_torch_transformer_encoder_layer(H, band):
    """The oracle's encoder layer with the reference swapped in against nn.TransformerEncoderLayer(src_mask= float, src_key_padding_mask=)."""
    B, L, E, FF = 2, 9, 4 * H, 32
    x, _, key_pad = _case(B, L, E, [9, 4], 8 + H)
    layer = torch.nn.TransformerEncoderLayer(E, H, FF, dropout=0.0, batch_first=True).double().train()
    sd = {k: v.detach() for k, v in layer.state_dict().items()}
    with R.swapped_in(band, 1.0):
        mine = O.encoder_layer(x, sd, "", key_pad, H)
    assert O.attention.__module__ == O.__name__                     # (swapped back)
    with torch.no_grad():
        ref = layer(x, src_mask=_float_mask(L, H, B, band, 1.0), src_key_padding_mask=key_pad)
    rows = BR.visible_rows(key_pad, band)
    assert (mine - ref)[rows].abs().max().item() < TOL
    assert torch.isfinite(mine).all()


def test_reference_without_a_gain_is_band_ref():
    B, L, E, H = 2, 7, 12, 3
    q, k, key_pad = _case(B, L, E, [7, 2], 3)
    for band in BANDS:
        a, pa = R.attention(q, k, q + k, key_pad, H, return_probs=True, band=band)
        b, pb = BR.attention(q, k, q + k, key_pad, H, return_probs=True, band=band)
        assert torch.equal(a, b) and torch.equal(pa, pb)


def test_swapped_in_uses_the_applied_gain():
    B, L, E, H = 1, 6, 8, 2
    q, k, key_pad = _case(B, L, E, [6], 9)
    with R.swapped_in((None, 0), 0.3):
        got = O.attention(q, k, q, key_pad, H)
    want = R.attention(q, k, q, key_pad, H, band=(None, 0), gain=runtime.position_bias(0.3))
    assert torch.equal(got, want)
    assert not torch.equal(got, R.attention(q, k, q, key_pad, H, band=(None, 0), gain=0.3))


# ---- runtime.position_bias -----------------------------------------------------------------------------------------------------------
def test_runtime_position_bias_is_checked_on_the_host():
    import train as tr
    assert tr.position_bias_settings({}) is None and tr.position_bias_settings({"runtime": {}}) is None
    assert tr.position_bias_settings({"runtime": {"position_bias": None}}) is None
    assert tr.position_bias_settings({"runtime": {"position_bias": 0}}) is None
    assert tr.position_bias_settings({"runtime": {"position_bias": 1.0}}) == 1.0
    assert tr.position_bias_settings({"runtime": {"position_bias": 2}}) == 2.0
    for bad in (-1, float("nan"), float("inf"), "1.0", True, {"gain": 1.0}, [1.0]):
        with pytest.raises(ValueError, match="runtime.position_bias"):
            tr.position_bias_settings({"runtime": {"position_bias": bad}})
    on = {"enabled": True, "teacher_checkpoint": "ck/teacher.pth"}
    assert "position_bias" not in tr.resolve_distill({"runtime": {"distill": on}})
    assert "position_bias" not in tr.resolve_distill({"runtime": {"distill": dict(on, teacher_position_bias=None)}})
    assert tr.resolve_distill({"runtime": {"distill": dict(on, teacher_position_bias=1.0)}})["position_bias"] == 1.0
    with pytest.raises(ValueError, match="teacher_position_bias"):
        tr.resolve_distill({"runtime": {"distill": dict(on, teacher_position_bias=-2)}})
    assert "teacher_position_bias" in tr.DISTILL_KEYS


def test_shipped_config_has_the_setting_switched_off():
    import train as tr
    from utils import get_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        cfg = get_config()
    finally:
        os.chdir(cwd)
    assert "position_bias" in cfg["runtime"] and cfg["runtime"]["position_bias"] is None
    assert tr.position_bias_settings(cfg) is None
    assert math.isclose(float(R.slopes(4, 1.0)[0]), 0.25)
