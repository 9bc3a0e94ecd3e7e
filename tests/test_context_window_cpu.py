"""Host side of the context band of the dialogue attention (M2FNet(context=(past, future))): the restatement the GPU tests take their
reference values from (tests/golden/band_ref.py) against torch's own attn_mask= / src_mask= arguments, the runtime.context block of
the config and src/train.py's check of it (raised before any GPU use), and that a model without a band keeps its plan keys."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import band_ref as R  # noqa: E402
import synth  # noqa: E402
from oracle import m2fnet_oracle as O  # noqa: E402
from mer_amd import runtime  # noqa: E402
from mer_amd.model import M2FNet, _Engine  # noqa: E402

BANDS = [(None, 0), (2, 0), (1, 1), (0, 0), (None, None), (3, None)]
TOL = 1e-12


def _case(B, L, E, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    text = torch.randn(B, L, E, generator=g, dtype=torch.float64)
    audio = torch.randn(B, L, E, generator=g, dtype=torch.float64)
    key_pad = torch.zeros(B, L, dtype=torch.bool)
    for b, n in enumerate(lengths):
        key_pad[b, n:] = True
    return text, audio, key_pad


def test_band_mask_is_the_rule():
    for L in (1, 5, 16):
        for past, future in BANDS:
            m = R.band_mask(L, past, future)
            for i in range(L):
                for j in range(L):
                    seen = (past is None or j >= i - past) and (future is None or j <= i + future)
                    assert bool(m[i, j]) == (not seen), (L, past, future, i, j)
    assert not R.band_mask(7, None, None).any()
    assert torch.equal(R.band_mask(6, None, 0), torch.triu(torch.ones(6, 6, dtype=torch.bool), diagonal=1))      # torch's causal mask


@pytest.mark.parametrize("band", BANDS)
def test_fusion_form_agrees_with_torch_multihead_attention(band):
    """query = text, key = audio, value = text (the fusion module's call) with attn_mask = the band and key_padding_mask: output and
    per-head probabilities, on the rows that see a key (torch gives NaN on the others; band_ref gives zeros there)."""
    B, L, E, H = 3, 11, 24, 4
    text, audio, key_pad = _case(B, L, E, [11, 3, 6], 5)
    mha = torch.nn.MultiheadAttention(E, H, dropout=0.0, batch_first=True).double().train()
    w, bias = mha.in_proj_weight.detach(), mha.in_proj_bias.detach()
    q = text @ w[:E].T + bias[:E]
    k = audio @ w[E:2 * E].T + bias[E:2 * E]
    v = text @ w[2 * E:].T + bias[2 * E:]
    o, p = R.attention(q, k, v, key_pad, H, return_probs=True, band=band)
    mine = o @ mha.out_proj.weight.detach().T + mha.out_proj.bias.detach()
    with torch.no_grad():
        ref, p_ref = mha(text, audio, text, key_padding_mask=key_pad, attn_mask=R.band_mask(L, *band), need_weights=True,
                         average_attn_weights=False)
    rows = R.visible_rows(key_pad, band)
    assert rows[~key_pad].all()                                     # a valid query always sees itself
    assert (mine - ref)[rows].abs().max().item() < TOL
    assert (p - p_ref).permute(0, 2, 1, 3)[rows].abs().max().item() < TOL
    assert torch.isfinite(mine).all() and torch.isfinite(p).all()
    empty = ~rows
    if empty.any():                                                 # the empty-row rule: P = 0 and a zero attention row
        assert torch.all(p.permute(0, 2, 1, 3)[empty] == 0) and torch.all(o[empty] == 0)
        assert torch.isnan(ref[empty]).all()                        # (what the rule is there for)
    hidden = (key_pad[:, None, None, :] | R.band_mask(L, *band)[None, None]).expand_as(p)
    assert torch.all(p[hidden] == 0)


def test_some_case_has_rows_without_a_visible_key():
    _, _, key_pad = _case(3, 11, 24, [11, 3, 6], 5)
    assert (~R.visible_rows(key_pad, (2, 0))).any() and R.visible_rows(key_pad, (None, 0)).all()


@pytest.mark.parametrize("band", BANDS)
def test_encoder_form_agrees_with_torch_transformer_encoder_layer(band):
    """The oracle's encoder layer with band_ref swapped in against nn.TransformerEncoderLayer(src_mask=, src_key_padding_mask=):
    .train() with dropout 0 keeps torch's fused inference path out of the way."""
    B, L, E, H, FF = 2, 9, 16, 2, 32
    x, _, key_pad = _case(B, L, E, [9, 4], 8)
    layer = torch.nn.TransformerEncoderLayer(E, H, FF, dropout=0.0, batch_first=True).double().train()
    sd = {k: v.detach() for k, v in layer.state_dict().items()}
    with R.swapped_in(band):
        mine = O.encoder_layer(x, sd, "", key_pad, H)
    assert O.attention.__module__ == O.__name__                     # (swapped back)
    with torch.no_grad():
        ref = layer(x, src_mask=R.band_mask(L, *band), src_key_padding_mask=key_pad)
    rows = R.visible_rows(key_pad, band)
    assert (mine - ref)[rows].abs().max().item() < TOL
    assert torch.isfinite(mine).all()


def test_unbanded_restatement_is_the_oracle():
    B, L, E, H = 2, 7, 12, 3
    q, k, key_pad = _case(B, L, E, [7, 2], 3)
    a, pa = R.attention(q, k, q + k, key_pad, H, return_probs=True)
    b, pb = O.attention(q, k, q + k, key_pad, H, return_probs=True)
    assert torch.equal(a, b) and torch.equal(pa, pb)


def test_empty_rows_give_no_gradient_and_no_nan():
    B, L, E, H = 1, 8, 8, 2
    q, k, key_pad = _case(B, L, E, [2], 4)
    q, k = q.requires_grad_(True), k.requires_grad_(True)
    v = (q.detach() - k.detach()).requires_grad_(True)
    o = R.attention(q, k, v, key_pad, H, band=(1, 0))
    o.sum().backward()
    rows = R.visible_rows(key_pad, (1, 0))[0]
    assert rows.tolist() == [True, True, True, False, False, False, False, False]
    for t in (q, k, v):
        assert torch.isfinite(t.grad).all()
    assert torch.all(q.grad[0, ~rows] == 0)


# ---- runtime.context ---------------------------------------------------------------------------------------------------------------
def _cfg(block):
    return {"runtime": {"context": block}}


def test_runtime_context_block_is_checked_on_the_host():
    import train as tr
    assert tr.context_settings({}) is None and tr.context_settings({"runtime": {}}) is None
    assert tr.context_settings(_cfg(None)) is None
    assert tr.context_settings(_cfg({"past": None, "future": None})) is None
    assert tr.context_settings(_cfg({})) is None
    assert tr.context_settings(_cfg({"past": None, "future": 0})) == (None, 0)
    assert tr.context_settings(_cfg({"future": 0})) == (None, 0)
    assert tr.context_settings(_cfg({"past": 8, "future": 0})) == (8, 0)
    assert tr.context_settings(_cfg({"past": 0})) == (0, None)
    for bad in ({"past": 1, "window": 3}, {"past": -1}, {"future": -2}, {"past": 1.5}, {"future": "0"}, {"past": True}, [4, 0], 4):
        with pytest.raises(ValueError, match="runtime.context"):
            tr.context_settings(_cfg(bad))


def test_shipped_config_has_the_block_switched_off():
    import train as tr
    from utils import get_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        cfg = get_config()
    finally:
        os.chdir(cwd)
    block = cfg["runtime"]["context"]
    assert dict(block) == {"past": None, "future": None} and tr.context_settings(cfg) is None


# ---- the model, without a device -------------------------------------------------------------------------------------------------
def test_model_stores_and_reports_the_band_without_a_device():
    cfg = synth.CASES["tiny_ragged"][0]
    assert M2FNet(cfg).context == (None, None)
    assert M2FNet(cfg, context=None).context == (None, None)
    m = M2FNet(cfg, context=(None, 0))
    assert m.context == (None, 0)
    m.set_context(8, 0)
    assert m.context == (8, 0)
    m.set_context(None, None)
    assert m.context == (None, None)
    m.set_context()
    assert m.context == (None, None)
    for bad in ((-1, 0), (0, -3), (1.0, 0), ("1", 0), (True, 0)):
        with pytest.raises(ValueError, match="context band"):
            M2FNet(cfg, context=bad)
        with pytest.raises(ValueError, match="context band"):
            m.set_context(*bad)
    assert m.context == (None, None)                                # (a refused setting changes nothing)
    assert runtime.context_band(None, None) == (-1, -1) and runtime.context_band(3, None) == (3, -1)


def test_default_plan_key_is_what_it_was():
    """Only a band extends the key (as `outputs` does): a model without one finds the plans, and the keys, it always had."""
    old = (8, 16, None, True, False, runtime.F32)
    assert _Engine.plan_key(8, 16, None, True, False, runtime.F32) == old
    assert _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (None, None)) == old
    assert _Engine.plan_key(8, 16, 128, True, True, runtime.BF16, (1, False)) == (8, 16, 128, True, True, runtime.BF16, (1, False))
    causal = _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (None, 0))
    window = _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (2, 0))
    assert causal[:6] == old and causal != old and window != causal and len({old, causal, window}) == 3
    assert _Engine.plan_key(8, 16, None, True, False, runtime.F32, (3, True), (2, 0)) not in (causal, window)


def test_new_entries_are_declared_and_exported():
    """The plan-level entries, and the kernel-level entries that CARRY the band: the forward ones in m2f_attn_opts, the backward ones as
    two plain arguments.  The per-feature entries (base name + "_band") are gone from the header, the bindings and the library."""
    header = open(runtime.HEADER_PATH).read()
    carriers = ("m2f_attention_fwd", "m2f_attention_bwd", "m2f_attention_varlen_fwd", "m2f_attention_varlen_bwd")
    for sym in carriers + ("m2f_plan_attention_band", "m2f_plan_get_attention_band"):
        assert sym in runtime.SIGNATURES and ("int " + sym + "(") in header, sym
        assert hasattr(runtime.lib(), sym), sym
    struct = header[header.index("typedef struct m2f_attn_opts {"):header.index("} m2f_attn_opts;")]
    fields = [n for n, _ in runtime.AttnOptsC._fields_]
    assert "int past, future;" in struct and "past" in fields and "future" in fields
    for sym in ("m2f_attention_fwd", "m2f_attention_varlen_fwd"):
        assert runtime.SIGNATURES[sym][1][-1] is ctypes.POINTER(runtime.AttnOptsC), sym
    for sym in ("m2f_attention_bwd", "m2f_attention_varlen_bwd"):
        assert runtime.SIGNATURES[sym][1][-2:] == [ctypes.c_int, ctypes.c_int], sym
        decl = header[header.index("int " + sym + "("):]
        assert decl[:decl.index(");")].rstrip().endswith("int past, int future"), sym
    for sym in carriers:
        old = sym + "_band"
        assert old not in runtime.SIGNATURES and old not in header and not hasattr(runtime.lib(), old), old
