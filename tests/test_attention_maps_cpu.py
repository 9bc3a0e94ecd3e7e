"""The yardstick of the attention-map tests, on the CPU: the recorder of tests/attention_maps_ref.py against the head-averaged weights
the real reference wrote into the fixtures and against nn.MultiheadAttention(need_weights=True) in float64; the site names of
layout.attention_sites; the stream's logical-column helper; and the argument checks of functional.attention_weights, which must raise
ValueError before a GPU is asked for."""
import os

import numpy as np
import pytest
import torch

import attention_maps_ref as A
import band_ref as R
import synth
from oracle import m2fnet_oracle as O
from mer_amd import functional as F
from mer_amd import layout, streaming

FIXTURES = ["tiny_ragged", "tiny_shared_norm", "tiny_odd_heads"]
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("name", FIXTURES)
def test_recorder_matches_the_reference_written_weights(golden_dir, name):
    fx = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    cfg, B, L, lengths, kind = synth.CASES[name]
    text, audio, key_pad, _ = synth.make_inputs(cfg, B, L, lengths, kind)
    with A.recording() as rec:
        logits = O.forward(synth.make_state_dict(cfg), cfg, text, audio, key_pad)
    assert list(rec) == [n for n, _, _ in layout.attention_sites(cfg)]
    p = rec["fusion_layers.0.multihead_attention"]
    assert p.shape == (B, cfg["FAM"]["n_head"], L, L)
    assert (p.mean(dim=1) - torch.from_numpy(fx["fam0_attn_avg"])).abs().max() < 1e-6          # (the bound of tests/test_oracle.py:78)
    assert (A.head_average(p) - torch.from_numpy(fx["fam0_attn_avg"])).abs().max() < 1e-6
    # the recorder changes nothing: the oracle's logits are the recorded reference's
    assert (logits - torch.from_numpy(fx["logits_eval"])).abs()[~key_pad].max() < 2e-5
    assert O.attention.__module__ == "oracle.m2fnet_oracle"                                  # ... and it is gone afterwards


@pytest.mark.parametrize("band", [(None, None), (None, 0), (2, 0), (1, 1)])
@pytest.mark.parametrize("average", [True, False])
def test_recorder_matches_torch_multihead_attention_in_float64(band, average):
    B, L, E, H = 3, 7, 24, 4
    g = torch.Generator().manual_seed(5)
    mha = torch.nn.MultiheadAttention(E, H, batch_first=True, dtype=torch.float64)
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.randn(3 * E, E, generator=g, dtype=torch.float64) * 0.3)
        mha.in_proj_bias.copy_(torch.randn(3 * E, generator=g, dtype=torch.float64) * 0.1)
    xq, xk = (torch.randn(B, L, E, generator=g, dtype=torch.float64) for _ in range(2))
    key_pad = torch.zeros(B, L, dtype=torch.bool)
    key_pad[1, 4:] = True
    key_pad[2, 1:] = True
    w, b = mha.in_proj_weight.detach(), mha.in_proj_bias.detach()
    q, k, v = xq @ w[:E].T + b[:E], xk @ w[E:2 * E].T + b[E:2 * E], xq @ w[2 * E:].T + b[2 * E:]
    with A.recording(band) as rec:
        O.attention(q, k, v, key_pad, H, name="fusion_layers.0.attn")
    p = rec["fusion_layers.0.multihead_attention"]
    mask = None if band == (None, None) else R.band_mask(L, *band)
    with torch.no_grad():
        _, want = mha(xq, xk, xq, key_padding_mask=key_pad, need_weights=True, attn_mask=mask, average_attn_weights=average)
    rows = R.visible_rows(key_pad, band)                     # rows that see a key (torch has NaN in the others, the recorder zeros)
    assert rows[~key_pad].all()
    got = A.head_average(p) if average else p
    sel = rows[:, :, None] if average else rows[:, None, :, None]
    err = (got - want)[sel.expand_as(got)].abs().max().item()
    assert err < 1e-12, err
    empty = ~rows
    if empty.any():
        assert torch.all((p.permute(0, 2, 1, 3))[empty] == 0)


def test_site_names_follow_the_state_dict():
    want = {
        "tiny_ragged": [("audio_encoders.0.layers.0.self_attn", 4, 12), ("audio_encoders.0.layers.1.self_attn", 4, 12),
                        ("text_encoders.0.layers.0.self_attn", 4, 16), ("text_encoders.0.layers.1.self_attn", 4, 16),
                        ("fusion_layers.0.multihead_attention", 4, 16), ("fusion_layers.1.multihead_attention", 4, 16)],
        "tiny_audio_only": [("audio_encoders.0.layers.0.self_attn", 4, 16), ("audio_encoders.0.layers.1.self_attn", 4, 16)],
        "tiny_text_only": [("text_encoders.0.layers.0.self_attn", 8, 8), ("text_encoders.0.layers.1.self_attn", 8, 8)],
        "tiny_no_fam": [("audio_encoders.0.layers.0.self_attn", 4, 8), ("text_encoders.0.layers.0.self_attn", 4, 16)],
        "tiny_shared_norm": [("audio_encoders.0.layers.0.self_attn", 2, 32), ("audio_encoders.1.layers.0.self_attn", 2, 32)]
        + [(f"text_encoders.{e}.layers.{l}.self_attn", 4, 8) for e in range(3) for l in range(2)]
        + [("fusion_layers.0.multihead_attention", 3, 16)],
    }
    for name, sites in want.items():
        cfg = synth.CASES[name][0]
        assert layout.attention_sites(cfg) == sites, name
        assert layout.attention_sites(layout.M2FConfig.from_model_config(cfg)) == sites
        keys = set(synth.make_state_dict(cfg))
        for n, _, _ in sites:                                # every name is the state_dict prefix of the site's parameters
            assert n + ".in_proj_weight" in keys and n + ".out_proj.weight" in keys, n
    for name in synth.CASES:                                 # ... and every in-projection of a model is a site
        cfg = synth.CASES[name][0]
        prefixes = [k[: -len(".in_proj_weight")] for k in synth.make_state_dict(cfg) if k.endswith(".in_proj_weight")]
        assert [n for n, _, _ in layout.attention_sites(cfg)] == prefixes, name


@pytest.mark.parametrize("C", [1, 4, 64])
def test_logical_columns_of_a_stream(C):
    for ring in (False, True):
        for n in (0, 1, C - 1, C, C + 1, 2 * C + 3):
            if n < 0:
                continue
            if not ring and n > C:
                with pytest.raises(ValueError):
                    streaming.logical_columns(n, C, ring)
                continue
            first, count = streaming.logical_columns(n, C, ring)
            live = list(range(n))[-C:] if n else []          # the utterances a cache of C rows holds after n of them
            assert count == len(live) and [first + t for t in range(count)] == live, (n, C, ring)
            if ring and n:                                   # utterance u sits in physical row u % C: the live ones fill distinct rows
                assert len({u % C for u in live}) == count
    with pytest.raises(ValueError):
        streaming.logical_columns(-1, C, True)
    with pytest.raises(ValueError):
        streaming.logical_columns(1, 0, True)


def test_attention_weights_refuses_bad_arguments_without_a_gpu():
    B, L, H = 2, 5, 3
    probs = torch.zeros(B * H, 16, 16)
    bad = [
        dict(probs=torch.zeros(B * H, 16, 8)),               # not [B*H, Lp, Lp]
        dict(probs=torch.zeros(B * H, 5, 5)),                # the unpadded shape
        dict(probs=probs.double()),
        dict(probs=torch.zeros(B * H, 16, 32)[:, :, ::2]),    # the right shape, not contiguous
        dict(H=0), dict(B=0), dict(L=513), dict(L=True),
        dict(key_pad=torch.zeros(B, L + 1, dtype=torch.bool)),
        dict(cu=torch.zeros(B + 1, dtype=torch.int64)),
        dict(cu=torch.zeros(B, dtype=torch.int32)),
        dict(key_pad=torch.zeros(B, L, dtype=torch.bool), cu=torch.zeros(B + 1, dtype=torch.int32)),
        dict(past=-1), dict(future=1.5),
    ]
    for kw in bad:
        args = dict(probs=probs, B=B, L=L, H=H)
        args.update(kw)
        with pytest.raises(ValueError):
            F.attention_weights(**args)


def test_runtime_attention_maps_is_read_and_validated_before_the_gpu_is_touched():
    import sys
    import yaml
    sys.path.insert(0, os.path.join(ROOT, "src"))
    import test as te
    from utils import AttrDict
    with open(os.path.join(ROOT, "src", "config.yaml")) as f:
        raw = yaml.safe_load(f)
    block = raw["runtime"]["attention_maps"]
    assert block == {"enabled": False, "file": "attention_maps.npz", "sites": []}
    cfg = AttrDict(raw)
    assert te.attention_maps_settings(cfg) is None                          # the shipped default: off

    def with_block(b, **rt):
        c = AttrDict(raw)
        c.runtime = AttrDict(dict(raw["runtime"], attention_maps=b, **rt))
        return c

    assert te.attention_maps_settings(with_block(None)) is None
    assert te.attention_maps_settings(with_block(dict(block, enabled=True))) == ("attention_maps.npz", None)
    fam0 = "fusion_layers.0.multihead_attention"
    assert te.attention_maps_settings(with_block(dict(enabled=True, file="m.npz", sites=[fam0]))) == ("m.npz", [fam0])
    for bad in (dict(enabled="yes", file="m.npz"), dict(enabled=True, file=""), dict(enabled=True, file=None),
                dict(enabled=True, file="m.npz", sites=fam0), dict(enabled=True, file="m.npz", sites=[3]),
                dict(enabled=True, file="m.npz", sites=["fusion_layers.99.multihead_attention"])):
        with pytest.raises(ValueError, match="runtime.attention_maps"):
            te.attention_maps_settings(with_block(bad))
    with pytest.raises(ValueError, match="runtime.streaming"):
        te.attention_maps_settings(with_block(dict(block, enabled=True), streaming=True, context={"past": None, "future": 0}))
