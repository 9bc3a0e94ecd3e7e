"""Host-side checks of the in-loop wav2vec2 audio encoder (wav2vec2.py): output lengths against the transformers fixtures,
state-dict layouts (transformers as is, torchaudio's renamed one), refused configurations and the grow-only workspace."""
import os

import numpy as np
import pytest
import torch

import synth_wav2vec2 as SW
import mer_amd  # noqa: F401
from mer_amd import wav2vec2 as W


@pytest.mark.parametrize("name", list(SW.CASES))
def test_output_length_formula_matches_fixture(golden_dir, name):
    c, lengths = SW.CASES[name]
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    got = [W.output_length(n, c["conv_kernel"], c["conv_stride"]) for n in lengths]
    assert got == fx["out_lengths"].tolist()
    enc = W.Wav2Vec2Encoder(c, precision="fp32")
    g = enc.geometry(len(lengths), max(lengths))
    assert g["S"] == max(got) and g["T"][-1] == max(got)


def test_hf_state_dict_loads_as_is():
    c = SW.TINY
    sd = SW.make_state_dict(c)                     # transformers' keys, parametrizations.weight.original0/1, masked_spec_embed
    enc = W.Wav2Vec2Encoder(c, precision="fp32")
    enc.load_state_dict(sd)
    pc = enc.encoder.pos_conv_embed.conv
    assert torch.equal(pc.weight_g, sd["encoder.pos_conv_embed.conv.parametrizations.weight.original0"])
    assert torch.equal(pc.weight_v, sd["encoder.pos_conv_embed.conv.parametrizations.weight.original1"])
    assert torch.equal(enc.encoder.layers[1].attention.q_proj.weight, sd["encoder.layers.1.attention.q_proj.weight"])
    # the older weight_norm names of the same tensors
    old = {k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v"): v
           for k, v in sd.items()}
    enc2 = W.Wav2Vec2Encoder(c, precision="fp32")
    enc2.load_state_dict(old)
    assert all(torch.equal(a, b) for a, b in zip(enc.state_dict().values(), enc2.state_dict().values()))


def test_torchaudio_rename_round_trips():
    c = SW.TINY
    sd = SW.make_state_dict(c)
    ta = W.to_torchaudio_keys(sd)
    assert "encoder.transformer.layers.0.attention.k_proj.weight" in ta
    assert "encoder.feature_projection.projection.weight" in ta
    assert "encoder.transformer.pos_conv_embed.conv.weight_g" in ta
    assert "feature_extractor.conv_layers.0.layer_norm.weight" in ta
    a = W.Wav2Vec2Encoder(c, precision="fp32")
    a.load_state_dict(sd)
    b = W.Wav2Vec2Encoder(c, precision="fp32")
    b.load_state_dict(ta)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize("change", [{"conv_bias": True}, {"do_stable_layer_norm": True}, {"feat_extract_norm": "layer"},
                                    {"hidden_act": "relu"}, {"feat_extract_activation": "gelu_new"},
                                    {"conv_dim": (32,) * 6 + (64,)}, {"num_conv_pos_embedding_groups": 64}])
def test_unsupported_configs_raise(change):
    with pytest.raises(NotImplementedError):
        W.Wav2Vec2Encoder(dict(SW.TINY, **change))


def test_workspace_is_one_grow_only_allocation():
    enc = W.Wav2Vec2Encoder(W.base_config(), precision="bf16")
    sizes = []
    for B, N in [(4, 48000), (2, 16000), (8, 9000), (4, 48000), (1, 1000)]:
        g = enc.geometry(B, N)
        buf = enc._workspace(g, torch.device("cpu"))
        sizes.append(buf.numel())
        assert buf.numel() >= g["floats"] * 4 + g["mapped"] * 2
    assert sizes == sorted(sizes)                                         # never shrinks
    assert len(set(sizes)) == 1                                           # the first batch (4 x 3 s) was the largest of them


def test_conv_pitches_hold_every_window():
    """Pitches P_{l-1} = s_l P_l, each at least the padded batch's frame count; the last valid window of every layer lies inside its
    utterance's pitch."""
    enc = W.Wav2Vec2Encoder(W.base_config(), precision="fp32")
    for N in (400, 645, 16000, 160000, 159999, 31337):
        g = enc.geometry(3, N)
        T, P = g["T"], g["P"]
        for l in range(len(T)):
            assert P[l] >= T[l]
            if l:
                assert P[l - 1] == enc.strides[l] * P[l]
                assert (T[l] - 1) * enc.strides[l] + enc.kernels[l] <= T[l - 1]


def test_batches_past_32_bit_addressing_run_in_utterance_chunks():
    """No matrix of any launch reaches 2^30 elements, however large the batch; the chunk size is capped by chunk_utterances too."""
    enc = W.Wav2Vec2Encoder(W.base_config(), precision="bf16")
    for B, N in [(64, 160000), (1500, 160000), (5000, 16000), (3, 400)]:
        g = enc.geometry(B, N)
        assert 1 <= g["ub"] <= B
        assert all(cnt < (1 << 30) for _, cnt in g["off"].values())
        if B * g["S"] * enc.inter >= (1 << 30):
            assert g["ub"] < B
    assert enc.geometry(1500, 160000)["ub"] < 1500
    enc.chunk_utterances = 16
    assert enc.geometry(64, 160000)["ub"] == 16
    assert enc.workspace_bytes(64, 160000) < W.Wav2Vec2Encoder(W.base_config(), precision="bf16").workspace_bytes(64, 160000)
