"""Streaming inference on the CPU: tests/golden/stream_ref.py - an incremental forward from per-site K / V lists cut to past + 1 rows -
against the oracle's full forward with tests/golden/band_ref.py swapped in (caching is exact under a multi-layer window), and the
argument refusals of M2FNet.stream, which need no GPU."""
import pytest
import torch

import band_ref as R
import long_cases
import stream_ref
import synth
from oracle import m2fnet_oracle as O
from mer_amd import streaming
from mer_amd.layout import M2FConfig
from mer_amd.model import M2FNet

CASES = [("tiny_ragged", None), ("tiny_ragged", 2), ("tiny_ragged", 0), ("tiny_shared_norm", 1), ("tiny_odd_heads", 5),
         ("tiny_no_fam", None), ("tiny_audio_only", 1), ("tiny_text_only", None), ("c2_slice", 3), ("long_tiny", None),
         ("long_tiny", 8), ("long_odd_heads", 70)]


def _case(name):
    if name in long_cases.CASES:
        return long_cases.inputs(name)
    cfg, B, L, lengths, kind = synth.CASES[name]
    return (cfg,) + synth.make_inputs(cfg, B, L, lengths, kind)


@pytest.mark.parametrize("name,past", CASES)
@pytest.mark.parametrize("dtype,bound", [(torch.float32, 1e-6), (torch.float64, 1e-12)])
def test_incremental_forward_reproduces_the_banded_oracle(name, past, dtype, bound):
    cfg, text, audio, key_pad, _ = _case(name)
    sd = {k: v.to(dtype) for k, v in synth.make_state_dict(cfg).items()}
    text, audio = text.to(dtype), audio.to(dtype)
    with R.swapped_in((past, 0)):
        want = O.forward(sd, cfg, text, audio, key_pad)
    got = stream_ref.run(sd, cfg, text, audio, key_pad, past)
    assert torch.isfinite(got).all()
    err = (got - want)[~key_pad].abs().max().item()
    print(f"{name} past={past} {dtype}: {err:.3e}")
    assert err < bound, err
    assert torch.all(got[key_pad] == 0)


def test_a_window_changes_the_numbers_and_a_wrong_window_is_seen():
    """(the pin can fail: the reference cut to another window does not match)"""
    cfg, text, audio, key_pad, _ = _case("tiny_ragged")
    sd = synth.make_state_dict(cfg)
    with R.swapped_in((2, 0)):
        want = O.forward(sd, cfg, text, audio, key_pad)
    got = stream_ref.run(sd, cfg, text, audio, key_pad, 3)
    assert (got - want)[~key_pad].abs().max().item() > 1e-4


# ---- refusals, before the GPU is touched ----------------------------------------------------------------------------------------------
def _model(context, dropout=0.0):
    return M2FNet(synth._cfg(48, 64, 64, 4, 4, 4, 1, 1, 1, dropout=dropout), context=context)


@pytest.mark.parametrize("context", [None, (None, None), (2, 1), (None, 3), (0, None)])
def test_a_band_that_looks_ahead_cannot_stream(context):
    with pytest.raises(ValueError, match="causal context band"):
        _model(context).eval().stream(4)


def test_training_mode_with_dropout_is_refused():
    m = _model((None, 0), dropout=0.1)
    with pytest.raises(RuntimeError, match="training mode with dropout > 0"):
        m.train().stream(4)
    # (without dropout a model in training mode scores what eval mode scores: not refused here - the next refusal is the capacity's)
    with pytest.raises(ValueError, match="capacity"):
        _model((None, 0)).train().stream(4, capacity=0)


@pytest.mark.parametrize("capacity", [0, -1, 513, 4096, 2.5, True])
def test_capacity_outside_1_to_512_is_refused(capacity):
    with pytest.raises(ValueError, match="capacity"):
        _model((None, 0)).eval().stream(4, capacity=capacity)
    with pytest.raises(ValueError, match="capacity"):
        _model((3, 0)).eval().stream(4, capacity=capacity)


def test_a_window_past_the_capacity_limit_is_refused():
    with pytest.raises(ValueError, match="capacity"):
        _model((512, 0)).eval().stream(4)


@pytest.mark.parametrize("n", [0, -3, 1.5, True])
def test_max_streams_must_be_a_positive_integer(n):
    with pytest.raises(ValueError, match="max_streams"):
        _model((None, 0)).eval().stream(n)


def test_capacity_defaults_and_is_raised_to_the_window():
    assert streaming.resolve_capacity(None, None) == 512
    assert streaming.resolve_capacity(None, 40) == 40
    assert streaming.resolve_capacity(8, None) == 9
    assert streaming.resolve_capacity(8, 3) == 9
    assert streaming.resolve_capacity(8, 20) == 20
    assert streaming.resolve_capacity(0, None) == 1
    assert streaming.resolve_capacity(511, None) == 512


def test_cache_bytes_formula():
    """2 * sum_sites pad(d_site) * S * C * 4 B: C3 width (roberta-large 1024 + wav2vec2 768, 8 heads), shipped depth, 64 streams of
    512 rows = 3.8 GB in fp32, half of it in bf16 mode."""
    c3 = dict(synth.C2P_MODEL, TEXT=dict(synth.C2P_MODEL["TEXT"], embedding_size=1024))
    cfg = M2FConfig.from_model_config(c3)
    sites = 6 * 768 + 6 * 1024 + 5 * 768
    assert streaming.cache_bytes(cfg, 64, 512) == 2 * sites * 64 * 512 * 4
    assert round(streaming.cache_bytes(cfg, 64, 512) / 1e9, 1) == 3.8
    assert streaming.cache_bytes(cfg, 64, 512, bf16=True) * 2 == streaming.cache_bytes(cfg, 64, 512)
    # head dims that are no multiple of the pad: 60 / 4 = 15 -> 16 floats per head
    odd = M2FConfig.from_model_config(synth.CASES["tiny_odd_heads"][0])
    assert streaming.cache_bytes(odd, 2, 3) == 2 * (1 * 4 * 16 + 1 * 72 + 3 * 96) * 2 * 3 * 4
