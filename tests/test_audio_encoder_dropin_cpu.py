"""Host-side checks of the in-loop audio encoder's data path (src/dataset.py): the WAV loader (16 kHz mono 16-bit PCM only,
truncated at 10 s), waveform items and their collation, and the `runtime.audio_encoder` config block."""
import os
import sys
import wave

import numpy as np
import pandas as pd
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))


def write_wav(path, samples, rate=16000, channels=1, width=2):
    pcm = np.clip(np.round(np.asarray(samples) * 32768.0), -32768, 32767).astype("<i2")
    if channels > 1:
        pcm = np.repeat(pcm, channels)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes() if width == 2 else np.zeros(len(pcm), dtype=np.uint8).tobytes())


def test_load_wav_reads_pcm16_and_truncates_at_10_s(tmp_path):
    import dataset as ds
    g = np.random.default_rng(0)
    x = g.uniform(-0.9, 0.9, size=16000 * 11).astype(np.float32)
    write_wav(tmp_path / "a.wav", x)
    w = ds.load_wav(tmp_path / "a.wav")
    assert w.dtype == torch.float32 and w.shape == (160000,)
    ref = np.clip(np.round(x[:160000] * 32768.0), -32768, 32767) / 32768.0
    assert np.array_equal(w.numpy(), ref.astype(np.float32))
    write_wav(tmp_path / "b.wav", x[:1234])
    assert ds.load_wav(tmp_path / "b.wav").shape == (1234,)


@pytest.mark.parametrize("kw", [{"rate": 8000}, {"rate": 44100}, {"channels": 2}, {"width": 1}])
def test_load_wav_refuses_what_it_cannot_read_exactly(tmp_path, kw):
    import dataset as ds
    write_wav(tmp_path / "x.wav", np.zeros(1600), **kw)
    with pytest.raises(ValueError):
        ds.load_wav(tmp_path / "x.wav")


def _table():
    rows = [("u", "joy", 3, 1), ("u", "neutral", 3, 0), ("u", "anger", 5, 0), ("u", "fear", 3, 2), ("u", "joy", 5, 1)]
    return pd.DataFrame(rows, columns=["Utterance", "Emotion", "Dialogue_ID", "Utterance_ID"])


def test_waveform_items_collate_to_the_valid_utterances_of_the_batch(tmp_path):
    import dataset as ds
    table = _table()
    lens = [900, 400, 1500, 700, 1100]
    for (d, u), n in zip(zip(table["Dialogue_ID"], table["Utterance_ID"]), lens):
        write_wav(tmp_path / f"dia{d}_utt{u}.wav", np.full(n, (d * 10 + u) / 100.0))
    waves = ds.load_waveforms(table, tmp_path)
    assert [w.shape[0] for w in waves] == lens
    text = torch.randn(len(table), 8)
    dset = ds.Dataset("train", text_embeddings=text, table=table, waveforms=waves)
    assert dset.audio_embeddings is None
    batch = ds.collate_fn([dset[0], dset[1]])                   # dialogue 3 (3 utterances), dialogue 5 (2)
    assert "audio" not in batch
    assert batch["padding_mask"].tolist() == [[False, False, False], [False, False, True]]
    assert batch["wave_index"].tolist() == [0, 1, 2, 3, 4]
    assert batch["wave_lengths"].tolist() == [400, 900, 700, 1500, 1100]    # Utterance_ID order within each dialogue
    assert batch["waveforms"].shape == (5, 1500)
    for j, n in enumerate(batch["wave_lengths"].tolist()):
        assert torch.count_nonzero(batch["waveforms"][j, n:]) == 0
    assert torch.allclose(batch["waveforms"][1, :900], torch.full((900,), 0.31), atol=1e-4)   # dia3_utt1
    # without waveforms, items and batches are exactly what they were
    plain = ds.Dataset("train", text_embeddings=text, audio_embeddings=torch.randn(len(table), 4), table=table)
    b = ds.collate_fn([plain[0], plain[1]])
    assert list(b) == ["text", "audio", "padding_mask", "emotion"]


def test_config_has_the_audio_encoder_block():
    from utils import get_config
    ae = get_config().runtime.audio_encoder
    assert set(ae) >= {"enabled", "precision", "geometry", "checkpoint", "wav_dir"}
    assert ae["enabled"] is False and ae["precision"] == "bf16" and ae["geometry"] == "base"
