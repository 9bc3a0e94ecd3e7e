"""GPU test of the in-loop audio encoder inside the training path: WAV files -> Dataset(waveforms=...) -> collate_fn ->
move_batch(audio_encoder=...) -> a tiny M2FNet (d_audio 64) step with a finite loss; move_batch's rows equal a direct encoder call."""
import os
import sys

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import synth  # noqa: E402
import synth_wav2vec2 as SW  # noqa: E402
from test_audio_encoder_dropin_cpu import write_wav  # noqa: E402


def _dataset(tmp_path, n_dia=5, seed=0):
    import dataset as ds
    g = np.random.default_rng(seed)
    rows = []
    for d in range(n_dia):
        for u in range(int(g.integers(1, 5))):
            rows.append((f"utt {d}-{u}", list(ds.EMOTIONS)[int(g.integers(0, 2))], d, u))
    table = pd.DataFrame(rows, columns=["Utterance", "Emotion", "Dialogue_ID", "Utterance_ID"])
    for d, u in zip(table["Dialogue_ID"], table["Utterance_ID"]):
        n = int(g.integers(2000, 9000))
        write_wav(os.path.join(tmp_path, f"dia{d}_utt{u}.wav"), 0.2 * np.sin(np.arange(n) * (0.01 + 0.003 * u)) + 0.02 * g.standard_normal(n))
    text = torch.from_numpy(g.standard_normal((len(rows), 64)).astype(np.float32))
    return ds.Dataset("train", text_embeddings=text, table=table, waveforms=ds.load_waveforms(table, tmp_path))


def test_waveforms_through_the_encoder_into_a_tiny_m2fnet(tmp_path):
    import dataset as ds
    import train as tr
    from metrics import move_batch
    dset = _dataset(str(tmp_path))
    batch = ds.collate_fn([dset[i] for i in range(len(dset))])
    enc = tr.build_audio_encoder({"precision": "fp32", "geometry": dict(SW.TINY)}, 64, torch.device("cuda:0"))
    enc.load_state_dict(SW.make_state_dict(SW.TINY))
    device = torch.device("cuda:0")
    text, audio, emotion, mask = move_batch(batch, device, audio_encoder=enc)
    B, L = mask.shape
    assert audio.shape == (B, L, 64)
    direct = enc.utterance_embeddings(batch["waveforms"].to(device), batch["wave_lengths"].to(device))
    assert torch.equal(audio[~mask], direct)                     # valid utterances in (dialogue, utterance) order
    assert torch.count_nonzero(audio[mask]) == 0
    cfg = synth._cfg(64, 64, 64, 4, 4, 4, 1, 1, 1)
    model = tr.M2FNet(cfg)
    model.load_state_dict(synth.make_state_dict(cfg))
    model = model.to(device).train()
    loss = model.train_step(text, audio, mask, emotion, use_graph=False)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and loss.item() > 0
