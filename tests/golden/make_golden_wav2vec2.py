"""Writes tests/golden/w2v_*.npz by running transformers.Wav2Vec2Model (feat_extract_norm="group", conv_bias=False,
do_stable_layer_norm=False: the architecture of the torchaudio WAV2VEC2_BASE that the reference's audio stage runs,
src/feature_extractors/audio_wav2vec2/embeddings.py:52-91) in eval mode on CPU, with the deterministic weights / waveforms of
synth_wav2vec2.py.  The model gets the padded batch and a sample mask, as the reference gets (audio, lengths), and the pooled
embedding is the mean of each utterance's valid frames (embeddings.py:80-85).  Fixtures hold outputs only.
usage: python tests/golden/make_golden_wav2vec2.py"""
import os
import sys

import numpy as np
import torch
from transformers import Wav2Vec2Config, Wav2Vec2Model

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_wav2vec2 as SW  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    torch.set_num_threads(8)
    for name, (c, lengths) in SW.CASES.items():
        model = Wav2Vec2Model(Wav2Vec2Config(**c)).eval()
        model.load_state_dict(SW.make_state_dict(c), strict=True)
        wave, lens = SW.make_batch(lengths)
        mask = (torch.arange(wave.shape[1])[None, :] < lens[:, None]).long()
        with torch.inference_mode():
            o = model(wave, attention_mask=mask)
        hid, feat = o.last_hidden_state, o.extract_features
        out_len = np.array([SW.out_length(n) for n in lengths], dtype=np.int64)
        assert hid.shape[1] == SW.out_length(max(lengths))
        pooled = np.stack([hid[b, :n].double().mean(0).numpy() for b, n in enumerate(out_len)]).astype(np.float32)
        feat_rows = np.stack([np.stack([feat[b, 0].numpy(), feat[b, n // 2].numpy(), feat[b, n - 1].numpy()]) for b, n in enumerate(out_len)])
        np.savez_compressed(os.path.join(OUT, name + ".npz"), pooled=pooled, out_lengths=out_len, feat_rows=feat_rows,
                            hidden_first=hid[:, 0].numpy(), hidden_last_valid=np.stack([hid[b, n - 1].numpy() for b, n in enumerate(out_len)]),
                            hidden_valid_abs=np.array([float(np.mean([hid[b, :n].double().abs().mean() for b, n in enumerate(out_len)]))]))
        print(name, tuple(hid.shape), out_len.tolist(), float(hid[0, : out_len[0]].abs().mean()))


if __name__ == "__main__":
    main()
