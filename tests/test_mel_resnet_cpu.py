"""Host-side checks of the audio_mel encoder (mer_amd.mel_resnet): the float64 oracle (tests/golden/mel_resnet_oracle.py) pinned
against independent implementations (transformers' audio_utils front end and ResNetModel), the pack-time folds, the frame count,
strict checkpoint loading, and the `runtime.audio_encoder.model` config key."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
sys.path.insert(0, ROOT)

import mel_resnet_oracle as O  # noqa: E402
import synth_mel_resnet as S  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import mel_resnet as MR  # noqa: E402


def _tf_mel_filters():
    from transformers.audio_utils import mel_filter_bank
    fb = mel_filter_bank(201, 128, 0.0, 8000.0, 16000, norm=None, mel_scale="slaney")      # [201, 128]
    s = fb.sum(axis=0, keepdims=True)
    return (fb / np.where(s > 0, s, 1.0)).T


def test_mel_filters_match_transformers():
    ref = _tf_mel_filters()
    assert np.abs(O.mel_filters() - ref).max() < 1e-11
    assert np.abs(MR.mel_filters() - ref).max() < 1e-11
    assert (ref.sum(axis=1) > 0).all()                  # no empty filter at 128 bands over 201 bins


@pytest.mark.parametrize("n", [8000, 23 * 160 - 1, 23 * 160, 23 * 160 + 1, 61234])
def test_front_end_matches_transformers_spectrogram(n):
    from transformers.audio_utils import spectrogram, window_function
    x = S.speech_like(n, seed=n)
    y = x.astype(np.float64) / np.abs(x.astype(np.float64)).max()
    ref = spectrogram(y, window_function(400, "hann", periodic=True).astype(np.float64), frame_length=400, hop_length=160, power=1.0, center=True,
                      pad_mode="constant", mel_filters=_tf_mel_filters().T, mel_floor=1e-300, log_mel=None, dtype=np.float64)
    mine = O.mel_power1(x, n)
    assert mine.shape == ref.T.shape == (MR.frame_count(n), 128)
    # (transformers holds the STFT as complex64: agreement to float32 resolution of the largest band; measured 3.9e-8)
    assert np.abs(mine - ref.T).max() <= 2e-7 * np.abs(ref).max()


def test_stft_basis_is_the_windowed_dft():
    x = np.random.default_rng(0).standard_normal(400)
    B = MR.stft_basis()
    spec = np.fft.rfft(x * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 400)))
    assert np.abs(x @ B[:, :201] - spec.real).max() < 1e-11
    assert np.abs(np.abs(x @ B[:, :201] + 1j * (x @ B[:, 201:])) - np.abs(spec)).max() < 1e-11


def test_frame_count():
    for n in [0, 1, 159, 160, 161, 8000, 23 * 160 - 1, 23 * 160, 23 * 160 + 1, 160000]:
        assert MR.frame_count(n) == 1 + n // 160
        if n:
            assert O.mel_power1(S.speech_like(n, 1), n).shape[0] == MR.frame_count(n)
    assert MR.frame_count(MR.MAX_SAMPLES) == MR.FRAMES == 1001


def test_spectrogram_levels_and_blank_images():
    x = S.speech_like(30000, 3)
    v = O.spectrogram(x, 30000, png_levels=False)
    q, scaled = O.spectrogram(x, 30000, png_levels=True, return_scaled=True)
    f = MR.frame_count(30000)
    assert v[:f].min() == 0.0 and v[:f].max() == 1.0 and not v[f:].any()
    assert np.array_equal(np.round(q[:f] * 255), np.floor(scaled)) and np.abs(q - v).max() < 1 / 255
    assert not O.spectrogram(np.zeros(5000, np.float32), 5000).any()           # silent clip: blank (the one deviation)


def _to_transformers(sd):
    out = {"embedder.embedder.convolution.weight": sd["resnet18.conv1.weight"]}
    for s in ("weight", "bias", "running_mean", "running_var"):
        out[f"embedder.embedder.normalization.{s}"] = sd[f"resnet18.bn1.{s}"]
    for li in range(4):
        for bi in range(2):
            p, q = f"resnet18.layer{li + 1}.{bi}", f"encoder.stages.{li}.layers.{bi}"
            pairs = [(".conv1", ".bn1", ".layer.0"), (".conv2", ".bn2", ".layer.1"), (".downsample.0", ".downsample.1", ".shortcut")]
            for cv, bn, dst in pairs:
                if p + cv + ".weight" not in sd:
                    continue
                out[q + dst + ".convolution.weight"] = sd[p + cv + ".weight"]
                for s in ("weight", "bias", "running_mean", "running_var"):
                    out[q + dst + ".normalization." + s] = sd[p + bn + "." + s]
    return out


def test_backbone_matches_transformers_resnet():
    from transformers import ResNetConfig, ResNetModel
    sd = S.make_state_dict(0)
    m = ResNetModel(ResNetConfig(layer_type="basic", depths=[2, 2, 2, 2], hidden_sizes=[64, 128, 256, 512], embedding_size=64))
    missing, unexpected = m.load_state_dict(_to_transformers(sd), strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)
    m = m.double().eval()
    w, l = S.batch([8000, 40000], seed=1)
    img = np.stack([O.spectrogram(w[i].numpy(), int(l[i])) for i in range(2)])
    x = torch.tensor(img)[:, None].repeat(1, 3, 1, 1)
    with torch.no_grad():
        ref = m(pixel_values=x).pooler_output.flatten(1)
    mine = O.backbone_features(img, sd)
    assert (mine - ref).abs().max().item() < 1e-10 * max(1.0, ref.abs().max().item())


def _folded_features(img, sd):
    """The backbone from the encoder's packed, folded weights (float64): one input channel, BatchNorm as weights + bias."""
    sd = {k: v.double() for k, v in sd.items()}

    def bn(p):
        return {s: sd[f"{p}.{s}"] for s in ("weight", "bias", "running_mean", "running_var")}

    def unpack(wpk, cin, k):
        return wpk.view(wpk.shape[0], k, k, cin).permute(0, 3, 1, 2)

    w49, b0 = MR.fold_stem(sd["resnet18.conv1.weight"], bn("resnet18.bn1"))
    x = torch.tensor(img)[:, None]
    x = F.max_pool2d(F.relu(F.conv2d(x, w49.t().reshape(64, 1, 7, 7), b0, stride=2, padding=3)), 3, 2, 1)
    for li, bi, cin, cout, st, ds in MR.block_names():
        p = f"resnet18.layer{li}.{bi}"
        w1, b1 = MR.fold_bn(sd[p + ".conv1.weight"], bn(p + ".bn1"))
        w2, b2 = MR.fold_bn(sd[p + ".conv2.weight"], bn(p + ".bn2"))
        t = F.relu(F.conv2d(x, unpack(MR.pack_conv(w1), cin, 3), b1, stride=st, padding=1))
        idn = x
        if ds:
            wd, bd = MR.fold_bn(sd[p + ".downsample.0.weight"], bn(p + ".downsample.1"))
            idn = F.conv2d(x, unpack(MR.pack_conv(wd), cin, 1), bd, stride=st)
        x = F.relu(F.conv2d(t, unpack(MR.pack_conv(w2), cout, 3), b2, padding=1) + idn)
    return x.mean(dim=(2, 3))


def test_bn_and_channel_folding_equal_the_unfolded_model():
    sd = S.make_state_dict(2)
    w, l = S.batch([20000, 7000], seed=2)
    img = np.stack([O.spectrogram(w[i].numpy(), int(l[i])) for i in range(2)])
    ref = O.backbone_features(img, sd)
    assert (_folded_features(img, sd) - ref).abs().max().item() < 1e-10 * ref.abs().max().item()


def test_strict_load_accepts_the_checkpoint_and_rejects_key_mismatches():
    sd = S.make_state_dict(0)
    enc = MR.MelResNetEncoder(precision="fp32")
    enc.load_state_dict({"model_state_dict": sd, "epoch": 3})                 # the reference's checkpoint dict
    assert torch.equal(enc.resnet18.layer3[0].downsample[0].weight, sd["resnet18.layer3.0.downsample.0.weight"])
    enc.load_state_dict(S.make_state_dict(0, num_batches_tracked=False))     # bare, without num_batches_tracked
    missing = dict(sd)
    del missing["resnet18.layer2.1.bn2.running_var"]
    with pytest.raises(RuntimeError):
        enc.load_state_dict(missing)
    extra = dict(sd)
    extra["projector.2.weight"] = torch.zeros(3)
    with pytest.raises(RuntimeError):
        enc.load_state_dict(extra)


def test_encoder_refuses_cpu():
    enc = MR.MelResNetEncoder(precision="fp32")
    with pytest.raises(Exception):
        enc.utterance_embeddings(torch.zeros(1, 8000), torch.tensor([8000]))


def test_model_key_defaults_to_wav2vec2():
    import yaml
    with open(os.path.join(ROOT, "src", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["runtime"]["audio_encoder"]["model"] == "wav2vec2"


def test_build_audio_encoder_checks_mel_width_and_heads_before_the_device():
    import train as tr
    bogus = torch.device("meta")                        # never reached: the checks come first
    with pytest.raises(ValueError, match="300"):
        tr.build_audio_encoder({"model": "mel_resnet18"}, 768, bogus)
    with pytest.raises(ValueError, match="n_head"):
        tr.build_audio_encoder({"model": "mel_resnet18"}, 300, bogus, n_head=8)
    with pytest.raises(ValueError, match="mel_resnet18"):
        tr.build_audio_encoder({"model": "resnet50"}, 300, bogus)
