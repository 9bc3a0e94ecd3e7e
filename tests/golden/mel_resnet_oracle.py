"""Float64 restatement of the reference's audio_mel embedding (src/feature_extractors/audio_mel: dataset.py _get_mel_spectrogram
and get_mel_spectrogram, model.py, embeddings.py save_embeddings), unfolded: the image has three identical channels, BatchNorm runs
as BatchNorm (eval mode), torchvision's resnet18 layer by layer.  numpy and torch.nn.functional only."""
import math

import numpy as np
import torch
import torch.nn.functional as F

N_FFT, HOP, N_MELS, SR, FMAX, FRAMES = 400, 160, 128, 16000, 8000.0, 1001
LOG_EPS = np.finfo(float).eps


def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    lin = f / (200.0 / 3)
    logv = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (math.log(6.4) / 27.0)
    return np.where(f >= 1000.0, logv, lin)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((math.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3) * m)


def mel_filters():
    """[128, 201]: Slaney triangles over 0 .. 8 kHz, rows divided by their L1 norm (norm=1)."""
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(FMAX), N_MELS + 2))
    fft_f = np.linspace(0.0, SR / 2, N_FFT // 2 + 1)
    w = np.zeros((N_MELS, fft_f.size))
    for i in range(N_MELS):
        lower = (fft_f - mel_f[i]) / (mel_f[i + 1] - mel_f[i])
        upper = (mel_f[i + 2] - fft_f) / (mel_f[i + 2] - mel_f[i + 1])
        w[i] = np.maximum(0.0, np.minimum(lower, upper))
    s = w.sum(axis=1, keepdims=True)
    return w / np.where(s > 0, s, 1.0)


def mel_power1(x, n):
    """Steps 1-4: [frames, 128] mel magnitudes of the first n samples (None for a silent clip)."""
    x = np.asarray(x, dtype=np.float64)[:n]
    peak = np.abs(x).max() if n else 0.0
    if peak == 0:
        return None
    y = np.pad(x / peak, N_FFT // 2, mode="constant")
    frames = 1 + n // HOP
    idx = np.arange(frames)[:, None] * HOP + np.arange(N_FFT)[None, :]
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N_FFT) / N_FFT)
    mag = np.abs(np.fft.rfft(y[idx] * win, axis=1))
    return mag @ mel_filters().T


def spectrogram(x, n, png_levels=True, return_scaled=False):
    """[1001, 128] image (one of its three identical channels).  return_scaled: also the float32 v * 255 of the valid frames (the
    value whose floor is the level), or None where the image is blank."""
    mel = mel_power1(x, n)
    img = np.zeros((FRAMES, N_MELS))
    scaled = None
    if mel is not None:
        lg = np.log(mel + LOG_EPS)
        lo, hi = lg.min(), lg.max()
        if hi > lo:                      # the reference divides by zero otherwise: defined as a blank image
            v = (lg - lo) / (hi - lo)
            scaled = (v * 255.0).astype(np.float32)
            img[: v.shape[0]] = np.floor(scaled) / 255.0 if png_levels else v
    return (img, scaled) if return_scaled else img


def _bn(x, sd, p):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)


def backbone_features(img, sd):
    """img [B, 1001, 128] float64 -> torchvision resnet18 pooled features [B, 512] (eval mode, three identical channels)."""
    sd = {k: v.double() for k, v in sd.items()}
    x = torch.as_tensor(img, dtype=torch.float64)[:, None].repeat(1, 3, 1, 1)
    x = F.relu(_bn(F.conv2d(x, sd["resnet18.conv1.weight"], stride=2, padding=3), sd, "resnet18.bn1"))
    x = F.max_pool2d(x, 3, 2, 1)
    for li, stride in zip(range(1, 5), (1, 2, 2, 2)):
        for bi in range(2):
            p = f"resnet18.layer{li}.{bi}"
            s = stride if bi == 0 else 1
            t = F.relu(_bn(F.conv2d(x, sd[p + ".conv1.weight"], stride=s, padding=1), sd, p + ".bn1"))
            t = _bn(F.conv2d(t, sd[p + ".conv2.weight"], padding=1), sd, p + ".bn2")
            idn = _bn(F.conv2d(x, sd[p + ".downsample.0.weight"], stride=s), sd, p + ".downsample.1") if p + ".downsample.0.weight" in sd else x
            x = F.relu(t + idn)
    return x.mean(dim=(2, 3))


def head(feat, sd):
    sd = {k: v.double() for k, v in sd.items()}
    h = F.relu(F.linear(feat, sd["resnet18.fc.weight"], sd["resnet18.fc.bias"]))
    e = F.linear(h, sd["projector.1.weight"], sd["projector.1.bias"])
    return e / e.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def embed(img, sd):
    """[B, 1001, 128] images -> [B, 300] unit rows."""
    return head(backbone_features(img, sd), sd)


def utterance_embeddings(waves, lengths, sd, png_levels=True):
    imgs = np.stack([spectrogram(w, int(n), png_levels) for w, n in zip(waves, lengths)])
    return embed(imgs, sd)
