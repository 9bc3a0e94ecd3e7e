"""Seeded audio_mel weights in the reference checkpoint's key layout (model.py: ``resnet18.*`` torchvision keys, ``projector.1.*``)
and seeded speech-like waveforms.  BatchNorm running statistics come from a float64 train-mode pass over seeded spectrograms with
gamma / beta drawn at random, so eval-mode activations keep a sane scale through the eight blocks (BatchNorm's defaults with
Kaiming weights let them grow block after block)."""
import numpy as np
import torch
import torch.nn.functional as F

STAGES = ((64, 1), (128, 2), (256, 2), (512, 2))


def _conv_shapes():
    sh = [("resnet18.conv1.weight", (64, 3, 7, 7), "resnet18.bn1")]
    cin = 64
    for li, (c, s) in enumerate(STAGES, start=1):
        for bi in range(2):
            p = f"resnet18.layer{li}.{bi}"
            st = s if bi == 0 else 1
            sh.append((p + ".conv1.weight", (c, cin, 3, 3), p + ".bn1"))
            sh.append((p + ".conv2.weight", (c, c, 3, 3), p + ".bn2"))
            if bi == 0 and (st != 1 or cin != c):
                sh.append((p + ".downsample.0.weight", (c, cin, 1, 1), p + ".downsample.1"))
            cin = c
    return sh


def _stat_images(g, n=3, rows=256):
    """Seeded smooth images in [0, 1] at 8-bit levels: the statistics pass's input."""
    t = np.linspace(0, 1, rows)[:, None]
    f = np.linspace(0, 1, 128)[None, :]
    out = []
    for _ in range(n):
        base = 0.5 + 0.25 * np.sin(2 * np.pi * (g.uniform(2, 9) * t + g.uniform(1, 5) * f)) * np.exp(-g.uniform(0, 2) * f)
        out.append(np.floor(np.clip(base + 0.1 * g.standard_normal((rows, 128)), 0, 1) * 255) / 255)
    return torch.tensor(np.stack(out))[:, None].repeat(1, 3, 1, 1)


def make_state_dict(seed=0, num_batches_tracked=True):
    g = np.random.default_rng(seed)
    sd = {}
    for name, shape, bn in _conv_shapes():
        fan_out = shape[0] * shape[2] * shape[3]
        sd[name] = torch.tensor(g.standard_normal(shape) * np.sqrt(2.0 / fan_out))
        c = shape[0]
        sd[bn + ".weight"] = torch.tensor(g.uniform(0.5, 1.5, c))
        sd[bn + ".bias"] = torch.tensor(g.normal(0.0, 0.2, c))
        sd[bn + ".running_mean"] = torch.zeros(c, dtype=torch.float64)
        sd[bn + ".running_var"] = torch.ones(c, dtype=torch.float64)
        if num_batches_tracked:
            sd[bn + ".num_batches_tracked"] = torch.tensor(1)
    for name, (o, i) in (("resnet18.fc", (1000, 512)), ("projector.1", (300, 1000))):
        sd[name + ".weight"] = torch.tensor(g.uniform(-1, 1, (o, i)) / np.sqrt(i))
        sd[name + ".bias"] = torch.tensor(g.uniform(-1, 1, o) / np.sqrt(i))

    # train-mode pass: each BatchNorm's running statistics := its batch statistics (momentum 1), in network order
    def bn(x, p):
        return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], True, 1.0, 1e-5)
    x = _stat_images(g)
    x = F.max_pool2d(F.relu(bn(F.conv2d(x, sd["resnet18.conv1.weight"], stride=2, padding=3), "resnet18.bn1")), 3, 2, 1)
    for li, (c, s) in enumerate(STAGES, start=1):
        for bi in range(2):
            p = f"resnet18.layer{li}.{bi}"
            st = s if bi == 0 else 1
            t = F.relu(bn(F.conv2d(x, sd[p + ".conv1.weight"], stride=st, padding=1), p + ".bn1"))
            t = bn(F.conv2d(t, sd[p + ".conv2.weight"], padding=1), p + ".bn2")
            idn = bn(F.conv2d(x, sd[p + ".downsample.0.weight"], stride=st), p + ".downsample.1") if p + ".downsample.0.weight" in sd else x
            x = F.relu(t + idn)
    return {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}


def speech_like(n, seed):
    """n samples at 16 kHz: a harmonic voice with a gliding pitch under a syllable envelope, and a noise floor."""
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    f0 = g.uniform(90, 220) * (1 + 0.15 * np.sin(2 * np.pi * g.uniform(0.3, 1.5) * t))
    phase = 2 * np.pi * np.cumsum(f0) / 16000.0
    voice = sum(np.sin(h * phase + g.uniform(0, 2 * np.pi)) / h for h in range(1, 12))
    env = np.clip(np.sin(2 * np.pi * g.uniform(2, 5) * t + g.uniform(0, 6)), 0, None) ** 2
    x = g.uniform(0.1, 0.6) * env * voice / 3 + 0.003 * g.standard_normal(n)
    return np.clip(x, -1, 1).astype(np.float32)


# lengths in samples: 0.5 .. 10 s, exactly 10 s, and multiples of 160 +- 1
LENGTHS = [8000, 160000, 23 * 160 - 1, 23 * 160, 23 * 160 + 1, 61234, 100000, 137 * 160 + 1]


def batch(lengths=LENGTHS, seed=0):
    """(waves [B, max n] zero-padded fp32, lengths int64)."""
    n = max(lengths)
    w = np.zeros((len(lengths), n), dtype=np.float32)
    for i, m in enumerate(lengths):
        w[i, :m] = speech_like(m, seed * 1000 + i)
    return torch.from_numpy(w), torch.tensor(lengths, dtype=torch.int64)
