"""Deterministic wav2vec2-shaped configs, weights and waveform batches for the audio-encoder parity tests (numpy Philox, so
fixtures hold outputs only).  Keys / shapes are those of transformers.Wav2Vec2Model(config).state_dict() with the library's
wav2vec2-base defaults (feat_extract_norm="group", conv_bias=False, do_stable_layer_norm=False): the architecture of the
torchaudio WAV2VEC2_BASE the reference's audio stage runs (src/feature_extractors/audio_wav2vec2/embeddings.py:52-91)."""
import numpy as np
import torch

CONV_KERNEL = (10, 3, 3, 3, 3, 2, 2)
CONV_STRIDE = (5, 2, 2, 2, 2, 2, 2)


def cfg(conv_dim, hidden, layers, heads, inter, pos_k, pos_g):
    return {"conv_dim": (conv_dim,) * 7, "conv_kernel": CONV_KERNEL, "conv_stride": CONV_STRIDE, "conv_bias": False,
            "feat_extract_norm": "group", "feat_extract_activation": "gelu", "do_stable_layer_norm": False,
            "hidden_size": hidden, "num_hidden_layers": layers, "num_attention_heads": heads, "intermediate_size": inter,
            "hidden_act": "gelu", "num_conv_pos_embeddings": pos_k, "num_conv_pos_embedding_groups": pos_g, "layer_norm_eps": 1e-5}


TINY = cfg(32, 64, 2, 4, 128, 16, 4)
# name -> (config, lengths in samples; the batch is padded to the longest)
CASES = {
    "w2v_tiny": (TINY, [4000, 4000]),
    "w2v_ragged": (TINY, [8000, 3200, 5600]),                     # about N, 0.4 N, 0.7 N: pins the GroupNorm-over-padding quirk
    "w2v_long": (TINY, [48000, 30000]),                           # 149 frames: three 64-row key blocks
    "w2v_base_width": (cfg(512, 768, 1, 12, 3072, 128, 16), [16000, 9000]),   # one wav2vec2-base layer, the base front end
}


def out_length(n, kernels=CONV_KERNEL, strides=CONV_STRIDE):
    for k, s in zip(kernels, strides):
        n = (n - k) // s + 1
    return n


def state_dict_shapes(c):
    C, d, F = c["conv_dim"][0], c["hidden_size"], c["intermediate_size"]
    K, G = c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
    sh = [("feature_extractor.conv_layers.0.conv.weight", (C, 1, c["conv_kernel"][0])),
          ("feature_extractor.conv_layers.0.layer_norm.weight", (C,)), ("feature_extractor.conv_layers.0.layer_norm.bias", (C,))]
    for i in range(1, 7):
        sh.append((f"feature_extractor.conv_layers.{i}.conv.weight", (C, C, c["conv_kernel"][i])))
    sh += [("feature_projection.layer_norm.weight", (C,)), ("feature_projection.layer_norm.bias", (C,)),
           ("feature_projection.projection.weight", (d, C)), ("feature_projection.projection.bias", (d,)),
           ("encoder.pos_conv_embed.conv.bias", (d,)),
           ("encoder.pos_conv_embed.conv.parametrizations.weight.original0", (1, 1, K)),
           ("encoder.pos_conv_embed.conv.parametrizations.weight.original1", (d, d // G, K)),
           ("encoder.layer_norm.weight", (d,)), ("encoder.layer_norm.bias", (d,))]
    for i in range(c["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            sh += [(p + f"attention.{n}.weight", (d, d)), (p + f"attention.{n}.bias", (d,))]
        sh += [(p + "layer_norm.weight", (d,)), (p + "layer_norm.bias", (d,)),
               (p + "feed_forward.intermediate_dense.weight", (F, d)), (p + "feed_forward.intermediate_dense.bias", (F,)),
               (p + "feed_forward.output_dense.weight", (d, F)), (p + "feed_forward.output_dense.bias", (d,)),
               (p + "final_layer_norm.weight", (d,)), (p + "final_layer_norm.bias", (d,))]
    return sh


def make_state_dict(c, seed=5):
    """Philox weights keyed by parameter index, scaled so activations stay O(1) through the stack."""
    d, K = c["hidden_size"], c["num_conv_pos_embeddings"]
    sd = {}
    for idx, (name, shape) in enumerate(state_dict_shapes(c)):
        g = np.random.Generator(np.random.Philox(key=seed * 100003 + idx))
        x = g.standard_normal(shape).astype(np.float64)
        if name.endswith("norm.weight"):
            x = 1.0 + 0.1 * x
        elif name.endswith(".bias"):
            x = 0.05 * x
        elif name.endswith("original0"):                   # weight-norm magnitude: effective taps ~ 1 / sqrt(fan-in)
            x = np.sqrt(d / K) * (1.0 + 0.1 * x)
        elif name.endswith("original1"):
            pass
        elif "conv_layers" in name:
            x = x / np.sqrt(shape[1] * shape[2]) * 1.5
        else:
            x = x / np.sqrt(shape[1]) * 1.5
        sd[name] = torch.from_numpy(np.asarray(x, dtype=np.float32))
    sd["masked_spec_embed"] = torch.zeros(d)
    return sd


def make_batch(lengths, seed=13):
    """(waveforms [B, max(lengths)] fp32 zero-padded, lengths int64 [B]): a few tones plus noise, amplitude ~0.3."""
    g = np.random.Generator(np.random.Philox(key=seed))
    N = max(lengths)
    w = np.zeros((len(lengths), N), dtype=np.float32)
    for b, n in enumerate(lengths):
        t = np.arange(n) / 16000.0
        f = g.uniform(80.0, 2000.0, size=3)
        ph = g.uniform(0, 2 * np.pi, size=3)
        sig = sum(0.1 * np.sin(2 * np.pi * f[i] * t + ph[i]) for i in range(3)) + 0.05 * g.standard_normal(n)
        w[b, :n] = sig.astype(np.float32)
    return torch.from_numpy(w), torch.tensor(lengths, dtype=torch.int64)
