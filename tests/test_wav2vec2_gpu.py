"""GPU parity of the in-loop wav2vec2 audio encoder (wav2vec2.py): each new kernel against float64 torch, the whole encoder
against the fixtures written by transformers.Wav2Vec2Model (make_golden_wav2vec2.py).  fp32 mode: 1e-4 on O(1) states; bf16 mode
(bf16 GEMM / positional-conv operands, fp32 accumulation, fp32 GroupNorm / LayerNorm / attention): mean 1e-2 / max 6e-2, as
test_roberta_gpu.py states for the text encoder, and pooled cosine >= 0.999."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import synth_wav2vec2 as SW
import mer_amd  # noqa: F401
from mer_amd import functional as F
from mer_amd import runtime
from mer_amd.wav2vec2 import Wav2Vec2Encoder

pytestmark = pytest.mark.gpu


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / np.sqrt(2.0)))


def _enc(c, precision):
    m = Wav2Vec2Encoder(c, precision=precision)
    m.load_state_dict(SW.make_state_dict(c))
    return m.cuda().eval()


# ---- kernel level ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,N,P_extra", [(32, 4003, 0), (512, 16000, 37)])
def test_conv0_groupnorm_gelu_matches_float64(C, N, P_extra):
    g = torch.Generator().manual_seed(1)
    B = 3
    wave = torch.zeros(B, N)
    for b, n in enumerate([N, int(0.4 * N), int(0.7 * N)]):
        wave[b, :n] = 0.3 * torch.randn(n, generator=g)
    w0 = torch.randn(C, 1, 10, generator=g) / 3
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    T0 = (N - 10) // 5 + 1
    y = TF.conv1d(wave.double()[:, None], w0.double(), stride=5)                   # [B, C, T0]: statistics over the PADDED axis
    y = _gelu64(TF.group_norm(y, C, gamma.double(), beta.double(), eps=1e-5)).transpose(1, 2)
    out = F.w2v_conv0(wave.cuda(), w0.cuda(), gamma.cuda(), beta.cuda(), 5, P0=T0 + P_extra).cpu().view(B, T0 + P_extra, C)
    assert (out[:, :T0].double() - y).abs().max().item() < 1e-4
    assert torch.count_nonzero(out[:, T0:]) == 0
    out16 = F.w2v_conv0(wave.cuda(), w0.cuda(), gamma.cuda(), beta.cuda(), 5, P0=T0 + P_extra, bf16_out=True).cpu().view(B, T0 + P_extra, C)
    assert (out16[:, :T0].double() - y).abs().max().item() < 2e-2
    again = F.w2v_conv0(wave.cuda(), w0.cuda(), gamma.cuda(), beta.cuda(), 5, P0=T0 + P_extra).cpu().view(B, T0 + P_extra, C)
    assert torch.equal(again, out)


@pytest.mark.parametrize("k,T_in", [(3, 63), (2, 64), (3, 40), (2, 41)])
@pytest.mark.parametrize("prec", [runtime.F32, runtime.BF16])
def test_conv_layer_gemm_windows_including_the_last_frame(k, T_in, prec):
    """Overlapping channels-last windows on the grouped GEMM: P_in = 64 rows per utterance, T_in valid; with T_in = P_in (k = 2) or
    P_in - 1 (k = 3) the last utterance's last window ends at the last row of its pitch."""
    C, s, P_in, B = 64, 2, 64, 3
    g = torch.Generator().manual_seed(k * 100 + T_in)
    x = torch.randn(B * P_in + 1, C, generator=g)
    w = torch.randn(C, C, k, generator=g) / np.sqrt(C * k)
    T_out = (T_in - k) // s + 1
    xr = x[: B * P_in].view(B, P_in, C)[:, :T_in].double().transpose(1, 2)
    ref = _gelu64(TF.conv1d(xr, w.double(), stride=s)).transpose(1, 2)            # [B, T_out, C]
    out = F.w2v_conv_layer(x.cuda(), w.cuda(), s, P_in, precision=prec).cpu().view(B, P_in // s, C)[:, :T_out]
    tol = 1e-4 if prec == runtime.F32 else 3e-2
    assert (out.double() - ref).abs().max().item() < tol
    assert (out[-1, -1].double() - ref[-1, -1]).abs().max().item() < tol              # last frame of the last utterance


def test_feat_layernorm_compacts_pitched_rows():
    B, S, P, C = 3, 21, 32, 512
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B * P, C, generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ref = TF.layer_norm(x.view(B, P, C)[:, :S].double(), (C,), gamma.double(), beta.double(), eps=1e-5).reshape(B * S, C)
    out = F.w2v_feat_layernorm(x.cuda(), B, S, P, gamma.cuda(), beta.cuda()).cpu()
    assert (out.double() - ref).abs().max().item() < 1e-4


@pytest.mark.parametrize("d,G,K,S,lengths", [(64, 4, 16, 70, [70, 45, 3]), (768, 16, 128, 130, [130, 64, 129]), (128, 4, 15, 9, [9, 5])])
@pytest.mark.parametrize("bf16", [False, True])
def test_pos_conv_near_length_and_ragged_tiles(d, G, K, S, lengths, bf16):
    B = len(lengths)
    g = torch.Generator().manual_seed(d + K)
    x = torch.randn(B * S, d, generator=g)
    w = torch.randn(d, d // G, K, generator=g) / np.sqrt(d // G * K)
    bias = 0.1 * torch.randn(d, generator=g)
    lens = torch.tensor(lengths)
    keep = (torch.arange(S)[None, :] < lens[:, None]).double()[..., None]
    xm = x.view(B, S, d).double() * keep
    y = TF.conv1d(xm.transpose(1, 2), w.double(), bias.double(), padding=K // 2, groups=G)[..., :S].transpose(1, 2)
    ref = (_gelu64(y) + xm).reshape(B * S, d)
    out = F.w2v_pos_conv(x.cuda(), lens.cuda(), w.cuda(), bias.cuda(), G, B, S, bf16=bf16).cpu()
    err = (out.double() - ref).abs()
    assert err.max().item() < (5e-2 if bf16 else 1e-4)
    if bf16:
        assert err.mean().item() < 1e-2


def test_masked_mean_pool():
    B, S, d = 4, 37, 96
    x = torch.randn(B, S, d, generator=torch.Generator().manual_seed(4))
    lens = torch.tensor([37, 1, 20, 0])
    out = F.w2v_masked_mean(x.cuda(), lens.cuda()).cpu()
    for b, n in enumerate(lens.tolist()):
        ref = x[b, :n].double().mean(0) if n else torch.zeros(d, dtype=torch.float64)
        assert (out[b].double() - ref).abs().max().item() < 1e-5


# ---- module level ------------------------------------------------------------------------------------------------------------

def _run_case(name, precision):
    c, lengths = SW.CASES[name]
    wave, lens = SW.make_batch(lengths)
    m = _enc(c, precision)
    hid, ol, feat = m(wave.cuda(), lens.cuda(), return_features=True)
    feat = feat.cpu()
    pooled = m.utterance_embeddings(wave.cuda(), lens.cuda()).cpu()
    return m, hid.cpu(), ol.cpu(), feat, pooled


@pytest.mark.parametrize("name", list(SW.CASES))
def test_fp32_matches_transformers_fixture(golden_dir, name):
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    _, hid, ol, feat, pooled = _run_case(name, "fp32")
    assert ol.tolist() == fx["out_lengths"].tolist()
    n = fx["out_lengths"]
    fr = np.stack([np.stack([feat[b, 0].numpy(), feat[b, k // 2].numpy(), feat[b, k - 1].numpy()]) for b, k in enumerate(n)])
    assert np.abs(fr - fx["feat_rows"]).max() < 1e-4
    assert np.abs(hid[:, 0].numpy() - fx["hidden_first"]).max() < 1e-4
    last = np.stack([hid[b, k - 1].numpy() for b, k in enumerate(n)])
    assert np.abs(last - fx["hidden_last_valid"]).max() < 1e-4
    assert np.abs(pooled.numpy() - fx["pooled"]).max() < 1e-4


@pytest.mark.parametrize("name", list(SW.CASES))
def test_bf16_matches_transformers_fixture(golden_dir, name):
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    _, hid, ol, _, pooled = _run_case(name, "bf16")
    n = fx["out_lengths"]
    assert ol.tolist() == n.tolist()
    last = np.stack([hid[b, k - 1].numpy() for b, k in enumerate(n)])
    err = np.abs(np.concatenate([hid[:, 0].numpy() - fx["hidden_first"], last - fx["hidden_last_valid"]]))   # the sampled hidden rows
    assert err.mean() < 1e-2 and err.max() < 6e-2, (err.mean(), err.max())
    err = np.abs(pooled.numpy() - fx["pooled"])
    assert err.mean() < 1e-2 and err.max() < 6e-2, (err.mean(), err.max())
    cos = torch.nn.functional.cosine_similarity(pooled.double(), torch.from_numpy(fx["pooled"]).double(), dim=1)
    assert cos.min().item() >= 0.999


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_reruns_are_bit_identical(precision):
    c, lengths = SW.CASES["w2v_ragged"]
    wave, lens = SW.make_batch(lengths)
    m = _enc(c, precision)
    a = m(wave.cuda(), lens.cuda())[0].cpu()
    p = m.utterance_embeddings(wave.cuda(), lens.cuda()).cpu()
    b = m(wave.cuda(), lens.cuda())[0].cpu()
    q = m.utterance_embeddings(wave.cuda(), lens.cuda()).cpu()
    assert torch.equal(a, b) and torch.equal(p, q)


def test_batch_of_one_equals_the_same_utterance_in_a_padded_batch():
    """The GroupNorm statistics cover the padded axis, so the comparison pads the single utterance to the same length."""
    c, lengths = SW.CASES["w2v_ragged"]
    wave, lens = SW.make_batch(lengths)
    m = _enc(c, "fp32")
    full = m.utterance_embeddings(wave.cuda(), lens.cuda()).cpu()
    for b in range(len(lengths)):
        one = m.utterance_embeddings(wave[b: b + 1].cuda(), lens[b: b + 1].cuda()).cpu()
        assert (one - full[b: b + 1]).abs().max().item() < 1e-5
    # and the quirk is real: trimming the padding changes a short utterance's embedding
    short = m.utterance_embeddings(wave[1:2, : lengths[1]].cuda(), lens[1:2].cuda()).cpu()
    assert (short - full[1:2]).abs().max().item() > 1e-3


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_utterance_chunks_change_no_result(precision):
    """The pipeline runs `ub` utterances at a time (32-bit addressing bound); chunks of one and two utterances agree with the whole batch."""
    c, lengths = SW.CASES["w2v_ragged"]
    wave, lens = SW.make_batch(lengths)
    m = _enc(c, precision)
    full_h, full_l = m(wave.cuda(), lens.cuda())
    full_p = m.utterance_embeddings(wave.cuda(), lens.cuda())
    tol = 1e-5 if precision == "fp32" else 2e-2
    for cu in (1, 2):
        m.chunk_utterances = cu
        assert m.geometry(len(lengths), wave.shape[1])["ub"] == cu
        h, l = m(wave.cuda(), lens.cuda())
        p = m.utterance_embeddings(wave.cuda(), lens.cuda())
        assert torch.equal(l, full_l)
        for b, n in enumerate(full_l.tolist()):
            assert (h[b, :n] - full_h[b, :n]).abs().max().item() < tol
        assert (p - full_p).abs().max().item() < tol


def test_conv0_scratch_mirror_matches_library():
    from mer_amd import wav2vec2 as W
    for B, C, T0 in [(1, 32, 1), (3, 512, 31999), (64, 512, 128), (2, 64, 129)]:
        assert W.conv0_scratch_floats(B, C, T0) == runtime.lib().m2f_w2v_conv0_scratch_floats(B, C, T0)
