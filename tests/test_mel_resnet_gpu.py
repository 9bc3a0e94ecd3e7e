"""GPU tests of the audio_mel encoder (mer_amd.mel_resnet, csrc/mel_resnet.hip) against the float64 oracle
(tests/golden/mel_resnet_oracle.py): the front end, every ResNet18 convolution shape on its own, the end-to-end embedding in fp32 and
bf16, batch independence, and the encoder as the training loop's audio source."""
import os
import sys

import numpy as np
import pandas as pd
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mel_resnet_oracle as O  # noqa: E402
import synth  # noqa: E402
import synth_mel_resnet as S  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import mel_resnet as MR  # noqa: E402

DEV = torch.device("cuda:0")
FRONT_TOL = 2e-5            # unquantised image values, max abs (values in [0, 1]; measured 9.0e-6)
FP32_TOL = 1e-4             # unit-norm embedding rows, fp32 mode, max abs (measured 3.4e-7 on identical images)
BF16_TOL = 5e-3             # unit-norm embedding rows, bf16 mode, max abs (measured 2.35e-3, about 2x margin)


@pytest.fixture(scope="module")
def sd():
    return S.make_state_dict(0)


@pytest.fixture(scope="module")
def wav():
    return S.batch()


def _enc(sd, precision, **kw):
    e = MR.MelResNetEncoder(precision=precision, **kw)
    e.load_state_dict(sd)
    return e.to(DEV).eval()


def test_front_end_against_the_oracle(wav):
    w, l = wav
    g = MR.frontend(w.to(DEV), l.to(DEV), png_levels=False).cpu().double().numpy()
    gq = MR.frontend(w.to(DEV), l.to(DEV), png_levels=True).cpu().double().numpy()
    worst = 0.0
    for i in range(len(l)):
        ref, scaled = O.spectrogram(w[i].numpy(), int(l[i]), png_levels=False, return_scaled=True)
        worst = max(worst, np.abs(g[i] - ref).max())
        f = MR.frame_count(int(l[i]))
        lv = np.round(gq[i] * 255)
        assert not lv[f:].any() and not g[i][f:].any()
        want = np.floor(scaled.astype(np.float64))
        diff = lv[:f] - want
        assert np.abs(diff).max() <= 1
        # a level may differ only where the oracle's v * 255 lies within 255 * FRONT_TOL of an integer
        near = np.abs(scaled - np.round(scaled)) <= 255 * FRONT_TOL
        assert not (diff != 0)[~near].any()
    print(f"front end: max abs {worst:.2e}")
    assert worst < FRONT_TOL


def _conv_ref(x, w, b, ks, s, res, relu):
    y = TF.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), stride=s, padding=ks // 2).permute(0, 2, 3, 1)
    if res is not None:
        y = y + res.double()
    return y.clamp_min(0) if relu else y


# every convolution of ResNet18's four stages: (B, H, W, Cin, Cout, ks, stride).  Layer4's 32 x 4 outputs fill whole 128-row tiles
# at any batch, so those forms also run on a shorter image (61 or 31 rows) whose M is not a tile multiple.
CONVS = [(1, 251, 32, 64, 64, 3, 1), (2, 251, 32, 64, 128, 3, 2), (2, 251, 32, 64, 128, 1, 2), (1, 126, 16, 128, 128, 3, 1),
         (3, 126, 16, 128, 256, 3, 2), (3, 126, 16, 128, 256, 1, 2), (3, 63, 8, 256, 256, 3, 1), (3, 63, 8, 256, 512, 3, 2),
         (3, 63, 8, 256, 512, 1, 2), (1, 32, 4, 512, 512, 3, 1), (3, 61, 8, 256, 512, 3, 2), (3, 61, 8, 256, 512, 1, 2),
         (3, 31, 4, 512, 512, 3, 1)]


@pytest.mark.parametrize("shape", CONVS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_conv_shape_against_float64(shape, bf16, with_res):
    B, H, W, Cin, Cout, ks, s = shape
    g = torch.Generator().manual_seed(H * Cin + ks + s)
    x = torch.rand(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / np.sqrt(Cin * ks * ks)
    b = 0.1 * torch.randn(Cout, generator=g)
    Ho, Wo = (H + 2 * (ks // 2) - ks) // s + 1, (W + 2 * (ks // 2) - ks) // s + 1
    assert (B * Ho * Wo) % 128 or Ho == 32
    res = torch.randn(B, Ho, Wo, Cout, generator=g) if with_res else None
    dt = torch.bfloat16 if bf16 else torch.float32
    xq, wq = x.to(dt), w.to(dt)
    rq = res.to(dt) if with_res else None
    ref = _conv_ref(xq.float(), wq.float(), b, ks, s, rq.float() if with_res else None, True)
    out = MR.conv(xq.to(DEV), MR.pack_conv(wq).to(DEV), b.to(DEV), ks, s, res=rq.to(DEV) if with_res else None, relu=True,
                  out_fp32=True).cpu()
    scale = ref.abs().max().item()
    assert out.shape == ref.shape
    assert (out.double() - ref).abs().max().item() < 2e-6 * scale * np.sqrt(Cin * ks * ks)
    assert (out[-1, -1, -1].double() - ref[-1, -1, -1]).abs().max().item() < 1e-4 * scale        # last row of the last tile
    if bf16:                                                      # the bf16 output is the rounded fp32 result
        o16 = MR.conv(xq.to(DEV), MR.pack_conv(wq).to(DEV), b.to(DEV), ks, s, res=rq.to(DEV) if with_res else None).cpu()
        assert o16.dtype == torch.bfloat16 and (o16.double() - ref).abs().max().item() <= 8e-3 * scale
    no_relu = MR.conv(xq.to(DEV), MR.pack_conv(wq).to(DEV), b.to(DEV), ks, s, relu=False, out_fp32=True).cpu()
    assert (no_relu.double() - _conv_ref(xq.float(), wq.float(), b, ks, s, None, False)).abs().max().item() < 1e-4 * scale
    assert (no_relu < 0).any()


@pytest.mark.parametrize("bf16", [False, True])
def test_stem_against_float64(sd, wav, bf16):
    w, l = wav
    img = torch.from_numpy(np.stack([O.spectrogram(w[i].numpy(), int(l[i])) for i in (0, 1)])).float()
    bn = {s: sd[f"resnet18.bn1.{s}"].double() for s in ("weight", "bias", "running_mean", "running_var")}
    w49, b0 = MR.fold_stem(sd["resnet18.conv1.weight"].double(), bn)
    x = img.double()[:, None]
    ref = TF.max_pool2d(TF.relu(TF.conv2d(x, w49.t().reshape(64, 1, 7, 7), b0, stride=2, padding=3)), 3, 2, 1).permute(0, 2, 3, 1)
    out = MR.stem(img.to(DEV), w49.float().to(DEV), b0.float().to(DEV), bf16_out=bf16).cpu().double()
    scale = ref.abs().max().item()
    assert out.shape == (2, 251, 32, 64)
    assert (out - ref).abs().max().item() < (8e-3 if bf16 else 1e-5) * scale


def test_head_against_float64(sd):
    g = torch.Generator().manual_seed(5)
    x = torch.rand(11, 128, 512, generator=g)
    ref = O.head(x.double().mean(dim=1), sd)
    w1t, w2t = sd["resnet18.fc.weight"].t().contiguous(), sd["projector.1.weight"].t().contiguous()
    out = MR.head(x.to(DEV), w1t.to(DEV), sd["resnet18.fc.bias"].to(DEV), w2t.to(DEV), sd["projector.1.bias"].to(DEV)).cpu()
    assert (out.double() - ref).abs().max().item() < 1e-5


@pytest.mark.parametrize("precision,tol", [("fp32", FP32_TOL), ("bf16", BF16_TOL)])
def test_end_to_end_on_identical_spectrograms(sd, wav, precision, tol):
    w, l = wav
    idx = [0, 1, 5]
    img = np.stack([O.spectrogram(w[i].numpy(), int(l[i])) for i in idx])
    ref = O.embed(img, sd)
    out = _enc(sd, precision).embed(torch.from_numpy(img).float()).cpu().double()
    err = (out - ref).abs().max().item()
    print(f"{precision} embedding: max abs {err:.2e}")
    assert err < tol
    assert (out.norm(dim=1) - 1).abs().max().item() < 1e-5


def test_waveform_to_embedding_fp32(sd, wav):
    w, l = wav
    idx = [0, 2, 3, 6]
    ws, ls = w[idx][:, : int(l[idx].max())], l[idx]
    ref = O.utterance_embeddings(ws.numpy(), ls.numpy(), sd, png_levels=False)
    enc = _enc(sd, "fp32", png_levels=False)
    out = enc.utterance_embeddings(ws.to(DEV), ls.to(DEV)).cpu().double()
    assert (out - ref).abs().max().item() < FP32_TOL
    # with levels: the oracle fed the GPU's levels (a level can legitimately differ where v * 255 sits on an integer)
    encq = _enc(sd, "fp32")
    spec = encq.spectrogram(ws.to(DEV), ls.to(DEV)).cpu().double().numpy()
    assert np.abs(np.round(spec * 255) - spec * 255).max() < 1e-4
    outq = encq.utterance_embeddings(ws.to(DEV), ls.to(DEV)).cpu().double()
    assert (outq - O.embed(spec, sd)).abs().max().item() < FP32_TOL


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_batch_independence_and_repeatability(sd, wav, precision):
    w, l = wav
    enc = _enc(sd, precision)
    all8 = enc.utterance_embeddings(w.to(DEV), l.to(DEV))
    again = enc.utterance_embeddings(w.to(DEV), l.to(DEV))
    assert torch.equal(all8, again)
    for i in (0, 3, 7):
        alone = enc.utterance_embeddings(w[i: i + 1, : int(l[i])].to(DEV), l[i: i + 1].to(DEV))
        assert torch.equal(alone[0], all8[i])
    chunked = _enc(sd, precision, chunk_utterances=2).utterance_embeddings(w.to(DEV), l.to(DEV))
    assert torch.equal(chunked, all8)


def test_silent_clip_gives_a_finite_unit_row(sd):
    enc = _enc(sd, "bf16")
    w = torch.zeros(2, 16000)
    w[1] = torch.from_numpy(S.speech_like(16000, 9))
    out = enc.utterance_embeddings(w.to(DEV), torch.tensor([16000, 16000]).to(DEV)).cpu()
    assert torch.isfinite(out).all() and abs(out[0].norm().item() - 1) < 1e-5
    assert not enc.spectrogram(w.to(DEV), torch.tensor([16000, 16000]).to(DEV))[0].any()
    ref = O.embed(np.zeros((1, 1001, 128)), sd)
    assert (out[0].double() - ref[0]).abs().max().item() < BF16_TOL


def test_reference_checkpoint_dict_loads(sd, wav):
    w, l = wav
    a = MR.MelResNetEncoder(precision="fp32")
    a.load_state_dict({"model_state_dict": sd, "epoch": 7, "optimizer_state_dict": {}})
    a = a.to(DEV).eval()
    b = _enc({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}, "fp32")
    assert torch.equal(a.utterance_embeddings(w[:2].to(DEV), l[:2].to(DEV)), b.utterance_embeddings(w[:2].to(DEV), l[:2].to(DEV)))


def test_wav_files_through_the_mel_encoder_into_a_tiny_m2fnet(tmp_path, sd):
    import dataset as ds
    import train as tr
    from metrics import move_batch
    from test_audio_encoder_dropin_cpu import write_wav
    g = np.random.default_rng(0)
    rows = []
    for d in range(4):
        for u in range(int(g.integers(1, 4))):
            rows.append((f"utt {d}-{u}", list(ds.EMOTIONS)[int(g.integers(0, 2))], d, u))
    table = pd.DataFrame(rows, columns=["Utterance", "Emotion", "Dialogue_ID", "Utterance_ID"])
    for i, (d, u) in enumerate(zip(table["Dialogue_ID"], table["Utterance_ID"])):
        write_wav(os.path.join(tmp_path, f"dia{d}_utt{u}.wav"), S.speech_like(int(g.integers(4000, 30000)), i))
    text = torch.from_numpy(g.standard_normal((len(rows), 64)).astype(np.float32))
    dset = ds.Dataset("train", text_embeddings=text, table=table, waveforms=ds.load_waveforms(table, str(tmp_path)))
    batch = ds.collate_fn([dset[i] for i in range(len(dset))])
    enc = tr.build_audio_encoder({"model": "mel_resnet18", "precision": "fp32"}, 300, DEV, n_head=4)
    assert isinstance(enc, MR.MelResNetEncoder)
    enc.load_state_dict(sd)
    text, audio, emotion, mask = move_batch(batch, DEV, audio_encoder=enc)
    B, L = mask.shape
    assert audio.shape == (B, L, 300)
    direct = enc.utterance_embeddings(batch["waveforms"].to(DEV), batch["wave_lengths"].to(DEV))
    assert torch.equal(audio[~mask], direct)
    assert torch.count_nonzero(audio[mask]) == 0
    cfg = synth._cfg(300, 64, 64, 4, 4, 4, 1, 1, 1)
    model = tr.M2FNet(cfg)
    model.load_state_dict(synth.make_state_dict(cfg))
    model = model.to(DEV).train()
    loss = model.train_step(text, audio, mask, emotion, use_graph=False)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and loss.item() > 0
