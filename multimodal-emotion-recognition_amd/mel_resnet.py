"""In-loop audio_mel encoder on the MI355X kernels: waveforms to 300-wide utterance embeddings.

The reference's third per-utterance feature extractor (src/feature_extractors/audio_mel) runs a torchvision ResNet18 on log-mel
spectrograms and projects its 1000 logits to 300 unit-norm features (model.py: resnet18 -> ReLU -> Linear(1000, 300) -> L2
normalise; embeddings.py runs it in eval mode).  ``MelResNetEncoder`` computes that here, front end included:

  spectrogram (fp32)     m2f_mel_frontend: y = x / max|x| over the valid samples; centred STFT (n_fft = win = 400, hop 160, periodic
                         Hann, zero padding); magnitudes; 128 Slaney mel filters over 0 .. 8 kHz with L1-normalised rows;
                         log(mel + 2.22e-16); min-max to [0, 1] over the valid frames; with ``png_levels`` the 8-bit levels
                         floor(v * 255) / 255 the reference's PNG cache returns on every read; zero rows up to 1001 frames
  stem                   m2f_mel_stem: 7x7/2 conv + BatchNorm + ReLU + 3x3/2 max pool; the image's three identical channels are
                         folded into one at pack time (the conv weights summed over input channels); fp32 in both modes
  layer1 .. layer4       m2f_mel_conv: implicit-GEMM NHWC convolution, BatchNorm folded into the weights and a bias, epilogue
                         residual + ReLU; bf16 operands / fp32 accumulation in bf16 mode, exact fp32 MFMA in fp32 mode
  head                   m2f_mel_head: average pool, fc 512 -> 1000, ReLU, 1000 -> 300, L2 normalise (fp32 in both modes)

Deviation from the reference: a silent clip (peak 0) and a spectrogram with max == min divide by zero there; here both give an
all-zero image (and so the embedding of a blank spectrogram).

Nothing couples the utterances of a batch, so an utterance's embedding does not depend on its partners or on the chunking.
State-dict keys are the reference checkpoint's (``resnet18.*``, ``projector.1.*``).  Inference only; no CPU fallback.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import runtime
from .runtime import check, lib, ptr, stream_ptr

SAMPLE_RATE = 16000
N_FFT = 400
HOP = 160
N_BINS = N_FFT // 2 + 1
N_MELS = 128
F_MAX = 8000.0
MAX_SAMPLES = 160000                   # 10 s: dataset.load_wav truncates there
FRAMES = 1 + MAX_SAMPLES // HOP        # 1001 image rows
LOG_EPS = 2.220446049250313e-16        # np.finfo(float).eps
# STFT padding of the centred frames.  Zero ("constant") padding is librosa 0.9's default for melspectrogram(center=True) as far as
# this project can tell without librosa installed; the front-end kernel implements exactly this mode.
PAD_MODE = "constant"
BN_EPS = 1e-5
EMBED = 300
STAGES = ((64, 1), (128, 2), (256, 2), (512, 2))     # (channels, stride of the first block) of layer1 .. layer4
DEFAULT_CHUNK = 64                     # utterances per pass when chunk_utterances is None (bounds the workspace)
_ALIGN = 256


def frame_count(n: int) -> int:
    """Frames of a centred STFT of n samples at hop 160: 1 + n // 160."""
    return 1 + int(n) // HOP


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz, min_log_mel, logstep = 200.0 / 3, 1000.0, 15.0, math.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz, min_log_mel, logstep = 200.0 / 3, 1000.0, 15.0, math.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filters() -> np.ndarray:
    """[128, 201] float64: triangular Slaney-scale filters over 0 .. 8 kHz, each row divided by its L1 norm (librosa's norm=1;
    an all-zero row stays zero)."""
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(F_MAX), N_MELS + 2))
    fft_f = np.linspace(0.0, SAMPLE_RATE / 2, N_BINS)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    w = np.maximum(0.0, np.minimum(-ramps[:-2] / fdiff[:-1, None], ramps[2:] / fdiff[1:, None]))
    l1 = w.sum(axis=1, keepdims=True)
    return np.where(l1 > 0, w / np.where(l1 > 0, l1, 1.0), 0.0)


def stft_basis() -> np.ndarray:
    """[400, 402] float64: periodic Hann window x cos (columns 0 .. 200) and x sin (201 .. 401) of the 201 DFT bins."""
    t = np.arange(N_FFT, dtype=np.float64)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * t / N_FFT)
    ang = 2 * np.pi * np.outer(t, np.arange(N_BINS)) / N_FFT
    return np.concatenate([win[:, None] * np.cos(ang), win[:, None] * np.sin(ang)], axis=1)


def fold_bn(w: torch.Tensor, bn: dict, eps: float = BN_EPS):
    """conv weight [Cout, ...] and eval BatchNorm -> (w * scale[o], shift), in the dtype of w (float64 in the tests)."""
    scale = bn["weight"].to(w.dtype) / torch.sqrt(bn["running_var"].to(w.dtype) + eps)
    shift = bn["bias"].to(w.dtype) - bn["running_mean"].to(w.dtype) * scale
    return w * scale.view(-1, *([1] * (w.dim() - 1))), shift


def fold_stem(w: torch.Tensor, bn: dict) -> tuple:
    """conv1 [64, 3, 7, 7] + bn1 -> ([49, 64] tap-major weights of one input channel, bias [64]): the three channels of the image are
    identical, so summing the weights over input channels computes the same convolution."""
    wf, b = fold_bn(w.sum(dim=1), bn)
    return wf.permute(1, 2, 0).reshape(49, w.shape[0]).contiguous(), b


def pack_conv(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, k, k] -> [Cout, k * k * Cin] (tap-major, channel-minor: a channels-last window's order)."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def block_names():
    """(layer, block, Cin, Cout, stride, has_downsample) of ResNet18's eight basic blocks."""
    out, cin = [], 64
    for li, (c, s) in enumerate(STAGES, start=1):
        for bi in range(2):
            st = s if bi == 0 else 1
            out.append((li, bi, cin, c, st, bi == 0 and (st != 1 or cin != c)))
            cin = c
    return out


def strip_checkpoint(state_dict) -> dict:
    """The reference checkpoint ({"model_state_dict": ...}) or a bare state_dict -> the state_dict without BatchNorm's
    num_batches_tracked (unused in eval mode)."""
    if isinstance(state_dict, dict) and "model_state_dict" in state_dict and not any(k.startswith("resnet18.") for k in state_dict):
        state_dict = state_dict["model_state_dict"]
    return {k: v for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}


# ---- kernel wrappers (the encoder's steps one at a time; the tests drive them) -------------------------------------------------------

def _l32(lengths, dev):
    return lengths.to(dev, torch.int32).contiguous()


def frontend(waveforms: torch.Tensor, lengths: torch.Tensor, png_levels: bool = True, out: Optional[torch.Tensor] = None,
             scratch: Optional[torch.Tensor] = None, consts=None) -> torch.Tensor:
    """waveforms [B, N] fp32 (padded), lengths [B] -> the stem's input image [B, 1001, 128] fp32."""
    runtime.require_gpu()
    B, N = waveforms.shape
    dev = waveforms.device
    basis, fbT = consts if consts is not None else _frontend_consts(dev)
    if out is None:
        out = torch.empty(B, FRAMES, N_MELS, dtype=torch.float32, device=dev)
    if scratch is None:
        scratch = torch.empty(int(lib().m2f_mel_frontend_scratch_floats(B)), dtype=torch.float32, device=dev)
    l32 = _l32(lengths, dev)
    check(lib().m2f_mel_frontend(B, N, ptr(waveforms.contiguous()), ptr(l32), ptr(basis), ptr(fbT), int(png_levels), ptr(scratch),
                                 ptr(out), stream_ptr()), "m2f_mel_frontend")
    return out


def _frontend_consts(dev):
    basis = torch.from_numpy(stft_basis()).float().to(dev).contiguous()
    fbT = torch.from_numpy(mel_filters().T.copy()).float().to(dev).contiguous()
    return basis, fbT


def stem(img: torch.Tensor, w49: torch.Tensor, bias: torch.Tensor, bf16_out: bool = False) -> torch.Tensor:
    """img [B, 1001, 128] fp32 -> max pool(ReLU(conv7x7/2(img, w49) + bias)): [B, 251, 32, 64] NHWC (bf16 when bf16_out)."""
    runtime.require_gpu()
    B = img.shape[0]
    out = torch.empty(B, 251, 32, 64, dtype=torch.bfloat16 if bf16_out else torch.float32, device=img.device)
    check(lib().m2f_mel_stem(B, ptr(img.contiguous()), ptr(w49.float().contiguous()), ptr(bias.float().contiguous()),
                             None if bf16_out else ptr(out), ptr(out) if bf16_out else None, stream_ptr()), "m2f_mel_stem")
    return out


def conv(x: torch.Tensor, wpk: torch.Tensor, bias: torch.Tensor, ks: int, stride: int, res: Optional[torch.Tensor] = None,
         relu: bool = True, out_fp32: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B, H, W, Cin] (bf16: bf16 mode, else fp32), wpk [Cout, ks * ks * Cin] (pack_conv; same dtype as x), pad ks // 2 ->
    act(conv + bias (+ res)) [B, Ho, Wo, Cout], bf16 in bf16 mode unless out_fp32."""
    runtime.require_gpu()
    B, H, W, Cin = x.shape
    Cout = wpk.shape[0]
    bf16 = x.dtype == torch.bfloat16
    assert wpk.dtype == x.dtype and (res is None or res.dtype == x.dtype)
    pad = ks // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    if out is None:
        out = torch.empty(B, Ho, Wo, Cout, dtype=torch.bfloat16 if bf16 and not out_fp32 else torch.float32, device=x.device)
    check(lib().m2f_mel_conv(B, H, W, Cin, Cout, ks, stride, ptr(x.contiguous()), ptr(wpk.contiguous()), ptr(bias.float().contiguous()),
                             ptr(res.contiguous()) if res is not None else None, ptr(out), int(bf16), int(out_fp32), int(relu),
                             stream_ptr()), "m2f_mel_conv")
    return out


def head(x: torch.Tensor, w1t: torch.Tensor, b1: torch.Tensor, w2t: torch.Tensor, b2: torch.Tensor,
         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B, HW, C] (fp32 or bf16) -> L2-normalised (ReLU(mean(x) W1^T + b1) W2^T + b2): [B, N2]."""
    runtime.require_gpu()
    B, HW, C = x.shape
    N1, N2 = w1t.shape[1], w2t.shape[1]
    if out is None:
        out = torch.empty(B, N2, dtype=torch.float32, device=x.device)
    check(lib().m2f_mel_head(B, HW, C, ptr(x.contiguous()), int(x.dtype == torch.bfloat16), ptr(w1t), ptr(b1), N1, ptr(w2t), ptr(b2), N2,
                             ptr(out), stream_ptr()), "m2f_mel_head")
    return out


# ---- the module ----------------------------------------------------------------------------------------------------------------------

class _BN(torch.nn.Module):
    """BatchNorm2d's eval-mode state (num_batches_tracked is not kept: eval mode never reads it)."""

    def __init__(self, c: int):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(c))
        self.bias = torch.nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))

    def params(self) -> dict:
        return {"weight": self.weight.detach(), "bias": self.bias.detach(), "running_mean": self.running_mean,
                "running_var": self.running_var}


def _conv_param(cout, cin, k):
    return torch.nn.Parameter(torch.zeros(cout, cin, k, k))


class MelResNetEncoder(torch.nn.Module):
    def __init__(self, precision: str = "bf16", png_levels: bool = True, chunk_utterances: Optional[int] = None):
        """precision: "bf16" (bf16 operands, fp32 accumulation in the convolutions) or "fp32".  png_levels: the 8-bit levels of the
        reference's PNG cache (what its embedding dump reads), False for the cache-miss values.  chunk_utterances: at most this many
        utterances per pass (None: DEFAULT_CHUNK); the chunking changes no result."""
        super().__init__()
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"precision {precision!r}: 'bf16' or 'fp32'")
        self.precision = runtime.F32 if precision == "fp32" else runtime.BF16
        self.png_levels = bool(png_levels)
        self.chunk_utterances = chunk_utterances
        r = self.resnet18 = torch.nn.Module()
        r.conv1 = torch.nn.Module()
        r.conv1.weight = _conv_param(64, 3, 7)
        r.bn1 = _BN(64)
        for li, bi, cin, cout, st, ds in block_names():
            if bi == 0:
                setattr(r, f"layer{li}", torch.nn.ModuleList())
            blk = torch.nn.Module()
            blk.conv1 = torch.nn.Module()
            blk.conv1.weight = _conv_param(cout, cin, 3)
            blk.bn1 = _BN(cout)
            blk.conv2 = torch.nn.Module()
            blk.conv2.weight = _conv_param(cout, cout, 3)
            blk.bn2 = _BN(cout)
            if ds:
                blk.downsample = torch.nn.ModuleList([torch.nn.Module(), _BN(cout)])
                blk.downsample[0].weight = _conv_param(cout, cin, 1)
            getattr(r, f"layer{li}").append(blk)
        r.fc = torch.nn.Linear(512, 1000)
        self.projector = torch.nn.ModuleList([torch.nn.ReLU(), torch.nn.Linear(1000, EMBED)])
        self._packed = None
        self._packed_versions = None
        self._ws = None              # one byte buffer, grown to the largest chunk seen
        self._ws_bytes = 0

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """The reference checkpoint ({"model_state_dict": ...}) or a bare state_dict in its key layout; strict by default."""
        out = super().load_state_dict(strip_checkpoint(state_dict), strict=strict, **kw)
        self._packed = None
        return out

    # ---- packed weights ---------------------------------------------------------------------------------------------
    def _versions(self):
        return tuple(p._version for p in self.parameters()) + tuple(b._version for b in self.buffers())

    def _pack(self):
        dev = self.resnet18.fc.weight.device
        if dev.type != "cuda":
            raise runtime.HipError("MelResNetEncoder runs on an MI355X only (move it with .to('cuda')): no CPU fallback")
        bf16 = self.precision == runtime.BF16
        r = self.resnet18

        def cw(w, bn):
            wf, b = fold_bn(w.detach().double(), bn.params())
            p = pack_conv(wf).float()
            return (p.to(torch.bfloat16).contiguous() if bf16 else p.contiguous()), b.float().contiguous()

        w49, b0 = fold_stem(r.conv1.weight.detach().double(), {k: v.double() for k, v in r.bn1.params().items()})
        P = {"stem_w": w49.float().contiguous(), "stem_b": b0.float().contiguous(), "blocks": []}
        for li, bi, cin, cout, st, ds in block_names():
            blk = getattr(r, f"layer{li}")[bi]
            e = {"cin": cin, "cout": cout, "stride": st}
            e["w1"], e["b1"] = cw(blk.conv1.weight, blk.bn1)
            e["w2"], e["b2"] = cw(blk.conv2.weight, blk.bn2)
            if ds:
                e["wd"], e["bd"] = cw(blk.downsample[0].weight, blk.downsample[1])
            P["blocks"].append(e)
        P["w1t"] = r.fc.weight.detach().float().t().contiguous()
        P["fb1"] = r.fc.bias.detach().float().contiguous()
        P["w2t"] = self.projector[1].weight.detach().float().t().contiguous()
        P["fb2"] = self.projector[1].bias.detach().float().contiguous()
        P["consts"] = _frontend_consts(dev)
        self._packed = P
        self._packed_versions = self._versions()

    def _ready(self):
        runtime.require_gpu()
        if self._packed is None or self._packed_versions != self._versions():
            self._pack()
        return self._packed

    # ---- workspace ----------------------------------------------------------------------------------------------------
    def chunk(self, B: int) -> int:
        return max(1, min(B, int(self.chunk_utterances) if self.chunk_utterances else DEFAULT_CHUNK))

    def workspace_layout(self, ub: int) -> dict:
        """Byte offsets of the regions of a chunk of ub utterances: the image, the front end's scratch, and four activation buffers
        as large as layer1's output (bf16 in bf16 mode)."""
        esz = 2 if self.precision == runtime.BF16 else 4
        act = ub * 251 * 32 * 64 * esz
        names = [("img", ub * FRAMES * N_MELS * 4), ("scratch", (ub + 63) // 64 * 64 * 4 + ub * FRAMES * N_MELS * 4),
                 ("a", act), ("b", act), ("c", act), ("d", act)]
        off, o = {}, 0
        for n, sz in names:
            off[n] = o
            o += (sz + _ALIGN - 1) // _ALIGN * _ALIGN
        return {"off": off, "bytes": o}

    def workspace_bytes(self, B: int) -> int:
        return self.workspace_layout(self.chunk(B))["bytes"]

    def _workspace(self, nbytes: int, dev):
        if self._ws is None or self._ws.device != dev or nbytes > self._ws_bytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self._ws_bytes = nbytes
        return self._ws

    # ---- forward ----------------------------------------------------------------------------------------------------
    def _backbone(self, img: torch.Tensor, ws: torch.Tensor, lay: dict, out: torch.Tensor):
        """img [nb, 1001, 128] fp32 (a view) -> out [nb, 300]; activations in the workspace's buffers a .. d."""
        P = self._packed
        nb = img.shape[0]
        bf16 = self.precision == runtime.BF16
        dt = torch.bfloat16 if bf16 else torch.float32
        esz = 2 if bf16 else 4

        def buf(name, H, W, C):
            o = lay["off"][name]
            return ws[o: o + nb * H * W * C * esz].view(dt).view(nb, H, W, C)

        x = buf("a", 251, 32, 64)
        check(lib().m2f_mel_stem(nb, ptr(img), ptr(P["stem_w"]), ptr(P["stem_b"]), None if bf16 else ptr(x), ptr(x) if bf16 else None,
                                 stream_ptr()), "m2f_mel_stem")
        H, W = 251, 32
        free = ["b", "c", "d"]
        cur = "a"
        for e in P["blocks"]:
            s, cout = e["stride"], e["cout"]
            Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
            t_name, o_name = free[0], free[1]
            t = conv(x, e["w1"], e["b1"], 3, s, relu=True, out=buf(t_name, Ho, Wo, cout))
            res = x
            if "wd" in e:
                res = conv(x, e["wd"], e["bd"], 1, s, relu=False, out=buf(free[2], Ho, Wo, cout))
            y = conv(t, e["w2"], e["b2"], 3, 1, res=res, relu=True, out=buf(o_name, Ho, Wo, cout))
            free = [cur, t_name, free[2]]
            cur, x, H, W = o_name, y, Ho, Wo
        head(x.view(nb, H * W, x.shape[-1]), P["w1t"], P["fb1"], P["w2t"], P["fb2"], out=out)

    @torch.no_grad()
    def spectrogram(self, waveforms: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        """waveforms [B, N] fp32 (zero-padded), lengths [B] sample counts (<= 160,000) -> [B, 1001, 128] fp32: the normalised
        log-mel image (8-bit levels / 255 with png_levels), zero rows behind frame lengths // 160."""
        P = self._ready()
        dev = self.resnet18.fc.weight.device
        wave, lengths = self._inputs(waveforms, lengths, dev)
        return frontend(wave, lengths, self.png_levels, consts=P["consts"])

    def _inputs(self, waveforms, lengths, dev):
        if waveforms.dim() != 2:
            raise ValueError("waveforms: [B, N]")
        if lengths.shape != (waveforms.shape[0],):
            raise ValueError("lengths: [B]")
        if int(lengths.max()) > min(MAX_SAMPLES, waveforms.shape[1]) or int(lengths.min()) < 0:
            raise ValueError(f"lengths: 0 .. min(N, {MAX_SAMPLES}) samples (dataset.load_wav truncates at 10 s)")
        return waveforms.to(dev, torch.float32).contiguous(), lengths.to(dev, torch.int32).contiguous()

    @torch.no_grad()
    def embed(self, spectrograms: torch.Tensor) -> torch.Tensor:
        """spectrograms [B, 1001, 128] (one channel of the reference's [B, 3, 1001, 128] image) -> [B, 300] unit rows."""
        P = self._ready()
        dev = self.resnet18.fc.weight.device
        if spectrograms.dim() != 3 or tuple(spectrograms.shape[1:]) != (FRAMES, N_MELS):
            raise ValueError(f"spectrograms: [B, {FRAMES}, {N_MELS}]")
        img = spectrograms.to(dev, torch.float32).contiguous()
        B = img.shape[0]
        ub = self.chunk(B)
        lay = self.workspace_layout(ub)
        ws = self._workspace(lay["bytes"], dev)
        out = torch.empty(B, EMBED, dtype=torch.float32, device=dev)
        for b0 in range(0, B, ub):
            nb = min(ub, B - b0)
            self._backbone(img[b0: b0 + nb], ws, lay, out[b0: b0 + nb])
        return out

    @torch.no_grad()
    def utterance_embeddings(self, waveforms: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        """waveforms [B, N] fp32 (zero-padded), lengths [B] -> [B, 300]: the reference's audio_mel embedding of each utterance."""
        P = self._ready()
        dev = self.resnet18.fc.weight.device
        wave, l32 = self._inputs(waveforms, lengths, dev)
        B, N = wave.shape
        ub = self.chunk(B)
        lay = self.workspace_layout(ub)
        ws = self._workspace(lay["bytes"], dev)
        out = torch.empty(B, EMBED, dtype=torch.float32, device=dev)
        o_img, o_scr = lay["off"]["img"], lay["off"]["scratch"]
        for b0 in range(0, B, ub):
            nb = min(ub, B - b0)
            img = ws[o_img: o_img + nb * FRAMES * N_MELS * 4].view(torch.float32).view(nb, FRAMES, N_MELS)
            scr = ws[o_scr: o_scr + int(lib().m2f_mel_frontend_scratch_floats(nb)) * 4].view(torch.float32)
            frontend(wave[b0: b0 + nb], l32[b0: b0 + nb], self.png_levels, out=img, scratch=scr, consts=P["consts"])
            self._backbone(img, ws, lay, out[b0: b0 + nb])
        return out

    def forward(self, waveforms: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        return self.utterance_embeddings(waveforms, lengths)
