"""In-loop audio feature extractor on the MI355X kernels: waveforms to utterance embeddings.

The reference makes its audio embeddings in a separate stage (src/feature_extractors/audio_wav2vec2/embeddings.py:52-91):
torchaudio's ``WAV2VEC2_BASE.get_model()`` runs on batches of 16 zero-padded 16 kHz waveforms with their sample counts, and the
embedding of an utterance is the mean of its valid output frames.  ``Wav2Vec2Encoder`` runs that model's eval-mode forward here:

  conv layer 0 + GroupNorm + GELU      m2f_w2v_conv0 (statistics over the PADDED batch's frames, as the reference: a short
                                       utterance's embedding depends on the longest waveform of its batch)
  conv layers 1..6 + GELU              the grouped GEMM on overlapping channels-last windows (no im2col copy, see below)
  feature LayerNorm + projection       m2f_w2v_feat_layernorm (pitched rows -> compact rows) + GEMM
  positional conv + GELU + residual    m2f_w2v_pos_conv (MFMA implicit GEMM; weight norm folded at pack time)
  encoder LayerNorm, post-LN layers    the kernels RoBERTa's encoder runs (packed Q/K/V GEMM, long-sequence attention with key
                                       mask, GEMM epilogues for bias / residual / exact GELU, LayerNorm)
  mean over valid frames               m2f_w2v_masked_mean

Conv stack rows.  Utterance b's frames of conv layer l live at rows b * P_l + t, with pitches P_{l-1} = s_l * P_l.  Output frame t of
layer l then reads the k_l consecutive rows from b * P_{l-1} + s_l * t on: with the activation viewed as a matrix of leading
dimension s_l * C, that window is the first s_l * C elements of row b * P_l + t plus the first (k_l - s_l) * C elements of the row
after it.  The GEMM takes those as its two k-segments (A0 = activation, A1 = activation + s_l * C, both with leading dimension
s_l * C), so every segment is no wider than its leading dimension and the bf16 launches stage from the shadows.  Rows t >= T_l of
a pitch hold junk that no valid window reads; windows never straddle two utterances.

State-dict keys are transformers' ``Wav2Vec2Model`` keys.  ``load_state_dict`` also takes torchaudio's layout (the AudioERC
checkpoints of the reference hold it through ``extract_wav2vec2_state_dict``).  Inference only; no CPU fallback.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import runtime
from .runtime import check, lib, ptr, stream_ptr

NT = 0
_ALIGN = 64
_ELEMS_MAX = 1 << 30             # per matrix of a launch: the GEMM kernels address their operands with 32-bit (byte) offsets
CONV0_CHUNK = 128                # frames per statistics chunk of m2f_w2v_conv0 (csrc/audio_conv.hip, CONV0_FCH)


def conv0_scratch_floats(B: int, C: int, T0: int) -> int:
    """Python mirror of m2f_w2v_conv0_scratch_floats: (mean, M2) per (utterance, chunk, channel) + (mean, rstd) per (utterance, channel)."""
    return 0 if B < 1 or C < 1 or T0 < 1 else 2 * B * C * (-(-T0 // CONV0_CHUNK) + 1)


def _get(cfg, name, default=None):
    if isinstance(cfg, dict):
        return cfg.get(name, default)
    return getattr(cfg, name, default)


def _al(n: int) -> int:
    return (n + _ALIGN - 1) // _ALIGN * _ALIGN


def output_length(n: int, kernels, strides) -> int:
    """Frames after the conv stack for n samples: floor((n - k) / s) + 1 per layer (torchaudio / transformers)."""
    for k, s in zip(kernels, strides):
        n = (n - k) // s + 1
    return n


def _rename(state_dict) -> dict:
    """transformers or torchaudio keys -> this module's keys.

    transformers (``Wav2Vec2Model.state_dict()``): taken as they are; the weight-normed positional conv comes as
    ``parametrizations.weight.original0/1`` (or ``weight_g`` / ``weight_v`` from older releases); ``masked_spec_embed`` (training-time
    masking) is ignored.  torchaudio (``wav2vec2_model(...).state_dict()``): ``encoder.transformer.*`` -> ``encoder.*`` and
    ``encoder.feature_projection.*`` -> ``feature_projection.*``; the remaining names coincide.  That table is written from
    torchaudio's module structure (components.py) and is not pinned by a test against torchaudio itself, which this project cannot
    install."""
    out = {}
    for k, v in state_dict.items():
        if k == "masked_spec_embed" or k.endswith("position_ids"):
            continue
        if k.startswith("encoder.transformer."):
            k = "encoder." + k[len("encoder.transformer."):]
        elif k.startswith("encoder.feature_projection."):
            k = k[len("encoder."):]
        k = k.replace("pos_conv_embed.conv.parametrizations.weight.original0", "pos_conv_embed.conv.weight_g")
        k = k.replace("pos_conv_embed.conv.parametrizations.weight.original1", "pos_conv_embed.conv.weight_v")
        out[k] = v
    return out


def to_torchaudio_keys(state_dict) -> dict:
    """This module's (or transformers') keys -> torchaudio's layout (the inverse of the rename ``load_state_dict`` applies)."""
    out = {}
    for k, v in _rename(state_dict).items():
        if k.startswith("feature_projection."):
            k = "encoder." + k
        elif k.startswith("encoder."):
            k = "encoder.transformer." + k[len("encoder."):]
        out[k] = v
    return out


class Wav2Vec2Encoder(torch.nn.Module):
    def __init__(self, config, precision: str = "bf16", chunk_utterances: Optional[int] = None):
        """chunk_utterances: at most this many utterances per pass through the pipeline (bounds the workspace; None: only the
        32-bit addressing bound of `geometry`)."""
        super().__init__()
        self.chunk_utterances = chunk_utterances
        if _get(config, "conv_bias", False):
            raise NotImplementedError("conv_bias=True: the wav2vec2-base front end has bias-free convolutions; only that is implemented")
        if _get(config, "do_stable_layer_norm", False) or _get(config, "feat_extract_norm", "group") != "group":
            raise NotImplementedError("layer-norm-first wav2vec2 (large / lv60: do_stable_layer_norm, feat_extract_norm='layer') "
                                      "is not implemented; only the base architecture")
        for name in ("hidden_act", "feat_extract_activation"):
            if _get(config, name, "gelu") != "gelu":
                raise NotImplementedError(f"{name}={_get(config, name)!r}: only the exact 'gelu' is implemented")
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"precision {precision!r}: 'bf16' or 'fp32'")
        dims = list(_get(config, "conv_dim", (512,) * 7))
        self.kernels = [int(k) for k in _get(config, "conv_kernel", (10, 3, 3, 3, 3, 2, 2))]
        self.strides = [int(s) for s in _get(config, "conv_stride", (5, 2, 2, 2, 2, 2, 2))]
        if len(set(dims)) != 1 or len(dims) != len(self.kernels) or len(dims) != len(self.strides) or len(dims) < 2:
            raise NotImplementedError("conv feature encoder: equal widths in every layer, at least two layers")
        self.C = C = int(dims[0])
        if self.kernels[0] > 16 or self.strides[0] > 8:
            raise NotImplementedError("conv layer 0: kernel <= 16, stride <= 8")
        for k, s in zip(self.kernels[1:], self.strides[1:]):
            if not s <= k <= 2 * s:
                raise NotImplementedError("conv layers 1..: stride <= kernel <= 2 * stride (two GEMM k-segments per window)")
        if C % 8 or C > 1024:
            raise NotImplementedError("conv_dim: a multiple of 8, at most 1024")
        self.d = d = int(_get(config, "hidden_size", 768))
        self.n_layers = int(_get(config, "num_hidden_layers", 12))
        self.n_head = int(_get(config, "num_attention_heads", 12))
        self.inter = Fi = int(_get(config, "intermediate_size", 3072))
        self.pos_k = int(_get(config, "num_conv_pos_embeddings", 128))
        self.pos_g = int(_get(config, "num_conv_pos_embedding_groups", 16))
        self.eps = float(_get(config, "layer_norm_eps", 1e-5))
        if d % self.n_head or d % 8 or Fi % 8 or d // self.n_head > 128 or (d // self.n_head) % 8:
            raise NotImplementedError("hidden size divisible by the heads, head dim a multiple of 8 and <= 128, sizes multiples of 8")
        if d % self.pos_g or (d // self.pos_g) % 16 or d // self.pos_g > 64 or self.pos_k > 256:
            raise NotImplementedError("positional conv: 16, 32, 48 or 64 channels per group, at most 256 taps")
        self.hd = d // self.n_head
        self.precision = runtime.F32 if precision == "fp32" else runtime.BF16

        self.feature_extractor = torch.nn.Module()
        self.feature_extractor.conv_layers = torch.nn.ModuleList()
        for i, k in enumerate(self.kernels):
            blk = torch.nn.Module()
            blk.conv = torch.nn.Conv1d(1 if i == 0 else C, C, k, stride=self.strides[i], bias=False)
            if i == 0:
                blk.layer_norm = torch.nn.GroupNorm(C, C, affine=True)
            self.feature_extractor.conv_layers.append(blk)
        self.feature_projection = torch.nn.Module()
        self.feature_projection.layer_norm = torch.nn.LayerNorm(C, eps=self.eps)
        self.feature_projection.projection = torch.nn.Linear(C, d)
        self.encoder = torch.nn.Module()
        self.encoder.pos_conv_embed = torch.nn.Module()
        pc = self.encoder.pos_conv_embed.conv = torch.nn.Module()
        pc.weight_g = torch.nn.Parameter(torch.ones(1, 1, self.pos_k))
        pc.weight_v = torch.nn.Parameter(torch.zeros(d, d // self.pos_g, self.pos_k))
        pc.bias = torch.nn.Parameter(torch.zeros(d))
        self.encoder.layer_norm = torch.nn.LayerNorm(d, eps=self.eps)
        self.encoder.layers = torch.nn.ModuleList()
        for _ in range(self.n_layers):
            lyr = torch.nn.Module()
            lyr.attention = torch.nn.Module()
            for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
                setattr(lyr.attention, n, torch.nn.Linear(d, d))
            lyr.layer_norm = torch.nn.LayerNorm(d, eps=self.eps)
            lyr.feed_forward = torch.nn.Module()
            lyr.feed_forward.intermediate_dense = torch.nn.Linear(d, Fi)
            lyr.feed_forward.output_dense = torch.nn.Linear(Fi, d)
            lyr.final_layer_norm = torch.nn.LayerNorm(d, eps=self.eps)
            self.encoder.layers.append(lyr)
        self._packed = None
        self._packed_versions = None
        self._ws = None              # one byte buffer (fp32 region + its bf16 image), grown to the largest batch seen
        self._ws_bytes = 0

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        out = super().load_state_dict(_rename(state_dict), strict=strict, **kw)
        self._packed = None
        return out

    # ---- packed weights ---------------------------------------------------------------------------------------------
    def _versions(self):
        return tuple(p._version for p in self.parameters())

    def _pack(self):
        dev = self.feature_projection.projection.weight.device
        if dev.type != "cuda":
            raise runtime.HipError("Wav2Vec2Encoder runs on an MI355X only (move it with .to('cuda')): no CPU fallback")
        bf16 = self.precision == runtime.BF16
        C = self.C

        def sh(w):
            return w.detach().to(torch.bfloat16).contiguous() if bf16 else None
        convs = self.feature_extractor.conv_layers
        P = {"w0": convs[0].conv.weight.detach().reshape(C, -1).float().contiguous(),
             "gn_g": convs[0].layer_norm.weight.detach().float().contiguous(), "gn_b": convs[0].layer_norm.bias.detach().float().contiguous()}
        conv = []
        for blk in convs[1:]:
            w = blk.conv.weight.detach().float()
            k = w.shape[2]
            weff = w.permute(0, 2, 1).reshape(C, k * C).contiguous()      # [o][tap][c]: a channels-last window's order
            conv.append({"w": weff, "w16": sh(weff), "k": k})
        P["conv"] = conv
        fp = self.feature_projection
        P["fln_g"], P["fln_b"] = fp.layer_norm.weight.detach().contiguous(), fp.layer_norm.bias.detach().contiguous()
        P["wp"], P["bp"] = fp.projection.weight.detach().contiguous(), fp.projection.bias.detach().contiguous()
        P["wp16"] = sh(P["wp"])
        pc = self.encoder.pos_conv_embed.conv
        G, K, d = self.pos_g, self.pos_k, self.d
        CG = d // G
        # weight norm over dim 2 (torch.nn.utils.weight_norm(conv, dim=2)): w[:, :, k] = g[k] * v[:, :, k] / ||v[:, :, k]||
        v = pc.weight_v.detach().double()
        w = (pc.weight_g.detach().double() * v / v.norm(dim=(0, 1), keepdim=True)).float()
        wpk = w.view(G, CG, CG, K).permute(0, 3, 1, 2).contiguous()     # [group][tap][o][c]
        P["pos_w"] = wpk.to(torch.bfloat16).contiguous() if bf16 else wpk
        P["pos_b"] = pc.bias.detach().float().contiguous()
        P["eln_g"], P["eln_b"] = self.encoder.layer_norm.weight.detach().contiguous(), self.encoder.layer_norm.bias.detach().contiguous()
        layers = []
        for lyr in self.encoder.layers:
            a = lyr.attention
            ent = {"wqkv": torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0).detach().contiguous(),
                   "bqkv": torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], 0).detach().contiguous(),
                   "wo": a.out_proj.weight.detach().contiguous(), "bo": a.out_proj.bias.detach(),
                   "g1": lyr.layer_norm.weight.detach(), "b1": lyr.layer_norm.bias.detach(),
                   "wi": lyr.feed_forward.intermediate_dense.weight.detach().contiguous(),
                   "bi": lyr.feed_forward.intermediate_dense.bias.detach(),
                   "wo2": lyr.feed_forward.output_dense.weight.detach().contiguous(), "bo2": lyr.feed_forward.output_dense.bias.detach(),
                   "g2": lyr.final_layer_norm.weight.detach(), "b2": lyr.final_layer_norm.bias.detach()}
            for k in ("wqkv", "wo", "wi", "wo2"):
                ent[k + "16"] = sh(ent[k])
            layers.append(ent)
        P["layers"] = layers
        self._packed = P
        self._packed_versions = self._versions()

    # ---- geometry and workspace ----------------------------------------------------------------------------------------
    def geometry(self, B: int, N: int) -> dict:
        """Frame counts T_l of the padded batch, the conv rows' pitches P_l, the utterances per chunk `ub` and the workspace layout
        (element offsets of the fp32 regions; the first `mapped` elements also have a bf16 image behind the fp32 part).

        The batch runs `ub` utterances at a time, the whole pipeline per chunk.  Every matrix a GEMM / attention / LayerNorm launch
        reads or writes stays below 2^30 elements: the GEMM kernels address operands with 32-bit offsets (the ring descriptors hold
        rows * ld * 2 bytes in an int).  All work is per utterance, so the chunking changes no result."""
        T, n = [], N
        for k, s in zip(self.kernels, self.strides):
            n = (n - k) // s + 1
            T.append(n)
        if T[-1] < 1:
            raise ValueError(f"{N} samples give no output frame: the conv stack needs at least "
                             f"{output_length_inverse(self.kernels, self.strides)} samples")
        L = len(T)
        mult = [1] * L                       # P_l = mult[l] * P_{L-1}
        for l in range(L - 2, -1, -1):
            mult[l] = mult[l + 1] * self.strides[l + 1]
        R = max(-(-T[l] // mult[l]) for l in range(L))
        P = [m * R for m in mult]
        C, d, Fi, S = self.C, self.d, self.inter, T[-1]
        slack = 4 * C                         # the second k-segment of a layer's last (junk) row reads one row past the region
        widest = max(P[0] * C + slack, S * max(3 * d, Fi, C))          # elements per utterance of the largest matrix
        ub = max(1, min(B, (_ELEMS_MAX - slack) // widest))
        if self.chunk_utterances:
            ub = min(ub, int(self.chunk_utterances))
        Tr = ub * S
        names = [("conv_a", ub * P[0] * C + slack), ("conv_b", ub * P[1] * C + slack), ("feat", Tr * C), ("qkv", Tr * 3 * d),
                 ("ctx", Tr * d), ("y1", Tr * d), ("h", Tr * Fi), ("x", Tr * d),
                 # (not mapped: read as fp32 only)
                 ("xp", Tr * d), ("t", Tr * d), ("scratch", conv0_scratch_floats(ub, C, T[0])), ("stats", 2 * Tr), ("pooled", ub * d)]
        off, o = {}, 0
        for name, cnt in names:
            off[name] = (o, cnt)
            o += _al(cnt)
            if name == "x":
                mapped = o
        return {"T": T, "P": P, "S": S, "ub": ub, "off": off, "floats": o, "mapped": mapped}

    def workspace_bytes(self, B: int, N: int) -> int:
        """Device bytes the workspace needs for a batch of B waveforms padded to N samples (fp32 regions + bf16 image in bf16 mode)."""
        g = self.geometry(B, N)
        return g["floats"] * 4 + (g["mapped"] * 2 if self.precision == runtime.BF16 else 0)

    def _workspace(self, g: dict, dev):
        """Grow-only: one byte buffer, reallocated only when a batch needs more than any batch before."""
        bf16 = self.precision == runtime.BF16
        need = g["floats"] * 4 + (g["mapped"] * 2 if bf16 else 0)
        if self._ws is None or self._ws.device != dev or need > self._ws_bytes:
            self._ws = None
            self._ws = torch.zeros(need, dtype=torch.uint8, device=dev)
            self._ws_bytes = need
        return self._ws

    # ---- forward ----------------------------------------------------------------------------------------------------
    def _run(self, waveforms: torch.Tensor, lengths: torch.Tensor, pool: bool, features: bool = False):
        runtime.require_gpu()
        if self._packed is None or self._packed_versions != self._versions():
            self._pack()
        Pk = self._packed
        if waveforms.dim() != 2:
            raise ValueError("waveforms: [B, N]")
        B, N = waveforms.shape
        dev = self.feature_projection.projection.weight.device
        wave = waveforms.to(dev, torch.float32).contiguous()
        g = self.geometry(B, N)
        T, P, S, ub = g["T"], g["P"], g["S"], g["ub"]
        C, d, H, hd, Fi = self.C, self.d, self.n_head, self.hd, self.inter
        prec = self.precision
        bf16 = prec == runtime.BF16
        ws = self._workspace(g, dev)
        base = ws.data_ptr()
        base16 = base + g["floats"] * 4

        def a32(name, extra=0):
            return base + (g["off"][name][0] + extra) * 4

        def a16(name, extra=0):
            return base16 + (g["off"][name][0] + extra) * 2

        def view(name, rows, cols):
            o = g["off"][name][0]
            return ws[o * 4: (o + rows * cols) * 4].view(torch.float32).view(rows, cols)

        # output lengths on the device (no host sync): floor((n - k) / s) + 1 per layer
        ol = lengths.to(dev, torch.int64)
        for k, s in zip(self.kernels, self.strides):
            ol = torch.div(ol - k, s, rounding_mode="floor") + 1
        ol = ol.clamp(0, S)
        ol32 = ol.to(torch.int32).contiguous()
        key_pad = (torch.arange(S, device=dev)[None, :] >= ol[:, None]).to(torch.uint8).contiguous()
        out = torch.empty((B, d) if pool else (B, S, d), dtype=torch.float32, device=dev)
        feat_out = torch.empty(B, S, C, dtype=torch.float32, device=dev) if features else None
        st = stream_ptr()
        L = lib()
        check(L.m2f_set_shadow_map(base if bf16 else None, base16 if bf16 else None, g["mapped"] if bf16 else 0), "m2f_set_shadow_map")
        try:
            for b0 in range(0, B, ub):              # ub utterances at a time (per-utterance work: the chunking changes no result)
                nb = min(ub, B - b0)
                Tr = nb * S
                # ---- conv stack -----------------------------------------------------------------------------------------
                cur = "conv_a"
                check(L.m2f_w2v_conv0(nb, N, wave.data_ptr() + b0 * N * 4, ptr(Pk["w0"]), self.kernels[0], self.strides[0], C, T[0], P[0],
                                      ptr(Pk["gn_g"]), ptr(Pk["gn_b"]), 1e-5, a32("scratch"), None if bf16 else a32(cur),
                                      a16(cur) if bf16 else None, st), "m2f_w2v_conv0")
                for l, cv in enumerate(Pk["conv"], start=1):
                    nxt = "conv_b" if cur == "conv_a" else "conv_a"
                    k, s = cv["k"], self.strides[l]
                    M, ld = nb * P[l], s * C
                    K0, K1 = s * C, (k - s) * C
                    last = l == len(Pk["conv"])
                    if bf16 and not last:
                        check(L.m2f_set_shadow_only(1), "m2f_set_shadow_only")
                    try:
                        check(L.m2f_gemm(prec, NT, M, C, K0, K1, a32(cur), ld, a32(cur, s * C) if K1 else None, ld if K1 else 0,
                                         ptr(cv["w"]), k * C, cv["w"].data_ptr() + K0 * 4 if K1 else None, k * C if K1 else 0,
                                         a32(nxt), C, None, None, 0, None, 0, 1.0, None, 0, 0, 2, 0, 0, 0.0, None, 0,
                                         None, None, 0,
                                         a16(cur) if bf16 else None, ld if bf16 else 0,
                                         a16(cur, s * C) if bf16 and K1 else None, ld if bf16 and K1 else 0,
                                         ptr(cv["w16"]) if bf16 else None, k * C if bf16 else 0,
                                         cv["w16"].data_ptr() + K0 * 2 if bf16 and K1 else None, k * C if bf16 and K1 else 0, st),
                              "m2f_gemm (conv layer)")
                    finally:
                        if bf16 and not last:
                            check(L.m2f_set_shadow_only(0), "m2f_set_shadow_only")
                    cur = nxt
                # feature LayerNorm: pitched rows -> compact rows b * S + t
                check(L.m2f_w2v_feat_layernorm(nb, S, P[-1], C, a32(cur), ptr(Pk["fln_g"]), ptr(Pk["fln_b"]), self.eps,
                                               a32("feat"), a16("feat") if bf16 else None, st), "m2f_w2v_feat_layernorm")
                v = {n: view(n, Tr, c) for n, c in (("feat", C), ("x", d), ("y1", d))}

                def linear(a_name, a_cols, w, w16, out_name, bias, res=None, act=0, out16_only=False):
                    if bf16 and out16_only:
                        check(L.m2f_set_shadow_only(1), "m2f_set_shadow_only")
                    try:
                        check(L.m2f_gemm(prec, NT, Tr, w.shape[0], a_cols, 0, a32(a_name), a_cols, None, 0, ptr(w), w.shape[1], None, 0,
                                         a32(out_name), w.shape[0], ptr(bias), ptr(res), res.stride(0) if res is not None else 0, None, 0,
                                         1.0, None, 0, 0, act, 0, 0, 0.0, None, 0, None, None, 0,
                                         a16(a_name) if bf16 else None, a_cols if bf16 else 0, None, 0,
                                         ptr(w16) if bf16 else None, w.shape[1] if bf16 else 0, None, 0, st), "m2f_gemm")
                    finally:
                        if bf16 and out16_only:
                            check(L.m2f_set_shadow_only(0), "m2f_set_shadow_only")

                # feature projection, then x + GELU(posconv(x)) with padded frames read as zero, then the encoder LayerNorm
                linear("feat", C, Pk["wp"], Pk["wp16"], "xp", Pk["bp"])
                lens = ol32[b0: b0 + nb]
                kp = key_pad[b0: b0 + nb]
                check(L.m2f_w2v_pos_conv(nb, S, d, self.pos_g, self.pos_k, a32("xp"), ptr(lens), ptr(Pk["pos_w"]), ptr(Pk["pos_b"]),
                                         a32("t"), int(bf16), st), "m2f_w2v_pos_conv")
                check(L.m2f_layernorm_fwd(Tr, d, a32("t"), ptr(Pk["eln_g"]), ptr(Pk["eln_b"]), None, a32("x"), a32("stats"), self.eps, st),
                      "m2f_layernorm_fwd")
                for Ly in Pk["layers"]:
                    linear("x", d, Ly["wqkv"], Ly["wqkv16"], "qkv", Ly["bqkv"], out16_only=True)
                    if bf16:
                        q16 = a16("qkv")
                        check(L.m2f_attention_long_fwd_bf16(nb, S, H, hd, q16, 3 * d, q16 + 2 * d, 3 * d, q16 + 4 * d, 3 * d, ptr(kp),
                                                            a16("ctx"), None, d, st), "m2f_attention_long_fwd_bf16")
                    else:
                        q = a32("qkv")
                        check(L.m2f_attention_long_fwd(nb, S, H, hd, q, 3 * d, q + 4 * d, 3 * d, q + 8 * d, 3 * d, ptr(kp), a32("ctx"),
                                                       d, st), "m2f_attention_long_fwd")
                    linear("ctx", d, Ly["wo"], Ly["wo16"], "t", Ly["bo"], res=v["x"])
                    check(L.m2f_layernorm_fwd(Tr, d, a32("t"), ptr(Ly["g1"]), ptr(Ly["b1"]), None, a32("y1"), a32("stats"), self.eps, st),
                          "m2f_layernorm_fwd")
                    linear("y1", d, Ly["wi"], Ly["wi16"], "h", Ly["bi"], act=2, out16_only=True)
                    linear("h", Fi, Ly["wo2"], Ly["wo216"], "t", Ly["bo2"], res=v["y1"])
                    check(L.m2f_layernorm_fwd(Tr, d, a32("t"), ptr(Ly["g2"]), ptr(Ly["b2"]), None, a32("x"), a32("stats"), self.eps, st),
                          "m2f_layernorm_fwd")
                if pool:
                    check(L.m2f_w2v_masked_mean(nb, S, d, a32("x"), ptr(lens), ptr(out[b0: b0 + nb]), st), "m2f_w2v_masked_mean")
                else:
                    out[b0: b0 + nb].copy_(v["x"].view(nb, S, d))
                if features:
                    feat_out[b0: b0 + nb].copy_(v["feat"].view(nb, S, C))
        finally:
            check(L.m2f_set_shadow_map(None, None, 0), "m2f_set_shadow_map")
        return out, ol, feat_out

    @torch.no_grad()
    def forward(self, waveforms: torch.Tensor, lengths: torch.Tensor, return_features: bool = False):
        """waveforms [B, N] fp32 (zero-padded to the longest), lengths [B] sample counts -> (hidden [B, S, d], out_lengths [B] int64),
        plus extract_features [B, S, C] (the feature LayerNorm's output) with return_features=True.  Rows at or past out_lengths[b]
        are don't-care (their keys are masked)."""
        out, ol, feat = self._run(waveforms, lengths, pool=False, features=return_features)
        return (out, ol, feat) if return_features else (out, ol)

    @torch.no_grad()
    def utterance_embeddings(self, waveforms: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        """[B, d]: the mean of each utterance's valid frames (embeddings.py:80-85)."""
        return self._run(waveforms, lengths, pool=True)[0]


def output_length_inverse(kernels, strides) -> int:
    """Smallest sample count that yields one output frame."""
    n = 1
    for k, s in reversed(list(zip(kernels, strides))):
        n = (n - 1) * s + k
    return n


def base_config() -> dict:
    """wav2vec2-base (torchaudio WAV2VEC2_BASE / transformers' Wav2Vec2Config defaults)."""
    return {"conv_dim": (512,) * 7, "conv_kernel": (10, 3, 3, 3, 3, 2, 2), "conv_stride": (5, 2, 2, 2, 2, 2, 2), "conv_bias": False,
            "feat_extract_norm": "group", "feat_extract_activation": "gelu", "do_stable_layer_norm": False, "hidden_size": 768,
            "num_hidden_layers": 12, "num_attention_heads": 12, "intermediate_size": 3072, "hidden_act": "gelu",
            "num_conv_pos_embeddings": 128, "num_conv_pos_embedding_groups": 16, "layer_norm_eps": 1e-5}
