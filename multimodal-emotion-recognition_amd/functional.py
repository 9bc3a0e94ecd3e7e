"""Thin Python wrappers over the kernel-level C entry points (include/m2fnet_hip.h).

Used by the parity tests (each HIP kernel against the oracle) and by the standalone
``FusionAttentionModule.forward``.  Tensors must be fp32 CUDA tensors; strides are passed as leading
dimensions, so column slices of a wider matrix are legal operands.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import runtime
from .runtime import lib, check, ptr, stream_ptr

NT, NN, TN = 0, 1, 2


def _ld(t: torch.Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1 and t.dtype == torch.float32 and t.is_cuda, "need fp32 CUDA row-major 2-D"
    return t.stride(0)


_SPLITK = {}


def _splitk_scratch(device):
    """(partial slabs, zeroed tickets, max tiles) per device for the split-K path of small launches."""
    if device not in _SPLITK:
        n = 512
        _SPLITK[device] = (torch.empty(n * 4 * 64 * 64, dtype=torch.float32, device=device),
                           torch.zeros(n, dtype=torch.int32, device=device), n)
    return _SPLITK[device]


def _shadow16(t: torch.Tensor) -> torch.Tensor:
    rows, cols = t.shape
    out = torch.zeros(rows, (cols + 7) // 8 * 8, dtype=torch.bfloat16, device=t.device)
    out[:, :cols] = t.to(torch.bfloat16)
    return out


def gemm(a: torch.Tensor, b: torch.Tensor, layout: int = NT, precision: int = runtime.F32,
         a1: Optional[torch.Tensor] = None, b1: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
         res: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None, gate_scale: float = 1.0,
         bias_grad: bool = False, relu_a: bool = False, relu_b: bool = False, relu_out: bool = False,
         out: Optional[torch.Tensor] = None, accumulate: bool = False, drop_site: int = 0, drop_p: float = 0.0,
         rng: Optional[torch.Tensor] = None, tile: int = 0, split_k: bool = False, src16: bool = False,
         shadows=None):
    """layout NT: a[M,K] b[N,K]; NN: a[M,K] b[K,N]; TN: a[K,M] b[K,N].  Returns C (and bias_grad[M] for TN).
    `shadows` = prebuilt bf16 images (a, a1, b, b1) replacing the per-call ones `src16=True` makes."""
    runtime.require_gpu()
    if layout == NT:
        M, K0 = a.shape; N = b.shape[0]
    elif layout == NN:
        M, K0 = a.shape; N = b.shape[1]
    else:
        K0, M = a.shape; N = b.shape[1]
    K1 = 0
    if a1 is not None:
        K1 = a1.shape[0] if layout == TN else a1.shape[1]
    c = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=a.device)
    # (accumulate: the kernel adds the column sums to bias_grad as it adds to C - a fresh buffer starts at zero)
    bg = (torch.zeros if accumulate else torch.empty)(M, dtype=torch.float32, device=a.device) if bias_grad else None
    ws, tickets, nmax = _splitk_scratch(a.device) if split_k else (None, None, 0)
    # bf16 shadows (test plumbing: in the plan the producer kernels write them): zero-padded to a multiple of 8 columns
    sh = list(shadows) if shadows is not None else [None if (t is None or not src16) else _shadow16(t) for t in (a, a1, b, b1)]
    shp = [(ptr(t), t.stride(0)) if t is not None else (None, 0) for t in sh]
    check(lib().m2f_gemm(precision, layout, M, N, K0, K1, ptr(a), _ld(a), ptr(a1), _ld(a1) if a1 is not None else 0,
                         ptr(b), _ld(b), ptr(b1), _ld(b1) if b1 is not None else 0, ptr(c), _ld(c), ptr(bias),
                         ptr(res), _ld(res) if res is not None else 0, ptr(gate), _ld(gate) if gate is not None else 0,
                         gate_scale, ptr(bg), int(relu_a), int(relu_b), int(relu_out), int(accumulate), drop_site,
                         drop_p, ptr(rng), tile, ptr(ws), ptr(tickets), nmax, shp[0][0], shp[0][1], shp[1][0], shp[1][1],
                         shp[2][0], shp[2][1], shp[3][0], shp[3][1], stream_ptr()), "m2f_gemm")
    return (c, bg) if bias_grad else c


def gemm_fp8(a8: torch.Tensor, b8: torch.Tensor, acc_scale: float, bias: Optional[torch.Tensor] = None,
             res: Optional[torch.Tensor] = None, activation: int = 0, out: Optional[torch.Tensor] = None,
             out8: Optional[torch.Tensor] = None, out8_scale: float = 1.0) -> torch.Tensor:
    """a8 [M, K], b8 [N, K] torch.float8_e4m3fn -> fp32 [M, N] = act(acc_scale * a8 b8^T + bias) + res, or - with `out8` -
    the same result quantised as e4m3(result * out8_scale) into out8 [M, N] (no fp32 output)."""
    runtime.require_gpu()
    assert a8.dtype == torch.float8_e4m3fn and b8.dtype == torch.float8_e4m3fn
    M, K = a8.shape
    N = b8.shape[0]
    if out8 is not None:
        assert out8.dtype == torch.float8_e4m3fn and out8.shape == (M, N)
        check(lib().m2f_gemm_fp8(M, N, K, ptr(a8), a8.stride(0), ptr(b8), b8.stride(0), float(acc_scale), None, out8.stride(0),
                                 ptr(bias), ptr(res), _ld(res) if res is not None else 0, int(activation), ptr(out8),
                                 float(out8_scale), stream_ptr()), "m2f_gemm_fp8")
        return out8
    c = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=a8.device)
    check(lib().m2f_gemm_fp8(M, N, K, ptr(a8), a8.stride(0), ptr(b8), b8.stride(0), float(acc_scale), ptr(c), _ld(c), ptr(bias),
                             ptr(res), _ld(res) if res is not None else 0, int(activation), None, 1.0, stream_ptr()), "m2f_gemm_fp8")
    return c


def quantize_fp8(src: torch.Tensor, scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """e4m3(clamp(src * scale, +-448)) of a contiguous fp32 tensor."""
    runtime.require_gpu()
    assert src.is_contiguous() and src.dtype == torch.float32
    dst = out if out is not None else torch.empty(src.shape, dtype=torch.float8_e4m3fn, device=src.device)
    check(lib().m2f_quantize_fp8(ptr(src), ptr(dst), src.numel(), float(scale), stream_ptr()), "m2f_quantize_fp8")
    return dst


def _attn_opts(who: str, H: int, rows: int, device, past, future, bias, speakers, speaker_heads) -> runtime.AttnOptsC:
    """The m2f_attn_opts of a forward launch of `rows` token rows: band, gain as applied, speaker heads with their ids (uint8 [rows] on
    `device`, kept alive by the descriptor).  Every option at None is the launch without it.  Raises ValueError before anything is
    launched."""
    o = runtime.AttnOptsC()
    o.bias_gain = runtime.position_bias(bias)
    heads = runtime.speaker_heads(speaker_heads, {"this launch": H})
    if heads is None:
        if speakers is not None:
            raise ValueError(f"{who}: speakers were given without speaker_heads=(n_same, n_other)")
    else:
        if speakers is None:
            raise ValueError(f"{who}: speaker_heads={heads} needs speakers (one id per utterance)")
        o.ids = runtime.speaker_ids(speakers, f"{who}: speakers").reshape(-1).contiguous().to(device)
        if o.ids.numel() != rows:
            raise ValueError(f"{who}: speakers must hold one id per token row ({rows}), got {o.ids.numel()}")
        o.n_same, o.n_other, o.speakers = heads[0], heads[1], ptr(o.ids)
    o.past, o.future = runtime.context_band(past, future)
    return o


speaker_head_class = runtime.speaker_head_class      # (the library's own statement of the rule: csrc/ops.h, m2f_attn_speaker_class)


def attention_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, key_pad: torch.Tensor, B: int, L: int, H: int,
                  drop_site: int = 0, drop_p: float = 0.0, rng: Optional[torch.Tensor] = None,
                  past: Optional[int] = None, future: Optional[int] = None, bias: Optional[float] = None,
                  speakers: Optional[torch.Tensor] = None, speaker_heads=None):
    """q/k/v: [B*L, H*hd] (possibly column slices).  Returns (out [B*L, H*hd], probs^T [B*H, Lp, Lp]).
    speakers / speaker_heads: speaker heads (`runtime.speaker_heads` has the rule) - speakers: one id per utterance, [B, L] or [B*L],
    uint8 / int32 / int64 with values 0 .. 255; speaker_heads = (n_same, n_other), n_same + n_other <= H.  The condition is ANDed with
    key padding and the band, the bias applies to what stays visible; a query whose head sees no key (an other-speaker head in a
    monologue) gets a zero row of probabilities and a zero output row.  speaker_heads=None is the call without the argument.
    past / future: context band - query slot i sees the valid keys of slots i - past .. i + future only (None = unlimited on that
    side; (None, 0) is causal).  Hidden keys have probability exactly 0; a query that sees no key at all (a pad slot whose band
    holds pad keys only) gets a zero row of probabilities and a zero output row, where torch's masked softmax gives NaN - pad
    slots under a band are not the reference's numbers.
    bias: gain of the distance-decay bias (`position_bias_slopes`; None or 0 = off, the entries called without it): a visible key's
    score gets -slope(h, H, gain) * |i - j|, the gain applied as `runtime.position_bias` rounds it.  The backward (`attention_bwd`) reads the saved probabilities and takes no gain."""
    runtime.require_gpu()
    opts = _attn_opts("attention_fwd", H, B * L, q.device, past, future, bias, speakers, speaker_heads)
    E = q.shape[1]
    hd = E // H
    out = torch.empty(B * L, E, dtype=torch.float32, device=q.device)
    Lp = 16 * ((L + 15) // 16)
    probs = torch.zeros(B * H, Lp, Lp, dtype=torch.float32, device=q.device)
    kp = key_pad.to(torch.uint8).contiguous()
    check(lib().m2f_attention_fwd(B, L, H, hd, ptr(q), _ld(q), ptr(k), _ld(k), ptr(v), _ld(v), ptr(kp), ptr(out), _ld(out), ptr(probs),
                                  drop_site, drop_p, ptr(rng), stream_ptr(), ctypes.byref(opts)), "m2f_attention_fwd")
    return out, probs


def position_bias_slopes(H: int, gain=1.0) -> torch.Tensor:
    """The per-head slopes of the distance-decay attention bias (ALiBi), fp32 [H] on the CPU: head h of H adds ``-slopes[h] * |i - j|``
    to the scaled score of query i and visible key j (positions inside the dialogue).  slopes[h] = gain * base(h, H); with
    n = 2^floor(log2 H): base = 2^(-8 (h + 1) / n) for h < n, 2^(-4 (2 (h - n) + 1) / n) for h >= n - the recipe for head counts that
    are no power of two (H = 4: 1/4, 1/16, 1/64, 1/256; H = 3: 1/16, 1/256, 1/4).  gain: as `runtime.position_bias` takes and rounds
    it (to bf16: what the kernels apply); None = 0: no bias.  No parameters: a constant of the model."""
    if isinstance(H, bool) or not isinstance(H, int) or H < 1:
        raise ValueError(f"position_bias_slopes: H must be an integer >= 1, got {H!r}")
    g = runtime.position_bias(gain)
    n = 1 << (H.bit_length() - 1)
    base = [2.0 ** (-8.0 * (h + 1) / n) if h < n else 2.0 ** (-4.0 * (2 * (h - n) + 1) / n) for h in range(H)]
    return torch.tensor([g * b for b in base], dtype=torch.float64).to(torch.float32)


def attention_weights(probs: torch.Tensor, B: int, L: int, H: int, key_pad: Optional[torch.Tensor] = None,
                      cu: Optional[torch.Tensor] = None, past: Optional[int] = None, future: Optional[int] = None,
                      average_heads: bool = True) -> torch.Tensor:
    """The attention map of one site (m2f_attention_weights, csrc/attention_weights.hip) out of the `probs` that `attention_fwd` /
    `attention_varlen_fwd` returned for the same B, L, H: what ``nn.MultiheadAttention(need_weights=True)`` returns, [B, L, L] (the
    fp32 sum over the heads in order times fp32(1 / H): ``average_attn_weights=True``) or, with ``average_heads=False``, [B, H, L, L].
    key_pad ([B, L] or [B*L], 1 = padded key) / cu (int32 [B + 1], packed rows) / past, future: what the forward was given.  An element
    is read from `probs` only inside the dialogue, at an unpadded key and inside the band; every other one is exactly 0 - whatever a
    reused `probs` buffer held there.  Pad-query rows of a padded batch hold their softmax numbers (as torch's do); a row that sees
    no key is zeros (torch: NaN)."""
    for name, v in (("B", B), ("L", L), ("H", H)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"attention_weights: {name} must be an integer >= 1, got {v!r}")
    if L > 512:
        raise ValueError(f"attention_weights: L <= 512 required, got {L}")
    Lp = 16 * ((L + 15) // 16)
    if not isinstance(probs, torch.Tensor) or probs.dtype != torch.float32 or tuple(probs.shape) != (B * H, Lp, Lp) or not probs.is_contiguous():
        raise ValueError(f"attention_weights: probs must be a contiguous fp32 [B*H, Lp, Lp] = [{B * H}, {Lp}, {Lp}] tensor "
                         f"(attention_fwd's second result), got {getattr(probs, 'dtype', None)} {tuple(getattr(probs, 'shape', ()))}")
    if key_pad is not None and cu is not None:
        raise ValueError("attention_weights: at most one of key_pad (padded rows) and cu (packed rows) may be given")
    if key_pad is not None and key_pad.numel() != B * L:
        raise ValueError(f"attention_weights: key_pad must hold B * L = {B * L} flags, got {tuple(key_pad.shape)}")
    if cu is not None and (cu.dtype != torch.int32 or tuple(cu.shape) != (B + 1,)):
        raise ValueError(f"attention_weights: cu must be int32 [B + 1] = [{B + 1}], got {cu.dtype} {tuple(cu.shape)}")
    band = runtime.context_band(past, future)           # (raises ValueError)
    runtime.require_gpu()
    kp = None if key_pad is None else key_pad.to(device=probs.device, dtype=torch.uint8).contiguous()
    cu = None if cu is None else cu.to(probs.device).contiguous()
    out = torch.empty((B, L, L) if average_heads else (B, H, L, L), dtype=torch.float32, device=probs.device)
    check(lib().m2f_attention_weights(B, L, H, ptr(probs), ptr(kp), ptr(cu), band[0], band[1], int(not average_heads), ptr(out),
                                      stream_ptr()), "m2f_attention_weights")
    return out


def attention_long_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, key_pad: Optional[torch.Tensor], B: int, S: int, H: int,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Token-level self-attention of the in-loop encoders' fp32 mode (m2f_attention_long_fwd): q / k / v [B*S, H*hd] fp32, possibly
    column slices of a wider matrix (token b*S + i at row b*S + i); key_pad uint8 / bool [B, S] (1 = padded key) or None.
    softmax(q k^T / sqrt(hd)) v over the valid keys per (sequence, head), any S, hd <= 128; a query whose keys are all padded gets a
    zero row.  `out`: a preallocated fp32 tensor of at least B*S rows and H*hd columns (a wider pitch is legal, the columns behind
    H*hd are left alone).  Returns the [B*S, H*hd] view of the result."""
    runtime.require_gpu()
    T, E = B * S, q.shape[1]
    if H < 1 or E % H or k.shape != q.shape or v.shape != q.shape or q.shape[0] != T:
        raise ValueError("attention_long_fwd: q / k / v hold B * S rows of H * hd columns")
    if out is None:
        out = torch.empty(T, E, dtype=torch.float32, device=q.device)
    if out.dim() != 2 or out.shape[0] < T or out.shape[1] < E:
        raise ValueError("attention_long_fwd: out needs at least B * S rows and H * hd columns")
    kp = None
    if key_pad is not None:
        if key_pad.numel() != T or key_pad.dtype not in (torch.uint8, torch.bool):
            raise ValueError("attention_long_fwd: key_pad uint8 / bool [B, S] required")
        kp = key_pad.to(device=q.device, dtype=torch.uint8).contiguous()
    check(lib().m2f_attention_long_fwd(B, S, H, E // H, ptr(q), _ld(q), ptr(k), _ld(k), ptr(v), _ld(v), ptr(kp), ptr(out), _ld(out),
                                       stream_ptr()), "m2f_attention_long_fwd")
    return out[:T, :E]


def embed_layernorm(ids: torch.Tensor, pos_ids: torch.Tensor, word: torch.Tensor, pos: torch.Tensor, type_row0: torch.Tensor,
                    gamma: torch.Tensor, beta: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """RoBERTa embeddings (m2f_embed_layernorm): LayerNorm(word[ids] + pos[pos_ids] + type_row0) * gamma + beta.  ids / pos_ids int64
    [T]; word [vocab, d], pos [max_pos, d] contiguous fp32; type_row0 / gamma / beta fp32 [d]; d % 4 == 0, d <= 2048.  `out`: a
    preallocated fp32 tensor of at least T rows and d columns (a wider pitch is legal).  Returns the [T, d] view of the result."""
    runtime.require_gpu()
    T, d = ids.numel(), word.shape[1]
    if ids.dtype != torch.int64 or pos_ids.dtype != torch.int64 or ids.dim() != 1 or pos_ids.shape != ids.shape:
        raise ValueError("embed_layernorm: ids and pos_ids int64 [T] required")
    for t in (word, pos):
        if t.dim() != 2 or t.shape[1] != d or t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError("embed_layernorm: the tables must be contiguous, 16-byte aligned fp32 [rows, d]")
    for t in (type_row0, gamma, beta):
        if t.shape != (d,) or t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError("embed_layernorm: type_row0 / gamma / beta must be contiguous, 16-byte aligned fp32 [d]")
    if T and (int(ids.min()) < 0 or int(ids.max()) >= word.shape[0] or int(pos_ids.min()) < 0 or int(pos_ids.max()) >= pos.shape[0]):
        raise ValueError("embed_layernorm: an id lies outside its table")
    if out is None:
        out = torch.empty(T, d, dtype=torch.float32, device=word.device)
    if out.dim() != 2 or out.shape[0] < T or out.shape[1] < d or out.data_ptr() % 16:
        raise ValueError("embed_layernorm: out needs at least T rows and d columns, 16-byte aligned")
    ids, pos_ids = ids.contiguous(), pos_ids.contiguous()
    check(lib().m2f_embed_layernorm(T, d, ptr(ids), ptr(pos_ids), ptr(word), ptr(pos), ptr(type_row0), ptr(gamma), ptr(beta), float(eps),
                                    ptr(out), _ld(out), stream_ptr()), "m2f_embed_layernorm")
    return out[:T, :d]


def attention_stream_caches(S: int, H: int, hd: int, capacity: int, bf16: bool = False, device="cuda", fill: float = 0.0):
    """(kcache, vcache) of one streaming-attention site: flat tensors viewed [S, H, capacity, pad(hd)], fp32 (pad to 4) or bf16 (pad to
    8), filled with `fill`."""
    n = lib().m2f_attention_stream_cache_elems(S, H, hd, capacity, int(bf16))
    if n < 0:
        raise runtime.HipError("m2f_attention_stream_cache_elems: " + lib().m2f_last_error().decode())
    hdp = (hd + 7) // 8 * 8 if bf16 else (hd + 3) // 4 * 4
    dt = torch.bfloat16 if bf16 else torch.float32
    return tuple(torch.full((S, H, capacity, hdp), fill, dtype=dt, device=device) for _ in range(2))


def _stream_opts(who: str, H: int, S: int, C: int, per_slot: int, device, bf16: bool, kc, vc, table, weights, bias, speakers,
                 speaker_cache, speaker_heads) -> runtime.AttnStreamOptsC:
    """The m2f_attn_stream_opts of a step (per_slot = 1) or chunk (per_slot = T) launch over S slots of capacity C, after the checks
    that need tensors (sizes and alignment are the library's to refuse): kc / vc are dense caches (table None) or page pools, weights
    the step's [S, H, C] rows of probabilities, bias the gain, speakers the new utterances' ids (uint8 [S * per_slot] on `device`, kept
    alive by the descriptor) beside the cached ones.  Raises ValueError before anything is launched."""
    o = runtime.AttnStreamOptsC()
    o.bias_gain = runtime.position_bias(bias)
    want = torch.bfloat16 if bf16 else torch.float32
    if table is not None:
        o.n_pages, o.page_rows = _paged_args(who, kc, vc, table, S, C, bf16)
        o.table, o.table_cols = ptr(table), table.shape[1]
    elif kc.dtype != want or vc.dtype != want or not kc.is_contiguous() or not vc.is_contiguous():
        raise ValueError(f"{who}: the caches must be contiguous " + ("bfloat16" if bf16 else "float32") + " tensors")
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != (S, H, C) or not weights.is_contiguous():
            raise ValueError(f"{who}: weights must be a contiguous fp32 [S, H, capacity] = [{S}, {H}, {C}] tensor")
        o.weights = ptr(weights)
    heads = runtime.speaker_heads(speaker_heads, {"this launch": H})
    if heads is None:
        if speakers is not None or speaker_cache is not None:
            raise ValueError(f"{who}: speakers / speaker_cache were given without speaker_heads=(n_same, n_other)")
        return o
    if speakers is None or speaker_cache is None:
        raise ValueError(f"{who}: speaker_heads={heads} needs speakers (the new utterances' ids) and speaker_cache (uint8 [S, capacity])")
    if (not isinstance(speaker_cache, torch.Tensor) or speaker_cache.dtype != torch.uint8 or tuple(speaker_cache.shape) != (S, C)
            or not speaker_cache.is_contiguous() or speaker_cache.device != device):
        raise ValueError(f"{who}: speaker_cache must be a contiguous uint8 [{S}, {C}] tensor on the launch's device")
    o.ids = runtime.speaker_ids(speakers, f"{who}: speakers").reshape(-1).contiguous().to(device)
    if o.ids.numel() != S * per_slot:
        raise ValueError(f"{who}: speakers must hold {S * per_slot} ids, got {o.ids.numel()}")
    o.n_same, o.n_other, o.spk_cache, o.spk_new = heads[0], heads[1], ptr(speaker_cache), ptr(o.ids)
    return o


def _stream_step(who: str, q, k, v, kc, vc, table, C: int, lengths, active, H: int, ring, bf16, weights, bias, speakers, speaker_cache,
                 speaker_heads) -> torch.Tensor:
    """`attention_stream` / `attention_stream_paged`: kc / vc are the caches (table None) or the pools of capacity C."""
    runtime.require_gpu()
    S, E = q.shape
    opts = _stream_opts(who, H, S, C, 1, q.device, bf16, kc, vc, table, weights, bias, speakers, speaker_cache, speaker_heads)
    if lengths.dtype != torch.int32 or lengths.numel() != S or active.numel() != S:
        raise ValueError(f"{who}: lengths int32 [S] and active [S] required")
    act = active.to(torch.uint8).contiguous()
    out = torch.empty(S, E, dtype=torch.float32, device=q.device)
    check(lib().m2f_attention_stream(S, H, E // H, ptr(q), _ld(q), ptr(k), _ld(k), ptr(v), _ld(v), ptr(kc), ptr(vc), C, int(ring), ptr(lengths),
                                     ptr(act), ptr(out), _ld(out), int(bf16), stream_ptr(), ctypes.byref(opts)), "m2f_attention_stream")
    return out


def _stream_chunk(who: str, q, k, v, kc, vc, table, S: int, C: int, lengths, new, H: int, T: int, ring, bf16, bias, speakers, speaker_cache,
                  speaker_heads) -> torch.Tensor:
    """`attention_stream_chunk` / `attention_stream_chunk_paged`: kc / vc are the caches (table None) or the pools of capacity C."""
    runtime.require_gpu()
    rows, E = q.shape
    opts = _stream_opts(who, H, S, C, T, q.device, bf16, kc, vc, table, None, bias, speakers, speaker_cache, speaker_heads)
    if not 1 <= T <= 64 or rows != S * T or k.shape[0] != rows or v.shape[0] != rows:
        raise ValueError(f"{who}: q / k / v hold S * T rows, 1 <= T <= 64")
    if lengths.dtype != torch.int32 or lengths.numel() != S or new.dtype != torch.int32 or new.numel() != S:
        raise ValueError(f"{who}: lengths int32 [S] and new int32 [S] required")
    out = torch.empty(rows, E, dtype=torch.float32, device=q.device)
    check(lib().m2f_attention_stream_chunk(S, T, H, E // H, ptr(q), _ld(q), ptr(k), _ld(k), ptr(v), _ld(v), ptr(kc), ptr(vc), C, int(ring),
                                           ptr(lengths), ptr(new), ptr(out), _ld(out), int(bf16), stream_ptr(), ctypes.byref(opts)),
          "m2f_attention_stream_chunk")
    return out


def stream_advance_speakers(lengths: torch.Tensor, active: torch.Tensor, speaker_cache: torch.Tensor, speakers: torch.Tensor,
                            ring: bool = False) -> None:
    """The launch that closes a step of a stream with speaker heads (m2f_stream_advance_speakers): for every active slot the new
    utterance's id goes into speaker_cache[s, lengths[s] % capacity] (ring) or [s, lengths[s]], then lengths[s] += 1.  Call it BEHIND
    the step's attention launches (`attention_stream(..., speaker_heads=)` reads the cache and does not write it)."""
    runtime.require_gpu()
    S, C = speaker_cache.shape
    if lengths.dtype != torch.int32 or lengths.numel() != S or active.numel() != S or speaker_cache.dtype != torch.uint8:
        raise ValueError("stream_advance_speakers: lengths int32 [S], active [S] and speaker_cache uint8 [S, capacity] required")
    act = active.to(torch.uint8).contiguous()
    ids = runtime.speaker_ids(speakers, "stream_advance_speakers: speakers").reshape(-1).contiguous()
    if ids.numel() != S:
        raise ValueError(f"stream_advance_speakers: speakers must hold {S} ids")
    check(lib().m2f_stream_advance_speakers(S, C, int(ring), ptr(lengths), ptr(act), ptr(speaker_cache), ptr(ids), stream_ptr()),
          "m2f_stream_advance_speakers")


def stream_advance_speakers_n(lengths: torch.Tensor, new: torch.Tensor, speaker_cache: torch.Tensor, speakers: torch.Tensor, T: int,
                              ring: bool = False) -> None:
    """... of a chunk call (m2f_stream_advance_speakers_n): slot s's first new[s] ids of speakers[s, :T] into the rows its chunk took -
    the rows `attention_stream_chunk` stored K / V to - then lengths[s] += new[s]."""
    runtime.require_gpu()
    S, C = speaker_cache.shape
    if lengths.dtype != torch.int32 or lengths.numel() != S or new.dtype != torch.int32 or new.numel() != S or speaker_cache.dtype != torch.uint8:
        raise ValueError("stream_advance_speakers_n: lengths int32 [S], new int32 [S] and speaker_cache uint8 [S, capacity] required")
    ids = runtime.speaker_ids(speakers, "stream_advance_speakers_n: speakers").reshape(-1).contiguous()
    if ids.numel() != S * T:
        raise ValueError(f"stream_advance_speakers_n: speakers must hold {S * T} ids")
    check(lib().m2f_stream_advance_speakers_n(S, T, C, int(ring), ptr(lengths), ptr(new), ptr(speaker_cache), ptr(ids), stream_ptr()),
          "m2f_stream_advance_speakers_n")


def attention_stream(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, lengths: torch.Tensor,
                     active: torch.Tensor, H: int, ring: bool = False, bf16: bool = False,
                     weights: Optional[torch.Tensor] = None, bias: Optional[float] = None, speakers: Optional[torch.Tensor] = None,
                     speaker_cache: Optional[torch.Tensor] = None, speaker_heads=None) -> torch.Tensor:
    """One streaming-attention launch (m2f_attention_stream): slot s takes the new rows q[s] / k[s] / v[s] ([S, H*hd] fp32, possibly column
    slices) against the rows it has cached.  kcache / vcache: `attention_stream_caches`; lengths int32 [S] = utterances cached so far
    (read, NOT advanced); active uint8 / bool [S].  An active slot stores its new K / V rows at row lengths % capacity (ring) or
    lengths (lengths < capacity required) and gets softmax(q K^T / sqrt(hd)) V over its min(lengths + 1, capacity) live rows; an
    inactive slot gets a zero row and its caches stay as they are.  Returns out [S, H*hd].
    weights: a contiguous fp32 [S, H, capacity] tensor - the launch (m2f_attn_stream_opts::weights, the weights-emitting form of the
    kernel) also fills it with each slot's row of attention probabilities in logical order: column t = the t-th oldest live utterance
    (`streaming.logical_columns`), the last live column the new one; zeros behind the live count and for inactive slots.  Same `out`, same bits.
    bias: gain of the distance-decay bias (`position_bias_slopes`; None or 0 = off, the entries called without it): the new utterance
    is at distance 0, the one cached before it at distance 1, ...; the cached rows do not depend on it.
    speakers / speaker_cache / speaker_heads: speaker heads (`runtime.speaker_heads`) - speakers: the new utterances' ids, [S];
    speaker_cache: uint8 [S, capacity], the cached utterances' ids by logical cache row, READ only (`stream_advance_speakers` stores
    the new ids and advances `lengths`); an other-speaker head with no other speaker in sight gives a zero row.  speaker_heads=None is
    the call without the arguments."""
    return _stream_step("attention_stream", q, k, v, kcache, vcache, None, kcache.shape[2], lengths, active, H, ring, bf16, weights, bias,
                        speakers, speaker_cache, speaker_heads)


def attention_stream_chunk(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor,
                           lengths: torch.Tensor, new: torch.Tensor, H: int, T: int, ring: bool = False, bf16: bool = False,
                           bias: Optional[float] = None, speakers: Optional[torch.Tensor] = None,
                           speaker_cache: Optional[torch.Tensor] = None, speaker_heads=None) -> torch.Tensor:
    """One chunk launch of the streaming attention (m2f_attention_stream_chunk): slot s takes its first new[s] (int32 [S], 0 .. T, T <= 64)
    rows of q / k / v ([S*T, H*hd] fp32, possibly column slices; rows s*T + t) against the rows it has cached - row by row what new[s]
    `attention_stream` launches give.  lengths int32 [S] is read, NOT advanced.  The new K / V rows go to rows (lengths + t) % capacity
    (ring) or lengths + t (lengths + new <= capacity required, else the slot is left untouched) - of more than `capacity` rows on a ring
    the last `capacity`.  Rows t >= new[s] of the result are zeros and their input rows are never read.  Returns out [S*T, H*hd].
    bias: as `attention_stream` - row t of a chunk is utterance lengths + t.
    speakers / speaker_cache / speaker_heads: speaker heads (`runtime.speaker_heads`) - speakers: the new utterances' ids, [S, T] (row s*T + t);
    speaker_cache: uint8 [S, capacity], the cached utterances' ids by logical cache row, READ only (`stream_advance_speakers_n` stores
    the new ids and advances `lengths`); an other-speaker head with no other speaker in sight gives a zero row.  speaker_heads=None is
    the call without the arguments."""
    return _stream_chunk("attention_stream_chunk", q, k, v, kcache, vcache, None, kcache.shape[0], kcache.shape[2], lengths, new, H, T, ring,
                         bf16, bias, speakers, speaker_cache, speaker_heads)


def attention_stream_pools(n_pages: int, H: int, hd: int, page_rows: int = 16, bf16: bool = False, device="cuda", fill: float = 0.0):
    """(kpool, vpool) of one paged streaming-attention site: tensors [n_pages, H, page_rows, pad(hd)], fp32 (pad to 4) or bf16 (pad to
    8), filled with `fill`.  page_rows: 16, 32 or 64."""
    n = lib().m2f_attention_stream_pool_elems(n_pages, H, hd, page_rows, int(bf16))
    if n < 0:
        raise runtime.HipError("m2f_attention_stream_pool_elems: " + lib().m2f_last_error().decode())
    hdp = (hd + 7) // 8 * 8 if bf16 else (hd + 3) // 4 * 4
    dt = torch.bfloat16 if bf16 else torch.float32
    return tuple(torch.full((n_pages, H, page_rows, hdp), fill, dtype=dt, device=device) for _ in range(2))


def _paged_args(who: str, kpool, vpool, table, S: int, capacity: int, bf16: bool):
    """(n_pages, page_rows) of a pool pair after the checks that need tensors; sizes and alignment are the library's to refuse."""
    want = torch.bfloat16 if bf16 else torch.float32
    if kpool.dtype != want or vpool.dtype != want or kpool.dim() != 4 or kpool.shape != vpool.shape:
        raise ValueError(f"{who}: the pools must be two " + ("bfloat16" if bf16 else "float32") + " tensors [n_pages, H, page_rows, pad(hd)]")
    if not kpool.is_contiguous() or not vpool.is_contiguous():
        raise ValueError(f"{who}: the pools must be contiguous")
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[0] != S or not table.is_contiguous():
        raise ValueError(f"{who}: the page table must be a contiguous int32 tensor [S, ceil(capacity / page_rows)]")
    return kpool.shape[0], kpool.shape[2]


def attention_stream_paged(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kpool: torch.Tensor, vpool: torch.Tensor, table: torch.Tensor,
                           lengths: torch.Tensor, active: torch.Tensor, H: int, capacity: int, ring: bool = False,
                           bf16: bool = False, weights: Optional[torch.Tensor] = None, bias: Optional[float] = None,
                           speakers: Optional[torch.Tensor] = None, speaker_cache: Optional[torch.Tensor] = None,
                           speaker_heads=None) -> torch.Tensor:
    """`attention_stream` over page pools (m2f_attn_stream_opts::table): logical cache row r of slot s - the row `attention_stream` calls r -
    is row r % page_rows of page table[s, r // page_rows].  kpool / vpool: `attention_stream_pools`; table int32 [S, ceil(capacity /
    page_rows)], read only at the entries of pages that hold a live row or take the new one.  The same bits as `attention_stream` on
    caches holding the same rows.  A refused argument raises before anything is launched.  Returns out [S, H*hd].
    weights: as `attention_stream` - the order is logical, so the rows are the dense launch's bits.
    bias: as `attention_stream`.  speakers / speaker_cache / speaker_heads: as `attention_stream` - speaker_cache stays the dense
    uint8 [S, capacity] array (logical rows: the page table never enters)."""
    return _stream_step("attention_stream_paged", q, k, v, kpool, vpool, table, capacity, lengths, active, H, ring, bf16, weights, bias,
                        speakers, speaker_cache, speaker_heads)


def attention_stream_chunk_paged(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kpool: torch.Tensor, vpool: torch.Tensor,
                                 table: torch.Tensor, lengths: torch.Tensor, new: torch.Tensor, H: int, T: int, capacity: int,
                                 ring: bool = False, bf16: bool = False, bias: Optional[float] = None,
                                 speakers: Optional[torch.Tensor] = None, speaker_cache: Optional[torch.Tensor] = None,
                                 speaker_heads=None) -> torch.Tensor:
    """`attention_stream_chunk` over page pools (m2f_attn_stream_opts::table; layout: `attention_stream_paged`).  q / k / v hold
    S * T rows, S = table.shape[0].  The same bits, output and stored rows, as the dense chunk launch.  Returns out [S*T, H*hd].
    bias: as `attention_stream_chunk`.  speakers / speaker_cache / speaker_heads: as `attention_stream_chunk`."""
    return _stream_chunk("attention_stream_chunk_paged", q, k, v, kpool, vpool, table, lengths.numel(), capacity, lengths, new, H, T, ring,
                         bf16, bias, speakers, speaker_cache, speaker_heads)


def _stream_cache_move(who: str, scatter: bool, kcache, vcache, hd: int, slots, lengths, row_offsets, packed, count, table, capacity, bf16):
    runtime.require_gpu()
    want = torch.bfloat16 if bf16 else torch.float32
    if kcache.dtype != want or vcache.dtype != want or kcache.dim() != 4 or kcache.shape != vcache.shape or not kcache.is_contiguous() \
            or not vcache.is_contiguous():
        raise ValueError(f"{who}: the caches must be two contiguous " + ("bfloat16" if bf16 else "float32") + " tensors of one 4-D shape")
    if packed.dtype != want or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError(f"{who}: packed must be a contiguous 1-D tensor of the caches' type")
    n = slots.numel()
    if slots.dtype != torch.int32 or lengths.dtype != torch.int32 or lengths.numel() != n or row_offsets.dtype != torch.int64 \
            or row_offsets.numel() != n:
        raise ValueError(f"{who}: slots int32 [n], lengths int32 [n] and row_offsets int64 [n] required")
    if scatter and (count is None or count.dtype != torch.int32):
        raise ValueError(f"{who}: count int32 [S] required")
    H = kcache.shape[1]
    tail = (ptr(count), stream_ptr()) if scatter else (stream_ptr(),)
    if table is None:
        S, C, paging = kcache.shape[0], kcache.shape[2], (None, 0, 0, 0)
    else:
        S, C = table.shape[0] if table.dim() == 2 else -1, capacity
        n_pages, R = _paged_args(who, kcache, vcache, table, S, capacity, bf16)
        paging = (ptr(table), table.shape[1], n_pages, R)
    if scatter and count.numel() != S:
        raise ValueError(f"{who}: count int32 [S] required")
    fn = lib().m2f_attention_stream_cache_scatter if scatter else lib().m2f_attention_stream_cache_gather
    check(fn(S, H, hd, ptr(kcache), ptr(vcache), *paging, C, int(bf16), n, ptr(slots), ptr(lengths), ptr(row_offsets), ptr(packed),
             packed.numel(), *tail), who)


def attention_stream_cache_gather(kcache: torch.Tensor, vcache: torch.Tensor, hd: int, slots: torch.Tensor, lengths: torch.Tensor,
                                  row_offsets: torch.Tensor, packed: torch.Tensor, table: Optional[torch.Tensor] = None,
                                  capacity: Optional[int] = None, bf16: bool = False) -> torch.Tensor:
    """One site's live cache rows -> `packed` (m2f_attention_stream_cache_gather, csrc/stream_cache.hip): entry e holds the
    min(lengths[e], capacity) physical rows 0 .. of slot slots[e] as [K, V][H][rows][pad(hd)] at element row_offsets[e] * 2 * H * pad(hd).
    kcache / vcache: `attention_stream_caches`, or with `table` (int32 [S, ceil(capacity / page_rows)]) and `capacity` the pools of
    `attention_stream_pools`.  slots, lengths int32 [n], row_offsets int64 [n] on the device.  Returns packed."""
    _stream_cache_move("attention_stream_cache_gather", False, kcache, vcache, hd, slots, lengths, row_offsets, packed, None, table, capacity, bf16)
    return packed


def attention_stream_cache_scatter(kcache: torch.Tensor, vcache: torch.Tensor, hd: int, slots: torch.Tensor, lengths: torch.Tensor,
                                   row_offsets: torch.Tensor, packed: torch.Tensor, count: torch.Tensor, table: Optional[torch.Tensor] = None,
                                   capacity: Optional[int] = None, bf16: bool = False) -> None:
    """The reverse of `attention_stream_cache_gather` (m2f_attention_stream_cache_scatter): `packed` -> the rows
    0 .. min(lengths[e], capacity) - 1 of slot slots[e], and count[slots[e]] = lengths[e]; nothing else is written."""
    _stream_cache_move("attention_stream_cache_scatter", True, kcache, vcache, hd, slots, lengths, row_offsets, packed, count, table, capacity, bf16)


def attention_bwd(q, k, v, key_pad, out, probs, dout, B: int, L: int, H: int, drop_site: int = 0, drop_p: float = 0.0,
                  rng: Optional[torch.Tensor] = None, past: Optional[int] = None,
                  future: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Backward of `attention_fwd` from its saved probabilities (which carry the band: past / future are the forward's)."""
    runtime.require_gpu()
    E = q.shape[1]
    hd = E // H
    dq, dk, dv = (torch.zeros(B * L, E, dtype=torch.float32, device=q.device) for _ in range(3))
    kp = key_pad.to(torch.uint8).contiguous()
    check(lib().m2f_attention_bwd(B, L, H, hd, ptr(q), _ld(q), ptr(k), _ld(k), ptr(v), _ld(v), ptr(kp), ptr(out),
                                  _ld(out), ptr(probs), ptr(dout), _ld(dout), ptr(dq), _ld(dq), ptr(dk), _ld(dk),
                                  ptr(dv), _ld(dv), drop_site, drop_p, ptr(rng), stream_ptr(),
                                  *runtime.context_band(past, future)), "m2f_attention_bwd")
    return dq, dk, dv


def _varlen_rows(cu: Optional[torch.Tensor], key_pad: Optional[torch.Tensor]):
    if (cu is None) == (key_pad is None):
        raise ValueError("give exactly one of cu (packed rows) and key_pad (padded rows)")
    cu32 = cu.to(torch.int32).contiguous() if cu is not None else None
    kp = key_pad.reshape(-1).to(torch.uint8).contiguous() if key_pad is not None else None
    return cu32, kp


def attention_varlen_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, B: int, L: int, H: int,
                         cu: Optional[torch.Tensor] = None, key_pad: Optional[torch.Tensor] = None, drop_site: int = 0,
                         drop_p: float = 0.0, rng: Optional[torch.Tensor] = None, past: Optional[int] = None,
                         future: Optional[int] = None, probs: Optional[torch.Tensor] = None, bias: Optional[float] = None,
                         speakers: Optional[torch.Tensor] = None, speaker_heads=None):
    """Long-dialogue attention (m2f_attention_varlen_fwd, L <= 512).  q/k/v: [T, H*hd] (possibly column slices) with either
    cu (int [B+1]: dialogue b = rows cu[b] .. cu[b+1]-1, T = q.shape[0]) or key_pad ([B, L] or [B*L], True = padded key;
    T = B*L).  Returns (out [T, H*hd], probs^T [B*H, Lp, Lp]).
    past / future: context band as in `attention_fwd`, over utterance positions inside the dialogue (packed: row minus cu[b]).  Pairs
    of 64-row blocks that the band hides as a whole are skipped: their part of the probabilities buffer is NOT written (zeros in
    the fresh buffer made here; whatever it held in a buffer passed as `probs`), and `attention_varlen_bwd` given the same band
    does not read it.
    bias: gain of the distance-decay bias (`position_bias_slopes`; None or 0 = off, the entries called without it): a visible key's
    score gets -slope(h, H, gain) * |i - j|, the gain applied as `runtime.position_bias` rounds it.
    speakers / speaker_heads: as `attention_fwd` - speakers holds one id per TOKEN ROW, in the rows' order ([T]; padded rows: [B, L]).
    No block pair is skipped on their account: every element of a visited block is written, a hidden one as 0."""
    runtime.require_gpu()
    T, E = q.shape
    opts = _attn_opts("attention_varlen_fwd", H, T, q.device, past, future, bias, speakers, speaker_heads)
    hd = E // H
    cu32, kp = _varlen_rows(cu, key_pad)
    out = torch.empty(T, E, dtype=torch.float32, device=q.device)
    Lp = 16 * ((L + 15) // 16)
    if probs is None:
        probs = torch.zeros(B * H, Lp, Lp, dtype=torch.float32, device=q.device)
    assert probs.shape == (B * H, Lp, Lp) and probs.is_contiguous() and probs.dtype == torch.float32 and probs.is_cuda
    check(lib().m2f_attention_varlen_fwd(B, L, H, hd, ptr(q), _ld(q), ptr(k), _ld(k), ptr(v), _ld(v), ptr(cu32), T, ptr(kp), ptr(out), _ld(out),
                                         ptr(probs), drop_site, drop_p, ptr(rng), stream_ptr(), ctypes.byref(opts)), "m2f_attention_varlen_fwd")
    return out, probs


def attention_varlen_bwd(q, k, v, out, probs, dout, B: int, L: int, H: int, cu: Optional[torch.Tensor] = None,
                         key_pad: Optional[torch.Tensor] = None, drop_site: int = 0, drop_p: float = 0.0,
                         rng: Optional[torch.Tensor] = None, past: Optional[int] = None,
                         future: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Backward of `attention_varlen_fwd` from its saved probabilities: (dq, dk, dv), each [T, H*hd].  past / future: the band of that
    forward (the block pairs it skipped are skipped here)."""
    runtime.require_gpu()
    T, E = q.shape
    hd = E // H
    cu32, kp = _varlen_rows(cu, key_pad)
    dq, dk, dv = (torch.zeros(T, E, dtype=torch.float32, device=q.device) for _ in range(3))
    check(lib().m2f_attention_varlen_bwd(B, L, H, hd, ptr(q), _ld(q), ptr(k), _ld(k), ptr(v), _ld(v), ptr(cu32), T, ptr(kp),
                                         ptr(out), _ld(out), ptr(probs), ptr(dout), _ld(dout), ptr(dq), _ld(dq), ptr(dk),
                                         _ld(dk), ptr(dv), _ld(dv), drop_site, drop_p, ptr(rng), stream_ptr(),
                                         *runtime.context_band(past, future)), "m2f_attention_varlen_bwd")
    return dq, dk, dv


def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, res: Optional[torch.Tensor] = None,
                  eps: float = 1e-5):
    runtime.require_gpu()
    T, d = x.shape
    out = torch.empty_like(x)
    stats = torch.empty(T, 2, dtype=torch.float32, device=x.device)
    check(lib().m2f_layernorm_fwd(T, d, ptr(x), ptr(gamma), ptr(beta), ptr(res), ptr(out), ptr(stats), eps,
                                  stream_ptr()), "m2f_layernorm_fwd")
    return out, stats


def layernorm_bwd(x, gamma, stats, dy, extra: Optional[torch.Tensor] = None):
    runtime.require_gpu()
    T, d = x.shape
    dx = torch.empty_like(x)
    partial = torch.empty((T + 3) // 4, 2, d, dtype=torch.float32, device=x.device)
    dg = torch.empty(d, dtype=torch.float32, device=x.device)
    db = torch.empty(d, dtype=torch.float32, device=x.device)
    check(lib().m2f_layernorm_bwd(T, d, ptr(x), ptr(gamma), ptr(stats), ptr(dy), ptr(extra), ptr(dx), ptr(partial),
                                  ptr(dg), ptr(db), stream_ptr()), "m2f_layernorm_bwd")
    return dx, dg, db


def layernorm_fwd_drop(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, res: Optional[torch.Tensor] = None,
                       eps: float = 1e-5, drop_site: int = 0, drop_p: float = 0.0, rng: Optional[torch.Tensor] = None):
    """dropout_site((res ? res : 0) + LayerNorm(x)) on [T, d] rows that may be column blocks of wider buffers (x, res and the
    result share one row stride; the result has x's).  Returns (out, stats)."""
    runtime.require_gpu()
    T, d = x.shape
    ld = _ld(x)
    assert res is None or _ld(res) == ld
    out = torch.zeros(T, ld, dtype=torch.float32, device=x.device)[:, :d]
    stats = torch.empty(T, 2, dtype=torch.float32, device=x.device)
    check(lib().m2f_layernorm_fwd_drop(T, d, ld, ptr(x), ptr(gamma), ptr(beta), ptr(res), ptr(out), ptr(stats), eps, drop_site,
                                       drop_p, ptr(rng), stream_ptr()), "m2f_layernorm_fwd_drop")
    return out, stats


def layernorm_bwd_masked(x, gamma, stats, dy, extra: Optional[torch.Tensor] = None, drop_site2: int = 0, drop_p: float = 0.0,
                         rng: Optional[torch.Tensor] = None):
    """LayerNorm backward with its second output: (dx = LNbwd(dy) (+ extra), dx_masked = LNbwd(dy) * keep(site2) / (1 - p),
    dgamma, dbeta); x, dy, extra share one row stride, dx and dx_masked get it too."""
    runtime.require_gpu()
    T, d = x.shape
    ld = _ld(x)
    assert _ld(dy) == ld and (extra is None or _ld(extra) == ld)
    dx = torch.zeros(T, ld, dtype=torch.float32, device=x.device)[:, :d]
    dxm = torch.zeros(T, ld, dtype=torch.float32, device=x.device)[:, :d]
    partial = torch.empty((T + 3) // 4, 2, d, dtype=torch.float32, device=x.device)
    dg = torch.empty(d, dtype=torch.float32, device=x.device)
    db = torch.empty(d, dtype=torch.float32, device=x.device)
    check(lib().m2f_layernorm_bwd_masked(T, d, ld, ptr(x), ptr(gamma), ptr(stats), ptr(dy), ptr(extra), ptr(dx), ptr(dxm),
                                         ptr(partial), ptr(dg), ptr(db), drop_site2, drop_p, ptr(rng), stream_ptr()),
          "m2f_layernorm_bwd_masked")
    return dx, dxm, dg, db


def dropout_rows(x: torch.Tensor, site: int, drop_p: float, rng: torch.Tensor, x2: Optional[torch.Tensor] = None,
                 site2: int = 0) -> None:
    """In place x[t, c] *= keep(site, t * d + c) / (1 - p) on [T, d] rows (stride ld >= d); x2: a second buffer of the same shape
    and stride with its own site, same launch."""
    runtime.require_gpu()
    T, d = x.shape
    assert x2 is None or (x2.shape == x.shape and _ld(x2) == _ld(x))
    check(lib().m2f_dropout_rows(ptr(x), ptr(x2), T, d, _ld(x), site, site2, drop_p, ptr(rng), stream_ptr()), "m2f_dropout_rows")


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor, class_w: Optional[torch.Tensor] = None,
                  label_smoothing: float = 0.1, normalise: bool = True):
    """logits [T, C], labels int64 [T] (-1 = ignore) -> (loss_out[4] = loss, den, num, -; dlogits [T, C])."""
    runtime.require_gpu()
    T, C = logits.shape
    terms = torch.empty(T, 2, dtype=torch.float32, device=logits.device)
    dl = torch.empty(T, C, dtype=torch.float32, device=logits.device)
    out = torch.zeros(4, dtype=torch.float32, device=logits.device)
    check(lib().m2f_cross_entropy(T, C, ptr(logits.contiguous()), ptr(labels.contiguous()), ptr(class_w),
                                  label_smoothing, int(normalise), ptr(terms), ptr(dl), ptr(out), stream_ptr()),
          "m2f_cross_entropy")
    return out, dl


def cross_entropy_distill(logits: torch.Tensor, teacher: torch.Tensor, labels: torch.Tensor, class_w: Optional[torch.Tensor] = None,
                          label_smoothing: float = 0.1, alpha: float = 0.5, temperature: float = 2.0, normalise: bool = True):
    """The distillation criterion (m2f_cross_entropy_distill): logits, teacher [T, C] fp32, labels int64 [T] (-1 = ignore) ->
    (loss_out[4] = loss, den, num, -; dlogits [T, C]) of (1 - alpha) * cross entropy + alpha * temperature^2 * KL(softmax(teacher /
    temperature) || softmax(logits / temperature)), both over the labelled rows with ONE denominator (sum of w_y).  alpha = 0 gives
    `cross_entropy`'s bits."""
    runtime.require_gpu()
    T, C = logits.shape
    if teacher.shape != logits.shape or teacher.dtype != torch.float32 or logits.dtype != torch.float32:
        raise ValueError(f"cross_entropy_distill: logits and teacher must be fp32 of one shape (got {tuple(logits.shape)} {logits.dtype}, "
                         f"{tuple(teacher.shape)} {teacher.dtype})")
    terms = torch.empty(T, 2, dtype=torch.float32, device=logits.device)
    dl = torch.empty(T, C, dtype=torch.float32, device=logits.device)
    out = torch.zeros(4, dtype=torch.float32, device=logits.device)
    hyper = torch.tensor([float(alpha), float(temperature)], dtype=torch.float32).to(logits.device, non_blocking=True)
    check(lib().m2f_cross_entropy_distill(T, C, ptr(logits.contiguous()), ptr(teacher.contiguous()), ptr(labels.contiguous()), ptr(class_w),
                                          label_smoothing, ptr(hyper), int(normalise), ptr(terms), ptr(dl), ptr(out), stream_ptr()),
          "m2f_cross_entropy_distill")
    return out, dl


def cross_entropy_focal(logits: torch.Tensor, labels: torch.Tensor, class_w: Optional[torch.Tensor] = None, label_smoothing: float = 0.1,
                        gamma: float = 2.0, normalise: bool = True, teacher: Optional[torch.Tensor] = None, alpha: float = 0.0,
                        temperature: float = 1.0):
    """The focal criterion (m2f_cross_entropy_focal): logits [T, C] fp32, labels int64 [T] (-1 = ignore) -> (loss_out[4] = loss, den,
    num, -; dlogits [T, C]) of the cross entropy with every labelled row's hard-label term scaled by (1 - p_y)^gamma, over the ONE
    denominator (sum of w_y).  gamma: a finite number in [0, 8] (ValueError otherwise); 0 gives `cross_entropy`'s bits.  teacher [T, C]
    fp32 with alpha, temperature adds the blend of `cross_entropy_distill` (the factor scales the hard-label term only; gamma = 0 then
    gives `cross_entropy_distill`'s bits)."""
    gamma = runtime.check_focal_gamma(gamma, "gamma", "cross_entropy_focal")
    runtime.require_gpu()
    T, C = logits.shape
    if logits.dtype != torch.float32:
        raise ValueError(f"cross_entropy_focal: logits must be fp32 (got {logits.dtype})")
    if teacher is not None and (teacher.shape != logits.shape or teacher.dtype != torch.float32):
        raise ValueError(f"cross_entropy_focal: logits and teacher must be fp32 of one shape (got {tuple(logits.shape)} {logits.dtype}, "
                         f"{tuple(teacher.shape)} {teacher.dtype})")
    terms = torch.empty(T, 2, dtype=torch.float32, device=logits.device)
    dl = torch.empty(T, C, dtype=torch.float32, device=logits.device)
    out = torch.zeros(4, dtype=torch.float32, device=logits.device)
    hyper = torch.tensor([float(alpha), float(temperature), gamma], dtype=torch.float32).to(logits.device, non_blocking=True)
    logits, labels = logits.contiguous(), labels.contiguous()
    teacher = teacher.contiguous() if teacher is not None else None
    check(lib().m2f_cross_entropy_focal(T, C, ptr(logits), ptr(teacher), ptr(labels), ptr(class_w), label_smoothing, ptr(hyper),
                                        ptr(hyper[2:]), int(normalise), ptr(terms), ptr(dl), ptr(out), stream_ptr()),
          "m2f_cross_entropy_focal")
    return out, dl


def _crf_dialogues(who: str, T: int, batch: Optional[int], cu_seqlens: Optional[torch.Tensor]):
    """(B, L, cu) of a CRF launch: `cu_seqlens` int32 [B + 1] on the device (dialogue b owns rows cu[b] .. cu[b+1]-1), or `batch`
    dialogues of T // batch rows each."""
    if cu_seqlens is not None:
        if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2:
            raise ValueError(f"{who}: cu_seqlens must be int32 [B + 1] (got {tuple(cu_seqlens.shape)} {cu_seqlens.dtype})")
        return cu_seqlens.numel() - 1, 0, cu_seqlens.contiguous()
    if batch is None or batch < 1 or T % batch:
        raise ValueError(f"{who}: without cu_seqlens, batch must divide the {T} rows (got batch={batch!r})")
    return batch, T // batch, None


def _crf_params(who: str, params: torch.Tensor, C: int) -> torch.Tensor:
    if not 2 <= C <= 16:
        raise ValueError(f"{who}: 2 <= C <= 16 required (got C = {C})")
    if params.dtype != torch.float32 or params.numel() != C * C + 2 * C:
        raise ValueError(f"{who}: params must be fp32 of C*C + 2*C = {C * C + 2 * C} elements "
                         f"[transitions | start | end] (got {params.numel()} {params.dtype})")
    return params.contiguous()


def crf_nll(logits: torch.Tensor, labels: torch.Tensor, params: torch.Tensor, batch: Optional[int] = None,
            cu_seqlens: Optional[torch.Tensor] = None, normalise: bool = True, param_grad: bool = True, logit_grad: bool = True):
    """Linear-chain CRF loss (m2f_crf_nll): logits [T, C] fp32, labels int64 [T] (-1 = off the chain), params fp32 [C*C + 2C] =
    [transitions | start | end]; dialogues by `cu_seqlens` (int32 [B + 1]) or `batch` equal spans of T // batch rows.
    -> (loss_out[4] = loss, den, num, -; dlogits [T, C]; dparams [C*C + 2C] or None with param_grad=False; loss_terms [T, 2]).
    logit_grad=False (with param_grad=False): the loss alone - the forward sweep, no dlogits (None)."""
    runtime.require_gpu()
    T, C = logits.shape
    if logits.dtype != torch.float32:
        raise ValueError(f"crf_nll: logits must be fp32 (got {logits.dtype})")
    params = _crf_params("crf_nll", params, C)
    B, L, cu = _crf_dialogues("crf_nll", T, batch, cu_seqlens)
    dev = logits.device
    scratch = torch.empty(int(lib().m2f_crf_scratch_floats(T, B, C)), dtype=torch.float32, device=dev)
    terms = torch.empty(T, 2, dtype=torch.float32, device=dev)
    if param_grad and not logit_grad:
        raise ValueError("crf_nll: param_grad needs logit_grad (the parameter gradient comes out of the backward sweep)")
    dl = torch.empty(T, C, dtype=torch.float32, device=dev) if logit_grad else None
    out = torch.zeros(4, dtype=torch.float32, device=dev)
    dp = torch.empty(C * C + 2 * C, dtype=torch.float32, device=dev) if param_grad else None
    logits, labels = logits.contiguous(), labels.contiguous()
    check(lib().m2f_crf_nll(T, C, B, L, ptr(cu), ptr(logits), ptr(labels), ptr(params), int(normalise), ptr(scratch), ptr(terms),
                            ptr(dl), ptr(dp), ptr(out), stream_ptr()), "m2f_crf_nll")
    return out, dl, dp, terms


def crf_viterbi(logits: torch.Tensor, mask: torch.Tensor, params: torch.Tensor, batch: Optional[int] = None,
                cu_seqlens: Optional[torch.Tensor] = None):
    """Viterbi path (m2f_crf_viterbi): logits [T, C] fp32, mask bool / uint8 [T] (True = off the chain) -> (pred int32 [T], -1 off the
    chain; score fp32 [B]).  The lowest class wins every tie."""
    runtime.require_gpu()
    T, C = logits.shape
    if logits.dtype != torch.float32:
        raise ValueError(f"crf_viterbi: logits must be fp32 (got {logits.dtype})")
    params = _crf_params("crf_viterbi", params, C)
    B, L, cu = _crf_dialogues("crf_viterbi", T, batch, cu_seqlens)
    dev = logits.device
    mask = mask.reshape(-1).to(torch.uint8).contiguous()
    if mask.numel() != T:
        raise ValueError(f"crf_viterbi: mask must have {T} elements (got {mask.numel()})")
    scratch = torch.empty(5 * T, dtype=torch.int32, device=dev)
    pred = torch.empty(T, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    logits = logits.contiguous()
    check(lib().m2f_crf_viterbi(T, C, B, L, ptr(cu), ptr(logits), ptr(mask), ptr(params), ptr(scratch), ptr(pred), ptr(score),
                                stream_ptr()), "m2f_crf_viterbi")
    return pred, score


def crf_filter(logits: torch.Tensor, params: torch.Tensor, phi: torch.Tensor, count: torch.Tensor,
               active: Optional[torch.Tensor] = None, n_new: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Forward filter (m2f_crf_filter), IN PLACE on phi [S, C] fp32: logits [S, C] (one row per active slot) or [S, rows, C] with
    n_new int32 [S] (slot s takes its first n_new[s] rows in order); count int32 [S] = utterances the slot held before the call (read
    only); active bool / uint8 [S] or None (all).  Returns phi."""
    runtime.require_gpu()
    S, C = phi.shape
    rows = 1 if logits.dim() == 2 else logits.shape[1]
    if logits.dtype != torch.float32 or phi.dtype != torch.float32 or not phi.is_contiguous() or logits.numel() != S * rows * C:
        raise ValueError(f"crf_filter: logits [S, C] or [S, rows, C] and a contiguous phi [S, C], both fp32, required "
                         f"(got {tuple(logits.shape)} {logits.dtype}, {tuple(phi.shape)} {phi.dtype})")
    params = _crf_params("crf_filter", params, C)
    if count.dtype != torch.int32 or count.numel() != S or (n_new is not None and (n_new.dtype != torch.int32 or n_new.numel() != S)):
        raise ValueError("crf_filter: count and n_new must be int32 [S]")
    if rows > 1 and n_new is None:
        raise ValueError("crf_filter: logits [S, rows, C] need n_new")
    active = active.reshape(-1).to(torch.uint8).contiguous() if active is not None else None
    logits, count = logits.contiguous(), count.contiguous()
    n_new = n_new.contiguous() if n_new is not None else None
    check(lib().m2f_crf_filter(S, C, rows, ptr(logits), ptr(params), ptr(count), ptr(active), ptr(n_new), ptr(phi), stream_ptr()),
          "m2f_crf_filter")
    return phi


def cross_entropy_rdrop(logits: torch.Tensor, partner: torch.Tensor, labels: torch.Tensor, class_w: Optional[torch.Tensor] = None,
                        label_smoothing: float = 0.1, alpha: float = 1.0, normalise: bool = True):
    """The R-Drop criterion (m2f_cross_entropy_rdrop): logits [T, C] fp32, partner int32 [T] (the twin ROW of every row - the same
    utterance under another dropout mask -, or -1), labels int64 [T] (-1 = ignore) -> (loss_out[4] = loss, den, num, kl; dlogits [T, C]) of
    the cross entropy plus alpha * w_y * 0.5 * (KL(p || q) + KL(q || p)) on every labelled row with a twin, over the ONE denominator
    (sum of w_y).  kl = sum of w_y * s_r WITHOUT alpha: loss = CE share + alpha * kl / den.  alpha: a finite number >= 0 (ValueError
    otherwise); 0 gives `cross_entropy`'s bits.  The map must pair rows of one label (``runtime.rdrop_partner`` builds it)."""
    alpha = runtime.check_rdrop_alpha(alpha, "alpha", "cross_entropy_rdrop")
    runtime.require_gpu()
    T, C = logits.shape
    if logits.dtype != torch.float32:
        raise ValueError(f"cross_entropy_rdrop: logits must be fp32 (got {logits.dtype})")
    if partner.shape != (T,) or partner.dtype != torch.int32 or partner.device != logits.device:
        raise ValueError(f"cross_entropy_rdrop: partner must be int32 [{T}] on {logits.device} (got {tuple(partner.shape)} {partner.dtype} "
                         f"on {partner.device})")
    terms = torch.empty(T, 3, dtype=torch.float32, device=logits.device)
    dl = torch.empty(T, C, dtype=torch.float32, device=logits.device)
    out = torch.zeros(4, dtype=torch.float32, device=logits.device)
    a = torch.tensor([alpha], dtype=torch.float32).to(logits.device, non_blocking=True)
    logits, labels, partner = logits.contiguous(), labels.contiguous(), partner.contiguous()
    check(lib().m2f_cross_entropy_rdrop(T, C, ptr(logits), ptr(partner), ptr(labels), ptr(class_w), label_smoothing, ptr(a),
                                        int(normalise), ptr(terms), ptr(dl), ptr(out), stream_ptr()), "m2f_cross_entropy_rdrop")
    return out, dl


def supcon(features: torch.Tensor, labels: torch.Tensor, class_w: Optional[torch.Tensor] = None, weight: float = 1.0,
           temperature: float = 0.1, n_classes: Optional[int] = None):
    """The supervised contrastive kernels on their own (m2f_supcon; csrc/supcon.hip holds the definition).  features: fp32 [N, D], rows
    contiguous (a row stride > D is read in place); labels int64 [N] (a label outside [0, n_classes) = not contrasted); class_w fp32
    [n_classes] or None; n_classes defaults to class_w's length, else to 1 + the largest label (one host read).  -> (row_terms [N, 4] =
    (lse_i, n_i, l_i, w_y l_i), dfeatures [N, D] = the gradient of ``weight * sum_i w_y l_i`` w.r.t. features, unnormalised).  Rows
    without a valid label or with a zero norm, and anchors without a positive, give exactly 0.  weight finite >= 0, temperature finite
    > 0 (ValueError otherwise).  Exact fp32, no atomics: the same bits at every call."""
    w, t = runtime.check_supcon_pair((weight, temperature), "(weight, temperature)", "supcon")
    runtime.require_gpu()
    if features.dim() != 2 or features.dtype != torch.float32 or features.stride(1) != 1 or features.stride(0) < features.shape[1]:
        raise ValueError(f"supcon: features must be fp32 [N, D] with contiguous rows (got {tuple(features.shape)} {features.dtype}, "
                         f"strides {features.stride()})")
    N, D = features.shape
    if labels.shape != (N,) or labels.dtype != torch.int64 or labels.device != features.device:
        raise ValueError(f"supcon: labels must be int64 [{N}] on {features.device} (got {tuple(labels.shape)} {labels.dtype} on {labels.device})")
    if class_w is not None:
        class_w = class_w.to(device=features.device, dtype=torch.float32).contiguous()
    C = int(n_classes) if n_classes is not None else (class_w.numel() if class_w is not None else max(int(labels.max()) + 1, 1))
    if class_w is not None and class_w.numel() < C:
        raise ValueError(f"supcon: class_w holds {class_w.numel()} weights for {C} classes")
    dev = features.device
    scratch = torch.empty(int(lib().m2f_supcon_scratch_floats(N, D)), dtype=torch.float32, device=dev)
    rows = torch.empty(N, 4, dtype=torch.float32, device=dev)
    dfeat = torch.empty(N, D, dtype=torch.float32, device=dev)
    hyper = torch.tensor([w, t], dtype=torch.float32).to(dev, non_blocking=True)
    labels = labels.contiguous()
    check(lib().m2f_supcon(N, D, C, ptr(features), features.stride(0), ptr(labels), ptr(class_w), ptr(hyper), ptr(scratch), ptr(rows),
                           ptr(dfeat), D, stream_ptr()), "m2f_supcon")
    return rows, dfeat


def _adv_rows(t: torch.Tensor, d: int) -> Tuple[torch.Tensor, bool]:
    """[T, d] fp32 rows as the adversarial kernels read them - 16-byte aligned rows of a stride that is a multiple of 4 -: the tensor
    itself when it is such a view, else a copy in such a buffer (and True: results travel back)."""
    if t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= (d + 3) // 4 * 4 and t.data_ptr() % 16 == 0:
        return t, False
    buf = torch.zeros(t.shape[0], (d + 7) // 8 * 8, dtype=torch.float32, device=t.device)
    buf[:, :d] = t
    return buf[:, :d], True


def adversarial_ascend(x_clean: torch.Tensor, g: Optional[torch.Tensor], delta: torch.Tensor, x: Optional[torch.Tensor] = None,
                       key_pad: Optional[torch.Tensor] = None, epsilon: float = 1.0, step_size: Optional[float] = None,
                       norm: str = "utterance"):
    """One ascent step of embedding-space adversarial training on its own (m2f_adv_ascend; csrc/adversarial.hip holds the definition):
    ``u = g / ||g||``, ``cand = delta + step_size * u`` (a zero or non-finite norm: ``cand = delta``), ``delta <- cand * min(1, epsilon
    / ||cand||)``, ``x <- x_clean + delta``; the norm is each row's L2 norm ("utterance") or the L2 norm over all rows that are not
    padding ("batch").  x_clean, g, delta, x: fp32 ``[..., d]`` of one shape on one device, the leading dimensions are the rows; g None
    = a zero gradient (the projection alone).  key_pad (bool / uint8, the leading shape; True = padding): those rows are neither read for
    a norm nor written.  delta is updated IN PLACE and x written (allocated when None: padding rows then hold x_clean); returns
    ``(delta, x)``.  Rows that are 16-byte aligned views with a stride that is a multiple of 4 (``buf[:, :d]`` of a padded buffer) are
    used in place - the columns behind d are never written -, anything else through a copy.  step_size None = epsilon.  Sums of squares
    in float64 in a fixed order, no atomics: the same bits at every call."""
    eps, step, _ = runtime.check_adv_hyper(epsilon, step_size, 0.0, "adversarial_ascend")
    kind = runtime.adv_norm_kind(norm, "adversarial_ascend")
    runtime.require_gpu()
    dev, shape = x_clean.device, x_clean.shape
    if x is None:
        x = x_clean.clone()
    for name, t in (("x_clean", x_clean), ("g", g), ("delta", delta), ("x", x)):
        if t is None and name == "g":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.shape != shape or t.device != dev or t.dim() < 2:
            raise ValueError(f"adversarial_ascend: {name} must be fp32 {tuple(shape)} on {dev} like x_clean (at least 2-D)")
    d = shape[-1]
    T = x_clean.numel() // d
    if T < 1 or d < 1:
        raise ValueError(f"adversarial_ascend: at least one row and one column required, got {tuple(shape)}")
    if key_pad is None:
        skip = torch.zeros(T, dtype=torch.uint8, device=dev)
    else:
        if key_pad.shape != shape[:-1] or key_pad.device != dev:
            raise ValueError(f"adversarial_ascend: key_pad must be {tuple(shape[:-1])} on {dev}, got {tuple(key_pad.shape)} on {key_pad.device}")
        skip = key_pad.reshape(T).to(torch.uint8).contiguous()

    def rows(t):
        t2 = t if t.dim() == 2 else t.reshape(T, d)          # (a view whenever the leading dimensions are contiguous; else a copy)
        r, copied = _adv_rows(t2, d)
        return r, copied or (t2.data_ptr() != t.data_ptr())

    xc, _ = rows(x_clean)
    gr = None if g is None else rows(g)[0]
    dl, dl_back = rows(delta)
    xo, xo_back = rows(x)
    scratch = torch.empty(int(lib().m2f_adv_scratch_bytes(T)) // 8, dtype=torch.float64, device=dev) if kind else None
    hyper = torch.tensor([eps, step], dtype=torch.float32).to(dev, non_blocking=True)
    check(lib().m2f_adv_ascend(T, d, xc.stride(0), ptr(xc), ptr(gr), ptr(dl), ptr(xo), ptr(skip), ptr(hyper), kind, ptr(scratch),
                               stream_ptr()), "m2f_adv_ascend")
    if dl_back:
        delta.copy_(dl.reshape(shape))
    if xo_back:
        x.copy_(xo.reshape(shape))
    return delta, x


def adversarial_init(delta: torch.Tensor, init_mag: float, rng: torch.Tensor, site: int, key_pad: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The uniform start of a perturbation on its own (m2f_adv_init): ``delta[t, c] <- fp32(init_mag / sqrt(d)) * (2 * (h >> 8) * 2^-24 -
    1)`` IN PLACE over the rows that are not padding, h the dropout hash of element ``t * d + c`` under `site` and the state `rng` (int32
    [4] on the device).  delta: fp32 [T, d], rows as `adversarial_ascend` takes them (else through a copy)."""
    _, _, mag = runtime.check_adv_hyper(0.0, None, init_mag, "adversarial_init")
    runtime.require_gpu()
    if delta.dim() != 2 or delta.dtype != torch.float32:
        raise ValueError(f"adversarial_init: delta must be fp32 [T, d], got {tuple(delta.shape)} {delta.dtype}")
    T, d = delta.shape
    skip = (torch.zeros(T, dtype=torch.uint8, device=delta.device) if key_pad is None else key_pad.reshape(T).to(torch.uint8).contiguous())
    dl, back = _adv_rows(delta, d)
    check(lib().m2f_adv_init(T, d, dl.stride(0), ptr(dl), ptr(skip), mag, ptr(rng), int(site) & 0xFFFFFFFF, stream_ptr()), "m2f_adv_init")
    if back:
        delta.copy_(dl)
    return delta


def _aux_rows(features: torch.Tensor, who: str) -> torch.Tensor:
    """fp32 [N, D] feature rows as the auxiliary head's kernels read them: 16-byte aligned rows of a stride that is a multiple of 4
    (read in place when they are; else copied once into such a buffer)."""
    if features.dim() != 2 or features.dtype != torch.float32:
        raise ValueError(f"{who}: features must be fp32 [N, D] (got {tuple(features.shape)} {features.dtype})")
    N, D = features.shape
    if D < 1 or D > 1024:
        raise ValueError(f"{who}: 1 <= D <= 1024 feature columns required (got {D})")
    if N > 0 and features.stride(1) == 1 and features.stride(0) >= (D + 3) // 4 * 4 and features.stride(0) % 4 == 0 and features.data_ptr() % 16 == 0:
        return features
    buf = torch.zeros(N, (D + 3) // 4 * 4, dtype=torch.float32, device=features.device)
    buf[:, :D] = features
    return buf[:, :D]


def _aux_block(params: torch.Tensor, D: int, who: str) -> int:
    """The class count of a head's block [W (A x D) | b (A)]; ValueError unless it is fp32, contiguous, 16-byte aligned, 2 <= A <= 16."""
    if params.dim() != 1 or params.dtype != torch.float32 or not params.is_contiguous() or params.data_ptr() % 16:
        raise ValueError(f"{who}: params must be one contiguous, 16-byte aligned fp32 block [W | b] (got {tuple(params.shape)} {params.dtype})")
    A, rest = divmod(params.numel(), D + 1)
    if rest or not 2 <= A <= 16:
        raise ValueError(f"{who}: params holds {params.numel()} floats: A * {D} + A with 2 <= A <= 16 expected")
    return A


def aux_head(features: torch.Tensor, labels: torch.Tensor, aux_labels: torch.Tensor, params: torch.Tensor,
             hyper: Tuple[float, float] = (1.0, 0.0), class_weights: Optional[torch.Tensor] = None, n_classes: Optional[int] = None):
    """The auxiliary label head's kernels on their own (m2f_aux_head; csrc/aux_head.hip holds the definition).  features: fp32 [N, D];
    labels / aux_labels int64 [N] (the primary and the second label; a row with either outside its range is ignored); params: the head's
    fp32 block [W (A x D) | b (A)]; hyper = (weight, label smoothing of the auxiliary term); class_weights: the PRIMARY classes' weights
    or None; n_classes defaults to their count, else to 1 + the largest primary label (one host read).
    -> (aux_logits [N, A] = W h + b for every row, row_terms [N] = w_y a_i, dfeatures [N, D] and dparams [A D + A] = the gradient of
    ``weight * sum_i w_y a_i`` w.r.t. features (no gate) and the block, unnormalised).  Ignored rows give exact zeros in the last three,
    whatever their features hold.  Exact fp32, no atomics: the same bits at every call."""
    from .aux_head import check_pair
    w, eps = check_pair(hyper[0], hyper[1], "aux_head")
    runtime.require_gpu()
    feat = _aux_rows(features, "aux_head")
    N, D = feat.shape
    A = _aux_block(params, D, "aux_head")
    dev = feat.device
    for name, t in (("labels", labels), ("aux_labels", aux_labels)):
        if t.shape != (N,) or t.dtype != torch.int64 or t.device != dev:
            raise ValueError(f"aux_head: {name} must be int64 [{N}] on {dev} (got {tuple(t.shape)} {t.dtype} on {t.device})")
    if class_weights is not None:
        class_weights = class_weights.to(device=dev, dtype=torch.float32).contiguous()
    C = int(n_classes) if n_classes is not None else (class_weights.numel() if class_weights is not None else max(int(labels.max()) + 1, 1))
    if class_weights is not None and class_weights.numel() < C:
        raise ValueError(f"aux_head: class_weights holds {class_weights.numel()} weights for {C} classes")
    scratch = torch.empty(int(lib().m2f_aux_head_scratch_floats(N, D, A)), dtype=torch.float32, device=dev)
    logits = torch.empty(N, A, dtype=torch.float32, device=dev)
    rows = torch.empty(N, dtype=torch.float32, device=dev)
    ldd = (D + 3) // 4 * 4
    dfeat = torch.zeros(N, ldd, dtype=torch.float32, device=dev)
    dparams = torch.empty(A * D + A, dtype=torch.float32, device=dev)
    hyp = torch.tensor([w, eps], dtype=torch.float32).to(dev, non_blocking=True)
    labels, aux_labels = labels.contiguous(), aux_labels.contiguous()
    check(lib().m2f_aux_head(N, D, A, C, ptr(feat), feat.stride(0), ptr(params), ptr(labels), ptr(aux_labels), ptr(class_weights), ptr(hyp),
                             ptr(scratch), ptr(logits), ptr(rows), ptr(dfeat), ldd, ptr(dparams), stream_ptr()), "m2f_aux_head")
    return logits, rows, dfeat[:, :D], dparams


def aux_head_forward(features: torch.Tensor, params: torch.Tensor, num_classes: int) -> torch.Tensor:
    """logits [N, A] = W h + b of the head's block over fp32 feature rows [N, D] (m2f_aux_head_forward: the rows kernel without a label)."""
    runtime.require_gpu()
    feat = _aux_rows(features, "aux_head_forward")
    N, D = feat.shape
    A = _aux_block(params, D, "aux_head_forward")
    if A != num_classes:
        raise ValueError(f"aux_head_forward: the block holds {A} classes, {num_classes} expected")
    logits = torch.empty(N, A, dtype=torch.float32, device=feat.device)
    check(lib().m2f_aux_head_forward(N, D, A, ptr(feat), feat.stride(0), ptr(params), None, ptr(logits), stream_ptr()),
          "m2f_aux_head_forward")
    return logits


def aux_head_backward(features: torch.Tensor, params: torch.Tensor, g: torch.Tensor, num_classes: int, want_features: bool = True,
                      want_params: bool = True):
    """(dfeatures [N, D] = g W or None, dparams [A D + A] = [g^T h | sum_i g_i] or None) from an upstream gradient g [N, A]
    (m2f_aux_head_backward: the join and parameter-gradient kernels of the step)."""
    runtime.require_gpu()
    feat = _aux_rows(features, "aux_head_backward")
    N, D = feat.shape
    A = _aux_block(params, D, "aux_head_backward")
    if A != num_classes or g.shape != (N, A) or g.dtype != torch.float32 or not g.is_contiguous():
        raise ValueError(f"aux_head_backward: g must be contiguous fp32 [{N}, {A}] (got {tuple(g.shape)} {g.dtype})")
    dev = feat.device
    scratch = torch.empty(int(lib().m2f_aux_head_scratch_floats(N, D, A)), dtype=torch.float32, device=dev)
    ldd = (D + 3) // 4 * 4
    dfeat = torch.zeros(N, ldd, dtype=torch.float32, device=dev) if want_features else None
    dparams = torch.empty(A * D + A, dtype=torch.float32, device=dev) if want_params else None
    check(lib().m2f_aux_head_backward(N, D, A, ptr(feat), feat.stride(0), ptr(params), ptr(g), ptr(scratch), ptr(dfeat), ldd, ptr(dparams),
                                      stream_ptr()), "m2f_aux_head_backward")
    return (dfeat[:, :D] if want_features else None), dparams


def aux_head_join(dh: torch.Tensor, g: torch.Tensor, params: torch.Tensor, h: Optional[torch.Tensor] = None, scale: float = 1.0,
                  weight: float = 1.0, gate_scale: float = 1.0, add: bool = True, shadow: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The step's join launch on the caller's buffers (m2f_aux_head_join), IN PLACE: dh[i, :] = (add: dh[i, :] +) gate * scale * weight *
    sum_c g[i, c] W[c, :], gate = (h[i, :] > 0 ? gate_scale : 0) or (h None) 1.  dh / h: fp32 [N, D] views with 16-byte aligned rows of
    one stride each (a multiple of 4; ValueError otherwise - nothing is copied, the launch writes dh itself); g fp32 [N, A]; params the
    head's block.  shadow: an int16 tensor of N * dh.stride(0) elements that receives the bf16 bits (nearest even) of every dh element the
    launch writes - what the step does to the plan's activation shadow in bf16 mode.  -> dh."""
    runtime.require_gpu()
    for name, t in (("dh", dh), ("h", h)):
        if t is None:
            continue
        if (t.dim() != 2 or t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) % 4 or t.stride(0) < (t.shape[1] + 3) // 4 * 4
                or t.data_ptr() % 16 or t.shape != dh.shape):
            raise ValueError(f"aux_head_join: {name} must be fp32 {tuple(dh.shape)} with 16-byte aligned rows, row stride a multiple of 4 "
                             f"(got {tuple(t.shape)} {t.dtype}, strides {t.stride()})")
    N, D = dh.shape
    A = _aux_block(params, D, "aux_head_join")
    if g.dim() != 2 or g.shape != (N, A) or g.dtype != torch.float32 or g.stride(1) != 1:
        raise ValueError(f"aux_head_join: g must be fp32 [{N}, {A}] (got {tuple(g.shape)} {g.dtype})")
    if shadow is not None and (shadow.dtype != torch.int16 or shadow.numel() != N * dh.stride(0) or not shadow.is_contiguous()):
        raise ValueError(f"aux_head_join: shadow must be a contiguous int16 tensor of {N * dh.stride(0)} elements")
    dev = dh.device
    pair = torch.tensor([float(scale), float(weight)], dtype=torch.float32).to(dev, non_blocking=True)
    check(lib().m2f_aux_head_join(N, D, A, ptr(dh), dh.stride(0), ptr(h), h.stride(0) if h is not None else 0, ptr(g), g.stride(0), ptr(params),
                                  pair.data_ptr(), pair.data_ptr() + 4, float(gate_scale), int(bool(add)), ptr(shadow), stream_ptr()),
          "m2f_aux_head_join")
    return dh


def fam_layer_forward(text, audio, key_pad, in_w, in_b, out_w, out_b, lin_w, lin_b, n_head: int,
                      precision: int = runtime.F32, past: Optional[int] = None, future: Optional[int] = None,
                      need_weights: bool = False, bias: Optional[float] = None, speakers: Optional[torch.Tensor] = None,
                      speaker_heads=None):
    """FusionAttentionModule.forward (reference src/model.py:13-20), dropout = identity.  past / future: context band of its
    attention (`attention_fwd`); the reference has none.  need_weights: also the head-averaged attention map [B, L, L] that the
    reference's own call computes and drops (`attention_weights`).  bias: gain of the distance-decay bias of its attention
    (`attention_fwd`); None = off.  speakers ([B, L]) / speaker_heads: speaker heads of its attention
    (`attention_fwd`) - utterance i has one speaker as text query and as audio key."""
    B, L, E = text.shape
    t = text.reshape(B * L, E).contiguous()
    a = audio.reshape(B * L, E).contiguous()
    q = gemm(t, in_w[:E], NT, precision, bias=in_b[:E])
    k = gemm(a, in_w[E:2 * E], NT, precision, bias=in_b[E:2 * E])
    v = gemm(t, in_w[2 * E:], NT, precision, bias=in_b[2 * E:])
    if L > 64:          # (the dialogue kernels of attention_fwd hold L <= 64; above, the long-dialogue kernels, padded form)
        att, probs = attention_varlen_fwd(q, k, v, B, L, n_head, key_pad=key_pad, past=past, future=future, bias=bias,
                                          speakers=speakers, speaker_heads=speaker_heads)
    else:
        att, probs = attention_fwd(q, k, v, key_pad.reshape(-1), B, L, n_head, past=past, future=future, bias=bias,
                                   speakers=speakers, speaker_heads=speaker_heads)
    x = gemm(att, out_w, NT, precision, bias=out_b)
    y = gemm(x, lin_w[:, :E], NT, precision, a1=t, b1=lin_w[:, E:], bias=lin_b, relu_a=True, relu_out=True)
    if need_weights:
        return y.view(B, L, E), attention_weights(probs, B, L, n_head, key_pad=key_pad, past=past, future=future)
    return y.view(B, L, E)


# ---- wav2vec2 audio encoder kernels (wav2vec2.py) ------------------------------------------------------------------------------

def w2v_conv0(wave: torch.Tensor, w0: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, stride: int, P0: Optional[int] = None,
              bf16_out: bool = False, eps: float = 1e-5) -> torch.Tensor:
    """Conv1d(1, C, k0, stride, bias=False) + GroupNorm(C, C) + exact GELU of the padded batch wave [B, N]: rows b * P0 + t
    ([B * P0, C]; rows T0 .. P0-1 zero) as fp32, or as bf16 when bf16_out."""
    runtime.require_gpu()
    B, N = wave.shape
    C, k0 = w0.shape[0], w0.shape[-1]
    T0 = (N - k0) // stride + 1
    P0 = T0 if P0 is None else P0
    scratch = torch.empty(int(lib().m2f_w2v_conv0_scratch_floats(B, C, T0)), dtype=torch.float32, device=wave.device)
    out = torch.empty(B * P0, C, dtype=torch.bfloat16 if bf16_out else torch.float32, device=wave.device)
    check(lib().m2f_w2v_conv0(B, N, ptr(wave.contiguous()), ptr(w0.reshape(C, k0).contiguous()), k0, stride, C, T0, P0, ptr(gamma),
                              ptr(beta), eps, ptr(scratch), None if bf16_out else ptr(out), ptr(out) if bf16_out else None,
                              stream_ptr()), "m2f_w2v_conv0")
    return out


def w2v_conv_layer(x: torch.Tensor, w: torch.Tensor, stride: int, P_in: int, precision: int = runtime.F32,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One conv layer of the wav2vec2 front end (Conv1d(C, C, k, stride, bias=False) + exact GELU) on the grouped GEMM, the way
    wav2vec2.py runs it: x [rows >= B * P_in + 1, C] holds utterance b's frames at rows b * P_in + t (P_in a multiple of stride;
    the row behind the last pitch must exist: the last junk window reads it).  Returns [B * P_in / stride, C], output frame t of
    utterance b at row b * P_in / stride + t.  w [C, C, k] with stride <= k <= 2 * stride.  `out`: a contiguous [B * P_in / stride, C]
    buffer to write instead of a new one."""
    runtime.require_gpu()
    C, _, k = w.shape
    assert P_in % stride == 0 and stride <= k <= 2 * stride and x.is_contiguous() and x.shape[1] == C
    B = (x.shape[0] - 1) // P_in
    M, ld, K0, K1 = B * P_in // stride, stride * C, stride * C, (k - stride) * C
    weff = w.permute(0, 2, 1).reshape(C, k * C).float().contiguous()
    if out is None:
        out = torch.empty(M, C, dtype=torch.float32, device=x.device)
    assert out.shape == (M, C) and out.is_contiguous() and out.dtype == torch.float32
    bf16 = precision == runtime.BF16
    x16 = x.to(torch.bfloat16).contiguous() if bf16 else None
    w16 = weff.to(torch.bfloat16).contiguous() if bf16 else None
    a1 = x.data_ptr() + ld * 4 if K1 else None
    check(lib().m2f_gemm(precision, NT, M, C, K0, K1, ptr(x), ld, a1, ld if K1 else 0, ptr(weff), k * C,
                         weff.data_ptr() + K0 * 4 if K1 else None, k * C if K1 else 0, ptr(out), C, None, None, 0, None, 0, 1.0, None,
                         0, 0, 2, 0, 0, 0.0, None, 0, None, None, 0,
                         ptr(x16), ld if bf16 else 0, x16.data_ptr() + ld * 2 if bf16 and K1 else None, ld if bf16 and K1 else 0,
                         ptr(w16), k * C if bf16 else 0, w16.data_ptr() + K0 * 2 if bf16 and K1 else None, k * C if bf16 and K1 else 0,
                         stream_ptr()), "m2f_gemm (conv layer)")
    return out


def w2v_feat_layernorm(x: torch.Tensor, B: int, S: int, P: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5):
    """LayerNorm of rows b * P + t (t < S) of x [>= B * P, C] -> [B * S, C] (row b * S + t)."""
    runtime.require_gpu()
    C = x.shape[1]
    out = torch.empty(B * S, C, dtype=torch.float32, device=x.device)
    check(lib().m2f_w2v_feat_layernorm(B, S, P, C, ptr(x.contiguous()), ptr(gamma), ptr(beta), eps, ptr(out), None, stream_ptr()),
          "m2f_w2v_feat_layernorm")
    return out


def w2v_pack_pos_weight(w: torch.Tensor, groups: int, bf16: bool = False) -> torch.Tensor:
    """Conv1d(d, d, K, groups) weight [d, d / groups, K] (weight norm already folded) -> the kernel's [group][tap][o][c]."""
    d, CG, K = w.shape
    p = w.float().view(groups, CG, CG, K).permute(0, 3, 1, 2).contiguous()
    return p.to(torch.bfloat16).contiguous() if bf16 else p


def w2v_pos_conv(x: torch.Tensor, lengths: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, groups: int, B: int, S: int,
                 bf16: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B * S, d] -> x + GELU(grouped conv(x) + bias) with padding K / 2, the extra frame of an even K dropped, rows at or past
    lengths[b] of x read as zero (the residual too).  w [d, d / groups, K] fp32.  `out`: a contiguous fp32 buffer shaped like x to
    write instead of a new one."""
    runtime.require_gpu()
    d = x.shape[1]
    K = w.shape[2]
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.is_contiguous() and out.dtype == torch.float32
    wpk = w2v_pack_pos_weight(w, groups, bf16)
    l32 = lengths.to(x.device, torch.int32).contiguous()
    check(lib().m2f_w2v_pos_conv(B, S, d, groups, K, ptr(x.contiguous()), ptr(l32), ptr(wpk), ptr(bias), ptr(out), int(bf16),
                                 stream_ptr()), "m2f_w2v_pos_conv")
    return out


def w2v_masked_mean(x: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
    """x [B, S, d] -> [B, d]: mean over the first lengths[b] frames."""
    runtime.require_gpu()
    B, S, d = x.shape
    out = torch.empty(B, d, dtype=torch.float32, device=x.device)
    l32 = lengths.to(x.device, torch.int32).contiguous()
    check(lib().m2f_w2v_masked_mean(B, S, d, ptr(x.contiguous()), ptr(l32), ptr(out), stream_ptr()), "m2f_w2v_masked_mean")
    return out


def grad_norm(cfg, grads: torch.Tensor, max_norm: float, den: Optional[torch.Tensor] = None, grid: int = 0,
              nontemporal: Optional[bool] = None) -> torch.Tensor:
    """Global L2 norm of a flat gradient buffer of `cfg`'s parameter layout (fp32 or bf16, at least the layout's length; only
    parameter elements count, the pads between tensors may hold anything) and torch.nn.utils.clip_grad_norm_'s coefficient for
    `max_norm`: -> 4 fp32 values (norm = sqrt(sum of squares) / den, coef = min(1, max_norm / (norm + 1e-6)), divisor = den / coef,
    sqrt(sum of squares)); den: nullable device scalar, absent = 1.  `grid` / `nontemporal`: launch shape of the reduction; the
    result does not depend on them."""
    runtime.require_gpu()
    assert grads.is_cuda and grads.dim() == 1 and grads.is_contiguous() and grads.dtype in (torch.float32, torch.bfloat16)
    assert grads.numel() >= runtime.verify_layout(cfg), "the buffer is shorter than the configuration's flat parameter layout"
    scratch = runtime.grad_norm_scratch(cfg, grads.device)
    record = torch.zeros(4, dtype=torch.float32, device=grads.device)
    runtime.grad_sumsq(cfg, grads, scratch, 0, -1, grid, nontemporal)
    runtime.grad_norm_finalize(cfg, scratch, record, max_norm, den)
    return record
