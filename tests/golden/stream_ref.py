"""Reference for streaming inference (M2FNet.stream, streaming.DialogueStream): a plain-torch INCREMENTAL forward of the model under a
causal context band (past, 0), one utterance at a time, from per-site lists of K / V rows cut to the last past + 1.

`Dialogue` is one live dialogue: `step(text_row, audio_row)` returns the logits of the utterance that has just arrived, computed from
that utterance's rows alone plus the cached K / V rows of every attention site - each encoder layer of each stack of both modalities,
every fusion layer (Q = V = text, K = audio).  It is built from the oracle's `linear` and `layer_norm` and restates its `forward`
site by site; tests/test_streaming_cpu.py pins it against `oracle.m2fnet_oracle.forward` under `band_ref.swapped_in((past, 0))`,
which is the statement that caching is exact under a multi-layer window (the receptive field grows with depth, the cached rows do
not change).  `run` feeds a padded batch dialogue by dialogue.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch
from torch import Tensor

from oracle import m2fnet_oracle as O

_get = O._get


class _Site:
    """K / V rows of one attention site, the last past + 1 of them."""

    def __init__(self, past: Optional[int]):
        self.k: List[Tensor] = []
        self.v: List[Tensor] = []
        self.keep = None if past is None else past + 1

    def attend(self, q: Tensor, k: Tensor, v: Tensor, n_head: int) -> Tensor:
        """q, k, v: the new rows [E]; appends k / v and returns softmax(q K^T / sqrt(hd)) V over the rows kept, [E]."""
        self.k.append(k)
        self.v.append(v)
        if self.keep is not None:
            self.k, self.v = self.k[-self.keep:], self.v[-self.keep:]
        E = q.shape[0]
        hd = E // n_head
        K = torch.stack(self.k).reshape(-1, n_head, hd).permute(1, 0, 2)          # [H, n, hd]
        V = torch.stack(self.v).reshape(-1, n_head, hd).permute(1, 0, 2)
        s = (K @ q.reshape(n_head, hd, 1)).squeeze(-1) * (1.0 / math.sqrt(hd))    # [H, n]
        s = s - s.max(dim=-1, keepdim=True).values
        p = torch.exp(s)
        p = p / p.sum(dim=-1, keepdim=True)
        return (p.unsqueeze(1) @ V).reshape(E)


class Dialogue:
    def __init__(self, sd: Dict[str, Tensor], cfg, past: Optional[int]):
        self.sd, self.cfg, self.past = sd, cfg, past
        self.sites: Dict[str, _Site] = {}
        self.n = 0

    def _site(self, name: str) -> _Site:
        if name not in self.sites:
            self.sites[name] = _Site(self.past)
        return self.sites[name]

    def _encoder_layer(self, x: Tensor, pre: str, n_head: int) -> Tensor:
        sd, E = self.sd, x.shape[-1]
        qkv = O.linear(x, sd[pre + "self_attn.in_proj_weight"], sd[pre + "self_attn.in_proj_bias"])
        a = self._site(pre).attend(qkv[:E], qkv[E:2 * E], qkv[2 * E:], n_head)
        a = O.linear(a, sd[pre + "self_attn.out_proj.weight"], sd[pre + "self_attn.out_proj.bias"])
        x = O.layer_norm(x + a, sd[pre + "norm1.weight"], sd[pre + "norm1.bias"])
        h = torch.relu(O.linear(x, sd[pre + "linear1.weight"], sd[pre + "linear1.bias"]))
        h = O.linear(h, sd[pre + "linear2.weight"], sd[pre + "linear2.bias"])
        return O.layer_norm(x + h, sd[pre + "norm2.weight"], sd[pre + "norm2.bias"])

    def _modality(self, x: Tensor, M, name: str) -> Tensor:
        sd = self.sd
        for e in range(_get(M, "n_transformers")):
            pre = f"{name}_encoders.{e}."
            y = x
            for l in range(_get(M, "n_encoder_layers")):
                y = self._encoder_layer(y, f"{pre}layers.{l}.", _get(M, "n_head"))
            x = x + O.layer_norm(y, sd[pre + "norm.weight"], sd[pre + "norm.bias"])
        return O.linear(x, sd[f"{name}_proj.weight"], sd[f"{name}_proj.bias"])

    def step(self, text: Optional[Tensor], audio: Optional[Tensor]) -> Tensor:
        """text [d_t], audio [d_a]: the new utterance -> its logits [C]."""
        sd, cfg = self.sd, self.cfg
        A, Tx, F, C = _get(cfg, "AUDIO"), _get(cfg, "TEXT"), _get(cfg, "FAM"), _get(cfg, "CLASSIFIER")
        a_on, t_on, f_on = bool(_get(A, "enabled")), bool(_get(Tx, "enabled")), bool(_get(F, "enabled"))
        if a_on:
            audio = self._modality(audio, A, "audio")
        if t_on:
            text = self._modality(text, Tx, "text")
        if f_on:
            E = text.shape[-1]
            for i in range(_get(F, "n_layers")):
                pre = f"fusion_layers.{i}."
                w, b = sd[pre + "multihead_attention.in_proj_weight"], sd[pre + "multihead_attention.in_proj_bias"]
                q = O.linear(text, w[:E], b[:E])
                k = O.linear(audio, w[E:2 * E], b[E:2 * E])
                v = O.linear(text, w[2 * E:], b[2 * E:])
                a = self._site(pre).attend(q, k, v, _get(F, "n_head"))
                x = O.linear(a, sd[pre + "multihead_attention.out_proj.weight"], sd[pre + "multihead_attention.out_proj.bias"])
                text = torch.relu(O.linear(torch.relu(torch.cat((x, text))), sd[pre + "linear.weight"], sd[pre + "linear.bias"]))
        x = torch.cat((audio, text)) if (a_on and t_on) else (text if t_on else audio)
        x = O.linear(x, sd["output_layer.0.weight"], sd["output_layer.0.bias"])
        idx = 0
        for _ in range(max(_get(C, "n_layers") - 2, 0)):
            idx += 2
            x = O.linear(torch.relu(x), sd[f"output_layer.{idx}.weight"], sd[f"output_layer.{idx}.bias"])
        idx += 3
        self.n += 1
        return O.linear(torch.relu(x), sd[f"output_layer.{idx}.weight"], sd[f"output_layer.{idx}.bias"])


def run(sd: Dict[str, Tensor], cfg, text: Tensor, audio: Tensor, key_pad: Tensor, past: Optional[int]) -> Tensor:
    """A padded batch [B, L, ...] utterance by utterance: logits [B, L, C], zeros at pad slots (which are never fed)."""
    B, L = key_pad.shape
    C = _get(_get(cfg, "CLASSIFIER"), "output_size")
    dtype = next(iter(sd.values())).dtype
    out = torch.zeros(B, L, C, dtype=dtype)
    for b in range(B):
        d = Dialogue(sd, cfg, past)
        for i in range(L):
            if not key_pad[b, i]:
                out[b, i] = d.step(text[b, i], audio[b, i])
    return out
