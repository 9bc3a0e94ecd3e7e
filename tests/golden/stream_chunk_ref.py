"""Reference for the chunk form of the streaming attention (functional.attention_stream_chunk, DialogueStream.prefill): plain torch,
float64, with the cache rows modelled explicitly - what `stream_ref._Site.attend` computes from a growing list, computed from a
cache of C rows and a count, so that the rows a launch must store, and the rows it must leave alone, are part of the statement.

One (slot, site): `kc` / `vc` are [C, E] (all heads of a row side by side), `n_old` utterances have been cached so far.  Utterance j
lives in row j % C of a ring (a window of C - 1 past utterances) or in row j of a plain cache (n_old + n <= C required).  Query t of a
chunk of n rows is utterance u = n_old + t; it sees utterances max(0, u - (C - 1)) .. u on a ring and 0 .. u on a plain cache, the
chunk's own keys and values taken from the rows given, never from the cache.  Afterwards the last min(n, C) rows of the chunk are in
the cache - earlier ones would have been overwritten by later rows of the same chunk - and every other row is as it was.
`tests/test_stream_prefill_cpu.py` pins this against `_Site.attend` called row by row.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch
from torch import Tensor


def position(u: int, C: int, ring: bool) -> int:
    """the cache row of utterance u"""
    return u % C if ring else u


def stored_rows(n_old: int, n: int, C: int, ring: bool):
    """[(chunk row t, cache row)] of the rows a chunk of n leaves in the cache: its last min(n, C)"""
    return [(t, position(n_old + t, C, ring)) for t in range(max(0, n - C), n)]


def chunk_attend(kc: Tensor, vc: Tensor, n_old: int, q: Tensor, k: Tensor, v: Tensor, n_head: int, ring: bool) -> Tensor:
    """q, k, v: the chunk's rows [n, E]; kc, vc: [C, E], updated IN PLACE.  Returns out [n, E].  Only the cached rows that some query
    of the chunk sees are read (a ring's row of utterance n_old - C, which the chunk's first row recycles, is not)."""
    C, E = kc.shape
    n = q.shape[0]
    hd = E // n_head
    if not ring and n_old + n > C:
        raise ValueError(f"a plain cache of {C} rows cannot take {n} utterances behind {n_old}")
    if n == 0:
        return torch.zeros(0, E, dtype=q.dtype, device=q.device)
    first = max(0, n_old - (C - 1)) if ring else 0                       # the oldest utterance the chunk's first query sees
    rows = torch.tensor([position(j, C, ring) for j in range(first, n_old)], dtype=torch.long, device=q.device)
    K = torch.cat([kc[rows], k]).reshape(-1, n_head, hd)                 # utterances first .. n_old + n - 1: the chunk's own from k / v
    V = torch.cat([vc[rows], v]).reshape(-1, n_head, hd)
    u = n_old + torch.arange(n, device=q.device)[:, None]
    j = first + torch.arange(K.shape[0], device=q.device)[None, :]
    seen = (j <= u) & ((j >= u - (C - 1)) if ring else torch.ones_like(j, dtype=torch.bool))
    s = torch.einsum("thd,mhd->htm", q.reshape(n, n_head, hd), K) * (1.0 / math.sqrt(hd))
    p = torch.softmax(s.masked_fill(~seen[None], float("-inf")), dim=-1)
    out = torch.einsum("htm,mhd->thd", p, V).reshape(n, E)
    for t, pos in stored_rows(n_old, n, C, ring):
        kc[pos], vc[pos] = k[t], v[t]
    return out


def new_caches(C: int, E: int, dtype=torch.float64) -> Tuple[Tensor, Tensor]:
    """rows that were never written hold NaN: a reader of a dead row is seen"""
    return torch.full((C, E), float("nan"), dtype=dtype), torch.full((C, E), float("nan"), dtype=dtype)
