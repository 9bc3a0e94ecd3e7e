"""Host replica of the device's dropout masks (csrc/common.h: m2f_mix32, m2f_site_key, m2f_keep), for tests only.

The mask of a dropout site is a pure integer function of (rng state, site, element index), so the host can say what it IS:
plain numpy uint32 arithmetic, vectorised.  On top of the three hash functions this file states the rules the kernels and the plan
builder follow - the threshold / scale of a probability, the element index of the row-wise kernels and of the attention kernels,
the order in which csrc/plan_build.hip hands out sites - and turns a plan's token layout into masks in the oracle's layout, so that
oracle/m2fnet_oracle.py can run with the device's own masks (its `drop` hook).  Nothing here is imported by the product.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch

U32 = np.uint32


def _u32(x):
    return np.asarray(x, dtype=np.uint64).astype(U32) if not isinstance(x, np.ndarray) or x.dtype != U32 else x


def mix32(x):
    """m2f_mix32 on a uint32 array (or scalar)."""
    with np.errstate(over="ignore"):
        x = _u32(x).copy()
        x ^= x >> U32(16)
        x *= U32(0x7FEB352D)
        x ^= x >> U32(15)
        x *= U32(0x846CA68B)
        x ^= x >> U32(16)
    return x


def site_key(state4, site):
    """m2f_site_key: state4 = (seed_lo, seed_hi, step_lo, step_hi) as non-negative ints below 2^32."""
    s = [U32(int(v) & 0xFFFFFFFF) for v in state4]
    with np.errstate(over="ignore"):
        k = mix32(s[0] ^ U32(0x9E3779B9))
        k = mix32(k ^ s[1])
        k = mix32(k + s[2] * U32(0x85EBCA6B))
        k = mix32(k ^ (s[3] + U32(int(site) & 0xFFFFFFFF) * U32(0xC2B2AE35)))
    return U32(k)


def keep(key, idx, thresh):
    """m2f_keep: bool array, True where element `idx` (uint32 array) survives."""
    key = U32(key)
    with np.errstate(over="ignore"):
        h = mix32(_u32(idx) * U32(0x9E3779B1) + key)
        h = mix32(h ^ (key >> U32(7)) ^ U32(0x68E31DA4))
    return h >= U32(thresh)


def thresh_scale(p):
    """(thresh, scale) of a dropout probability: thresh = min(2^32 - 1, floor(p 2^32)) with p the fp32 value the C ABI receives,
    scale = fp32(1 / (1 - p)) in fp32 arithmetic (csrc/plan.hip: drop_thresh / drop_scale; csrc/entry_kernels.hip: drop_params)."""
    pf = np.float32(p)
    thresh = int(min(4294967295.0, np.floor(float(pf) * 4294967296.0)))
    with np.errstate(divide="ignore"):
        scale = np.float32(1.0) / (np.float32(1.0) - pf)
    return thresh, float(np.float32(scale))


def state_of(rng):
    """A device rng tensor (4 x int32) -> four Python ints in [0, 2^32)."""
    return [int(v) & 0xFFFFFFFF for v in rng.detach().cpu().tolist()]


def rows_index(row_ids, N):
    """uint32 element index [len(row_ids), N] of the row-wise kernels: row * N + col, wrapping in 32 bits as the kernels' own
    arithmetic does."""
    r = np.asarray(row_ids, dtype=np.uint64)
    return ((r[:, None] * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)).astype(U32)


def rows_mask(state4, site, p, rows, N):
    """Keep mask [rows, N] of the row-wise kernels (GEMM epilogues, LayerNorm forward / backward, the in-place kernel): element
    (row, col) has index row * N + col in uint32 arithmetic, N the LOGICAL width (never the leading dimension)."""
    thresh, _ = thresh_scale(p)
    return keep(site_key(state4, site), rows_index(np.arange(rows), N), thresh)


def attn_mask(state4, site, p, B, H, L):
    """Keep mask [B, H, L(query i), L(key j)] of the attention kernels: index ((b H + h) L + i) L + j, L the PLAN's L."""
    thresh, _ = thresh_scale(p)
    n = np.uint64(B) * np.uint64(H) * np.uint64(L) * np.uint64(L)
    idx = np.arange(int(n), dtype=np.uint64).astype(U32).reshape(B, H, L, L)
    return keep(site_key(state4, site), idx, thresh)


def _sec(cfg, name):
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def site_map(cfg):
    """The dropout sites of a train plan of the reference-style model config `cfg`, by name, in the order csrc/plan_build.hip's
    Builder::site() hands them out (from 1): audio branch then text branch - per encoder stack and layer `attn, dropout1, ff,
    dropout2`, after the last stack `pre_proj`, then `post_proj` -, per fusion layer `attn, out`, then the classifier's one
    dropout.  The names are the ones oracle/m2fnet_oracle.py passes to its `drop` hook."""
    sites = OrderedDict()

    def add(name):
        assert name not in sites, name
        sites[name] = len(sites) + 1

    for mod in ("audio", "text"):
        m = _sec(cfg, mod.upper())
        if not _sec(m, "enabled"):
            continue
        nt, nl = _sec(m, "n_transformers"), _sec(m, "n_encoder_layers")
        for e in range(nt):
            for l in range(nl):
                for what in ("attn", "dropout1", "ff", "dropout2"):
                    add(f"{mod}_encoders.{e}.layers.{l}.{what}")
            if e == nt - 1:
                add(f"{mod}.pre_proj")
        add(f"{mod}.post_proj")
    fam = _sec(cfg, "FAM")
    if _sec(fam, "enabled"):
        for i in range(_sec(fam, "n_layers")):
            add(f"fusion_layers.{i}.attn")
            add(f"fusion_layers.{i}.out")
    add("classifier")
    return sites


def plan_row_map(plan, B, L):
    """Token row of every (dialogue, slot) of a [B, L] batch in `plan` (a mer_amd.runtime.Plan that has been given the batch):
    padded plans b * plan.L + i, packed plans cu[b] + i (taken from the plan's own scatter map; pad slots, which own no row
    there, point at the spare row - nothing valid depends on them)."""
    if plan.packed:
        return plan._dst.detach().cpu().numpy().astype(np.int64)
    return np.arange(B, dtype=np.int64)[:, None] * plan.L + np.arange(L, dtype=np.int64)[None, :]


class PlanMasks:
    """The `drop` hook of the oracle under the masks a plan draws from rng state `state4`: __call__(name, x) -> x * keep * scale.
    Row-wise sites take x [B, L, N] (mask rows through the plan's row map, width N), attention sites x [B, H, L, L] (the plan's B
    and L index the mask, the batch's corner of it is used).  `seen` lists the names the oracle asked for."""

    def __init__(self, cfg, state4, p, plan_B, plan_L, plan_T, row_map):
        self.sites = site_map(cfg)
        self.state, self.p = list(state4), float(p)
        self.B, self.L, self.T = int(plan_B), int(plan_L), int(plan_T)
        self.rows = np.asarray(row_map)
        self.scale = thresh_scale(p)[1]
        self.seen = []
        self._cache = {}

    @classmethod
    def of_plan(cls, cfg, plan, state4, B, L):
        return cls(cfg, state4, plan.cfg.dropout, plan.B, plan.L, plan.T, plan_row_map(plan, B, L))

    def mask(self, name, shape):
        key = (name, tuple(shape))
        if key not in self._cache:
            site = self.sites[name]
            if len(shape) == 4:
                B, H, L, _ = shape
                m = attn_mask(self.state, site, self.p, self.B, H, self.L)[:B, :, :L, :L]
            else:
                N = shape[-1]
                m = rows_mask(self.state, site, self.p, self.T, N)[self.rows]
            self._cache[key] = torch.from_numpy(np.ascontiguousarray(m))
        return self._cache[key]

    def __call__(self, name, x):
        self.seen.append(name)
        return x * (self.mask(name, x.shape).to(x.dtype) * self.scale)
