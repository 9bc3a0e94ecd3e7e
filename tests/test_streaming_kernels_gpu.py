"""functional.attention_stream (csrc/attention_stream.hip, the m2f_attention_stream C entry) against float64 torch: every head dim
in use, capacities around the 64-row pass boundary and at the limit, plain caches and rings, counts 0 / 1 / C - 1 / C / 2C + 1 mixed in
one launch, strided operands, inactive slots, the row the launch stores, dead rows full of NaN, and bit-reproducibility."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402
from test_context_window_kernels_gpu import _close  # noqa: E402

DEV = "cuda"
SHAPES = [(1, 4, 12), (5, 4, 15), (3, 12, 25), (4, 4, 75), (8, 8, 96), (64, 8, 128)]
CAPACITIES = [1, 3, 64, 65, 512]


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _pad8(w):
    return (w + 7) // 8 * 8


def _counts(C, ring):
    c = [0, 1, C - 1] + ([C, 2 * C + 1] if ring else [])
    return sorted({x for x in c if x >= 0 and (ring or x < C)})


def _live_rows(n, C, ring):
    """(cache rows that are live before the launch, the row the new utterance takes)"""
    pos = n % C if ring else n
    rows = [r for r in range(min(n, C)) if r != pos]
    return rows, pos


def _fill(S, H, hd, C, lens, ring, bf16, seed):
    """Caches holding NaN everywhere but in the live rows (random values there, zeros in their pad columns, as the kernel stores rows;
    bf16 caches: exact bf16 values)."""
    kc, vc = F.attention_stream_caches(S, H, hd, C, bf16=bf16, device=DEV, fill=float("nan"))
    for s, n in enumerate(lens):
        rows, _ = _live_rows(n, C, ring)
        if rows:
            idx = torch.tensor(rows, device=DEV)
            kc[s, :, idx], vc[s, :, idx] = 0.0, 0.0                           # (a stored row's pad columns hold zeros)
            kc[s, :, idx, :hd] = _rand(H, len(rows), hd, seed=seed + 7 * s).to(kc.dtype)
            vc[s, :, idx, :hd] = _rand(H, len(rows), hd, seed=seed + 7 * s + 3).to(vc.dtype)
    return kc, vc


def _reference(q, k, v, kc, vc, lens, active, H, hd, C, ring):
    """float64: out [S, H*hd]"""
    S = q.shape[0]
    out = torch.zeros(S, H * hd, dtype=torch.float64, device=DEV)
    for s, n in enumerate(lens):
        if not active[s]:
            continue
        rows, _ = _live_rows(n, C, ring)
        idx = torch.tensor(rows, dtype=torch.long, device=DEV)
        K = torch.cat([kc[s, :, idx, :hd].double(), k[s].double().reshape(H, 1, hd)], dim=1)          # [H, n, hd]
        V = torch.cat([vc[s, :, idx, :hd].double(), v[s].double().reshape(H, 1, hd)], dim=1)
        sc = (K @ q[s].double().reshape(H, hd, 1)).squeeze(-1) / math.sqrt(hd)
        p = torch.softmax(sc, dim=-1)
        out[s] = (p.unsqueeze(1) @ V).reshape(H * hd)
    return out


def _launches(S, C, ring):
    """count vectors that together put every count of `_counts` into some slot, mixed inside a launch"""
    c = _counts(C, ring)
    return [[c[(s + o) % len(c)] for s in range(S)] for o in range(0, len(c), S)]


def _check(S, H, hd, C, ring, bf16, tol, seed=0):
    d = H * hd
    for li, lens in enumerate(_launches(S, C, ring)):
        qkv = _rand(S, _pad8(3 * d), seed=seed + li)                       # strided slices of a pad8(3d) buffer, as the plans hold them
        q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:3 * d]
        active = [not (S >= 3 and s % 3 == 1) for s in range(S)]
        kc, vc = _fill(S, H, hd, C, lens, ring, bf16, seed + 100 * li)
        kc0, vc0 = kc.clone(), vc.clone()
        lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
        act = torch.tensor(active, device=DEV)
        want = _reference(q, k, v, kc0, vc0, lens, active, H, hd, C, ring)
        out = F.attention_stream(q, k, v, kc, vc, lengths, act, H, ring=ring, bf16=bf16)
        assert torch.isfinite(out).all(), "a dead cache row was read"
        _close(out.double(), want, tol, f"S={S} H={H} hd={hd} C={C} ring={ring} bf16={bf16} counts={sorted(set(lens))}")
        assert torch.equal(lengths.cpu(), torch.tensor(lens, dtype=torch.int32)), "the launch must not advance the counts"
        bits = lambda t: t.view(torch.int16 if bf16 else torch.int32)          # noqa: E731  (NaN rows compare as bits)
        for s, n in enumerate(lens):
            if not active[s]:
                assert torch.all(out[s] == 0)
                assert torch.equal(bits(kc[s]), bits(kc0[s])) and torch.equal(bits(vc[s]), bits(vc0[s]))
                continue
            _, pos = _live_rows(n, C, ring)
            newk, newv = k[s].reshape(H, hd), v[s].reshape(H, hd)
            if bf16:
                newk, newv = newk.to(torch.bfloat16), newv.to(torch.bfloat16)
            assert torch.equal(kc[s, :, pos, :hd], newk) and torch.equal(vc[s, :, pos, :hd], newv)
            assert torch.all(kc[s, :, pos, hd:] == 0) and torch.all(vc[s, :, pos, hd:] == 0)
            keep = torch.ones(C, dtype=torch.bool, device=DEV)
            keep[pos] = False                                                 # every other row: untouched
            assert torch.equal(bits(kc[s][:, keep]), bits(kc0[s][:, keep])) and torch.equal(bits(vc[s][:, keep]), bits(vc0[s][:, keep]))
            if n == 0:
                assert torch.equal(out[s], newv.float().reshape(-1)), "count 0: the new V row itself"
        again = F.attention_stream(q, k, v, kc, vc, lengths, act, H, ring=ring, bf16=bf16)
        assert torch.equal(out, again), "two identical launches must give identical bits"


@pytest.mark.parametrize("C", CAPACITIES)
@pytest.mark.parametrize("S,H,hd", SHAPES)
def test_fp32_against_float64(S, H, hd, C):
    for ring in (False, True):
        _check(S, H, hd, C, ring, False, 2e-5, seed=S + hd + C)


@pytest.mark.parametrize("C", CAPACITIES)
@pytest.mark.parametrize("S,H,hd", SHAPES)
def test_bf16_form_within_the_banded_kernels_bound(S, H, hd, C):
    for ring in (False, True):
        _check(S, H, hd, C, ring, True, 3e-2, seed=S + hd + C)


def test_fusion_form_operands_in_two_buffers():
    """q and v are slices of one [S, pad8(2E)] buffer, k lives in another (the fusion layers' projections)"""
    S, H, hd, C = 6, 8, 96, 65
    E = H * hd
    qv, kb = _rand(S, _pad8(2 * E), seed=1), _rand(S, _pad8(E), seed=2)
    q, v, k = qv[:, :E], qv[:, E:2 * E], kb[:, :E]
    lens = [0, 1, 64, 65, 131, 7]
    kc, vc = _fill(S, H, hd, C, lens, True, False, 5)
    want = _reference(q, k, v, kc.clone(), vc.clone(), lens, [True] * S, H, hd, C, True)
    out = F.attention_stream(q, k, v, kc, vc, torch.tensor(lens, dtype=torch.int32, device=DEV), torch.ones(S, device=DEV), H, ring=True)
    _close(out.double(), want, 2e-5, "fusion form")


def test_a_dialogue_grown_row_by_row_matches_full_causal_attention():
    """n launches on one slot's caches, the host advancing the count: row i equals causal attention over rows 0 .. i, and under a
    ring of 4 rows attention over rows i - 3 .. i"""
    S, H, hd, n = 2, 4, 15, 11
    E = H * hd
    q, k, v = _rand(n, S, E, seed=3), _rand(n, S, E, seed=4), _rand(n, S, E, seed=5)
    for ring, C in ((False, 16), (True, 4)):
        kc, vc = F.attention_stream_caches(S, H, hd, C, device=DEV, fill=float("nan"))
        for i in range(n):
            lengths = torch.full((S,), i, dtype=torch.int32, device=DEV)
            out = F.attention_stream(q[i], k[i], v[i], kc, vc, lengths, torch.ones(S, device=DEV), H, ring=ring)
            lo = max(0, i - (C - 1)) if ring else 0
            for s in range(S):
                K, V = k[lo:i + 1, s].double().reshape(-1, H, hd).permute(1, 0, 2), v[lo:i + 1, s].double().reshape(-1, H, hd).permute(1, 0, 2)
                p = torch.softmax((K @ q[i, s].double().reshape(H, hd, 1)).squeeze(-1) / math.sqrt(hd), dim=-1)
                _close(out[s].double(), (p.unsqueeze(1) @ V).reshape(E), 2e-5, f"ring={ring} row {i} slot {s}")


def test_bad_arguments_are_refused():
    S, H, hd, C = 2, 2, 16, 4
    q = _rand(S, H * hd)
    kc, vc = F.attention_stream_caches(S, H, hd, C, device=DEV)
    lengths, act = torch.zeros(S, dtype=torch.int32, device=DEV), torch.ones(S, device=DEV)
    with pytest.raises(ValueError):
        F.attention_stream(q, q, q, kc, vc, lengths, act, H, bf16=True)          # fp32 caches in bf16 mode
    with pytest.raises(ValueError):
        F.attention_stream(q, q, q, kc, vc, lengths.long(), act, H)
    with pytest.raises(mer_amd.runtime.HipError):
        F.attention_stream_caches(S, H, 129, C, device=DEV)
    with pytest.raises(mer_amd.runtime.HipError):
        F.attention_stream_caches(S, H, hd, 513, device=DEV)
