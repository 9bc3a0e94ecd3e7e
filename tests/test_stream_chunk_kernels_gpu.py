"""functional.attention_stream_chunk (csrc/attention_stream_chunk.hip, the m2f_attention_stream_chunk C entry) against the float64
chunk reference of tests/golden/stream_chunk_ref.py: every head-dim path, capacities around the 64-row block boundary and at the
limit, chunk lengths 1 / 3 / 16 / 64, plain caches and rings, old counts 0 / 1 / C - 1 / C / 2C + 1 and new counts 0 / 1 / T - 1 / T
mixed in one launch (rings with more new rows than the ring holds, wraps inside a chunk, plain caches filled to their last row), dead
cache rows and unread input rows full of NaN, the rows a launch stores and the rows it must leave alone, equivalence to single-row
`attention_stream` launches, the fusion form's operands, and bit-reproducibility."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import stream_chunk_ref as CR  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402
from test_context_window_kernels_gpu import _close  # noqa: E402

DEV = "cuda"
SHAPES = [(1, 4, 12), (5, 4, 15), (3, 12, 25), (4, 8, 96), (2, 8, 128)]
CAPACITIES = [1, 3, 64, 65, 512]
CHUNKS = [1, 3, 16, 64]
TOL_F32, TOL_BF16 = 2e-5, 3e-2          # the bounds of tests/test_streaming_kernels_gpu.py


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def _pad8(w):
    return (w + 7) // 8 * 8


def _combos(C, T, ring):
    """(n_old, n_new) pairs every launch set must cover"""
    olds = [0, 1, C - 1] + ([C, 2 * C + 1] if ring else [])
    news = [0, 1, T - 1, T]
    pairs = {(o, n) for o in olds for n in news if o >= 0 and n >= 0 and (ring or o + n <= C)}
    if not ring:
        pairs |= {(C - n, n) for n in (1, T - 1, T) if 0 < n <= C}        # filled exactly to the last row
    return sorted(pairs)


def _launches(S, C, T, ring):
    c = _combos(C, T, ring)
    return [[c[(o + s) % len(c)] for s in range(S)] for o in range(0, len(c), S)]


def _live_rows(n, C, ring):
    """cache rows some query may see before the launch (a ring's row n % C holds the utterance that has just left every window)"""
    pos = n % C if ring else n
    return [r for r in range(min(n, C)) if r != pos]


def _fill(S, H, hd, C, olds, ring, bf16, seed):
    """NaN everywhere but in the live rows (random values, zero pad columns; bf16 caches: exact bf16 values)"""
    kc, vc = F.attention_stream_caches(S, H, hd, C, bf16=bf16, device=DEV, fill=float("nan"))
    for s, n in enumerate(olds):
        rows = _live_rows(n, C, ring)
        if rows:
            idx = torch.tensor(rows, device=DEV)
            kc[s, :, idx], vc[s, :, idx] = 0.0, 0.0
            kc[s, :, idx, :hd] = _rand(H, len(rows), hd, seed=seed + 7 * s).to(kc.dtype)
            vc[s, :, idx, :hd] = _rand(H, len(rows), hd, seed=seed + 7 * s + 3).to(vc.dtype)
    return kc, vc


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _rows_of(cache, s, hd):
    """[C, H*hd] float64 view of a slot's cache rows, as the reference holds them"""
    H, C = cache.shape[1], cache.shape[2]
    return cache[s, :, :, :hd].double().permute(1, 0, 2).reshape(C, H * hd)


def _operands(S, T, d, news, seed, fusion=False):
    """strided slices as the plans hold them, rows past a slot's count full of NaN"""
    if fusion:
        qv, kb = _rand(S * T, _pad8(2 * d), seed=seed), _rand(S * T, _pad8(d), seed=seed + 1)
        bufs, (q, v, k) = (qv, kb), (qv[:, :d], qv[:, d:2 * d], kb[:, :d])
    else:
        qkv = _rand(S * T, _pad8(3 * d), seed=seed)
        bufs, (q, k, v) = (qkv,), (qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:3 * d])
    for s, n in enumerate(news):
        for b in bufs:
            b[s * T + n: (s + 1) * T] = float("nan")
    return q, k, v


def _one_launch(S, H, hd, C, T, ring, bf16, tol, pairs, seed, fusion=False, steps=True):
    d = H * hd
    olds, news = [p[0] for p in pairs], [p[1] for p in pairs]
    q, k, v = _operands(S, T, d, news, seed, fusion)
    kc, vc = _fill(S, H, hd, C, olds, ring, bf16, seed + 1000)
    kc0, vc0 = kc.clone(), vc.clone()
    lengths = torch.tensor(olds, dtype=torch.int32, device=DEV)
    new = torch.tensor(news, dtype=torch.int32, device=DEV)
    what = f"S={S} H={H} hd={hd} C={C} T={T} ring={ring} bf16={bf16} (n_old, n_new)={pairs}"

    out = F.attention_stream_chunk(q, k, v, kc, vc, lengths, new, H, T, ring=ring, bf16=bf16)
    assert torch.isfinite(out).all(), "a dead cache row or an input row past the count was read: " + what
    assert torch.equal(lengths.cpu(), torch.tensor(olds, dtype=torch.int32)), "the launch must not advance the counts"

    want = torch.zeros(S * T, d, dtype=torch.float64, device=DEV)
    for s, (n_old, n) in enumerate(pairs):
        r = slice(s * T, s * T + n)
        assert torch.all(out[s * T + n: (s + 1) * T] == 0), "rows past the count must be zero"
        if n == 0:
            assert torch.equal(_bits(kc[s]), _bits(kc0[s])) and torch.equal(_bits(vc[s]), _bits(vc0[s])), "n_new = 0: the slot is untouched"
            continue
        rk, rv = _rows_of(kc0, s, hd), _rows_of(vc0, s, hd)
        want[r] = CR.chunk_attend(rk, rv, n_old, q[r].double(), k[r].double(), v[r].double(), H, ring)
        keep = torch.ones(C, dtype=torch.bool, device=DEV)
        for t, pos in CR.stored_rows(n_old, n, C, ring):
            newk, newv = k[s * T + t].reshape(H, hd), v[s * T + t].reshape(H, hd)
            if bf16:
                newk, newv = newk.to(torch.bfloat16), newv.to(torch.bfloat16)
            assert torch.equal(kc[s, :, pos, :hd], newk) and torch.equal(vc[s, :, pos, :hd], newv), f"stored row {pos}: " + what
            assert torch.all(kc[s, :, pos, hd:] == 0) and torch.all(vc[s, :, pos, hd:] == 0), "pad columns must be zero"
            keep[pos] = False
        assert torch.equal(_bits(kc[s][:, keep]), _bits(kc0[s][:, keep])) and torch.equal(_bits(vc[s][:, keep]), _bits(vc0[s][:, keep])), \
            "a row the chunk does not store was written: " + what
    _close(out.double(), want, tol, what)

    # two launches from restored copies of the caches: the same bits (the launch mutates a ring, so not on the mutated caches)
    kc2, vc2 = kc0.clone(), vc0.clone()
    again = F.attention_stream_chunk(q, k, v, kc2, vc2, lengths, new, H, T, ring=ring, bf16=bf16)
    assert torch.equal(out, again) and torch.equal(_bits(kc2), _bits(kc)) and torch.equal(_bits(vc2), _bits(vc)), "not reproducible: " + what

    if steps:      # the same rows through single-row launches: bit-identical caches, outputs within the bound
        kc3, vc3 = kc0.clone(), vc0.clone()
        q3, k3, v3 = (torch.nan_to_num(x.reshape(S, T, -1), nan=0.0) for x in (q, k, v))
        got = torch.zeros(S, T, d, device=DEV)
        for t in range(max(news)):
            act = torch.tensor([n > t for n in news], device=DEV)
            got[:, t] = F.attention_stream(q3[:, t], k3[:, t], v3[:, t], kc3, vc3, lengths + t, act, H, ring=ring, bf16=bf16)
        assert torch.equal(_bits(kc3), _bits(kc)) and torch.equal(_bits(vc3), _bits(vc)), "caches differ from the step launches': " + what
        _close(out.double(), got.reshape(S * T, d).double(), tol, "vs steps, " + what)


def _check(S, H, hd, C, T, bf16):
    tol = TOL_BF16 if bf16 else TOL_F32
    for ring in (False, True):
        for li, pairs in enumerate(_launches(S, C, T, ring)):
            _one_launch(S, H, hd, C, T, ring, bf16, tol, pairs, seed=S + hd + C + T + 31 * li)


@pytest.mark.parametrize("T", CHUNKS)
@pytest.mark.parametrize("C", CAPACITIES)
@pytest.mark.parametrize("S,H,hd", SHAPES)
def test_fp32_against_float64(S, H, hd, C, T):
    _check(S, H, hd, C, T, False)


@pytest.mark.parametrize("T", CHUNKS)
@pytest.mark.parametrize("C", CAPACITIES)
@pytest.mark.parametrize("S,H,hd", SHAPES)
def test_bf16_form_within_the_banded_kernels_bound(S, H, hd, C, T):
    _check(S, H, hd, C, T, True)


def test_the_grid_holds_the_cases_it_must():
    assert (3, 16) in _combos(3, 16, True) and (7, 16) in _combos(3, 16, True)          # n_new > C on a ring, mid-ring
    assert (3, 3) in _combos(1, 3, True)                                                # C = 1: every query sees itself only
    assert (2, 16) in _combos(3, 16, True) and (63, 64) in _combos(64, 64, True)         # a wrap inside the chunk
    assert (48, 16) in _combos(64, 16, False) and (0, 64) in _combos(64, 64, False) and (448, 64) in _combos(512, 64, False)
    assert all(o + n <= C for C in CAPACITIES for T in CHUNKS for o, n in _combos(C, T, False))


def test_fusion_form_operands_in_two_buffers():
    """q and v are slices of one [S*T, pad8(2E)] buffer, k lives in another (the fusion layers' projections)"""
    S, H, hd, C, T = 6, 8, 96, 65, 16
    _one_launch(S, H, hd, C, T, True, False, TOL_F32, [(0, 16), (1, 15), (64, 16), (65, 3), (131, 16), (7, 0)], seed=5, fusion=True)
    _one_launch(S, H, hd, C, T, False, True, TOL_BF16, [(0, 16), (49, 16), (64, 1), (65, 0), (30, 15), (7, 1)], seed=6, fusion=True)


def test_a_plain_cache_the_chunk_would_overfill_is_left_alone():
    """(the host refuses it first; the kernel treats the slot as not live, as the step kernel treats a full one)"""
    S, H, hd, C, T = 2, 4, 16, 8, 4
    q, k, v = _operands(S, T, H * hd, [4, 4], 1)
    kc, vc = _fill(S, H, hd, C, [5, 4], False, False, 2)
    kc0 = kc.clone()
    out = F.attention_stream_chunk(q, k, v, kc, vc, torch.tensor([5, 4], dtype=torch.int32, device=DEV),
                                   torch.tensor([4, 4], dtype=torch.int32, device=DEV), H, T)
    assert torch.all(out[:T] == 0) and torch.equal(_bits(kc[0]), _bits(kc0[0]))
    assert torch.isfinite(out).all() and out[T:].abs().max() > 0 and torch.isfinite(kc[1]).all()


def test_bad_arguments_are_refused():
    S, H, hd, C, T = 2, 2, 16, 4, 4
    q = _rand(S * T, H * hd)
    kc, vc = F.attention_stream_caches(S, H, hd, C, device=DEV)
    lengths, new = torch.zeros(S, dtype=torch.int32, device=DEV), torch.ones(S, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        F.attention_stream_chunk(q, q, q, kc, vc, lengths, new, H, T, bf16=True)          # fp32 caches in bf16 mode
    with pytest.raises(ValueError):
        F.attention_stream_chunk(q, q, q, kc, vc, lengths, new.long(), H, T)
    with pytest.raises(ValueError):
        F.attention_stream_chunk(q, q, q, kc, vc, lengths, new, H, 65)
    with pytest.raises(ValueError):
        F.attention_stream_chunk(q[:-1], q[:-1], q[:-1], kc, vc, lengths, new, H, T)
