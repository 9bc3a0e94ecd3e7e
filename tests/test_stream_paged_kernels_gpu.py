"""functional.attention_stream_paged / attention_stream_chunk_paged (the paged forms in csrc/attention_stream.hip and
csrc/attention_stream_chunk.hip) against the dense kernels, bit for bit.

Every case builds the dense caches of tests/test_streaming_kernels_gpu.py (NaN everywhere but the live rows), scatters them into a
NaN pool through a scrambled page table - pages of different slots interleave, the ids of a slot descend - and points every table
entry the launch has no business reading at one canary page full of NaN (a valid id: a wrong read shows as NaN, never as a fault).
The paged launch must then give the dense launch's output bits, leave the pool exactly as the dense caches scattered AFTER the dense
launch (so the new rows sit at (table[s][pos / R], pos % R), rounded once, pad columns zero, and every other bit, the canary page
included, is unchanged), not advance the counts, and repeat itself bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402
from test_context_window_kernels_gpu import _close  # noqa: E402
from test_streaming_kernels_gpu import _fill, _live_rows, _pad8, _rand, _reference  # noqa: E402  (the dense test's construction)
from test_stream_chunk_kernels_gpu import TOL_BF16, TOL_F32, _fill as _fill_chunk, _operands  # noqa: E402

DEV = "cuda"
SHAPES = [(1, 4, 12), (5, 4, 15), (4, 4, 75), (8, 8, 128)]
PAGE_ROWS = [16, 64]
CAPACITIES = [1, 3, 17, 65, 512]
CHUNKS = [2, 16, 64]


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _counts(C, R, ring):
    c = [0, 1, R - 1, R, R + 1, C - 1] + ([C, 2 * C + 1] if ring else [])
    return sorted({n for n in c if n >= 0 and (ring or n < C)})


def _table(S, C, R, touched):
    """touched[s] = rows of slot s the launch may touch (0: the slot reads no entry).  -> (table int32 [S, ceil(C/R)] on the device,
    n_pages, canary id).  Entries e < ceil(touched[s] / R) get pages of their own, handed out level by level from the LAST entry down,
    so the slots interleave and a slot's ids descend; the canary sits in the middle of the id range; every other entry names it."""
    tw = -(-C // R)
    pairs = sorted(((e, s) for s in range(S) for e in range(-(-touched[s] // R))), key=lambda p: (-p[0], p[1]))
    canary = len(pairs) // 2
    table = torch.full((S, tw), canary, dtype=torch.int32)
    for i, (e, s) in enumerate(pairs):
        table[s, e] = i + (i >= canary)
    for s in range(S):                                          # what the docstring promises
        own = table[s, :-(-touched[s] // R)].tolist()
        assert canary not in own and own == sorted(own, reverse=True)
    return table.to(DEV), len(pairs) + 1, canary


def _scatter(kc, vc, table, n_pages, R, touched, bf16, hd):
    """The dense caches' rows into NaN pools through the table (whole pages of the entries with a page of their own; the rows of a
    page past the capacity stay NaN)."""
    S, H, C, _ = kc.shape
    kp, vp = F.attention_stream_pools(n_pages, H, hd, R, bf16=bf16, device=DEV, fill=float("nan"))
    assert kp.shape == (n_pages, H, R, kc.shape[3]) and kp.dtype == kc.dtype
    host = table.cpu()
    for s in range(S):
        for e in range(-(-touched[s] // R)):
            rows = slice(e * R, min((e + 1) * R, C))
            page = int(host[s, e])
            kp[page, :, : rows.stop - rows.start] = kc[s, :, rows]
            vp[page, :, : rows.stop - rows.start] = vc[s, :, rows]
    return kp, vp


def _step_launches(S, C, R, ring):
    c = _counts(C, R, ring)
    return [[c[(s + o) % len(c)] for s in range(S)] for o in range(0, len(c), S)]


def _check_step(S, H, hd, C, R, ring, bf16, tol, seed):
    d = H * hd
    for li, lens in enumerate(_step_launches(S, C, R, ring)):
        what = f"S={S} H={H} hd={hd} C={C} R={R} ring={ring} bf16={bf16} counts={lens}"
        qkv = _rand(S, _pad8(3 * d), seed=seed + li)
        q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:3 * d]
        active = [not (S >= 3 and s % 3 == 1) for s in range(S)]
        kc, vc = _fill(S, H, hd, C, lens, ring, bf16, seed + 100 * li)
        touched = [min(n + 1, C) if a else 0 for n, a in zip(lens, active)]
        table, n_pages, canary = _table(S, C, R, touched)
        kp, vp = _scatter(kc, vc, table, n_pages, R, touched, bf16, hd)
        kp0, vp0 = kp.clone(), vp.clone()
        lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
        act = torch.tensor(active, device=DEV)
        want64 = _reference(q, k, v, kc.clone(), vc.clone(), lens, active, H, hd, C, ring)

        dense = F.attention_stream(q, k, v, kc, vc, lengths, act, H, ring=ring, bf16=bf16)
        out = F.attention_stream_paged(q, k, v, kp, vp, table, lengths, act, H, C, ring=ring, bf16=bf16)
        assert torch.isfinite(out).all(), "a dead row, a stale page or the canary was read: " + what                 # (b)
        assert torch.equal(out, dense), "not the dense kernel's bits: " + what                                       # (a)
        _close(out.double(), want64, tol, what)                                                                      # (c)
        assert torch.equal(lengths.cpu(), torch.tensor(lens, dtype=torch.int32)), "the launch must not advance the counts"   # (f)
        host = table.cpu()
        for s, n in enumerate(lens):                                                                                 # (d)
            if not active[s]:
                continue
            _, pos = _live_rows(n, C, ring)
            page, row = int(host[s, pos // R]), pos % R
            newk, newv = k[s].reshape(H, hd), v[s].reshape(H, hd)
            if bf16:
                newk, newv = newk.to(torch.bfloat16), newv.to(torch.bfloat16)
            assert torch.equal(kp[page, :, row, :hd], newk) and torch.equal(vp[page, :, row, :hd], newv), "the new row: " + what
            assert torch.all(kp[page, :, row, hd:] == 0) and torch.all(vp[page, :, row, hd:] == 0), "pad columns must be zero"
        wk, wv = _scatter(kc, vc, table, n_pages, R, touched, bf16, hd)         # the dense caches AFTER the dense launch, same map     (e)
        assert torch.equal(_bits(kp), _bits(wk)) and torch.equal(_bits(vp), _bits(wv)), "a bit outside the new rows changed: " + what
        assert torch.equal(_bits(kp[canary]), _bits(kp0[canary])) and torch.isnan(kp[canary].float()).all()
        assert torch.equal(_bits(vp[canary]), _bits(vp0[canary]))
        again = F.attention_stream_paged(q, k, v, kp, vp, table, lengths, act, H, C, ring=ring, bf16=bf16)          # (g)
        assert torch.equal(out, again) and torch.equal(_bits(kp), _bits(wk)), "two identical launches must give identical bits"


@pytest.mark.parametrize("C", CAPACITIES)
@pytest.mark.parametrize("S,H,hd", SHAPES)
def test_step_fp32_gives_the_dense_bits(S, H, hd, C):
    for R in PAGE_ROWS:
        for ring in (False, True):
            _check_step(S, H, hd, C, R, ring, False, TOL_F32, seed=S + hd + C + R)


@pytest.mark.parametrize("C", CAPACITIES)
@pytest.mark.parametrize("S,H,hd", SHAPES)
def test_step_bf16_gives_the_dense_bits(S, H, hd, C):
    for R in PAGE_ROWS:
        for ring in (False, True):
            _check_step(S, H, hd, C, R, ring, True, TOL_BF16, seed=S + hd + C + R)


# ---- chunk form -------------------------------------------------------------------------------------------------------------------
def _chunk_pairs(C, T, R, ring):
    """(n_old, n_new): histories at and around a page boundary and (R = 16: inside a block of four pages) the 64-row block boundary,
    new counts 0 / 1 / T and, on a ring, one above C"""
    olds = sorted({n for n in (0, 1, R - 1, R + 1, 63, 65, C - 1) + ((C, 2 * C + 1) if ring else ()) if n >= 0 and (ring or n <= C)})
    news = [0, 1, T] + ([C + 1] if ring and C + 1 <= T else [])
    pairs = []
    for i, o in enumerate(olds):
        for n in (news[i % len(news)], news[(i + 1) % len(news)], T):
            if (ring or o + n <= C) and (o, n) not in pairs:
                pairs.append((o, n))
    return pairs


def _check_chunk(S, H, hd, C, T, R, ring, bf16, seed):
    d = H * hd
    allp = _chunk_pairs(C, T, R, ring)
    for li in range(0, len(allp), S):
        pairs = [allp[(li + s) % len(allp)] for s in range(S)]
        what = f"S={S} H={H} hd={hd} C={C} T={T} R={R} ring={ring} bf16={bf16} (n_old, n_new)={pairs}"
        olds, news = [p[0] for p in pairs], [p[1] for p in pairs]
        q, k, v = _operands(S, T, d, news, seed + li)
        kc, vc = _fill_chunk(S, H, hd, C, olds, ring, bf16, seed + 1000 + li)
        touched = [min(o + n, C) if n > 0 else 0 for o, n in pairs]
        table, n_pages, canary = _table(S, C, R, touched)
        kp, vp = _scatter(kc, vc, table, n_pages, R, touched, bf16, hd)
        lengths = torch.tensor(olds, dtype=torch.int32, device=DEV)
        new = torch.tensor(news, dtype=torch.int32, device=DEV)

        dense = F.attention_stream_chunk(q, k, v, kc, vc, lengths, new, H, T, ring=ring, bf16=bf16)
        out = F.attention_stream_chunk_paged(q, k, v, kp, vp, table, lengths, new, H, T, C, ring=ring, bf16=bf16)
        assert torch.isfinite(out).all(), "a dead row, a stale page, the canary or an input row past the count was read: " + what
        assert torch.equal(out, dense), "not the dense chunk kernel's bits: " + what
        wk, wv = _scatter(kc, vc, table, n_pages, R, touched, bf16, hd)         # the dense caches after the dense launch, same map
        assert torch.equal(_bits(kp), _bits(wk)) and torch.equal(_bits(vp), _bits(wv)), "the pools differ from the dense caches: " + what
        assert torch.isnan(kp[canary].float()).all() and torch.isnan(vp[canary].float()).all()
        assert torch.equal(lengths.cpu(), torch.tensor(olds, dtype=torch.int32))


@pytest.mark.parametrize("T", CHUNKS)
@pytest.mark.parametrize("C", CAPACITIES)
@pytest.mark.parametrize("S,H,hd", SHAPES)
def test_chunk_gives_the_dense_bits(S, H, hd, C, T):
    for R in PAGE_ROWS:
        for ring in (False, True):
            for bf16 in (False, True):
                _check_chunk(S, H, hd, C, T, R, ring, bf16, seed=S + hd + C + T + R)


def test_the_chunk_pairs_straddle_page_and_block_boundaries():
    """(the construction above does what it says)"""
    pairs = _chunk_pairs(512, 16, 16, False)
    assert any(o < 16 < o + n for o, n in pairs) and any(o < 64 < o + n for o, n in pairs) and any(o > 64 and n == 16 for o, n in pairs)
    assert {n for _, n in pairs} == {0, 1, 16}
    assert any(n == 4 for _, n in _chunk_pairs(3, 16, 16, True)), "a ring takes more new rows than it holds"
    assert all(o + n <= 65 for o, n in _chunk_pairs(65, 64, 64, False))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    S, H, hd, C, R, T = 2, 2, 16, 40, 16, 4
    HipError = mer_amd.runtime.HipError
    q, qT = _rand(S, H * hd), _rand(S * T, H * hd)
    lengths, act = torch.zeros(S, dtype=torch.int32, device=DEV), torch.ones(S, device=DEV)
    new = torch.ones(S, dtype=torch.int32, device=DEV)
    table = torch.zeros(S, 3, dtype=torch.int32, device=DEV)
    kp, vp = F.attention_stream_pools(4, H, hd, R, device=DEV, fill=float("nan"))

    def both(exc, kp=kp, vp=vp, table=table, C=C, q=q, qT=qT, H=H, bf16=False):
        with pytest.raises(exc):
            F.attention_stream_paged(q, q, q, kp, vp, table, lengths, act, H, C, bf16=bf16)
        with pytest.raises(exc):
            F.attention_stream_chunk_paged(qT, qT, qT, kp, vp, table, lengths, new, H, T, C, bf16=bf16)

    for rows in (8, 48, 128):                                   # page_rows outside {16, 32, 64}
        with pytest.raises(HipError):
            F.attention_stream_pools(4, H, hd, rows, device=DEV)
        bad = torch.full((4, H, rows, hd), float("nan"), device=DEV)
        both(HipError, kp=bad, vp=bad.clone(), table=torch.zeros(S, -(-C // rows), dtype=torch.int32, device=DEV))
    flat = torch.full((kp.numel() + 4,), float("nan"), device=DEV)
    off = flat[1: 1 + kp.numel()].view(kp.shape)                # 4 bytes off a 16-byte boundary
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    both(HipError, kp=off)
    both(HipError, vp=off)
    both(HipError, table=torch.zeros(S, 2, dtype=torch.int32, device=DEV))      # not ceil(40 / 16) columns
    both(HipError, table=torch.zeros(S, 4, dtype=torch.int32, device=DEV))
    both(ValueError, table=torch.zeros(S, 3, dtype=torch.int64, device=DEV))
    both(ValueError, table=torch.zeros(S + 1, 3, dtype=torch.int32, device=DEV))
    both(HipError, C=513, table=torch.zeros(S, 33, dtype=torch.int32, device=DEV))
    wide, wideT = _rand(S, H * 129), _rand(S * T, H * 129)
    kw, vw = (torch.full((4, H, R, 132), float("nan"), device=DEV) for _ in range(2))
    both(HipError, q=wide, qT=wideT, kp=kw, vp=vw)              # hd = 129
    with pytest.raises(HipError):
        F.attention_stream_pools(4, H, 129, R, device=DEV)
    both(ValueError, bf16=True)                                 # fp32 pools in bf16 mode
    torch.cuda.synchronize()
    assert torch.isnan(kp).all() and torch.isnan(vp).all() and torch.isnan(flat).all(), "a refused call launched something"
    assert torch.all(table == 0)
