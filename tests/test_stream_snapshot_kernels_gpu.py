"""functional.attention_stream_cache_gather / _scatter (csrc/stream_cache.hip), one site through the kernel-level C entries, bit for bit.

Dense: H = 3, hd = 5 (pad 8 in fp32 and bf16) and 12 (bf16 pad 16), C = 5, entries of lengths {0, 1, 4, 5, 7, 13} - min(length, C) rows
each - in shuffled slots among bystanders.  `ring=False` fills the caches with random BIT PATTERNS, pad columns included (the kernels
move bytes); `ring=True` fills them by stepping the ring form of the attention kernel until the slots hold those lengths, so the rings
have wrapped with len % C != 0, and also checks that a step on the restored caches gives the bits of a step on the original ones.
Paged: C = 40, page_rows = 16, a shuffled table on a pool of 9 pages, lengths {0, 1, 16, 17, 40}: runs that cross a page boundary, a
partly filled last page, two pages nobody holds.

Gather equals a reference built by indexing, and leaves a guard band behind the packed rows alone; scatter into caches pre-filled
with a sentinel bit pattern writes the live rows and the counts and no other byte (rows past the entry's, other slots, unheld pages);
gather after scatter returns the packed bytes; the dense and the paged form give the same packed bytes from the same logical state."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402

DEV = "cuda"
H = 3
GUARD = 64                                      # elements behind the packed rows that no launch may touch
COUNT_SENTINEL = -77


def _dt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _pad(hd, bf16):
    q = 8 if bf16 else 4
    return -(-hd // q) * q


def _random_bits(shape, bf16, seed):
    g = torch.Generator().manual_seed(seed)
    if bf16:
        return torch.randint(-2 ** 15, 2 ** 15, shape, generator=g, dtype=torch.int16).to(DEV).view(torch.bfloat16)
    return torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, dtype=torch.int64).to(torch.int32).to(DEV).view(torch.float32)


def _sentinel(shape, bf16):
    """a NaN with a payload: any byte written shows in the integer view"""
    if bf16:
        return torch.full(shape, 0x7FC1, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    return torch.full(shape, 0x7FC12345, dtype=torch.int32, device=DEV).view(torch.float32)


def _is_sentinel(t):
    return bool(torch.all(_bits(t) == (0x7FC1 if t.dtype == torch.bfloat16 else 0x7FC12345)))


def _entries(slots, lengths, C):
    rows = [min(n, C) for n in lengths]
    offsets = [sum(rows[:e]) for e in range(len(rows))]
    dev = lambda x, dt: torch.tensor(x, dtype=dt, device=DEV)       # noqa: E731
    return rows, offsets, dev(slots, torch.int32), dev(lengths, torch.int32), dev(offsets, torch.int64)


def _reference(kc, vc, slots, rows):
    """[K, V][H][rows_e][pad(hd)] of slot slots[e] per entry, by indexing dense [S][H][C][pad(hd)] caches"""
    parts = []
    for s, r in zip(slots, rows):
        parts += [kc[s, :, :r].reshape(-1), vc[s, :, :r].reshape(-1)]
    return torch.cat(parts)


def _packed_buffer(n, bf16):
    return _sentinel((n + GUARD,), bf16)


# ---- dense ------------------------------------------------------------------------------------------------------------------------
S_DENSE, C_DENSE = 8, 5
LENGTHS = [0, 1, 4, 5, 7, 13]
SLOTS = [5, 0, 7, 2, 3, 6]                      # slots 1 and 4 are bystanders


def _ring_state(hd, bf16, seed):
    """The caches after stepping the ring kernel until slot SLOTS[e] holds LENGTHS[e] utterances (bystanders: 3), NaN-free live rows,
    zero pad columns, stale sentinel rows where nothing was stored yet."""
    lens = [3] * S_DENSE
    for s, n in zip(SLOTS, LENGTHS):
        lens[s] = n
    kc, vc = _sentinel((S_DENSE, H, C_DENSE, _pad(hd, bf16)), bf16), _sentinel((S_DENSE, H, C_DENSE, _pad(hd, bf16)), bf16)
    count = torch.zeros(S_DENSE, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(seed)
    for i in range(max(lens)):
        qkv = torch.randn(S_DENSE, 3 * H * hd + 8, generator=g).to(DEV)
        act = torch.tensor([n > i for n in lens], device=DEV)
        F.attention_stream(qkv[:, : H * hd], qkv[:, H * hd: 2 * H * hd], qkv[:, 2 * H * hd: 3 * H * hd], kc, vc, count, act, H, ring=True,
                           bf16=bf16)
        count += act.to(torch.int32)
    assert count.tolist() == lens
    return kc, vc, lens


def _dense_state(hd, bf16, ring, seed):
    if ring:
        return _ring_state(hd, bf16, seed)
    shape = (S_DENSE, H, C_DENSE, _pad(hd, bf16))
    lens = [3] * S_DENSE
    for s, n in zip(SLOTS, LENGTHS):
        lens[s] = n
    return _random_bits(shape, bf16, seed), _random_bits(shape, bf16, seed + 1), lens


@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("hd", [5, 12])
def test_dense_gather_scatter_round_trip(hd, bf16, ring):
    kc, vc, lens = _dense_state(hd, bf16, ring, seed=hd + 2 * bf16)
    kc0, vc0 = kc.clone(), vc.clone()
    rows, offsets, slots, lengths, offs = _entries(SLOTS, LENGTHS, C_DENSE)
    assert rows == [0, 1, 4, 5, 5, 5]
    W = 2 * H * _pad(hd, bf16)
    total = sum(rows) * W
    want = _reference(kc, vc, SLOTS, rows)
    assert want.numel() == total

    # gather: the reference's bits, nothing behind them, the caches only read
    packed = F.attention_stream_cache_gather(kc, vc, hd, slots, lengths, offs, _packed_buffer(total, bf16), bf16=bf16)
    assert torch.equal(_bits(packed[:total]), _bits(want)), "gather differs from the indexed reference"
    assert _is_sentinel(packed[total:]), "the guard band behind the packed rows was written"
    assert torch.equal(_bits(kc), _bits(kc0)) and torch.equal(_bits(vc), _bits(vc0))

    # scatter into sentinel caches, other slots: the live rows and the counts, no other byte
    target = [2, 6, 1, 7, 0, 4]
    _, _, tslots, _, _ = _entries(target, LENGTHS, C_DENSE)
    k2, v2 = _sentinel(kc.shape, bf16), _sentinel(vc.shape, bf16)
    count = torch.full((S_DENSE,), COUNT_SENTINEL, dtype=torch.int32, device=DEV)
    F.attention_stream_cache_scatter(k2, v2, hd, tslots, lengths, offs, packed, count, bf16=bf16)
    wk, wv, wc = _sentinel(kc.shape, bf16), _sentinel(vc.shape, bf16), [COUNT_SENTINEL] * S_DENSE
    for src, dst, r, n in zip(SLOTS, target, rows, LENGTHS):
        wk[dst, :, :r], wv[dst, :, :r] = kc[src, :, :r], vc[src, :, :r]
        wc[dst] = n
    assert torch.equal(_bits(k2), _bits(wk)) and torch.equal(_bits(v2), _bits(wv)), "scatter wrote a wrong byte or one too many"
    assert count.tolist() == wc, "count[slot] = length for the listed slots, the others untouched"
    assert _is_sentinel(k2[3]) and _is_sentinel(k2[5]) and _is_sentinel(k2[6, :, 1:])          # bystanders, rows past the entry's

    # gather after scatter: the packed bytes
    again = F.attention_stream_cache_gather(k2, v2, hd, tslots, lengths, offs, _packed_buffer(total, bf16), bf16=bf16)
    assert torch.equal(_bits(again), _bits(packed))

    if ring:    # one more step of every restored dialogue gives the bits of that step on the original caches
        g = torch.Generator().manual_seed(99)
        qkv = torch.randn(S_DENSE, 3 * H * hd + 8, generator=g).to(DEV)
        perm = torch.tensor(SLOTS, device=DEV)
        q2 = torch.zeros_like(qkv)
        q2[torch.tensor(target, device=DEV)] = qkv[perm]
        d = H * hd
        act = torch.zeros(S_DENSE, dtype=torch.bool, device=DEV)
        act[perm] = True
        act2 = torch.zeros_like(act)
        act2[torch.tensor(target, device=DEV)] = True
        out = F.attention_stream(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:3 * d], kc, vc, torch.tensor(lens, dtype=torch.int32, device=DEV),
                                 act, H, ring=True, bf16=bf16)
        out2 = F.attention_stream(q2[:, :d], q2[:, d:2 * d], q2[:, 2 * d:3 * d], k2, v2, count.clamp(min=0), act2, H, ring=True, bf16=bf16)
        assert torch.isfinite(out[perm]).all()
        assert torch.equal(out2[torch.tensor(target, device=DEV)], out[perm]), "a step on the restored ring differs"


# ---- paged ------------------------------------------------------------------------------------------------------------------------
C_PAGED, R, N_PAGES = 40, 16, 9
P_LENGTHS = [0, 1, 16, 17, 40]
P_SLOTS = [3, 1, 4, 0, 2]
TABLE = {1: [6], 4: [2], 0: [8, 0], 2: [5, 7, 3]}               # pages 1 and 4 are held by nobody
CANARY = 4


def _table():
    t = torch.full((5, 3), CANARY, dtype=torch.int32)
    for s, pages in TABLE.items():
        t[s, : len(pages)] = torch.tensor(pages, dtype=torch.int32)
    assert not torch.equal(t[:, 0], torch.arange(5, dtype=torch.int32))
    return t.to(DEV)


def _to_pools(kc, vc, bf16, fill_bits):
    """the dense logical caches' rows through the table into pools holding `fill_bits` elsewhere (whole pages of the held entries)"""
    shape = (N_PAGES, H, R, kc.shape[3])
    kp, vp = (_sentinel(shape, bf16), _sentinel(shape, bf16)) if fill_bits is None else (_random_bits(shape, bf16, fill_bits),
                                                                                      _random_bits(shape, bf16, fill_bits + 1))
    for s, pages in TABLE.items():
        for e, page in enumerate(pages):
            n = min(R, C_PAGED - e * R)
            kp[page, :, :n], vp[page, :, :n] = kc[s, :, e * R: e * R + n], vc[s, :, e * R: e * R + n]
    return kp, vp


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("hd", [5, 12])
def test_paged_gather_scatter_and_the_dense_form_give_the_same_bytes(hd, bf16):
    shape = (5, H, C_PAGED, _pad(hd, bf16))
    kc, vc = _random_bits(shape, bf16, 11 + hd), _random_bits(shape, bf16, 12 + hd)
    kp, vp = _to_pools(kc, vc, bf16, fill_bits=40 + hd)
    kp0, vp0 = kp.clone(), vp.clone()
    table = _table()
    rows, offsets, slots, lengths, offs = _entries(P_SLOTS, P_LENGTHS, C_PAGED)
    assert rows == P_LENGTHS
    total = sum(rows) * 2 * H * _pad(hd, bf16)
    want = _reference(kc, vc, P_SLOTS, rows)

    dense = F.attention_stream_cache_gather(kc, vc, hd, slots, lengths, offs, _packed_buffer(total, bf16), bf16=bf16)
    paged = F.attention_stream_cache_gather(kp, vp, hd, slots, lengths, offs, _packed_buffer(total, bf16), table=table, capacity=C_PAGED,
                                            bf16=bf16)
    assert torch.equal(_bits(paged[:total]), _bits(want)), "paged gather differs from the indexed reference"
    assert torch.equal(_bits(paged), _bits(dense)), "the dense and the paged form must give the same packed bytes"
    assert _is_sentinel(paged[total:])
    assert torch.equal(_bits(kp), _bits(kp0)) and torch.equal(_bits(vp), _bits(vp0))

    # scatter into sentinel pools through the same table: the live rows only - not the rest of a partly filled page, not pages 1 and 4
    k2, v2 = _sentinel(kp.shape, bf16), _sentinel(vp.shape, bf16)
    count = torch.full((5,), COUNT_SENTINEL, dtype=torch.int32, device=DEV)
    F.attention_stream_cache_scatter(k2, v2, hd, slots, lengths, offs, paged, count, table=table, capacity=C_PAGED, bf16=bf16)
    wk, wv = _sentinel(kp.shape, bf16), _sentinel(vp.shape, bf16)
    for s, r in zip(P_SLOTS, rows):
        for e in range(-(-r // R)):
            n = min(R, r - e * R)
            page = TABLE[s][e]
            wk[page, :, :n], wv[page, :, :n] = kc[s, :, e * R: e * R + n], vc[s, :, e * R: e * R + n]
    assert torch.equal(_bits(k2), _bits(wk)) and torch.equal(_bits(v2), _bits(wv)), "paged scatter wrote a wrong byte or one too many"
    assert _is_sentinel(k2[1]) and _is_sentinel(k2[CANARY]) and _is_sentinel(v2[1]) and _is_sentinel(v2[CANARY]), "an unheld page was written"
    assert _is_sentinel(k2[0, :, 1:]) and _is_sentinel(k2[3, :, 8:]), "rows past the entry's in its last page"
    want_count = [COUNT_SENTINEL] * 5
    for s, n in zip(P_SLOTS, P_LENGTHS):
        want_count[s] = n
    assert count.tolist() == want_count

    again = F.attention_stream_cache_gather(k2, v2, hd, slots, lengths, offs, _packed_buffer(total, bf16), table=table, capacity=C_PAGED,
                                            bf16=bf16)
    assert torch.equal(_bits(again), _bits(paged))

    # paged -> dense: the packed bytes of one form restore the other
    k3, v3 = _sentinel(kc.shape, bf16), _sentinel(vc.shape, bf16)
    F.attention_stream_cache_scatter(k3, v3, hd, slots, lengths, offs, paged, count, bf16=bf16)
    for s, r in zip(P_SLOTS, rows):
        assert torch.equal(_bits(k3[s, :, :r]), _bits(kc[s, :, :r])) and _is_sentinel(k3[s, :, r:])
        assert torch.equal(_bits(v3[s, :, :r]), _bits(vc[s, :, :r])) and _is_sentinel(v3[s, :, r:])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_out_of_range_entries_are_skipped_and_bad_arguments_refused():
    hd, bf16 = 5, False
    shape = (S_DENSE, H, C_DENSE, _pad(hd, bf16))
    kc, vc = _random_bits(shape, bf16, 1), _random_bits(shape, bf16, 2)
    W = 2 * H * _pad(hd, bf16)
    # entries: a good one, a slot past S, a negative length, rows past the end of the buffer
    slots = torch.tensor([2, S_DENSE, 1, 3], dtype=torch.int32, device=DEV)
    lengths = torch.tensor([2, 2, -1, 5], dtype=torch.int32, device=DEV)
    offs = torch.tensor([0, 2, 4, 6], dtype=torch.int64, device=DEV)
    packed = _sentinel((8 * W,), bf16)                          # rows 6 .. 10 of the last entry do not fit 8 rows
    F.attention_stream_cache_gather(kc, vc, hd, slots, lengths, offs, packed, bf16=bf16)
    assert torch.equal(_bits(packed[: 2 * W]), _bits(_reference(kc, vc, [2], [2]))) and _is_sentinel(packed[2 * W:])
    k2, v2 = _sentinel(shape, bf16), _sentinel(shape, bf16)
    count = torch.full((S_DENSE,), COUNT_SENTINEL, dtype=torch.int32, device=DEV)
    F.attention_stream_cache_scatter(k2, v2, hd, slots, lengths, offs, packed, count, bf16=bf16)
    assert count.tolist() == [COUNT_SENTINEL, COUNT_SENTINEL, 2] + [COUNT_SENTINEL] * 5
    assert _is_sentinel(k2[:2]) and _is_sentinel(k2[3:]) and _is_sentinel(k2[2, :, 2:])

    HipError = mer_amd.runtime.HipError
    good = (slots[:1], lengths[:1], offs[:1])
    with pytest.raises(ValueError):
        F.attention_stream_cache_gather(kc, vc, hd, *good, packed, bf16=True)               # fp32 caches in bf16 mode
    with pytest.raises(ValueError):
        F.attention_stream_cache_gather(kc, vc, hd, good[0], good[1], offs[:1].to(torch.int32), packed, bf16=bf16)
    with pytest.raises(HipError):
        F.attention_stream_cache_gather(kc, vc, hd, *good, packed[1:], bf16=bf16)           # 4 bytes off a 16-byte boundary
    wide = torch.zeros(2, H, 4, 132, device=DEV)
    with pytest.raises(HipError):
        F.attention_stream_cache_gather(wide, wide.clone(), 129, *good, packed, bf16=bf16)  # hd = 129
    pool = torch.zeros(4, H, 16, 8, device=DEV)
    with pytest.raises(HipError):                                                           # not ceil(40 / 16) table columns
        F.attention_stream_cache_gather(pool, pool.clone(), hd, *good, packed, table=torch.zeros(S_DENSE, 2, dtype=torch.int32, device=DEV),
                                        capacity=40, bf16=bf16)
    torch.cuda.synchronize()
    assert _is_sentinel(packed[2 * W:])
