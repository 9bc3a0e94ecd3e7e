"""The chunk rule of streaming prefill, without a GPU: tests/golden/stream_chunk_ref.py (explicit cache rows, positions u % C, the
last-C store rule) pinned against `stream_ref._Site.attend` called row by row; the chunk schedule as a pure function; and the
host-side refusals of `model.stream(max_chunk=...)` / `DialogueStream.prefill`."""
import pytest
import torch

import stream_chunk_ref as CR
import stream_ref
import synth
from mer_amd import streaming
from mer_amd.model import M2FNet

H, HD = 2, 5
E = H * HD

# (C, ring, chunk lengths): below, at and above C; wraps in mid-chunk; a plain cache filled exactly to its last row
SEQUENCES = [
    (1, True, [1, 1, 3, 2]), (1, False, [1]),
    (3, True, [1, 2, 3, 5, 2, 7, 1]), (3, True, [2, 2, 2]), (3, True, [4]), (3, False, [1, 2]), (3, False, [3]),
    (9, True, [4, 9, 3, 11, 8, 19, 1, 9]), (9, True, [8, 2, 9]), (9, False, [2, 3, 4]), (9, False, [9]), (9, False, [1, 1, 1]),
]


def _rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(n, E, generator=g, dtype=torch.float64) for _ in range(3))


@pytest.mark.parametrize("C,ring,chunks", SEQUENCES)
def test_chunks_equal_row_by_row_attend_in_outputs_and_kept_rows(C, ring, chunks):
    site = stream_ref._Site(C - 1 if ring else None)
    kc, vc = CR.new_caches(C, E)
    n_old = 0
    for ci, n in enumerate(chunks):
        q, k, v = _rows(n, 100 * C + 10 * ci + int(ring))
        wrap = ring and n_old % C + n > C
        before_k = kc.clone()
        out = CR.chunk_attend(kc, vc, n_old, q, k, v, H, ring)
        want = torch.stack([site.attend(q[t], k[t], v[t], H) for t in range(n)])
        assert torch.isfinite(out).all(), "a dead row was read"
        assert (out - want).abs().max().item() < 1e-12, (C, ring, ci, wrap)
        n_old += n
        # the kept rows: the site's list holds the last min(n_old, C) utterances in order; utterance j lives in row j % C (ring) / j
        first = n_old - len(site.k)
        assert len(site.k) == (min(n_old, C) if ring else n_old)
        for i, (rk, rv) in enumerate(zip(site.k, site.v)):
            pos = CR.position(first + i, C, ring)
            assert torch.equal(kc[pos], rk) and torch.equal(vc[pos], rv)
        # every row the chunk did not store is bit-untouched (NaN rows compare as bits)
        stored = {pos for _, pos in CR.stored_rows(n_old - n, n, C, ring)}
        for r in range(C):
            if r not in stored:
                assert torch.equal(kc[r].view(torch.int64), before_k[r].view(torch.int64))
    if not ring:
        assert torch.isnan(kc[n_old:]).all() and torch.isfinite(kc[:n_old]).all()


def test_the_sequences_cover_wraps_in_mid_chunk_and_chunks_longer_than_the_ring():
    wraps = longer = exact = 0
    for C, ring, chunks in SEQUENCES:
        n_old = 0
        for n in chunks:
            wraps += ring and n_old >= 1 and n_old % C != 0 and n_old % C + n > C
            longer += ring and n > C
            n_old += n
        exact += (not ring) and n_old == C
    assert wraps >= 6 and longer >= 6 and exact >= 4


def test_a_plain_cache_refuses_a_chunk_past_its_last_row():
    kc, vc = CR.new_caches(3, E)
    with pytest.raises(ValueError):
        CR.chunk_attend(kc, vc, 2, *_rows(2, 0), H, False)


def test_only_the_last_C_rows_of_a_long_chunk_are_stored():
    assert CR.stored_rows(5, 7, 3, True) == [(4, 0), (5, 1), (6, 2)]
    assert CR.stored_rows(2, 2, 3, True) == [(0, 2), (1, 0)]
    assert CR.stored_rows(2, 4, 9, False) == [(0, 2), (1, 3), (2, 4), (3, 5)]
    assert CR.stored_rows(0, 5, 1, True) == [(4, 0)]


# ---- the chunk schedule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 4, 16, 64])
@pytest.mark.parametrize("counts", [[0], [1], [64], [65], [0, 0, 0], [3, 0, 17, 64, 1], [128, 127, 129, 0], [512, 300]])
def test_chunk_schedule_sums_to_the_counts_in_entries_of_at_most_T(counts, T):
    calls = streaming.chunk_schedule(counts, T)
    assert len(calls) == (max(counts) + T - 1) // T
    assert all(len(c) == len(counts) and all(0 <= x <= T for x in c) for c in calls)
    assert [sum(c[s] for c in calls) for s in range(len(counts))] == counts
    for s, n in enumerate(counts):                       # a slot's rows go in order: full chunks, one remainder, then nothing
        col = [c[s] for c in calls]
        assert col == [T] * (n // T) + ([n % T] if n % T else []) + [0] * (len(calls) - (n + T - 1) // T)
    assert all(any(c) for c in calls), "no empty call"


def test_chunk_schedule_refuses_bad_arguments():
    with pytest.raises(ValueError):
        streaming.chunk_schedule([1, 2], 0)
    with pytest.raises(ValueError):
        streaming.chunk_schedule([1, -1], 4)


def test_prefix_counts_sees_the_collate_layout_only():
    v = torch.tensor([[1, 1, 1, 0], [1, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1]], dtype=torch.bool)
    assert streaming.prefix_counts(v) == [3, 1, 0, 4]
    v[1, 2] = True                                        # a hole: not a prefix
    assert streaming.prefix_counts(v) is None


# ---- refusals, before the GPU is touched -----------------------------------------------------------------------------------------------
def _model(context):
    return M2FNet(synth._cfg(48, 64, 64, 4, 4, 4, 1, 1, 1, dropout=0.0), context=context)


@pytest.mark.parametrize("max_chunk", [0, -1, 65, 1024, 2.0, True, None, "16"])
def test_max_chunk_outside_1_to_64_is_refused(max_chunk):
    with pytest.raises(ValueError, match="max_chunk"):
        _model((None, 0)).eval().stream(4, max_chunk=max_chunk)
    with pytest.raises(ValueError, match="max_chunk"):
        streaming.resolve_max_chunk(max_chunk)


def test_max_chunk_in_range_is_accepted():
    assert [streaming.resolve_max_chunk(t) for t in (1, 2, 16, 64)] == [1, 2, 16, 64]


def test_a_history_past_the_capacity_is_refused_for_the_whole_call():
    streaming.check_prefill_fits([0, 500, 512], [512, 12, 0], 512, None)            # to the last row; a full slot that takes nothing
    with pytest.raises(RuntimeError, match="capacity"):
        streaming.check_prefill_fits([0, 500], [4, 13], 512, None)
    with pytest.raises(RuntimeError, match=r"slot\(s\) \[1\]"):
        streaming.check_prefill_fits([0, 3], [4, 2], 4, None)
    streaming.check_prefill_fits([10 ** 6], [600], 9, 8)                             # a ring has no length limit
