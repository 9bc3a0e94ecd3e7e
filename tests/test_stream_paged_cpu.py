"""The host side of the paged streaming caches, without a GPU: streaming.PageAllocator (lowest id first, one page per boundary
crossed, a ring's bound, reset and reuse, exhaustion that changes nothing, table against lists), the sizes (`pages_needed`,
`cache_bytes_paged`), the float64 reference of paged addressing (tests/golden/stream_paged_ref.py) against the dense reference on the
same histories, the plan's sizing pass at 4,096 slots, and the settings that are refused before the GPU is touched."""
import ctypes
import os
import random

import pytest
import torch
import yaml

import stream_paged_ref as PR
import stream_ref
import synth
import mer_amd  # noqa: F401
from mer_amd import layout, runtime, streaming
from mer_amd.streaming import PageAllocator, pages_needed

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _shipped():
    with open(os.path.join(ROOT, "src", "config.yaml")) as f:
        return layout.M2FConfig.from_model_config(yaml.safe_load(f)["model"])


def _consistent(al):
    held = [p for pages in al.slot_pages for p in pages]
    assert len(held) == len(set(held)), "a page is held twice"
    assert sorted(held + sorted(al._free)) == list(range(al.pages)), "a page is lost or both free and held"
    assert al.pages_free == al.pages - len(held)
    for s, pages in enumerate(al.slot_pages):
        assert al.table[s, :len(pages)].tolist() == pages, "the table differs from the slot's list"
    assert al.table.dtype == torch.int32 and al.table.shape == (al.slots, -(-al.capacity // al.page_rows))


def _grow(al, lengths, new, ring):
    """what DialogueStream does before a call: the pages for new[s] more utterances per slot"""
    al.take(pages_needed(lengths, new, al.capacity, al.page_rows, ring))
    return [n + a for n, a in zip(lengths, new)]


# ---- allocator --------------------------------------------------------------------------------------------------------------------
def test_the_lowest_free_id_goes_first_and_slots_interleave():
    al = PageAllocator(8, 3, 64, 16)
    assert al.pages_free == 8 and al.table.eq(0).all()
    al.take([1, 1, 1])
    assert al.slot_pages == [[0], [1], [2]]
    al.take([1, 0, 2])
    assert al.slot_pages == [[0, 3], [1], [2, 4, 5]] and al.pages_free == 2
    _consistent(al)


@pytest.mark.parametrize("R", [16, 32, 64])
def test_a_slot_takes_exactly_one_page_when_it_crosses_a_page_boundary(R):
    al = PageAllocator(6, 2, 512, R)
    lengths = [0, 0]
    for step in range(2 * R + 1):
        held = [len(p) for p in al.slot_pages]
        lengths = _grow(al, lengths, [1, 0], False)
        gained = len(al.slot_pages[0]) - held[0]
        assert gained == (1 if step % R == 0 else 0), f"row {step}: {gained} page(s)"      # rows 0, R, 2R open a page; R-1 -> R: one
        assert len(al.slot_pages[1]) == 0
    assert al.slot_pages[0] == [0, 1, 2] and lengths == [2 * R + 1, 0]
    _consistent(al)


@pytest.mark.parametrize("past,R", [(0, 16), (2, 16), (16, 16), (40, 16), (40, 32), (99, 64)])
def test_a_ring_never_holds_more_than_its_rows_need_however_long_the_dialogue(past, R):
    C = past + 1
    bound = -(-C // R)
    al = PageAllocator(bound + 1, 1, C, R)
    lengths = [0]
    for _ in range(3 * C + 5):
        lengths = _grow(al, lengths, [1], True)
        assert len(al.slot_pages[0]) == min(-(-lengths[0] // R), bound)
    lengths = _grow(al, lengths, [2 * C + 1], True)             # a chunk longer than the ring
    assert len(al.slot_pages[0]) == bound and al.pages_free == 1
    _consistent(al)


def test_reset_returns_pages_and_they_are_handed_out_again():
    al = PageAllocator(6, 3, 64, 16)
    al.take([2, 1, 3])
    assert al.pages_free == 0 and al.slot_pages == [[0, 1], [2], [3, 4, 5]]
    al.release([0, 2])
    assert al.pages_free == 5 and al.slot_pages == [[], [2], []]
    al.take([0, 2, 1])                                          # the returned pages, the lowest first
    assert al.slot_pages == [[], [2, 0, 1], [3]] and al.pages_free == 2
    _consistent(al)
    al.release()
    assert al.pages_free == 6 and all(p == [] for p in al.slot_pages)
    _consistent(al)


def test_exhaustion_raises_naming_the_slots_and_changes_nothing():
    al = PageAllocator(4, 4, 64, 16)
    al.take([1, 0, 2, 0])
    al.dirty = False
    before = ([list(p) for p in al.slot_pages], al.table.clone(), sorted(al._free))
    with pytest.raises(RuntimeError, match=r"slot\(s\) \[3\]") as e:
        al.take([0, 1, 0, 1])                                   # one page left: slot 1 gets it, slot 3 goes without
    assert "1 free of 4" in str(e.value)
    with pytest.raises(RuntimeError, match=r"slot\(s\) \[1, 2\]"):
        al.take([0, 2, 1, 0])
    assert ([list(p) for p in al.slot_pages], sorted(al._free)) == (before[0], before[2])
    assert torch.equal(al.table, before[1]) and not al.dirty
    with pytest.raises(ValueError):
        al.take([1, 1])                                         # not one count per slot
    with pytest.raises(ValueError):
        al.take([0, 0, 3, 0])                                   # more pages than a slot's rows can use
    al.take([0, 1, 0, 0])
    assert al.pages_free == 0 and al.dirty
    _consistent(al)


def test_the_table_follows_a_random_run_of_growth_and_resets():
    rng = random.Random(5)
    S, C, R = 7, 100, 16
    al = PageAllocator(20, S, C, R)
    lengths = [0] * S
    for _ in range(300):
        if rng.random() < 0.15:
            slots = rng.sample(range(S), rng.randint(1, 3))
            al.release(slots)
            for s in slots:
                lengths[s] = 0
        new = [rng.choice([0, 1, 1, 3, 17]) if rng.random() < 0.6 else 0 for _ in range(S)]
        new = [min(a, C - n) for n, a in zip(lengths, new)]
        need = pages_needed(lengths, new, C, R, False)
        if sum(need) > al.pages_free:
            with pytest.raises(RuntimeError):
                al.take(need)
        else:
            lengths = _grow(al, lengths, new, False)
        _consistent(al)
        assert [len(p) for p in al.slot_pages] == [-(-n // R) for n in lengths]


# ---- sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [16, 32, 64])
@pytest.mark.parametrize("C", [1, 3, 17, 65, 512])
def test_pages_needed_at_the_counts_around_a_page_and_the_capacity(C, R):
    pages = lambda rows: -(-rows // R)          # noqa: E731
    counts = sorted({n for n in (0, 1, R - 1, R, R + 1, C - 1) if 0 <= n <= C})
    for ring in (False, True):
        for n in counts + ([C, 2 * C + 1] if ring else []):
            assert pages_needed([0], [n], C, R, ring) == [pages(min(n, C))], (n, ring)           # from an empty slot: what it holds
            if ring or n < C:
                step = pages_needed([n], [1], C, R, ring)[0]
                assert step == (1 if n < C and n % R == 0 else 0), (n, ring, step)                  # the next utterance
            for a in (0, 1, R, C):
                if ring or n + a <= C:
                    assert pages_needed([n], [a], C, R, ring) == [pages(min(n + a, C)) - pages(min(n, C))]
    with pytest.raises(ValueError):
        pages_needed([C], [1], C, R, False)
    assert pages_needed([0, R - 1, R], [1, 1, 1], 512, R, False) == [1, 0, 1]


def test_cache_bytes_paged_equals_the_dense_bytes_at_the_same_number_of_rows():
    for cfg in (_shipped(), layout.M2FConfig.from_model_config(synth.CASES["tiny_odd_heads"][0])):
        for bf16 in (False, True):
            for S, C, R in ((64, 512, 16), (8, 64, 32), (3, 64, 64)):
                assert streaming.cache_bytes_paged(cfg, S * C // R, R, bf16) == streaming.cache_bytes(cfg, S, C, bf16)
            assert streaming.cache_bytes_paged(cfg, 10, 32, bf16) == 2 * streaming.cache_bytes_paged(cfg, 10, 16, bf16)
    # the issue's figure: 2,048 pages of 16 rows are the 64 x 512 rows of the dense C3 stream
    assert streaming.cache_bytes_paged(_shipped(), 2048, 16) == streaming.cache_bytes(_shipped(), 64, 512)


# ---- the reference of paged addressing --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring,C,R", [(False, 40, 16), (True, 5, 16), (True, 37, 16), (True, 37, 32), (False, 70, 64)])
def test_paged_reference_equals_the_dense_reference_on_the_same_histories(ring, C, R):
    """ragged dialogues fed in an interleaved order, a reset in mid-run whose pages go to other slots: every output equals, bit for
    bit in float64, what a dense per-slot site gives"""
    rng = random.Random(C * R + ring)
    S, H, hd = 4, 3, 5
    E = H * hd
    al = PageAllocator(S * -(-C // R) - 1, S, C, R)
    site = PR.PagedSite(al.pages, R, C, ring, E)
    dense = [stream_ref._Site(C - 1 if ring else None) for _ in range(S)]
    lengths = [0] * S
    g = torch.Generator().manual_seed(3)
    limit = 3 * C if ring else C
    rounds = 6 * max(C, 40)
    for it in range(rounds):
        s = rng.randrange(S)
        if it == rounds // 2:                                       # two slots start over; their pages go back to the pool
            for r in (0, 2):
                al.release([r])
                lengths[r], dense[r] = 0, stream_ref._Site(C - 1 if ring else None)
        if lengths[s] >= limit:
            continue
        need = pages_needed(lengths, [int(i == s) for i in range(S)], C, R, ring)
        if sum(need) > al.pages_free:
            continue
        al.take(need)
        q, k, v = (torch.randn(E, generator=g, dtype=torch.float64) for _ in range(3))
        got = site.attend(q, k, v, H, al.table[s].tolist(), lengths[s])
        want = dense[s].attend(q, k, v, H)
        assert torch.isfinite(got).all() and torch.equal(got, want), (it, s, lengths[s])
        lengths[s] += 1
    assert max(lengths) > min(R, C), "no dialogue crossed a page boundary or wrapped its ring"
    pages = [p for ps in al.slot_pages for p in ps]
    assert pages != sorted(pages) or len(pages) < 2, "the pages of the slots never interleaved"


# ---- the plan's sizing pass -------------------------------------------------------------------------------------------------------
def test_a_paged_plan_sizes_for_4096_slots_and_its_memory_follows_the_pages():
    cfg = _shipped()
    cc, lib = runtime.config_to_c(cfg), runtime.lib()
    size = lambda S, pages, R=16, prec=runtime.BF16: lib.m2f_stream_paged_workspace_bytes(ctypes.byref(cc), S, 512, -1, prec, pages, R, 1)  # noqa: E731
    n4096 = size(4096, 2048)
    assert n4096 > 0, lib.m2f_last_error()
    pools = streaming.cache_bytes_paged(cfg, 2048, 16, bf16=True)
    dense64 = lib.m2f_stream_workspace_bytes(ctypes.byref(cc), 64, 512, -1, runtime.BF16, 1)
    assert pools == streaming.cache_bytes(cfg, 64, 512, bf16=True) < dense64
    assert pools < n4096 < dense64 + 4096 * 2 * 2 ** 20          # 4,096 slots on the memory of 64 dense ones, plus activations per row
    slack = 2 ** 20                                               # (the arena aligns every buffer: the sums differ by its gaps)
    assert abs(size(4096, 4096) - n4096 - pools) < slack          # the pools grow with the pages ...
    assert 0 < size(512, 2048) < n4096                            # ... and only activations and the table with the slots
    assert abs(size(64, 2048, 32) - size(64, 2048, 16) - pools) < slack
    for bad in (8, 0, 48, 128):
        assert size(64, 16, bad) < 0 and b"page_rows" in lib.m2f_last_error()
    assert size(64, 0) < 0 and b"n_pages" in lib.m2f_last_error()


# ---- settings ---------------------------------------------------------------------------------------------------------------------
def test_settings_are_refused_on_the_host():
    assert streaming.resolve_pages(None, 16) == (None, 16) and streaming.resolve_pages(320, 64) == (320, 64)
    for pages, rows in ((0, 16), (-1, 16), (True, 16), (1.5, 16), (4, 8), (4, 48), (4, True), (None, 17)):
        with pytest.raises(ValueError):
            streaming.resolve_pages(pages, rows)
    from mer_amd.model import M2FNet
    m = M2FNet(synth.CASES["tiny_ragged"][0], context=(None, 0)).eval()
    with pytest.raises(ValueError, match="page_rows"):
        m.stream(4, pages=8, page_rows=24)
    with pytest.raises(ValueError, match="pages"):
        m.stream(4, pages=0)


def test_runtime_stream_pages_is_read_and_validated_before_the_gpu_is_touched():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "src"))
    import test as te
    from utils import AttrDict
    with open(os.path.join(ROOT, "src", "config.yaml")) as f:
        raw = yaml.safe_load(f)
    assert raw["runtime"]["stream_pages"] == 0
    cfg = AttrDict(raw)
    assert te.stream_pages_settings(cfg) == 0
    for value, want in ((None, 0), (0, 0), (1, 1), (2048, 2048)):
        cfg.runtime = AttrDict(dict(raw["runtime"], stream_pages=value))
        assert te.stream_pages_settings(cfg) == want
    for value in (-1, True, 2.5, "many"):
        cfg.runtime = AttrDict(dict(raw["runtime"], stream_pages=value))
        with pytest.raises(ValueError, match="runtime.stream_pages"):
            te.stream_pages_settings(cfg)
