"""The host side of stream snapshots, without a GPU: the layout arithmetic of the packed format (row width, row offsets, segment starts)
against a torch reference built by indexing [S][H][C][pad(hd)] tensors, the signature, StreamSnapshot's select / state_dict /
from_state_dict / torch.save round trip on CPU tensors, the validation errors that need no device, and the page arithmetic of the
all-or-nothing restore on streaming.PageAllocator alone."""
import io

import pytest
import torch

import synth
import mer_amd  # noqa: F401
from mer_amd import streaming
from mer_amd.layout import M2FConfig
from mer_amd.streaming import PageAllocator, StreamSnapshot

SITES = ((3, 5), (2, 12), (3, 5))          # (H, hd): pads 8 / 12 in fp32, 8 / 16 in bf16


def _pad(hd, bf16):
    q = 8 if bf16 else 4
    return -(-hd // q) * q


def _caches(sites, S, C, bf16, seed=0):
    """Per site (K, V) as [S][H][C][pad(hd)], every element a different value"""
    g = torch.Generator().manual_seed(seed)
    dt = torch.bfloat16 if bf16 else torch.float32
    return [tuple(torch.randn(S, H, C, _pad(hd, bf16), generator=g).to(dt) for _ in range(2)) for H, hd in sites]


def _reference(caches, slots, rows):
    """The packed tensor by indexing: entry e = [site][K, V][H][rows_e][pad(hd)] of slot slots[e], entries concatenated"""
    parts = []
    for s, r in zip(slots, rows):
        for k, v in caches:
            parts += [k[s, :, :r].reshape(-1), v[s, :, :r].reshape(-1)]
    return torch.cat(parts)


# ---- layout -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name", ["tiny_ragged", "tiny_odd_heads", "c3_slice_l16"])
def test_row_width_is_the_one_row_cache_over_the_element_size(name, bf16):
    cfg = M2FConfig.from_model_config(synth.CASES[name][0])
    W = streaming.snapshot_row_elems(streaming.config_sites(cfg), bf16)
    assert W * (2 if bf16 else 4) == streaming.cache_bytes(cfg, 1, 1, bf16)
    assert W * (2 if bf16 else 4) % 16 == 0


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("ring", [None, 5])
def test_offsets_and_segment_starts_against_indexing(bf16, ring):
    S, C = 7, 5 if ring else 16
    lengths = [0, 1, 4, 5, 7, 13, 2]
    slots = [6, 0, 3, 1, 5, 2, 4]
    caches = _caches(SITES, S, C, bf16)
    rows = streaming.snapshot_rows(lengths, ring)
    assert rows == ([min(n, 5) for n in lengths] if ring else lengths)
    if ring is None:
        rows = [min(r, C) for r in rows]
    offsets = streaming.snapshot_row_offsets(rows)
    assert offsets == [sum(rows[:e]) for e in range(len(rows))]
    W = streaming.snapshot_row_elems(SITES, bf16)
    assert W == sum(2 * H * _pad(hd, bf16) for H, hd in SITES)
    want = _reference(caches, slots, rows)
    assert want.numel() == sum(rows) * W
    esize = 2 if bf16 else 4
    segs = streaming.snapshot_segments(SITES, bf16, rows)
    for e, (s, r) in enumerate(zip(slots, rows)):
        assert segs[e][0][0] == offsets[e] * W, "an entry starts at row_offsets[e] * W"
        i = 0
        for (H, hd), (k, v) in zip(SITES, caches):
            for t in (k, v):
                for h in range(H):
                    start, n = segs[e][i]
                    assert n == r * _pad(hd, bf16) and start * esize % 16 == 0
                    assert torch.equal(want[start: start + n], t[s, h, :r].reshape(-1)), (e, i)
                    i += 1
        assert i == len(segs[e]) and segs[e][-1][0] + segs[e][-1][1] == (offsets[e] + r) * W


# ---- signature --------------------------------------------------------------------------------------------------------------------
def test_signatures_compare_geometry_precision_window_and_ring_capacity():
    sig = streaming.make_signature(SITES, False, 3, 4)
    assert sig == streaming.make_signature([list(s) for s in SITES], 0, 3, 4)
    assert sig != streaming.make_signature(SITES[1:] + SITES[:1], False, 3, 4), "the order of the sites counts"
    assert sig != streaming.make_signature(SITES, True, 3, 4)
    assert sig != streaming.make_signature(SITES, False, 2, 4)
    assert sig != streaming.make_signature(SITES, False, 3, 6)
    assert sig != streaming.make_signature(SITES, False, None, 4)
    plain = streaming.make_signature(SITES, False, None, 64)
    assert plain == streaming.make_signature(SITES, False, None, 128), "a plain snapshot fits any capacity that holds it"
    assert plain[3] is None and sig[3] == 4


# ---- StreamSnapshot ---------------------------------------------------------------------------------------------------------------
def _snap(bf16=False, ring=None, lengths=(0, 1, 4, 5, 7, 13, 2)):
    S, C = len(lengths), ring or 16
    caches = _caches(SITES, S, C, bf16, seed=3)
    rows = streaming.snapshot_rows(lengths, ring)
    sig = streaming.make_signature(SITES, bf16, None if ring is None else ring - 1, C)
    return StreamSnapshot(_reference(caches, range(S), rows), lengths, streaming.snapshot_row_offsets(rows), sig), caches


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("ring", [None, 5])
def test_select_picks_entries_and_keeps_true_lengths(bf16, ring):
    snap, caches = _snap(bf16, ring)
    assert len(snap) == 7 and snap.nbytes == snap.data.numel() * (2 if bf16 else 4)
    assert snap.data.numel() == sum(snap.rows) * snap.row_elems
    pick = snap.select([5, 0, 2, 5])
    rows = [snap.rows[i] for i in (5, 0, 2, 5)]
    assert pick.lengths == [13, 0, 4, 13] and pick.rows == rows and pick.signature == snap.signature
    assert pick.row_offsets == [0, rows[0], rows[0], rows[0] + rows[2]]
    assert torch.equal(pick.data, _reference(caches, [5, 0, 2, 5], rows))
    assert len(snap.select([])) == 0 and snap.select([]).data.numel() == 0
    with pytest.raises(ValueError):
        snap.select([7])


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("ring", [None, 5])
def test_state_dict_round_trip_through_torch_save(bf16, ring):
    snap, _ = _snap(bf16, ring)
    d = snap.state_dict()

    def plain(x):
        return isinstance(x, (int, torch.Tensor)) and not isinstance(x, bool) or isinstance(x, list) and all(plain(y) for y in x)
    assert all(plain(v) for v in d.values()), "tensors, ints and lists only"
    buf = io.BytesIO()
    torch.save(d, buf)
    buf.seek(0)
    back = StreamSnapshot.from_state_dict(torch.load(buf, weights_only=True))
    assert back.signature == snap.signature and back.lengths == snap.lengths and back.row_offsets == snap.row_offsets
    assert back.data.dtype == snap.data.dtype and torch.equal(back.data, snap.data)
    moved = back.cpu().to("cpu")
    assert torch.equal(moved.data, snap.data) and moved.lengths == snap.lengths


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("ring", [None, 5])
def test_entry_views_are_the_cache_rows(bf16, ring):
    snap, caches = _snap(bf16, ring)
    for e, r in enumerate(snap.rows):
        views = snap.entry(e)
        assert len(views) == len(SITES)
        for (k, v), (ck, cv) in zip(views, caches):
            assert k.shape == (ck.shape[1], r, ck.shape[3]) and torch.equal(k, ck[e, :, :r]) and torch.equal(v, cv[e, :, :r])
            assert k.numel() == 0 or k.data_ptr() >= snap.data.data_ptr(), "views, not copies"
    with pytest.raises(ValueError):
        snap.entry(len(snap))


def test_a_snapshot_refuses_data_that_does_not_match_its_lists():
    snap, _ = _snap()
    with pytest.raises(ValueError):
        StreamSnapshot(snap.data[:-1], snap.lengths, snap.row_offsets, snap.signature)
    with pytest.raises(ValueError):
        StreamSnapshot(snap.data.to(torch.bfloat16), snap.lengths, snap.row_offsets, snap.signature)
    with pytest.raises(ValueError):
        StreamSnapshot(snap.data, snap.lengths, [o + 1 for o in snap.row_offsets], snap.signature)
    with pytest.raises(ValueError):
        StreamSnapshot(snap.data, [-1] + snap.lengths[1:], snap.row_offsets, snap.signature)
    d = snap.state_dict()
    d["ring"] = 4                                               # a ring capacity without a window
    with pytest.raises(ValueError):
        StreamSnapshot.from_state_dict(d)


# ---- validation that needs no device ----------------------------------------------------------------------------------------------
def test_restore_slots_must_be_distinct_in_range_and_one_per_entry():
    assert streaming.check_restore_slots([3, 0, 7], 3, 8) == [3, 0, 7]
    assert streaming.check_restore_slots(range(2), 2, 2) == [0, 1]
    for slots, entries in (([1, 1], 2), ([0, 8], 2), ([-1], 1), ([0, 1], 3), ([0, 1, 2], 2)):
        with pytest.raises(ValueError):
            streaming.check_restore_slots(slots, entries, 8)


def test_a_plain_cache_refuses_an_entry_longer_than_its_capacity():
    streaming.check_restore_fits([64, 0, 12], [0, 1, 2], 64, None)
    with pytest.raises(RuntimeError, match=r"\[5\]"):
        streaming.check_restore_fits([64, 65], [2, 5], 64, None)
    streaming.check_restore_fits([64, 6500], [2, 5], 4, 3)      # a ring has no length limit


# ---- all-or-nothing page arithmetic -------------------------------------------------------------------------------------------------
def _state(al):
    return [list(p) for p in al.slot_pages], sorted(al._free), al.table.clone(), al.dirty


def test_replace_counts_the_targets_own_pages_and_takes_the_lowest_ids():
    al = PageAllocator(6, 4, 64, 16)
    al.take([2, 1, 0, 3])                                       # slots 0: [0, 1], 1: [2], 3: [3, 4, 5]; nothing free
    assert al.pages_free == 0
    al.dirty = False
    assert al.replace_shortfall([3, 2], [1, 2]) == []           # slot 3's three pages cover both
    al.replace([3, 2], [1, 2], "restore")
    assert al.slot_pages == [[0, 1], [2], [3, 4], [5]] and al.pages_free == 0 and al.dirty      # (handed out in slot order)
    assert al.table[3, 0] == 5 and al.table[2, :2].tolist() == [3, 4]
    al.replace([0], [0], "restore")                             # an empty entry: the slot's pages return
    assert al.slot_pages[0] == [] and al.pages_free == 2
    al.replace([1, 0], [2, 1], "restore")
    assert al.slot_pages[0] == [0] and al.slot_pages[1] == [1, 2] and al.pages_free == 0


def test_a_replace_that_does_not_fit_names_the_slots_and_changes_nothing():
    al = PageAllocator(6, 4, 64, 16)
    al.take([2, 1, 0, 2])                                       # one page free
    before = _state(al)
    assert al.replace_shortfall([2, 1], [1, 2]) == [1]          # 1 free + 1 held by slot 1 = 2 < 3
    with pytest.raises(RuntimeError, match=r"slot\(s\) \[1\]"):
        al.replace([2, 1], [1, 2], "DialogueStream.restore")
    after = _state(al)
    assert after[:2] == before[:2] and torch.equal(after[2], before[2]) and after[3] == before[3]
    assert al.replace_shortfall([2, 1], [3, 3]) == [2, 1]
    for slots, need in (([1, 1], [1, 1]), ([4], [1]), ([0], [5]), ([0, 1], [1])):      # duplicates, range, past the slot's width
        with pytest.raises(ValueError):
            al.replace(slots, need)
    assert _state(al)[:2] == before[:2]
    al.replace([0, 1, 3], [1, 1, 4], "restore")                 # exactly what they hold plus the free page
    assert al.pages_free == 0 and [len(p) for p in al.slot_pages] == [1, 1, 0, 4]


def test_allocator_state_round_trip():
    al = PageAllocator(6, 4, 64, 16)
    al.take([2, 1, 0, 2])
    saved, before = al.state(), _state(al)
    al.dirty = False
    al.replace([0, 3], [1, 3], "restore")
    assert _state(al)[:2] != before[:2]
    al.set_state(saved)
    after = _state(al)
    assert after[:2] == before[:2] and torch.equal(after[2], before[2]) and al.dirty, "the old table must travel again"
    al.take([0, 0, 1, 0])
    assert al.slot_pages[2] == [5] and torch.equal(saved[2], before[2]), "a saved state is a copy"
