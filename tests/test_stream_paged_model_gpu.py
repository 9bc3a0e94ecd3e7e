"""M2FNet.stream(pages=..., page_rows=16) against the dense stream of the same model, bit for bit: one script of ragged steps with a
changing mask, a chunked prefill, a reset in mid-run whose pages go to other slots, further steps and a `run`, on a pool smaller than
the dense caches; a pool that runs out (RuntimeError naming the slot, nothing changed, the same step after a reset); and 256 slots on
320 pages, more than a dense cache of that capacity would be asked to hold, sampled against a dense stream of 8."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import streaming  # noqa: E402
from test_streaming_model_gpu import _model  # noqa: E402

CFG = synth.CASES["tiny_ragged"][0]             # both modalities and a fusion stack
S = 8


def _inputs(B, L, seed=11):
    text, audio, _, _ = synth.make_inputs(CFG, B, L, None, "randn", seed=seed)
    return text.cuda(), audio.cuda()


def _held(st):
    """pages each slot must hold for its length"""
    return [-(-min(n, st.capacity) // st.page_rows) for n in st.lengths]


def _same_state(paged, dense):
    assert paged.lengths == dense.lengths
    assert paged.plan.len.cpu().tolist() == paged.lengths == dense.plan.len.cpu().tolist()
    al = paged.allocator
    assert [len(p) for p in al.slot_pages] == _held(paged)
    assert al.pages_free == paged.pages - sum(_held(paged)) == paged.pages_free
    held = [p for ps in al.slot_pages for p in ps]
    assert len(set(held)) == len(held)
    for s, ps in enumerate(al.slot_pages):
        assert paged.plan.table[s, :len(ps)].cpu().tolist() == ps, "the device's table differs from the allocator's"


def _steps(paged, dense, text, audio, first, counts):
    """counts[s] steps per slot from row first[s] of its dialogue, a changing mask; every step's logits must be equal"""
    for i in range(max(counts)):
        act = [i < c for c in counts]
        rows = torch.tensor([min(f + i, text.shape[1] - 1) for f in first], device="cuda")
        t, a = text[torch.arange(S), rows], audio[torch.arange(S), rows]
        got, want = paged.step(t, a, act), dense.step(t, a, act)
        assert torch.isfinite(got).all() and torch.equal(got, want), f"step {i}, active {act}"
    return [f + c for f, c in zip(first, counts)]


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("past", [None, 3])
def test_one_script_through_a_paged_and_a_dense_stream_gives_the_same_bits(past, precision, use_graph):
    m = _model(CFG, past, precision)
    capacity, pages = (64, 12) if past is None else (4, 6)
    assert pages < S * -(-capacity // 16)                       # fewer pages than the dense caches have rows for
    text, audio = _inputs(S, 64)
    with torch.inference_mode():
        paged = m.stream(S, capacity=capacity, use_graph=use_graph, max_chunk=16, pages=pages, page_rows=16)
        dense = m.stream(S, capacity=capacity, use_graph=use_graph, max_chunk=16)
        assert paged.pages == pages and paged.page_rows == 16 and dense.pages is None and dense.allocator is None
        assert paged.capacity == dense.capacity == capacity
        assert paged.plan.cache_bytes() == streaming.cache_bytes_paged(paged.plan.cfg, pages, 16, bf16=precision == "bf16")
        if past is None:                                        # (a ring of 4 rows still takes whole pages of 16)
            assert paged.plan.cache_bytes() < dense.plan.cache_bytes()
        # ragged dialogues fed by step, slots 6 and 7 idle
        at = _steps(paged, dense, text, audio, [0] * S, [20, 3, 17, 9, 1, 12, 0, 0])
        _same_state(paged, dense)
        # a prefill, 16 rows per slot and call, some slots taking nothing
        counts = [18, 0, 5, 20, 0, 7, 0, 0]
        n = max(counts)
        t, a = (torch.stack([x[s, at[s]: at[s] + n] for s in range(S)]) for x in (text, audio))
        got, want = paged.prefill(t, a, counts), dense.prefill(t, a, counts)
        assert torch.isfinite(got).all() and torch.equal(got, want), "prefill"
        at = [p + c for p, c in zip(at, counts)]
        _same_state(paged, dense)
        assert paged.lengths == [38, 3, 22, 29, 1, 19, 0, 0]
        # two slots start over in mid-run; their pages go to other slots
        freed = set(paged.allocator.slot_pages[0]) | set(paged.allocator.slot_pages[3])
        assert len(freed) == (5 if past is None else 2)
        paged.reset([0, 3])
        dense.reset([0, 3])
        at[0] = at[3] = 0
        _same_state(paged, dense)
        at = _steps(paged, dense, text, audio, at, [0, 14, 11, 0, 0, 0, 18, 5])
        _same_state(paged, dense)
        assert freed & (set(paged.allocator.slot_pages[6]) | set(paged.allocator.slot_pages[7])), "the freed pages were not handed out again"
        # run on a padded batch (it resets the slots it uses; the two behind them make room first)
        paged.reset([6, 7])
        dense.reset([6, 7])
        lengths = [12, 1, 7, 9, 3, 12]
        bt, ba = _inputs(6, 12, seed=5)
        mask = (torch.arange(12)[None, :] >= torch.tensor(lengths)[:, None]).cuda()
        got, want = paged.run(bt, ba, mask), dense.run(bt, ba, mask)
        assert torch.isfinite(got).all() and torch.equal(got, want), "run"
        assert torch.all(got[mask] == 0)
        _same_state(paged, dense)
        assert paged.lengths == lengths + [0, 0]
    paged.close()
    dense.close()


@pytest.mark.parametrize("use_graph", [True, False])
def test_a_pool_that_runs_out_raises_naming_the_slot_and_changes_nothing(use_graph):
    m = _model(CFG, None)
    text, audio = _inputs(4, 4)
    with torch.inference_mode():
        paged = m.stream(4, capacity=64, use_graph=use_graph, pages=3)
        dense = m.stream(4, capacity=64, use_graph=use_graph)
        first, second = [True, True, True, False], [False, True, True, True]
        assert torch.equal(paged.step(text[:, 0], audio[:, 0], first), dense.step(text[:, 0], audio[:, 0], first))
        assert paged.pages_free == 0
        torch.cuda.synchronize()
        before = (list(paged.lengths), [list(p) for p in paged.allocator.slot_pages], paged.allocator.table.clone(), paged.plan.workspace.clone())
        with pytest.raises(RuntimeError, match=r"slot\(s\) \[3\]"):
            paged.step(text[:, 1], audio[:, 1], second)             # slot 3 needs its first page and none is free
        with pytest.raises(RuntimeError, match=r"slot\(s\) \[3\]"):
            paged.prefill(text[:, 1:3], audio[:, 1:3], [0, 2, 0, 1])
        torch.cuda.synchronize()
        assert paged.lengths == before[0] == [1, 1, 1, 0] and [list(p) for p in paged.allocator.slot_pages] == before[1]
        assert torch.equal(paged.allocator.table, before[2]) and paged.pages_free == 0
        assert torch.equal(paged.plan.workspace, before[3]), "a refused step changed the device's state"
        assert paged.plan.len.cpu().tolist() == [1, 1, 1, 0]
        paged.reset([0])
        dense.reset([0])
        assert paged.pages_free == 1
        got = paged.step(text[:, 1], audio[:, 1], second)           # the same step, now that a page is free
        assert torch.equal(got, dense.step(text[:, 1], audio[:, 1], second)) and torch.isfinite(got).all()
        assert paged.lengths == dense.lengths == [0, 2, 2, 1] and paged.allocator.slot_pages[3] == [0]
    paged.close()
    dense.close()


def test_256_slots_on_320_pages_match_a_dense_stream_of_the_sampled_dialogues():
    """capacity 512 without a window: dense caches would reserve 256 * 512 rows per site, the pool holds 320 * 16"""
    big, L = 256, 20
    m = _model(CFG, None)
    lengths = [1 + (7 * s) % 20 for s in range(big)]
    assert set(lengths) == set(range(1, 21)) and sum(-(-n // 16) for n in lengths) <= 320
    text, audio = _inputs(big, L, seed=3)
    mask = (torch.arange(L)[None, :] >= torch.tensor(lengths)[:, None]).cuda()
    sample = [0, 5, 37, 99, 128, 200, 251, 255]
    assert max(lengths[s] for s in sample) > 16 > min(lengths[s] for s in sample)
    with torch.inference_mode():
        paged = m.stream(big, pages=320, page_rows=16)
        assert paged.capacity == 512 and paged.plan.cache_bytes() == streaming.cache_bytes_paged(paged.plan.cfg, 320, 16)
        assert paged.plan.cache_bytes() * 25 < streaming.cache_bytes(paged.plan.cfg, big, 512)
        got = paged.run(text, audio, mask)
        assert paged.lengths == lengths and paged.plan.len.cpu().tolist() == lengths
        assert paged.pages_free == 320 - sum(-(-n // 16) for n in lengths)
        dense = m.stream(8)
        want = dense.run(text[sample], audio[sample], mask[sample])
    assert torch.isfinite(got).all() and torch.all(got[mask] == 0)
    assert torch.equal(got[sample], want)
    paged.close()
    dense.close()
