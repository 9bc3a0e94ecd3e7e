"""DialogueStream.prefill / M2FNet.stream(max_chunk=T) against the oracle with tests/golden/band_ref.py swapped in, at valid slots:
every model shape and band of tests/test_streaming_model_gpu.py plus the C3-width slice in both precisions, chunk lengths 4 / 16 / 64
(below, around and above the rings' capacities), `run` through chunks, a history prefilled and then continued by steps, steps
continued by a prefill, ragged counts with zeros, the capacity boundary, graph replay against eager launches, reset, new weights, and
the default max_chunk = 1 left bit for bit as it was."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from test_streaming_model_gpu import TOL_LOGITS, TOL_LOGITS_BF16, _case, _cuda, _err, _model, _oracle  # noqa: E402  (one oracle per case and band)

CASES = [("tiny_ragged", None), ("tiny_ragged", 2), ("tiny_ragged", 0), ("tiny_shared_norm", 1), ("tiny_odd_heads", 5),
         ("tiny_no_fam", None), ("tiny_audio_only", None), ("tiny_text_only", None), ("c2_slice", 3), ("long_tiny", None), ("long_tiny", 8)]
CHUNKS = [4, 16, 64]


def _tol(precision):
    return TOL_LOGITS if precision == "fp32" else TOL_LOGITS_BF16


def _prefill(st, t, a, start, stop, got):
    """slot s takes rows start[s] .. stop[s] - 1 of its dialogue in one prefill call; the rows behind a slot's count hold NaN"""
    S = st.max_streams
    counts = [max(e - b, 0) for b, e in zip(start, stop)] + [0] * (S - len(start))
    n = max(counts)
    xs = []
    for x in (t, a):
        buf = torch.full((S, n, x.shape[2]), float("nan"), device=x.device)
        for s, (b, c) in enumerate(zip(start, counts)):
            buf[s, :c] = x[s, b: b + c]
        xs.append(buf)
    before = list(st.lengths)
    logits = st.prefill(xs[0], xs[1], counts)
    assert logits.shape == (S, n, got.shape[2]) and torch.isfinite(logits).all()
    assert st.lengths == [l + c for l, c in zip(before, counts)]
    for s, c in enumerate(counts):
        assert torch.all(logits[s, c:] == 0), "logits past the count must be zero"
        if s < len(start):
            got[s, start[s]: start[s] + c] = logits[s, :c]


def _steps(st, t, a, start, stop, got):
    """... one step per row"""
    S, B = st.max_streams, len(start)
    for i in range(max(max(e - b, 0) for b, e in zip(start, stop))):
        act = [b + i < e for b, e in zip(start, stop)] + [False] * (S - B)
        rows = torch.tensor([min(b + i, t.shape[1] - 1) for b in start], device=t.device)
        pad = lambda x: torch.cat([x[torch.arange(B), rows], torch.zeros(S - B, x.shape[2], device=x.device)])          # noqa: E731
        out = st.step(pad(t), pad(a), act)
        for s in range(B):
            if act[s]:
                got[s, start[s] + i] = out[s]


def _check_against(got, ref, key_pad, tol, what):
    err = _err(got.cpu(), ref, key_pad)
    print(f"{what}: logits err {err:.3e} (bound {tol:.0e})")
    assert err < tol, (what, err)


def _all_ways(name, past, T, precision="fp32", **kw):
    cfg, text, audio, key_pad, _ = _case(name)
    ref, tol = _oracle(name, past), _tol(precision)
    B, L = key_pad.shape
    lengths = (~key_pad).sum(1).tolist()
    m = _model(cfg, past, precision)
    st = m.stream(B + 1, max_chunk=T, **kw)
    assert st.max_chunk == T and st.chunk_plan is not None
    t, a, kp = _cuda(text, audio, key_pad)
    what = f"{name} past={past} T={T} {precision} capacity={st.capacity}"
    with torch.inference_mode():
        # run, T columns per call
        _check_against(st.run(t, a, kp), ref, key_pad, tol, what + " run")
        assert st.lengths == lengths + [0] and st.plan.len.cpu().tolist() == st.lengths
        # each dialogue's first half in one prefill, the rest by steps
        st.reset()
        got = torch.zeros(B, L, ref.shape[2], device="cuda")
        half = [n // 2 for n in lengths]
        _prefill(st, t, a, [0] * B, half, got)
        assert st.plan.len.cpu().tolist() == half + [0]
        _steps(st, t, a, half, lengths, got)
        _check_against(got, ref, key_pad, tol, what + " prefill, then steps")
        assert st.lengths == lengths + [0] and st.plan.len.cpu().tolist() == st.lengths
        # steps first, then the rest in one prefill (dialogues the steps have finished take nothing: counts of zero beside live state)
        st.reset()
        got = torch.zeros(B, L, ref.shape[2], device="cuda")
        head = [min(2, n) for n in lengths]
        _steps(st, t, a, [0] * B, head, got)
        _prefill(st, t, a, head, lengths, got)
        _check_against(got, ref, key_pad, tol, what + " steps, then prefill")
        assert st.lengths == lengths + [0] and st.plan.len.cpu().tolist() == st.lengths
    st.close()
    return st


@pytest.mark.parametrize("T", CHUNKS)
@pytest.mark.parametrize("name,past", CASES)
def test_prefill_matches_the_banded_oracle(name, past, T):
    st = _all_ways(name, past, T)
    assert st.capacity == (512 if past is None else past + 1)


@pytest.mark.parametrize("T", CHUNKS)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_c3_width_causal(precision, T):
    """head dims 128 (text) and 96 (audio, fusion)"""
    _all_ways("c3_slice_l16", None, T, precision, capacity=16)


@pytest.mark.parametrize("past", [None, 2])
def test_ragged_counts_with_zeros_while_other_slots_hold_state(past):
    cfg, text, audio, key_pad, _ = _case("tiny_ragged")
    ref = _oracle("tiny_ragged", past)
    B, L = key_pad.shape
    lengths = (~key_pad).sum(1).tolist()                       # 9 / 1 / 4 / 7 / 2
    m = _model(cfg, past)
    st = m.stream(B, max_chunk=4)
    t, a = _cuda(text, audio)
    got = torch.zeros(B, L, ref.shape[2], device="cuda")
    with torch.inference_mode():
        first = [5, 0, 4, 1, 0]                                # two calls; slots 1 and 4 take nothing
        _prefill(st, t, a, [0] * B, first, got)
        assert st.plan.len.cpu().tolist() == first
        second = [5, 1, 4, 7, 0]                               # slots 0 and 2 hold state and take nothing; slot 3 goes on over two calls
        _prefill(st, t, a, first, second, got)
        assert st.plan.len.cpu().tolist() == second
        _prefill(st, t, a, second, lengths, got)
    _check_against(got, ref, key_pad, TOL_LOGITS, f"ragged counts past={past}")
    assert st.lengths == lengths and st.plan.len.cpu().tolist() == lengths


def test_capacity_boundary_of_a_stream_without_a_window():
    """long_512: the chunks fill the caches to the last row; a prefill that would pass it raises before anything is launched"""
    cfg, text, audio, key_pad, _ = _case("long_512")
    m = _model(cfg, None)
    st = m.stream(2, max_chunk=64)
    t, a, kp = _cuda(text, audio, key_pad)
    with torch.inference_mode():
        _check_against(st.run(t, a, kp), _oracle("long_512", None), key_pad, TOL_LOGITS, "long_512 T=64")
        assert st.lengths == [512, 300] and st.capacity == 512 and st.plan.len.cpu().tolist() == [512, 300]
        with pytest.raises(RuntimeError, match="capacity"):
            st.prefill(t[:, :3], a[:, :3], [1, 3])
        with pytest.raises(RuntimeError, match="capacity"):
            st.prefill(t[:, :213], a[:, :213], [0, 213])
        assert st.lengths == [512, 300] and st.plan.len.cpu().tolist() == [512, 300]
        out = st.prefill(t[:, :212], a[:, :212], [0, 212])                 # the other slot goes on, to its own last row
    assert st.lengths == [512, 512] and st.plan.len.cpu().tolist() == [512, 512]
    assert torch.all(out[0] == 0) and torch.isfinite(out).all()


@pytest.mark.parametrize("past", [None, 2])
def test_graph_replay_equals_eager_launches_and_a_second_pass_equals_the_first(past):
    cfg, text, audio, key_pad, _ = _case("tiny_ragged")
    batch = _cuda(text, audio, key_pad)
    m = _model(cfg, past)
    with torch.inference_mode():
        graph, eager = m.stream(6, use_graph=True, max_chunk=4), m.stream(6, use_graph=False, max_chunk=4)
        first = graph.run(*batch)
        assert torch.equal(first, eager.run(*batch))
        graph.reset()
        assert graph.lengths == [0] * 6 and graph.plan.len.cpu().tolist() == [0] * 6
        assert torch.equal(graph.run(*batch), first)
    assert _err(first.cpu(), _oracle("tiny_ragged", past), key_pad) < TOL_LOGITS


@pytest.mark.parametrize("past", [None, 2])
def test_max_chunk_1_is_the_stream_it_was(past):
    cfg, text, audio, key_pad, _ = _case("tiny_ragged")
    batch = _cuda(text, audio, key_pad)
    B = key_pad.shape[0]
    lengths = (~key_pad).sum(1).tolist()
    m = _model(cfg, past)
    with torch.inference_mode():
        plain, one = m.stream(B), m.stream(B, max_chunk=1)
        assert one.chunk_plan is None and one.max_chunk == 1
        want = plain.run(*batch)
        assert torch.equal(one.run(*batch), want)
        one.reset()
        got = one.prefill(batch[0], batch[1], lengths)         # through `step`: the same bits at the valid slots, zeros behind the counts
        assert torch.equal(got, want) and one.lengths == lengths


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_new_weights_and_a_reset_follow_the_oracle_of_the_new_weights(precision):
    name, past = "tiny_ragged", None
    cfg, text, audio, key_pad, _ = _case(name)
    batch = _cuda(text, audio, key_pad)
    tol = _tol(precision)
    m = _model(cfg, past, precision)
    st = m.stream(5, max_chunk=4)
    with torch.inference_mode():
        assert _err(st.run(*batch).cpu(), _oracle(name, past), key_pad) < tol
    m.load_state_dict(synth.make_state_dict(cfg, seed=8))
    st.reset()
    with torch.inference_mode():
        second = st.run(*batch).cpu()
    err = _err(second, _oracle(name, past, 8), key_pad)
    print(f"{precision}: after load_state_dict + reset {err:.3e}")
    assert err < tol, err
    if precision == "bf16":
        assert m.engine().shadows_fresh()                  # the chunk call that re-cast the shared shadows declared them current ...
        with torch.inference_mode():
            st.reset()
            assert torch.equal(st.run(*batch).cpu(), second)          # ... and the calls that skip the casts compute the same bits


def test_refusals_leave_every_length_as_it_was():
    cfg, text, audio, key_pad, _ = _case("tiny_ragged")
    t, a = _cuda(text, audio)
    B = key_pad.shape[0]
    m = _model(cfg, None)
    st = m.stream(B, capacity=8, max_chunk=4)
    with torch.inference_mode():
        st.prefill(t[:, :3], a[:, :3], [3, 0, 1, 2, 0])
        before = list(st.lengths)
        with pytest.raises(ValueError):
            st.prefill(t[:2, :3], a[:2, :3])                               # not one row block per slot
        with pytest.raises(ValueError):
            st.prefill(t[:, :3], a[:, :2])
        with pytest.raises(ValueError):
            st.prefill(t[:, :3], a[:, :3], [4, 0, 0, 0, 0])                # a count past the rows given
        with pytest.raises(ValueError):
            st.prefill(t[:, :3], a[:, :3], [1, 1])
        with pytest.raises(RuntimeError, match="capacity"):
            st.prefill(t[:, :6], a[:, :6], [6, 1, 1, 1, 1])                # 3 + 6 > 8, checked for the whole call
        assert st.lengths == before and st.plan.len.cpu().tolist() == before
    with pytest.raises(ValueError, match="max_chunk"):
        m.stream(B, max_chunk=65)


@pytest.mark.parametrize("past", [None, 2])
def test_run_with_a_hole_in_a_mask_row_feeds_column_by_column(past):
    """a batch that is not in the collate layout goes through `step` on a stream with a chunk plan too: the bits of a max_chunk = 1
    stream, before and after chunk calls on the same stream"""
    cfg, text, audio, key_pad, _ = _case("tiny_ragged")
    t, a, kp = _cuda(text, audio, key_pad)
    holed = key_pad.clone()
    holed[0, 3] = True                                         # dialogue 0: utterances 0 - 2 and 4 - 8
    assert mer_amd.streaming.prefix_counts(~holed) is None and mer_amd.streaming.prefix_counts(~key_pad) is not None
    B = key_pad.shape[0]
    m = _model(cfg, past)
    with torch.inference_mode():
        one, chunked = m.stream(B), m.stream(B, max_chunk=4)
        want = one.run(t, a, holed.cuda())
        assert torch.equal(chunked.run(t, a, holed.cuda()), want)
        assert chunked.lengths == one.lengths == (~holed).sum(1).tolist() and chunked.plan.len.cpu().tolist() == chunked.lengths
        through_chunks = chunked.run(t, a, kp)                 # the chunk plan, then the fallback again on the same stream
        assert _err(through_chunks.cpu(), _oracle("tiny_ragged", past), key_pad) < TOL_LOGITS
        assert torch.equal(chunked.run(t, a, holed.cuda()), want)
        assert torch.equal(chunked.run(t, a, kp), through_chunks)
