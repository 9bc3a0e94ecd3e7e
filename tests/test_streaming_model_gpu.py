"""M2FNet.stream / streaming.DialogueStream against the oracle with tests/golden/band_ref.py swapped in, at valid slots: every model
shape of the fixtures under causal and windowed bands (rings that wrap), long dialogues up to the capacity, graph replay against eager
launches, reset and reuse of slots, ragged driving with active masks, new weights (the shadow freshness rule in bf16 mode), and the
models that never stream left bit for bit as they were."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import band_ref as R  # noqa: E402
import long_cases  # noqa: E402
import synth  # noqa: E402
from oracle import m2fnet_oracle as O  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import streaming  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402

TOL_LOGITS = 1e-4               # the eval-logits bound of tests/test_context_window_model_gpu.py
TOL_LOGITS_BF16 = 3e-2          # tests/test_model_gpu.py


def _case(name):
    if name in long_cases.CASES:
        return long_cases.inputs(name)
    cfg, B, L, lengths, kind = synth.CASES[name]
    return (cfg,) + synth.make_inputs(cfg, B, L, lengths, kind)


@functools.lru_cache(maxsize=None)
def _oracle(name, past, seed=7):
    """logits of the oracle under (past, 0); computed once per (case, band, weights) and never written to"""
    cfg, text, audio, key_pad, _ = _case(name)
    with R.swapped_in((past, 0)):
        logits = O.forward(synth.make_state_dict(cfg, seed=seed), cfg, text, audio, key_pad)
    assert torch.isfinite(logits).all()
    return logits


def _model(cfg, past, precision="fp32", seed=7):
    m = M2FNet(cfg, precision=precision, context=(past, 0))
    m.load_state_dict(synth.make_state_dict(cfg, seed=seed))
    return m.to("cuda").eval()


def _cuda(*ts):
    return [t.cuda() for t in ts]


def _err(logits, ref, key_pad):
    assert torch.isfinite(logits).all()
    assert torch.all(logits[key_pad] == 0), "pad slots must hold zeros"
    return (logits.cpu() - ref).abs()[~key_pad].max().item()


def _check(name, past, precision="fp32", extra_slots=1, **kw):
    cfg, text, audio, key_pad, _ = _case(name)
    ref = _oracle(name, past)
    m = _model(cfg, past, precision)
    st = m.stream(key_pad.shape[0] + extra_slots, **kw)
    with torch.inference_mode():
        logits = st.run(*_cuda(text, audio, key_pad)).cpu()
    err = _err(logits, ref, key_pad)
    tol = TOL_LOGITS if precision == "fp32" else TOL_LOGITS_BF16
    print(f"{name} past={past} {precision} capacity={st.capacity}: logits err {err:.3e} (bound {tol:.0e})")
    assert err < tol, err
    lengths = (~key_pad).sum(1).tolist()
    assert st.lengths == lengths + [0] * extra_slots
    assert st.plan.len.cpu().tolist() == st.lengths                      # the device's counts are the host mirror's
    return m, st, logits


# ---- against the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,past", [("tiny_ragged", None), ("tiny_ragged", 2), ("tiny_ragged", 0), ("tiny_shared_norm", 1),
                                       ("tiny_odd_heads", 5), ("tiny_no_fam", None), ("tiny_audio_only", None),
                                       ("tiny_text_only", None), ("c2_slice", 3), ("long_tiny", None), ("long_tiny", 8)])
def test_stream_matches_the_banded_oracle(name, past):
    _, st, _ = _check(name, past)
    assert st.capacity == (512 if past is None else past + 1)
    if (name, past) == ("tiny_ragged", 2):
        assert max(st.lengths) == 9 and st.capacity == 3                 # the ring wraps three times
    if (name, past) == ("long_tiny", 8):
        assert max(st.lengths) == 110 and st.capacity == 9


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_c3_width_causal(precision):
    """head dims 128 (text) and 96 (audio, fusion)"""
    _, st, _ = _check("c3_slice_l16", None, precision, capacity=16)
    assert st.plan.cache_bytes() == streaming.cache_bytes(st.plan.cfg, st.max_streams, 16, bf16=precision == "bf16")


def test_capacity_boundary_of_a_stream_without_a_window():
    """long_512: 512 utterances fill the caches to the last row; the 513th step of that slot raises before anything is launched"""
    m, st, _ = _check("long_512", None, extra_slots=0)
    cfg, text, audio, _, _ = _case("long_512")
    assert st.lengths == [512, 300] and st.capacity == 512
    t, a = _cuda(text[:, 0].contiguous(), audio[:, 0].contiguous())
    with torch.inference_mode():
        with pytest.raises(RuntimeError, match="capacity"):
            st.step(t, a)
        assert st.lengths == [512, 300] and st.plan.len.cpu().tolist() == [512, 300]
        out = st.step(t, a, active=[False, True])                         # the other slot goes on
    assert st.lengths == [512, 301] and torch.all(out[0] == 0) and torch.isfinite(out).all()


# ---- graph replay, reset -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("past", [None, 2])
def test_graph_replay_equals_eager_launches_and_a_second_pass_equals_the_first(past):
    cfg, text, audio, key_pad, _ = _case("tiny_ragged")
    batch = _cuda(text, audio, key_pad)
    m = _model(cfg, past)
    with torch.inference_mode():
        graph, eager = m.stream(6, use_graph=True), m.stream(6, use_graph=False)
        first = graph.run(*batch)
        assert torch.equal(first, eager.run(*batch))
        graph.reset()
        assert graph.lengths == [0] * 6 and graph.plan.len.cpu().tolist() == [0] * 6
        assert torch.equal(graph.run(*batch), first)
    assert _err(first.cpu(), _oracle("tiny_ragged", past), key_pad) < TOL_LOGITS


def test_ragged_driving_with_active_masks_and_reused_slots():
    """Five dialogues of 9 / 1 / 4 / 7 / 2 utterances through TWO slots: a slot that finishes is reset and takes the next dialogue,
    the slots advance independently, and every dialogue matches its oracle rows."""
    past = 2
    cfg, text, audio, key_pad, _ = _case("tiny_ragged")
    ref = _oracle("tiny_ragged", past)
    lengths = (~key_pad).sum(1).tolist()
    m = _model(cfg, past)
    st = m.stream(2)
    t, a = _cuda(text, audio)
    queue = [0, 2, 1, 3, 4]                   # slot 0 takes the long dialogue first; a shorter one follows it in the same slot
    cur, pos = [None, None], [0, 0]
    got = torch.zeros_like(ref)
    steps = 0
    with torch.inference_mode():
        while queue or any(c is not None for c in cur):
            for s in range(2):
                if cur[s] is None and queue:
                    cur[s], pos[s] = queue.pop(0), 0
                    st.reset([s])
                    assert st.lengths[s] == 0
            act = [c is not None for c in cur]
            rows_t = torch.stack([t[cur[s], pos[s]] if act[s] else torch.zeros_like(t[0, 0]) for s in range(2)])
            rows_a = torch.stack([a[cur[s], pos[s]] if act[s] else torch.zeros_like(a[0, 0]) for s in range(2)])
            out = st.step(rows_t, rows_a, active=act)
            steps += 1
            for s in range(2):
                if not act[s]:
                    assert torch.all(out[s] == 0)
                    continue
                got[cur[s], pos[s]] = out[s].cpu()
                pos[s] += 1
                assert st.lengths[s] == pos[s]
                if pos[s] == lengths[cur[s]]:
                    cur[s] = None
    assert steps < sum(lengths)               # (the slots really ran side by side)
    err = (got - ref).abs()[~key_pad].max().item()
    print(f"ragged driving: {err:.3e}")
    assert err < TOL_LOGITS, err


def test_stale_rows_behind_a_reset_are_never_read():
    """a slot reset after a longer dialogue still holds that dialogue's rows: the next dialogue is bit for bit what a fresh stream gives"""
    cfg, text, audio, key_pad, _ = _case("tiny_ragged")
    m = _model(cfg, None)
    t, a = _cuda(text, audio)
    with torch.inference_mode():
        st = m.stream(1, capacity=16)
        for i in range(9):
            st.step(t[0:1, i], a[0:1, i])
        st.reset()
        fresh = m.stream(1, capacity=16)
        for i in range(4):
            assert torch.equal(st.step(t[2:3, i], a[2:3, i]), fresh.step(t[2:3, i], a[2:3, i]))


# ---- weights -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_new_weights_and_a_reset_follow_the_oracle_of_the_new_weights(precision):
    name, past = "tiny_ragged", None
    cfg, text, audio, key_pad, _ = _case(name)
    batch = _cuda(text, audio, key_pad)
    tol = TOL_LOGITS if precision == "fp32" else TOL_LOGITS_BF16
    m = _model(cfg, past, precision)
    st = m.stream(5)
    with torch.inference_mode():
        assert _err(st.run(*batch).cpu(), _oracle(name, past), key_pad) < tol
    m.load_state_dict(synth.make_state_dict(cfg, seed=8))
    st.reset()
    with torch.inference_mode():
        second = st.run(*batch).cpu()
    new = _oracle(name, past, 8)
    assert (new - _oracle(name, past)).abs()[~key_pad].max().item() > 10 * tol          # (the weights change the numbers: the test can fail)
    err = _err(second, new, key_pad)
    print(f"{precision}: after load_state_dict + reset {err:.3e}")
    assert err < tol, err
    if precision == "bf16":
        assert m.engine().shadows_fresh()                  # the step that re-cast the shared shadows declared them current ...
        with torch.inference_mode():
            st.reset()
            assert torch.equal(st.run(*batch).cpu(), second)          # ... and the steps that skip the casts compute the same bits


# ---- the default path ------------------------------------------------------------------------------------------------------------------
def test_models_that_never_stream_compute_the_bits_they_computed_before():
    cfg, text, audio, key_pad, _ = _case("tiny_ragged")
    batch = _cuda(text, audio, key_pad)

    def default_model():
        m = M2FNet(cfg)
        m.load_state_dict(synth.make_state_dict(cfg))
        return m.to("cuda").eval()

    plain, causal = default_model(), _model(cfg, None)
    with torch.inference_mode():
        before, before_causal = plain(*batch).clone(), causal(*batch).clone()
        st = causal.stream(5)
        streamed = st.run(*batch)
        assert torch.equal(plain(*batch), before)                      # a model with the default context, beside a live stream
        assert torch.equal(causal(*batch), before_causal)              # the streaming model's own forward
        assert torch.equal(default_model()(*batch), before)            # a model built afterwards
        assert (streamed - before_causal).abs()[~key_pad.cuda()].max().item() < 2 * TOL_LOGITS
    assert all(not isinstance(pl, mer_amd.runtime.StreamPlan) for pl in causal.engine().plans.values())
