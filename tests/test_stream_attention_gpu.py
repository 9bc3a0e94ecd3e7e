"""Attention rows of a stream: the weights-emitting form of the step kernel (csrc/attention_stream.hip; functional.attention_stream(...,
weights=)) against the float64 causal / windowed softmax, dense and paged, fp32 and bf16 caches, plain caches and rings - and
model.stream(..., attention=True) / DialogueStream.attention against the offline maps of M2FNet.attention_maps at every site.

Bounds: 2e-5 (fp32 caches) and 3e-2 (bf16 caches) at kernel level, the bounds of tests/test_streaming_kernels_gpu.py; at model level
2 x the eval-logits bound 1e-4, the margin tests/test_streaming_model_gpu.py gives a stream against the forward (both sides are within
1e-4 of the oracle).  Probabilities are O(1): the bounds are absolute."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_maps_ref as A  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402
from mer_amd import streaming  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402

DEV = "cuda"
TOL_LOGITS = 1e-4


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


# ---- kernel level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ring", [False, True], ids=["plain", "ring"])
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("hd", [20, 128])
def test_rows_of_a_dialogue_grown_row_by_row(hd, C, ring, bf16):
    """Slots 0 and 2 grow one dialogue each, slot 1 never takes an utterance.  A ring of C rows is driven past two wraps (C = 8) or one
    (C = 64); a plain cache to its last row."""
    S, H, R = 3, 2, 16
    E = H * hd
    n = (2 * C + 3 if C == 8 else C + 5) if ring else C
    tol = 3e-2 if bf16 else 2e-5
    q, k, v = (_rand(n, S, E, seed=400 + i) for i in range(3))
    kc, vc = F.attention_stream_caches(S, H, hd, C, bf16=bf16, device=DEV, fill=float("nan"))
    kc2, vc2 = kc.clone(), vc.clone()
    tw = -(-C // R)
    kp, vp = F.attention_stream_pools(S * tw, H, hd, R, bf16=bf16, device=DEV, fill=float("nan"))
    table = torch.arange(S * tw, dtype=torch.int32).flip(0).reshape(tw, S).t().contiguous().to(DEV)      # slots interleave, ids descend
    act = torch.tensor([True, False, True], device=DEV)
    worst = 0.0
    for i in range(n):
        lengths = torch.full((S,), i, dtype=torch.int32, device=DEV)
        w = torch.full((S, H, C), float("nan"), device=DEV)
        wp = torch.full((S, H, C), float("nan"), device=DEV)
        out = F.attention_stream(q[i], k[i], v[i], kc, vc, lengths, act, H, ring=ring, bf16=bf16, weights=w)
        outp = F.attention_stream_paged(q[i], k[i], v[i], kp, vp, table, lengths, act, H, C, ring=ring, bf16=bf16, weights=wp)
        plain = F.attention_stream(q[i], k[i], v[i], kc2, vc2, lengths, act, H, ring=ring, bf16=bf16)
        assert torch.equal(out, plain), f"row {i}: the weights form must give the plain form's output bits"
        assert torch.equal(outp, out) and torch.equal(wp, w), f"row {i}: dense and paged rows must be the same bits"
        assert torch.isfinite(w).all(), f"row {i}: every element of the rows must be written"
        first, count = streaming.logical_columns(i + 1, C, ring)
        assert first == (max(0, i - (C - 1)) if ring else 0) and count == i + 1 - first
        assert torch.all(w[1] == 0), "an inactive slot gets a row of zeros"
        assert torch.all(w[:, :, count:] == 0), "columns behind the live count are zeros"
        for s in (0, 2):
            K = k[first: i + 1, s].double().reshape(count, H, hd).permute(1, 0, 2)                      # [H, count, hd]
            p = torch.softmax((K @ q[i, s].double().reshape(H, hd, 1)).squeeze(-1) / math.sqrt(hd), dim=-1)
            worst = max(worst, (w[s, :, :count].double() - p).abs().max().item())
    print(f"hd={hd} C={C} ring={ring} bf16={bf16}: {n} rows, max |row - float64 softmax| = {worst:.3e} (bound {tol:.0e})")
    assert worst < tol, worst


def test_bad_weights_buffers_are_refused():
    S, H, hd, C = 2, 2, 16, 4
    q = _rand(S, H * hd)
    kc, vc = F.attention_stream_caches(S, H, hd, C, device=DEV)
    lengths, act = torch.zeros(S, dtype=torch.int32, device=DEV), torch.ones(S, device=DEV)
    for bad in (torch.zeros(S, H, C + 1, device=DEV), torch.zeros(S, H, C, device=DEV, dtype=torch.float64),
                torch.zeros(S, H, 2 * C, device=DEV)[:, :, ::2]):
        with pytest.raises(ValueError):
            F.attention_stream(q, q, q, kc, vc, lengths, act, H, weights=bad)


# ---- model level -------------------------------------------------------------------------------------------------------------------
def _model(cfg, past):
    m = M2FNet(cfg, context=(past, 0))
    m.load_state_dict(synth.make_state_dict(cfg))
    return m.to("cuda").eval()


def _rows(x, i, S):
    """column i of a [B, L, d] batch as the [S, d] rows of a step (slots B .. S - 1: zeros)"""
    out = torch.zeros(S, x.shape[2], device=x.device)
    out[: x.shape[0]] = x[:, i]
    return out


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("past", [None, 3])
def test_stream_rows_match_the_offline_causal_maps(past, use_graph):
    cfg, B, L, lengths, kind = synth.CASES["tiny_ragged"]
    text, audio, key_pad, _ = synth.make_inputs(cfg, B, L, lengths, kind)
    t, a, kp = text.cuda(), audio.cuda(), key_pad.cuda()
    m = _model(cfg, past)
    _, offline = m.attention_maps(t, a, kp, average_heads=False)
    offline = {n: v.cpu() for n, v in offline.items()}
    S = B + 1
    st = m.stream(S, capacity=16 if past is None else None, use_graph=use_graph, attention=True)
    ref = m.stream(S, capacity=16 if past is None else None, use_graph=use_graph)
    C = st.capacity
    assert C == (16 if past is None else past + 1)
    with pytest.raises(RuntimeError, match="step first"):
        st.attention()
    with pytest.raises(RuntimeError, match="attention=True"):
        ref.attention()
    worst = 0.0
    with torch.inference_mode():
        for i in range(L):
            act = (~key_pad[:, i]).tolist() + [False]
            logits = st.step(_rows(t, i, S), _rows(a, i, S), active=act)
            assert torch.equal(logits, ref.step(_rows(t, i, S), _rows(a, i, S), active=act)), f"column {i}: logits must not change by a bit"
            att = st.attention(average_heads=False)
            avg = st.attention()
            assert list(att.weights) == list(offline)
            for s in range(S):
                if not act[s]:
                    assert att.count[s] == 0
                    continue
                lo = 0 if past is None else max(0, i - past)
                assert (att.first[s], att.count[s]) == (lo, i + 1 - lo), (s, i)
            for name, w in att.weights.items():
                assert w.shape == (S, offline[name].shape[1], C) and avg.weights[name].shape == (S, C)
                assert torch.equal(avg.weights[name], A.head_average(w[:, :, None])[:, 0]), name       # the head-average rule, exactly
                w = w.cpu()
                for s in range(S):
                    n = att.count[s]
                    assert torch.all(w[s, :, n:] == 0), (name, s, i)
                    if n:
                        want = offline[name][s, :, i, att.first[s]: att.first[s] + n]
                        worst = max(worst, (w[s, :, :n] - want).abs().max().item())
    print(f"tiny_ragged past={past} graph={use_graph}: max |stream row - offline map| = {worst:.3e} (bound {2 * TOL_LOGITS:.0e})")
    assert worst < 2 * TOL_LOGITS, worst
    assert st.lengths == lengths + [0]
    some = st.attention(sites=["fusion_layers.1.multihead_attention"])
    assert list(some.weights) == ["fusion_layers.1.multihead_attention"]
    with pytest.raises(ValueError, match="unknown attention site"):
        st.attention(sites=["fusion_layers.9.multihead_attention"])
    st.reset([0])
    with pytest.raises(RuntimeError, match="step first"):
        st.attention()


def test_attention_after_prefill_raises_and_a_step_answers_again():
    cfg, B, L, lengths, kind = synth.CASES["tiny_ragged"]
    text, audio, key_pad, _ = synth.make_inputs(cfg, B, L, lengths, kind)
    t, a = text.cuda(), audio.cuda()
    m = _model(cfg, None)
    st = m.stream(B, capacity=16, max_chunk=4, attention=True)
    plain = m.stream(B, capacity=16, max_chunk=4)
    with torch.inference_mode():
        got = st.prefill(t[:, :4], a[:, :4], counts=[4, 1, 4, 4, 2])
        assert torch.equal(got, plain.prefill(t[:, :4], a[:, :4], counts=[4, 1, 4, 4, 2]))
        with pytest.raises(RuntimeError, match="step first"):
            st.attention()
        act = [True, False, False, True, False]                          # dialogues 0 and 3 go on with their fifth utterance
        logits = st.step(t[:, 4], a[:, 4], active=act)
        assert torch.equal(logits, plain.step(t[:, 4], a[:, 4], active=act))
        att = st.attention()
    assert att.first == [0] * B and att.count == [5, 0, 0, 5, 0]
    _, offline = m.attention_maps(t, a, key_pad.cuda())
    for name, w in att.weights.items():
        for s in (0, 3):
            assert (w[s, :5] - offline[name][s, 4, :5]).abs().max().item() < 2 * TOL_LOGITS, (name, s)
        assert torch.all(w[[1, 2, 4]] == 0)
