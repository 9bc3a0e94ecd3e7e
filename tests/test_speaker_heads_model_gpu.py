"""M2FNet with speaker-aware attention heads (M2FNet(speaker_heads=(n_same, n_other)), set_speaker_heads) against the oracle with
tests/golden/speaker_heads_ref.py swapped in for its attention: eval logits, train_step loss and gradients, input gradients, padded /
bucketed / packed / long-dialogue plans with and without a position bias, a shuffled batch (speakers follow the layout), attention
maps, graph replay while the speakers change, bf16, streaming (run, steps, prefill, paged, snapshots), the default model untouched bit
for bit, the refusals, and the drop-in loop's runtime.speaker_heads."""
import functools
import os
import sys

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import attention_maps_ref as A  # noqa: E402
import band_ref as BR  # noqa: E402
import long_cases  # noqa: E402
import speaker_heads_ref as R  # noqa: E402
import synth  # noqa: E402
from oracle import m2fnet_oracle as O  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import layout  # noqa: E402
from mer_amd.distill import Distiller  # noqa: E402
from mer_amd.dp import DataParallelStep  # noqa: E402
from mer_amd.model import FusionAttentionModule, M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam  # noqa: E402

HEADS = (1, 1)
TOL_LOGITS, TOL_LOSS = 1e-4, 2e-5       # tests/test_context_window_model_gpu.py
TOL_LOGITS_BF16 = 3e-2                  # tests/test_model_gpu.py
TOL_MAPS = 1e-4                         # tests/test_attention_maps_model_gpu.py, fp32


def _case(name):
    if name in long_cases.CASES:
        return long_cases.inputs(name)
    cfg, B, L, lengths, kind = synth.CASES[name]
    return (cfg,) + synth.make_inputs(cfg, B, L, lengths, kind)


def _spk(B, L, shift=0):
    """int64 [B, L]: three speakers taking turns of two utterances, id 255 among them; the last dialogue is a monologue"""
    i = torch.arange(L)
    s = ((i // 2)[None, :] + torch.arange(B)[:, None] + shift) % 3
    s[s == 2] = 255
    s[B - 1] = 11
    return s


@functools.lru_cache(maxsize=None)
def _speakers(name, shift=0):
    key_pad = _case(name)[3]
    return _spk(*key_pad.shape, shift)


@functools.lru_cache(maxsize=None)
def _oracle(name, band, gain=None, heads=HEADS, shift=0):
    """(logits, loss, gradients with "text" / "audio") of the oracle under the band, the gain and the speaker heads"""
    cfg, text, audio, key_pad, emotion = _case(name)
    with R.swapped_in(band, gain, _speakers(name, shift), heads):
        logits, loss, grads = O.loss_and_grads(synth.make_state_dict(cfg), cfg, text, audio, key_pad, emotion, input_grads=True)
    assert torch.isfinite(logits).all()
    return logits, float(loss), grads


@functools.lru_cache(maxsize=None)
def _oracle_forward(name, past, heads=HEADS, seed=7):
    """eval logits of the oracle under (past, 0) and the speaker heads with the weights of `seed` (the streaming tests' weights)"""
    cfg, text, audio, key_pad, _ = _case(name)
    with R.swapped_in((past, 0), None, _speakers(name), heads):
        logits = O.forward(synth.make_state_dict(cfg, seed=seed), cfg, text, audio, key_pad)
    assert torch.isfinite(logits).all()
    return logits


def _model(cfg, precision="fp32", train=False, seed=None, **kw):
    m = M2FNet(cfg, precision=precision, **kw)
    m.load_state_dict(synth.make_state_dict(cfg) if seed is None else synth.make_state_dict(cfg, seed=seed))
    m = m.to("cuda")
    return m.train() if train else m.eval()


def _cuda(*ts):
    return [t.cuda() for t in ts]


def _check_grads(m, grads, label):
    for k, p in m.named_parameters():
        g, ref = p.grad.detach().cpu().double(), grads[k].double()
        assert torch.isfinite(g).all(), (label, k)
        err = (g - ref).abs().max().item()
        assert err <= 3e-5 + 1e-3 * ref.abs().max().item(), (label, k, err)


def _check_model(name, band, gain=None, heads=HEADS, **kw):
    cfg, text, audio, key_pad, emotion = _case(name)
    spk = _speakers(name)
    ref_logits, ref_loss, grads = _oracle(name, band, gain, heads)
    # the test can fail: the oracle WITHOUT the speaker condition is more than ten bounds away on this very case
    plain = _oracle(name, band, gain, None)[0]
    shift = (plain - ref_logits).abs()[~key_pad].max().item()
    print(f"{name} {band}: the speaker heads move the oracle's logits by {shift:.3e} (bound {TOL_LOGITS:.0e})")
    assert shift > 10 * TOL_LOGITS, shift
    t, a, kp, em, sp = _cuda(text, audio, key_pad, emotion, spk)
    m = _model(cfg, context=band, position_bias=gain, speaker_heads=heads, **kw)
    assert m.context == band and m.speaker_heads == heads
    with torch.inference_mode():
        logits = m(t, a, kp, speakers=sp).cpu()
    assert torch.isfinite(logits).all()
    err = (logits - ref_logits).abs()[~key_pad].max().item()
    print(f"{name} {band} gain {gain} heads {heads} {kw}: eval logits err {err:.3e}")
    assert err < TOL_LOGITS, err
    m.train()
    loss = m.train_step(t, a, kp, em, use_graph=False, speakers=sp)
    print(f"{name} {band}: loss {loss.item():.7f} vs {ref_loss:.7f}")
    assert abs(loss.item() - ref_loss) < TOL_LOSS, (loss.item(), ref_loss)
    _check_grads(m, grads, "train_step")
    for pl in m.engine().plans.values():
        assert pl.band == band and pl.speakers == heads
    # the autograd path, with the input gradients
    m2 = _model(cfg, train=True, context=band, position_bias=gain, speaker_heads=heads, **kw)
    tg, ag = t.clone().requires_grad_(True), a.clone().requires_grad_(True)
    crit = torch.nn.CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    crit(m2(tg, ag, kp, speakers=sp).permute(0, 2, 1), em).backward()
    _check_grads(m2, grads, "autograd")
    cfg_on = {"text": cfg["TEXT"]["enabled"], "audio": cfg["AUDIO"]["enabled"]}
    for which, got in (("text", tg.grad), ("audio", ag.grad)):
        if not cfg_on[which]:
            continue
        got, ref = got.cpu(), grads[which]
        assert torch.isfinite(got).all(), which
        err = (got - ref)[~key_pad].abs().max().item()
        assert err <= 3e-5 + 1e-3 * ref[~key_pad].abs().max().item(), (which, err)
    return m


@pytest.mark.parametrize("gain", [None, 1.0], ids=["nobias", "bias"])
@pytest.mark.parametrize("band", [(None, None), (None, 0), (2, 0)], ids=str)
def test_tiny_ragged_matches_the_oracle(band, gain):
    """bucketed plans (the default): a 5 x 9 batch in an 8 x 16 plan"""
    m = _check_model("tiny_ragged", band, gain)
    assert any((pl.B, pl.L) != (5, 9) for pl in m.engine().plans.values())


def test_exact_padded_plan_matches_the_oracle():
    m = _check_model("tiny_ragged", (None, 0), 1.0, shape_buckets=False)
    assert all((pl.B, pl.L) == (5, 9) and not pl.packed for pl in m.engine().plans.values())


@pytest.mark.parametrize("band,gain", [((None, None), 1.0), ((None, 0), None), ((2, 0), 1.0)], ids=str)
def test_exact_padded_plan_matches_the_oracle_under_the_other_settings(band, gain):
    m = _check_model("tiny_ragged", band, gain, shape_buckets=False)
    assert all((pl.B, pl.L) == (5, 9) and not pl.packed for pl in m.engine().plans.values())


@pytest.mark.parametrize("band,gain", [((None, None), None), ((None, 0), 1.0), ((2, 0), None), ((2, 0), 1.0)], ids=str)
def test_packed_plan_matches_the_oracle(band, gain):
    m = _check_model("tiny_ragged", band, gain, packed=True)
    assert any(pl.packed for pl in m.engine().plans.values())


def test_two_same_speaker_heads_match_the_oracle():
    _check_model("tiny_ragged", (None, None), heads=(2, 0))


def test_odd_head_counts_match_the_oracle_causal():
    """head counts 4, 3 and 2: (1, 1) fills the smallest site"""
    _check_model("tiny_odd_heads", (None, 0))


@pytest.mark.parametrize("name", ["tiny_no_fam", "tiny_audio_only"])
def test_partial_models_match_the_oracle_causal(name):
    _check_model(name, (None, 0))


@pytest.mark.parametrize("band,gain", [((None, None), None), ((None, 0), 1.0), ((8, 0), None)], ids=str)
def test_long_dialogues_match_the_oracle(band, gain):
    _check_model("long_tiny", band, gain)


@pytest.mark.parametrize("kw", [dict(), dict(packed=True)], ids=["bucketed", "packed"])
def test_shuffling_the_batch_permutes_the_logits(kw):
    """speakers follow the layout: dialogue b keeps ITS ids wherever it sits in the batch"""
    cfg, text, audio, key_pad, _ = _case("tiny_ragged")
    B, L = key_pad.shape
    # turns of b + 1 utterances in dialogue b: every dialogue has its own pattern of equal speakers (only equality matters)
    ids = (torch.arange(L)[None, :] // (torch.arange(B)[:, None] + 1)) % 2
    t, a, kp, sp = _cuda(text, audio, key_pad, ids)
    m = _model(cfg, context=(None, 0), speaker_heads=HEADS, **kw)
    perm = torch.tensor([3, 0, 4, 2, 1], device="cuda")
    with torch.inference_mode():
        base = m(t, a, kp, speakers=sp).clone()
        shuffled = m(t[perm], a[perm], kp[perm], speakers=sp[perm]).clone()
    valid = ~kp[perm]
    err = (shuffled - base[perm]).abs()[valid].max().item()
    print(f"shuffled vs permuted logits: {err:.3e}")
    assert err < TOL_LOGITS
    with torch.inference_mode():                                    # ... and ids that did NOT follow would have been seen
        wrong = m(t[perm], a[perm], kp[perm], speakers=sp).clone()
    assert (wrong - base[perm]).abs()[valid].max().item() > 10 * TOL_LOGITS


def test_graph_replay_with_fused_adam_follows_the_oracle_trajectory_while_speakers_change():
    band = (None, 0)
    cfg, text, audio, key_pad, emotion = _case("tiny_ragged")
    sd = synth.make_state_dict(cfg)
    uniq, order = {}, []
    for k, v in sd.items():
        if id(v) not in uniq:
            uniq[id(v)] = k
            order.append(k)
    params = [sd[k] for k in order]
    mo, vo = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    want = []
    for step in range(1, 4):
        with R.swapped_in(band, None, _speakers("tiny_ragged", step), HEADS):
            _, loss, grads = O.loss_and_grads(sd, cfg, text, audio, key_pad, emotion)
        want.append(loss.item())
        O.adam_step(params, [grads[k] for k in order], mo, vo, step, lr=1e-3, weight_decay=0.01)
    m = _model(cfg, train=True, context=band, speaker_heads=HEADS)
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01)
    batch = _cuda(text, audio, key_pad, emotion)
    got = []
    for step in range(1, 4):
        got.append(m.train_step(*batch, use_graph=True, speakers=_speakers("tiny_ragged", step).cuda()).item())
        opt.step()
    print("losses", got, "oracle", want)
    assert np.allclose(got, want, rtol=0, atol=1e-4), (got, want)
    assert len(m.engine().plans) == 1


def test_bf16_mode_within_the_stated_tolerance_causal():
    band = (None, 0)
    cfg, text, audio, key_pad, emotion = _case("tiny_ragged")
    ref_logits, _, _ = _oracle("tiny_ragged", band)
    sp = _speakers("tiny_ragged").cuda()
    m = _model(cfg, precision="bf16", context=band, speaker_heads=HEADS)
    with torch.inference_mode():
        logits = m(*_cuda(text, audio, key_pad), speakers=sp).cpu()
    err = (logits - ref_logits).abs()[~key_pad].max().item()
    print(f"bf16 causal, speaker heads: eval logits err {err:.3e}")
    assert err < TOL_LOGITS_BF16, err
    m.train()
    loss = m.train_step(*_cuda(text, audio, key_pad, emotion), use_graph=False, speakers=sp)
    assert torch.isfinite(loss)
    for k, p in m.named_parameters():
        assert p.grad is None or torch.isfinite(p.grad).all(), k


# ---- attention maps ------------------------------------------------------------------------------------------------------------------
def test_last_attention_equals_the_oracles_probabilities_at_every_site():
    band = (None, 0)
    cfg, text, audio, key_pad, _ = _case("tiny_odd_heads")
    spk = _speakers("tiny_odd_heads")
    plain = O.attention
    rec = {}

    def wrapper(q, k, v, kp, n_head, return_probs=False, drop=None, name=""):
        o, p = R.attention(q, k, v, kp, n_head, True, drop, name, band, 0.0, spk, HEADS)
        rec[A.site_name(name)] = p.detach()
        return (o, p) if return_probs else o

    O.attention = wrapper
    try:
        O.forward(synth.make_state_dict(cfg), cfg, text, audio, key_pad)
    finally:
        O.attention = plain
    assert list(rec) == [n for n, _, _ in layout.attention_sites(cfg)]
    m = _model(cfg, context=band, speaker_heads=HEADS)
    _, maps = m.attention_maps(*_cuda(text, audio, key_pad), average_heads=False, speakers=spk.cuda())
    rows = (~key_pad)[:, None, :, None]
    worst = 0.0
    for name, p in rec.items():
        got = maps[name].cpu().double()
        assert got.shape == p.shape and torch.isfinite(got).all(), name
        worst = max(worst, (got - p.double()).abs()[rows.expand_as(got)].max().item())
        hidden = R.speaker_hidden(spk, p.shape[1], HEADS)
        assert torch.all(got[hidden] == 0), f"{name}: pairs the speaker heads hide must be exactly 0"
    print(f"max |map - oracle probabilities| over {len(rec)} sites = {worst:.3e}")
    assert worst < TOL_MAPS, worst


# ---- streaming -----------------------------------------------------------------------------------------------------------------------
def _stream_err(logits, ref, key_pad):
    assert torch.isfinite(logits).all() and torch.all(logits[key_pad] == 0)
    return (logits.cpu() - ref).abs()[~key_pad].max().item()


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name,past", [("tiny_ragged", None), ("tiny_ragged", 3)])
def test_stream_matches_the_oracle(name, past, precision, use_graph):
    cfg, text, audio, key_pad, _ = _case(name)
    ref = _oracle_forward(name, past)
    tol = TOL_LOGITS if precision == "fp32" else TOL_LOGITS_BF16
    m = _model(cfg, precision, seed=7, context=(past, 0), speaker_heads=HEADS)
    B, L = key_pad.shape
    t, a, kp, sp = _cuda(text, audio, key_pad, _speakers(name))
    lengths = (~key_pad).sum(1).tolist()
    with torch.inference_mode():
        offline = m(t, a, kp, speakers=sp).cpu()
        assert (offline - ref).abs()[~key_pad].max().item() < tol
        st = m.stream(B + 1, use_graph=use_graph, max_chunk=4)
        assert st.speaker_heads == HEADS and st.plan.speakers == HEADS and st.chunk_plan.speakers == HEADS
        assert st.speaker_cache.shape == (B + 1, st.capacity) and st.speaker_cache.dtype == torch.uint8
        ran = st.run(t, a, kp, speakers=sp).cpu()                   # (the chunk plan: four columns per call)
        err = _stream_err(ran, ref, key_pad)
        print(f"{name} past={past} {precision} run: {err:.3e} (bound {tol:.0e})")
        assert err < tol, err
        # step by step, a dense and a paged stream side by side
        dense, paged = m.stream(B, use_graph=use_graph), m.stream(B, use_graph=use_graph, pages=4 * B * -(-L // 16), page_rows=16)
        stepped = torch.zeros_like(ran)
        for i in range(L):
            act = (~key_pad[:, i]).tolist()
            if not any(act):
                continue
            o = dense.step(t[:, i], a[:, i], act, speakers=sp[:, i])
            assert torch.equal(o, paged.step(t[:, i], a[:, i], act, speakers=sp[:, i])), "paged must give the dense stream's bits"
            stepped[:, i] = o.cpu()
        assert torch.equal(dense.speaker_cache, paged.speaker_cache)
        err = _stream_err(stepped, ref, key_pad)
        print(f"{name} past={past} {precision} steps: {err:.3e}")
        assert err < tol, err
        # prefill the first half through the chunk plan, then steps
        st.reset()
        half = [n // 2 for n in lengths] + [0]
        n_pre = max(half)
        pad_rows = lambda x: torch.cat([x[:, :n_pre], torch.zeros(1, n_pre, x.shape[2], device=x.device)])          # noqa: E731
        sp1 = torch.cat([sp, sp[:1]])
        pre = st.prefill(pad_rows(t), pad_rows(a), half, speakers=sp1[:, :n_pre])
        mixed = torch.zeros_like(ran)
        for b in range(B):
            mixed[b, :half[b]] = pre[b, :half[b]].cpu()
        for i in range(L):
            act = [half[b] <= i < lengths[b] for b in range(B)] + [False]
            if not any(act):
                continue
            o = st.step(torch.cat([t[:, i], t[:1, 0]]), torch.cat([a[:, i], a[:1, 0]]), act, speakers=sp1[:, i])
            for b in range(B):
                if act[b]:
                    mixed[b, i] = o[b].cpu()
        err = _stream_err(mixed, ref, key_pad)
        print(f"{name} past={past} {precision} prefill + steps: {err:.3e}")
        assert err < tol, err


@pytest.mark.parametrize("src_kw,dst_kw", [(dict(), dict(pages=64, page_rows=16)), (dict(pages=64, page_rows=16), dict(pages=64, page_rows=32))],
                         ids=["dense-to-paged", "rows16-to-rows32"])
def test_snapshot_reset_restore_continues_bit_for_bit(src_kw, dst_kw):
    name, past = "tiny_ragged", 3
    cfg, text, audio, key_pad, _ = _case(name)
    m = _model(cfg, seed=7, context=(past, 0), speaker_heads=HEADS)
    B, L = key_pad.shape
    t, a, sp = _cuda(text, audio, _speakers(name))
    with torch.inference_mode():
        st, twin, other = m.stream(B, **src_kw), m.stream(B, **src_kw), m.stream(B, **dst_kw)
        for i in range(6):                                           # (past the ring's four rows)
            st.step(t[:, i], a[:, i], speakers=sp[:, i])
            twin.step(t[:, i], a[:, i], speakers=sp[:, i])
        snap = st.snapshot()
        assert snap.speakers is not None and snap.speakers.dtype == torch.uint8 and snap.speakers.numel() == sum(snap.rows)
        back = type(snap).from_state_dict(snap.cpu().state_dict()).to("cuda")
        assert torch.equal(back.speakers, snap.speakers) and torch.equal(back.data, snap.data)
        st.reset()
        st.restore(back)
        other.restore(snap.select(list(range(B))))
        evicted = twin.evict([1])                                    # ... and a round trip of one slot through the host
        twin.restore(evicted.to("cuda"), [1])
        st.fork(0, 0)
        for i in range(6, L):
            want = twin.step(t[:, i], a[:, i], speakers=sp[:, i])
            assert torch.equal(st.step(t[:, i], a[:, i], speakers=sp[:, i]), want)
            assert torch.equal(other.step(t[:, i], a[:, i], speakers=sp[:, i]), want)
    # a mismatching snapshot is refused and the stream is left untouched
    plain = _model(cfg, seed=7, context=(past, 0))
    with torch.inference_mode():
        ps = plain.stream(B)
        for i in range(3):
            ps.step(t[:, i], a[:, i])
        psnap = ps.snapshot()
        assert psnap.speakers is None and "speakers" not in psnap.state_dict()
        lengths, cache = list(st.lengths), st.speaker_cache.clone()
        with pytest.raises(RuntimeError, match="speaker"):
            st.restore(psnap)
        assert st.lengths == lengths and torch.equal(st.speaker_cache, cache)
        plen = list(ps.lengths)
        with pytest.raises(RuntimeError, match="speaker"):
            ps.restore(snap)
        assert ps.lengths == plen
        with pytest.raises(ValueError, match="no speaker heads"):
            ps.step(t[:, 3], a[:, 3], speakers=sp[:, 3])
        with pytest.raises(ValueError, match="speakers="):
            st.step(t[:, 0], a[:, 0])


def test_a_stream_refuses_to_run_after_set_speaker_heads_until_it_is_reset():
    name, past = "tiny_ragged", None
    cfg, text, audio, key_pad, _ = _case(name)
    m = _model(cfg, seed=7, context=(past, 0), speaker_heads=HEADS)
    t, a, kp, sp = _cuda(text, audio, key_pad, _speakers(name))
    with torch.inference_mode():
        st = m.stream(key_pad.shape[0], max_chunk=4)
        first = st.run(t, a, kp, speakers=sp)
        snap = st.snapshot()
        m.set_speaker_heads(2, 0)
        assert st.speaker_heads == HEADS
        for call in (lambda: st.step(t[:, 0], a[:, 0], speakers=sp[:, 0]), lambda: st.prefill(t[:, :2], a[:, :2], speakers=sp[:, :2]),
                     lambda: st.run(t, a, kp, speakers=sp), lambda: st.restore(snap)):
            with pytest.raises(RuntimeError, match="speaker heads"):
                call()
        st.reset()                                                   # the whole stream: it takes the model's setting
        assert st.speaker_heads == (2, 0) and st.plan.speakers == (2, 0) and st.chunk_plan.speakers == (2, 0)
        second = st.run(t, a, kp, speakers=sp)
        ref = _oracle_forward(name, past, (2, 0))
        assert _stream_err(second.cpu(), ref, key_pad) < TOL_LOGITS
        assert not torch.equal(first, second)
        m.set_speaker_heads(None)                                    # off: the stream of a model that never had the setting
        st.reset()
        assert st.speaker_heads is None and st.speaker_cache is None and st.plan.speakers is None
        off = st.run(t, a, kp)
        with BR.swapped_in((None, 0)):
            ref0 = O.forward(synth.make_state_dict(cfg, seed=7), cfg, text, audio, key_pad)
        assert _stream_err(off.cpu(), ref0, key_pad) < TOL_LOGITS
        m.set_speaker_heads(*HEADS)
        st.reset()
        assert torch.equal(st.run(t, a, kp, speakers=sp), first)


# ---- the default model is untouched --------------------------------------------------------------------------------------------------
def _logits_and_grads(m, batch, **kw):
    m.eval()
    with torch.inference_mode():
        logits = m(*batch[:3], **kw).clone()
    m.train()
    m.train_step(*batch, use_graph=False, **kw)
    return logits, [p.grad.clone() for p in m.parameters()]


def test_default_model_is_bit_for_bit_what_it_was_and_settings_keep_their_plans():
    cfg, text, audio, key_pad, emotion = _case("tiny_ragged")
    batch = _cuda(text, audio, key_pad, emotion)
    sp = _speakers("tiny_ragged").cuda()
    want_logits, want_grads = _logits_and_grads(_model(cfg), batch)
    ref_logits = _oracle("tiny_ragged", (None, None))[0]
    assert (want_logits.cpu() - ref_logits).abs()[~key_pad].max().item() > 10 * TOL_LOGITS      # (the setting changes the numbers)
    got_logits, got_grads = _logits_and_grads(_model(cfg, speaker_heads=None), batch)
    assert torch.equal(got_logits, want_logits) and all(torch.equal(x, y) for x, y in zip(got_grads, want_grads))

    m = _model(cfg, speaker_heads=HEADS)
    aware_logits, _ = _logits_and_grads(m, batch, speakers=sp)
    assert (aware_logits.cpu() - ref_logits).abs()[~key_pad].max().item() < TOL_LOGITS
    eng = m.engine()
    aware = dict(eng.plans)
    assert len(aware) == 2 and all(k[-2] == ("speaker_heads", 1, 1) for k in aware)
    m.set_speaker_heads(None)
    assert m.speaker_heads is None
    got_logits, got_grads = _logits_and_grads(m, batch)
    assert torch.equal(got_logits, want_logits) and all(torch.equal(x, y) for x, y in zip(got_grads, want_grads))
    assert len(eng.plans) == 4 and all(eng.plans[k] is pl for k, pl in aware.items())           # new plans beside the old ones
    never = _model(cfg)
    _logits_and_grads(never, batch)
    assert {k for k in eng.plans if k not in aware} == set(never.engine().plans)                # the keys of a model that never heard of it
    for k, pl in eng.plans.items():
        assert pl.speakers == (HEADS if k in aware else None), k
        assert (len(k) == 8) == (k in aware)
    m.set_speaker_heads(*HEADS)                                      # and back: the setting's own plans, still holding it
    again, _ = _logits_and_grads(m, batch, speakers=sp)
    assert torch.equal(again, aware_logits) and len(eng.plans) == 4


def test_a_plain_stream_is_untouched_by_a_speaker_stream():
    cfg, text, audio, key_pad, _ = _case("tiny_ragged")
    batch = _cuda(text, audio, key_pad)
    sp = _speakers("tiny_ragged").cuda()
    plain, aware = _model(cfg, seed=7, context=(None, 0)), _model(cfg, seed=7, context=(None, 0), speaker_heads=HEADS)
    with torch.inference_mode():
        st = plain.stream(key_pad.shape[0])
        assert st.speaker_heads is None and st.plan.speakers is None and st.speaker_cache is None
        before = st.run(*batch).clone()
        other = aware.stream(key_pad.shape[0]).run(*batch, speakers=sp)
        assert not torch.equal(other, before)
        assert torch.equal(st.run(*batch), before)
    with BR.swapped_in((None, 0)):
        ref = O.forward(synth.make_state_dict(cfg, seed=7), cfg, text, audio, key_pad)
    assert _stream_err(before.cpu(), ref, key_pad) < TOL_LOGITS


# ---- refusals, Distiller, the standalone fusion module --------------------------------------------------------------------------------
def test_refusals_and_the_distiller():
    cfg, text, audio, key_pad, emotion = _case("tiny_ragged")
    t, a, kp, em, sp = _cuda(text, audio, key_pad, emotion, _speakers("tiny_ragged"))
    with pytest.raises(ValueError, match="exceeds the 2 heads of"):
        M2FNet(_case("tiny_odd_heads")[0], speaker_heads=(2, 1))     # (4, 3 and 2 heads: 3 do not fit the fusion layers' 2)
    m = _model(cfg, train=True, speaker_heads=HEADS)
    with pytest.raises(ValueError, match="pass speakers="):
        m(t, a, kp)
    with pytest.raises(ValueError, match="pass speakers="):
        m.train_step(t, a, kp, em)
    bad = sp.clone()
    bad[0, 0] = 256
    with pytest.raises(ValueError, match="0 .. 255"):
        m.train_step(t, a, kp, em, speakers=bad)
    with pytest.raises(ValueError, match=r"\[B, L\]"):
        m.train_step(t, a, kp, em, speakers=sp[:, :-1])
    plain = _model(cfg, train=True)
    with pytest.raises(ValueError, match="no speaker heads"):
        plain(t, a, kp, speakers=sp)
    # DataParallelStep: refused by name, before any launch or collective - at construction and, set later, at the call
    with pytest.raises(ValueError, match="DataParallelStep"):
        DataParallelStep(m, FusedAdam(m, lr=1e-3))
    step = DataParallelStep(plain, FusedAdam(plain, lr=1e-3))
    plain.set_speaker_heads(*HEADS)
    with pytest.raises(ValueError, match="DataParallelStep"):
        step(t, a, kp, em)
    plain.set_speaker_heads(None)
    # Distiller: each under its own setting; the ids go to whichever has one
    teacher = _model(cfg, seed=7)
    d = Distiller(m, teacher, alpha=0.5, temperature=2.0)
    with pytest.raises(ValueError, match="pass speakers="):
        d.train_step(t, a, kp, em)
    loss = d.train_step(t, a, kp, em, speakers=sp, use_graph=False)
    want = m.train_step(t, a, kp, em, speakers=sp, use_graph=False, teacher_logits=teacher(t, a, kp).detach(), distill=(0.5, 2.0))
    assert torch.equal(loss, want)
    d2 = Distiller(_model(cfg, train=True), _model(cfg, seed=7, speaker_heads=HEADS))
    assert torch.isfinite(d2.train_step(t, a, kp, em, speakers=sp, use_graph=False))
    with pytest.raises(ValueError, match="neither"):
        Distiller(_model(cfg, train=True), teacher).train_step(t, a, kp, em, speakers=sp)


def test_standalone_fusion_module_takes_speakers():
    B, L, E, H = 3, 9, 64, 4
    g = torch.Generator().manual_seed(3)
    text, audio = torch.randn(B, L, E, generator=g).cuda(), torch.randn(B, L, E, generator=g).cuda()
    kp = torch.zeros(B, L, dtype=torch.bool, device="cuda")
    kp[1, 5:] = True
    sp = _spk(B, L).cuda()
    torch.manual_seed(0)
    fam = FusionAttentionModule(E, H, 0.0, speaker_heads=HEADS).cuda().eval()
    torch.manual_seed(0)
    plain = FusionAttentionModule(E, H, 0.0).cuda().eval()
    with torch.no_grad():
        y, w = fam(text, audio, kp, need_weights=True, speakers=sp)
        y0 = plain(text, audio, kp)
        with pytest.raises(ValueError, match="pass speakers="):
            fam(text, audio, kp)
        with pytest.raises(ValueError, match="no speaker heads"):
            plain(text, audio, kp, speakers=sp)
    assert torch.isfinite(y).all() and (y - y0).abs().max().item() > 1e-3 and w.shape == (B, L, L)
    with pytest.raises(ValueError, match="exceeds"):
        FusionAttentionModule(E, H, 0.0, speaker_heads=(3, 2))


# ---- drop-in loop --------------------------------------------------------------------------------------------------------------------
def _dataset(n_dia, d_t, d_a, seed):
    import dataset as ds
    g = np.random.default_rng(seed)
    rows = []
    for d in range(n_dia):
        for u in range(int(g.integers(1, 10))):
            rows.append((f"utt {d}-{u}", list(ds.EMOTIONS)[int(g.integers(0, 7))], d, u, ["Ross", "Rachel", "Joey"][int(g.integers(0, 3))]))
    order = g.permutation(len(rows))
    table = pd.DataFrame([rows[i] for i in order], columns=["Utterance", "Emotion", "Dialogue_ID", "Utterance_ID", "Speaker"])
    text = torch.from_numpy(g.standard_normal((len(rows), d_t)).astype(np.float32))
    audio = torch.from_numpy(g.standard_normal((len(rows), d_a)).astype(np.float32))
    return ds.Dataset("train", text_embeddings=text, audio_embeddings=audio, table=table, speakers=True)


def test_drop_in_loop_trains_validates_and_tests_under_runtime_speaker_heads(tmp_path, monkeypatch):
    monkeypatch.chdir(ROOT)
    import dataset as ds
    import train as tr
    import test as te
    from utils import AttrDict, get_config
    cfg = AttrDict(dict(get_config()))
    assert tr.speaker_heads_settings(cfg) is None                    # (the key is absent from the shipped configuration)
    cfg.model = AttrDict(synth._cfg(40, 48, 64, 4, 4, 4, 1, 1, 1, dropout=0.1))
    cfg.runtime = AttrDict(dict(cfg.runtime, context=AttrDict(past=4, future=0), speaker_heads=AttrDict(same=1, other=2)))
    cfg.solver = AttrDict(dict(cfg.solver, epochs=1, lr=2e-3, early_stopping=AttrDict(enabled=False, patience=2, restore_best_weights=False),
                               scheduler=AttrDict(enabled=False, scheduler_fn="ExponentialLR", gamma=0.9)))
    cfg.checkpoint = AttrDict(save_path=str(tmp_path / "ck" / "m2fnet.pth"), load_path=str(tmp_path / "ck" / "m2fnet.pth"),
                              save_checkpoint=False, load_checkpoint=False)
    assert tr.speaker_heads_settings(cfg) == (1, 2)
    with pytest.raises(ValueError, match="single process"):
        tr.speaker_heads_settings(cfg, world=2)
    d_train, d_val = _dataset(24, 48, 40, 1), _dataset(8, 48, 40, 2)
    dl_train = torch.utils.data.DataLoader(d_train, collate_fn=ds.collate_fn, batch_size=8, shuffle=True)
    dl_val = torch.utils.data.DataLoader(d_val, collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = tr.build_model(cfg, device)                             # (what train.py's main builds)
    assert model.speaker_heads == (1, 2) and model.context == (4, 0)
    crit = tr.M2FCrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    opt = tr.FusedAdam(model, lr=cfg.solver.lr, weight_decay=cfg.solver.weight_decay)
    out = tr.training_loop(model, dl_train, dl_val, crit, opt, None, 0, cfg, device)
    assert len(out["loss_values"]) == 1 and np.isfinite(out["loss_values"][0]) and np.isfinite(out["val_loss_values"][0])
    loss_v, acc, f1 = tr.validate(model, dl_val, crit, device)
    assert np.isfinite(loss_v) and 0.0 <= acc <= 1.0 and 0.0 <= f1 <= 1.0
    plans = model.engine().plans
    assert plans and all(pl.speakers == (1, 2) and pl.band == (4, 0) for pl in plans.values())   # train and validation plans alike
    tested = te.build_model(cfg, device)                            # (what test.py's main builds)
    assert tested.speaker_heads == (1, 2)
    tested.load_state_dict(model.state_dict())
    acc_t, f1_t = te.test(tested, dl_val, device)
    assert abs(acc_t - acc) < 1e-9 and abs(f1_t - f1) < 1e-9
    # the device-scored pass and the streamed test pass: the same model through eval_step / a DialogueStream
    tested.device_metrics = True
    acc_d, _ = te.test(tested, dl_val, device)
    assert abs(acc_d - acc) < 1e-6
    streamed = te.build_model(cfg, device)
    streamed.load_state_dict(model.state_dict())
    streamed.streaming, streamed.stream_chunk, streamed.stream_pages = True, 1, 0
    acc_s, f1_s = te.test(streamed, dl_val, device)
    assert abs(acc_s - acc) < 0.05 and 0.0 <= f1_s <= 1.0          # (the same weights and rule through other kernels: the labels agree up to near-ties)
