"""M2FNet under the distance-decay attention bias (M2FNet(position_bias=gain), set_position_bias) against the oracle with
tests/golden/position_bias_ref.py swapped in for its attention: eval logits, train_step loss and gradients, input gradients, packed /
graph / bf16 variants, long dialogues, attention maps, streaming (run, steps, prefill, paged, snapshots), the default model untouched
bit for bit, and the drop-in loop's runtime.position_bias."""
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
import position_bias_ref as R  # noqa: E402
import synth  # noqa: E402
from oracle import m2fnet_oracle as O  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import layout  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam  # noqa: E402

GAIN = 1.0
TOL_LOGITS, TOL_LOSS = 1e-4, 2e-5       # tests/test_context_window_model_gpu.py
TOL_LOGITS_BF16 = 3e-2                  # tests/test_model_gpu.py
TOL_MAPS = 1e-4                         # tests/test_attention_maps_model_gpu.py, fp32


def _case(name):
    if name in long_cases.CASES:
        return long_cases.inputs(name)
    cfg, B, L, lengths, kind = synth.CASES[name]
    return (cfg,) + synth.make_inputs(cfg, B, L, lengths, kind)


@functools.lru_cache(maxsize=None)
def _oracle(name, band, gain=GAIN):
    """(logits, loss, gradients with "text" / "audio") of the oracle under the band and the gain; once per (case, band, gain)"""
    cfg, text, audio, key_pad, emotion = _case(name)
    with R.swapped_in(band, gain):
        logits, loss, grads = O.loss_and_grads(synth.make_state_dict(cfg), cfg, text, audio, key_pad, emotion, input_grads=True)
    assert torch.isfinite(logits).all()
    return logits, float(loss), grads


@functools.lru_cache(maxsize=None)
def _oracle_forward(name, past, gain=GAIN, seed=7):
    """eval logits of the oracle under (past, 0) and the gain with the weights of `seed` (the streaming tests' weights)"""
    cfg, text, audio, key_pad, _ = _case(name)
    with R.swapped_in((past, 0), gain):
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


def _check_model(name, band, gain=GAIN, **kw):
    cfg, text, audio, key_pad, emotion = _case(name)
    ref_logits, ref_loss, grads = _oracle(name, band, gain)
    # the test can fail: the oracle WITHOUT the term is more than ten bounds away on this very case
    plain = _oracle(name, band, None)[0]
    shift = (plain - ref_logits).abs()[~key_pad].max().item()
    print(f"{name} {band}: the term moves the oracle's logits by {shift:.3e}")
    assert shift > 10 * TOL_LOGITS, shift
    t, a, kp, em = _cuda(text, audio, key_pad, emotion)
    m = _model(cfg, context=band, position_bias=gain, **kw)
    assert m.context == band and m.position_bias == R.applied_gain(gain)
    with torch.inference_mode():
        logits = m(t, a, kp).cpu()
    assert torch.isfinite(logits).all()
    err = (logits - ref_logits).abs()[~key_pad].max().item()
    print(f"{name} {band} gain {gain} {kw}: eval logits err {err:.3e}")
    assert err < TOL_LOGITS, err
    m.train()
    loss = m.train_step(t, a, kp, em, use_graph=False)
    print(f"{name} {band}: loss {loss.item():.7f} vs {ref_loss:.7f}")
    assert abs(loss.item() - ref_loss) < TOL_LOSS, (loss.item(), ref_loss)
    _check_grads(m, grads, "train_step")
    for pl in m.engine().plans.values():
        assert pl.band == band and pl.bias == R.applied_gain(gain)
    # the autograd path, with the input gradients
    m2 = _model(cfg, train=True, context=band, position_bias=gain, **kw)
    tg, ag = t.clone().requires_grad_(True), a.clone().requires_grad_(True)
    crit = torch.nn.CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    crit(m2(tg, ag, kp).permute(0, 2, 1), em).backward()
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


@pytest.mark.parametrize("band", [(None, None), (None, 0), (2, 0)], ids=str)
def test_tiny_ragged_matches_the_oracle_under_the_bias(band):
    _check_model("tiny_ragged", band)


def test_odd_head_counts_match_the_oracle_causal():
    """head counts 4, 3 and 2: the slopes of a count that is no power of two"""
    _check_model("tiny_odd_heads", (None, 0))


@pytest.mark.parametrize("name", ["tiny_no_fam", "tiny_audio_only"])
def test_partial_models_match_the_oracle_causal(name):
    _check_model(name, (None, 0))


@pytest.mark.parametrize("band", [(None, 0), (8, 0)], ids=str)
def test_long_dialogues_match_the_oracle_under_the_bias(band):
    _check_model("long_tiny", band)


def test_packed_plan_matches_the_oracle_under_the_bias():
    m = _check_model("tiny_ragged", (None, 0), packed=True)
    assert any(pl.packed for pl in m.engine().plans.values())


def test_a_rounded_gain_matches_the_oracle_at_the_applied_value():
    m = _check_model("tiny_ragged", (None, 0), gain=0.3)
    assert m.position_bias == R.applied_gain(0.3) != 0.3


def test_graph_replay_with_fused_adam_follows_the_oracle_trajectory():
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
    with R.swapped_in(band, GAIN):
        for step in range(1, 4):
            _, loss, grads = O.loss_and_grads(sd, cfg, text, audio, key_pad, emotion)
            want.append(loss.item())
            O.adam_step(params, [grads[k] for k in order], mo, vo, step, lr=1e-3, weight_decay=0.01)
    m = _model(cfg, train=True, context=band, position_bias=GAIN)
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01)
    batch = _cuda(text, audio, key_pad, emotion)
    got = []
    for _ in range(3):
        got.append(m.train_step(*batch, use_graph=True).item())
        opt.step()
    print("losses", got, "oracle", want)
    assert np.allclose(got, want, rtol=0, atol=1e-4), (got, want)
    assert want[2] < want[0]


def test_bf16_mode_within_the_stated_tolerance_causal():
    """(does not discriminate at this size: the kernel-level probabilities of tests/test_position_bias_kernels_gpu.py do)"""
    band = (None, 0)
    cfg, text, audio, key_pad, emotion = _case("tiny_ragged")
    ref_logits, _, _ = _oracle("tiny_ragged", band)
    m = _model(cfg, precision="bf16", context=band, position_bias=GAIN)
    with torch.inference_mode():
        logits = m(*_cuda(text, audio, key_pad)).cpu()
    err = (logits - ref_logits).abs()[~key_pad].max().item()
    print(f"bf16 causal, gain 1: eval logits err {err:.3e}")
    assert err < TOL_LOGITS_BF16, err
    m.train()
    loss = m.train_step(*_cuda(text, audio, key_pad, emotion), use_graph=False)
    assert torch.isfinite(loss)
    for k, p in m.named_parameters():
        assert p.grad is None or torch.isfinite(p.grad).all(), k


# ---- attention maps ------------------------------------------------------------------------------------------------------------------
def test_last_attention_equals_the_oracles_probabilities_at_every_site():
    band = (None, 0)
    cfg, text, audio, key_pad, _ = _case("tiny_odd_heads")
    plain = O.attention
    rec = {}

    def wrapper(q, k, v, kp, n_head, return_probs=False, drop=None, name=""):
        o, p = R.attention(q, k, v, kp, n_head, True, drop, name, band, R.applied_gain(GAIN))
        rec[A.site_name(name)] = p.detach()
        return (o, p) if return_probs else o

    O.attention = wrapper
    try:
        O.forward(synth.make_state_dict(cfg), cfg, text, audio, key_pad)
    finally:
        O.attention = plain
    assert list(rec) == [n for n, _, _ in layout.attention_sites(cfg)]
    m = _model(cfg, context=band, position_bias=GAIN)
    with torch.no_grad():
        m(*_cuda(text, audio, key_pad))
    maps = m.last_attention(average_heads=False)
    rows = (~key_pad)[:, None, :, None]
    worst = 0.0
    for name, p in rec.items():
        got = maps[name].cpu().double()
        assert got.shape == p.shape and torch.isfinite(got).all(), name
        worst = max(worst, (got - p.double()).abs()[rows.expand_as(got)].max().item())
    print(f"max |map - oracle probabilities| over {len(rec)} sites = {worst:.3e}")
    assert worst < TOL_MAPS, worst


# ---- streaming -----------------------------------------------------------------------------------------------------------------------
def _stream_err(logits, ref, key_pad):
    assert torch.isfinite(logits).all() and torch.all(logits[key_pad] == 0)
    return (logits.cpu() - ref).abs()[~key_pad].max().item()


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name,past", [("tiny_ragged", None), ("tiny_ragged", 3), ("tiny_odd_heads", None), ("tiny_odd_heads", 3)])
def test_stream_matches_the_biased_oracle(name, past, precision, use_graph):
    cfg, text, audio, key_pad, _ = _case(name)
    ref = _oracle_forward(name, past)
    tol = TOL_LOGITS if precision == "fp32" else TOL_LOGITS_BF16
    m = _model(cfg, precision, seed=7, context=(past, 0), position_bias=GAIN)
    B, L = key_pad.shape
    t, a, kp = _cuda(text, audio, key_pad)
    lengths = (~key_pad).sum(1).tolist()
    with torch.inference_mode():
        st = m.stream(B + 1, use_graph=use_graph, max_chunk=4)
        assert st.position_bias == GAIN and st.plan.bias == GAIN and st.chunk_plan.bias == GAIN
        ran = st.run(t, a, kp).cpu()                                 # (the chunk plan: four columns per call)
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
            o = dense.step(t[:, i], a[:, i], act)
            assert torch.equal(o, paged.step(t[:, i], a[:, i], act)), "paged must give the dense stream's bits"
            stepped[:, i] = o.cpu()
        err = _stream_err(stepped, ref, key_pad)
        print(f"{name} past={past} {precision} steps: {err:.3e}")
        assert err < tol, err
        # prefill the first half through the chunk plan, then steps
        st.reset()
        half = [n // 2 for n in lengths] + [0]
        n_pre = max(half)
        pad_rows = lambda x: torch.cat([x[:, :n_pre], torch.zeros(1, n_pre, x.shape[2], device=x.device)])          # noqa: E731
        pre = st.prefill(pad_rows(t), pad_rows(a), half)
        mixed = torch.zeros_like(ran)
        for b in range(B):
            mixed[b, :half[b]] = pre[b, :half[b]].cpu()
        for i in range(L):
            act = [half[b] <= i < lengths[b] for b in range(B)] + [False]
            if not any(act):
                continue
            o = st.step(torch.cat([t[:, i], t[:1, 0]]), torch.cat([a[:, i], a[:1, 0]]), act)
            for b in range(B):
                if act[b]:
                    mixed[b, i] = o[b].cpu()
        err = _stream_err(mixed, ref, key_pad)
        print(f"{name} past={past} {precision} prefill + steps: {err:.3e}")
        assert err < tol, err


def test_snapshot_reset_restore_continues_bit_for_bit():
    name, past = "tiny_ragged", 3
    cfg, text, audio, key_pad, _ = _case(name)
    m = _model(cfg, seed=7, context=(past, 0), position_bias=GAIN)
    B, L = key_pad.shape
    t, a = _cuda(text, audio)
    with torch.inference_mode():
        st, twin = m.stream(B), m.stream(B)
        for i in range(5):
            st.step(t[:, i], a[:, i])
            twin.step(t[:, i], a[:, i])
        snap = st.snapshot()
        st.reset()
        st.restore(snap)
        for i in range(5, L):
            assert torch.equal(st.step(t[:, i], a[:, i]), twin.step(t[:, i], a[:, i]))


def test_a_stream_refuses_to_run_under_another_gain_until_it_is_reset():
    name, past = "tiny_ragged", None
    cfg, text, audio, key_pad, _ = _case(name)
    m = _model(cfg, seed=7, context=(past, 0), position_bias=GAIN)
    t, a, kp = _cuda(text, audio, key_pad)
    with torch.inference_mode():
        st = m.stream(key_pad.shape[0], max_chunk=4)
        first = st.run(t, a, kp)
        snap = st.snapshot()
        m.set_position_bias(0.5)
        assert st.position_bias == GAIN
        for call in (lambda: st.step(t[:, 0], a[:, 0]), lambda: st.prefill(t[:, :2], a[:, :2]), lambda: st.run(t, a, kp),
                     lambda: st.restore(snap)):
            with pytest.raises(RuntimeError, match="position bias"):
                call()
        st.reset()                                                   # the whole stream: it takes the model's gain
        assert st.position_bias == 0.5 and st.plan.bias == 0.5 and st.chunk_plan.bias == 0.5
        second = st.run(t, a, kp)
        ref = _oracle_forward(name, past, 0.5)
        assert _stream_err(second.cpu(), ref, key_pad) < TOL_LOGITS
        assert not torch.equal(first, second)
        m.set_position_bias(GAIN)
        st.reset()
        assert torch.equal(st.run(t, a, kp), first)


# ---- the default model is untouched --------------------------------------------------------------------------------------------------
def _logits_and_grads(m, batch):
    m.eval()
    with torch.inference_mode():
        logits = m(*batch[:3]).clone()
    m.train()
    m.train_step(*batch, use_graph=False)
    return logits, [p.grad.clone() for p in m.parameters()]


def test_default_model_is_bit_for_bit_what_it_was_and_gains_keep_their_plans():
    cfg, text, audio, key_pad, emotion = _case("tiny_ragged")
    batch = _cuda(text, audio, key_pad, emotion)
    want_logits, want_grads = _logits_and_grads(_model(cfg), batch)
    ref_logits = _oracle("tiny_ragged", (None, None))[0]
    assert (want_logits.cpu() - ref_logits).abs()[~key_pad].max().item() > 10 * TOL_LOGITS      # (the term changes the numbers)
    for kw in (dict(position_bias=None), dict(position_bias=0.0)):
        got_logits, got_grads = _logits_and_grads(_model(cfg, **kw), batch)
        assert torch.equal(got_logits, want_logits) and all(torch.equal(x, y) for x, y in zip(got_grads, want_grads))

    m = _model(cfg, position_bias=GAIN)
    biased_logits, _ = _logits_and_grads(m, batch)
    assert (biased_logits.cpu() - ref_logits).abs()[~key_pad].max().item() < TOL_LOGITS
    eng = m.engine()
    biased = dict(eng.plans)
    assert len(biased) == 2 and all(k[-2] == ("position_bias", 1.0) for k in biased)
    m.set_position_bias(None)
    assert m.position_bias is None
    got_logits, got_grads = _logits_and_grads(m, batch)
    assert torch.equal(got_logits, want_logits) and all(torch.equal(x, y) for x, y in zip(got_grads, want_grads))
    assert len(eng.plans) == 4 and all(eng.plans[k] is pl for k, pl in biased.items())          # new plans beside the old ones
    never = _model(cfg)
    _logits_and_grads(never, batch)
    assert {k for k in eng.plans if k not in biased} == set(never.engine().plans)               # the keys of a model that never heard of it
    for k, pl in eng.plans.items():
        assert pl.bias == (GAIN if k in biased else 0.0), k
        assert (len(k) == 8) == (k in biased)
    m.set_position_bias(GAIN)                                        # and back: the gain's own plans, still holding it
    again, _ = _logits_and_grads(m, batch)
    assert torch.equal(again, biased_logits) and len(eng.plans) == 4


def test_an_unbiased_stream_is_untouched_by_a_biased_one():
    cfg, text, audio, key_pad, _ = _case("tiny_ragged")
    batch = _cuda(text, audio, key_pad)
    plain, biased = _model(cfg, seed=7, context=(None, 0)), _model(cfg, seed=7, context=(None, 0), position_bias=GAIN)
    with torch.inference_mode():
        st = plain.stream(key_pad.shape[0])
        assert st.position_bias is None and st.plan.bias == 0.0
        before = st.run(*batch).clone()
        other = biased.stream(key_pad.shape[0]).run(*batch)
        assert not torch.equal(other, before)
        assert torch.equal(st.run(*batch), before)
    with BR.swapped_in((None, 0)):
        ref = O.forward(synth.make_state_dict(cfg, seed=7), cfg, text, audio, key_pad)
    assert _stream_err(before.cpu(), ref, key_pad) < TOL_LOGITS


# ---- drop-in loop --------------------------------------------------------------------------------------------------------------------
def _dataset(n_dia, d_t, d_a, seed):
    import dataset as ds
    g = np.random.default_rng(seed)
    rows = []
    for d in range(n_dia):
        for u in range(int(g.integers(1, 10))):
            rows.append((f"utt {d}-{u}", list(ds.EMOTIONS)[int(g.integers(0, 7))], d, u))
    order = g.permutation(len(rows))
    table = pd.DataFrame([rows[i] for i in order], columns=["Utterance", "Emotion", "Dialogue_ID", "Utterance_ID"])
    text = torch.from_numpy(g.standard_normal((len(rows), d_t)).astype(np.float32))
    audio = torch.from_numpy(g.standard_normal((len(rows), d_a)).astype(np.float32))
    return ds.Dataset("train", text_embeddings=text, audio_embeddings=audio, table=table)


def test_drop_in_loop_trains_validates_and_tests_under_runtime_position_bias(tmp_path, monkeypatch):
    monkeypatch.chdir(ROOT)
    import dataset as ds
    import train as tr
    import test as te
    from utils import AttrDict, get_config
    cfg = AttrDict(dict(get_config()))
    cfg.model = AttrDict(synth._cfg(40, 48, 64, 4, 4, 4, 1, 1, 1, dropout=0.1))
    cfg.runtime = AttrDict(dict(cfg.runtime, context=AttrDict(past=4, future=0), position_bias=1.0))
    cfg.solver = AttrDict(dict(cfg.solver, epochs=1, lr=2e-3, early_stopping=AttrDict(enabled=False, patience=2, restore_best_weights=False),
                               scheduler=AttrDict(enabled=False, scheduler_fn="ExponentialLR", gamma=0.9)))
    cfg.checkpoint = AttrDict(save_path=str(tmp_path / "ck" / "m2fnet.pth"), load_path=str(tmp_path / "ck" / "m2fnet.pth"),
                              save_checkpoint=False, load_checkpoint=False)
    assert tr.position_bias_settings(cfg) == 1.0
    d_train, d_val = _dataset(24, 48, 40, 1), _dataset(8, 48, 40, 2)
    dl_train = torch.utils.data.DataLoader(d_train, collate_fn=ds.collate_fn, batch_size=8, shuffle=True)
    dl_val = torch.utils.data.DataLoader(d_val, collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = tr.build_model(cfg, device)                             # (what train.py's main builds)
    assert model.position_bias == 1.0 and model.context == (4, 0)
    crit = tr.M2FCrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    opt = tr.FusedAdam(model, lr=cfg.solver.lr, weight_decay=cfg.solver.weight_decay)
    out = tr.training_loop(model, dl_train, dl_val, crit, opt, None, 0, cfg, device)
    assert len(out["loss_values"]) == 1 and np.isfinite(out["loss_values"][0]) and np.isfinite(out["val_loss_values"][0])
    loss_v, acc, f1 = tr.validate(model, dl_val, crit, device)
    assert np.isfinite(loss_v) and 0.0 <= acc <= 1.0 and 0.0 <= f1 <= 1.0
    plans = model.engine().plans
    assert plans and all(pl.bias == 1.0 and pl.band == (4, 0) for pl in plans.values())          # train and validation plans alike
    tested = te.build_model(cfg, device)                            # (what test.py's main builds)
    assert tested.position_bias == 1.0
    tested.load_state_dict(model.state_dict())
    acc_t, f1_t = te.test(tested, dl_val, device)
    assert abs(acc_t - acc) < 1e-9 and abs(f1_t - f1) < 1e-9
    assert all(pl.bias == 1.0 for pl in tested.engine().plans.values())
    # the streamed test pass: the same model through a DialogueStream
    streamed = te.build_model(cfg, device)
    streamed.load_state_dict(model.state_dict())
    streamed.streaming, streamed.stream_chunk, streamed.stream_pages = True, 1, 0
    acc_s, f1_s = te.test(streamed, dl_val, device)
    assert abs(acc_s - acc) < 0.05 and 0.0 <= f1_s <= 1.0          # (the same weights and rule through other kernels: the labels agree up to near-ties)
