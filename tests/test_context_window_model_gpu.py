"""M2FNet under a context band (M2FNet(context=(past, future)), set_context) against the oracle with tests/golden/band_ref.py swapped in
for its attention: eval logits, train_step loss and gradients, input gradients, packed / graph / bf16 variants, long dialogues,
blindness to the future at model level, the default model untouched, and the drop-in loop's runtime.context."""
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

import band_ref as R  # noqa: E402
import long_cases  # noqa: E402
import synth  # noqa: E402
from oracle import m2fnet_oracle as O  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam  # noqa: E402

TOL_LOGITS_BF16 = 3e-2          # tests/test_model_gpu.py


def _case(name):
    if name in long_cases.CASES:
        return long_cases.inputs(name)
    cfg, B, L, lengths, kind = synth.CASES[name]
    return (cfg,) + synth.make_inputs(cfg, B, L, lengths, kind)


@functools.lru_cache(maxsize=None)
def _oracle(name, band):
    """(logits, loss, gradients with "text" / "audio") of the oracle under the band; computed once per (case, band)"""
    cfg, text, audio, key_pad, emotion = _case(name)
    with R.swapped_in(band):
        logits, loss, grads = O.loss_and_grads(synth.make_state_dict(cfg), cfg, text, audio, key_pad, emotion, input_grads=True)
    assert torch.isfinite(logits).all()
    return logits, float(loss), grads


def _model(cfg, precision="fp32", train=False, **kw):
    m = M2FNet(cfg, precision=precision, **kw)
    m.load_state_dict(synth.make_state_dict(cfg))
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


def _check_model(name, band, **kw):
    cfg, text, audio, key_pad, emotion = _case(name)
    ref_logits, ref_loss, grads = _oracle(name, band)
    t, a, kp, em = _cuda(text, audio, key_pad, emotion)
    m = _model(cfg, context=band, **kw)
    assert m.context == band
    with torch.inference_mode():
        logits = m(t, a, kp).cpu()
    assert torch.isfinite(logits).all()
    err = (logits - ref_logits).abs()[~key_pad].max().item()
    print(f"{name} {band} {kw}: eval logits err {err:.3e}")
    assert err < 1e-4, err
    m.train()
    loss = m.train_step(t, a, kp, em, use_graph=False)
    print(f"{name} {band}: loss {loss.item():.7f} vs {ref_loss:.7f}")
    assert abs(loss.item() - ref_loss) < 2e-5, (loss.item(), ref_loss)
    _check_grads(m, grads, "train_step")
    for pl in m.engine().plans.values():
        assert pl.band == band
    # the autograd path, with the input gradients
    m2 = _model(cfg, train=True, context=band, **kw)
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
        assert err <= 3e-5 + 1e-3 * ref[~key_pad].abs().max().item(), (which, err)      # (the bound of test_input_grads_gpu.py)
    return m


@pytest.mark.parametrize("band", [(None, 0), (2, 0), (1, 1)])
def test_tiny_ragged_matches_the_oracle_under_the_band(band):
    _check_model("tiny_ragged", band)


def test_bucketed_plan_has_pad_queries_that_see_no_key():
    """(what tiny_ragged under (2, 0) is in the list for: 9 utterances in a 16-slot plan)"""
    _, _, _, key_pad, _ = _case("tiny_ragged")
    kp16 = torch.ones(key_pad.shape[0], 16, dtype=torch.bool)
    kp16[:, :key_pad.shape[1]] = key_pad
    assert (~R.visible_rows(kp16, (2, 0))).any()


@pytest.mark.parametrize("name", ["tiny_no_fam", "tiny_audio_only"])
def test_partial_models_match_the_oracle_causal(name):
    _check_model(name, (None, 0))


@pytest.mark.parametrize("band", [(None, 0), (8, 0)])
def test_long_dialogues_match_the_oracle_under_the_band(band):
    _check_model("long_tiny", band)


def test_packed_plan_matches_the_oracle_under_the_band():
    m = _check_model("tiny_ragged", (2, 0), packed=True)
    assert any(pl.packed for pl in m.engine().plans.values())


def test_graph_replay_with_fused_adam_follows_the_oracle_trajectory():
    band = (2, 0)
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
    with R.swapped_in(band):
        for step in range(1, 4):
            _, loss, grads = O.loss_and_grads(sd, cfg, text, audio, key_pad, emotion)
            want.append(loss.item())
            O.adam_step(params, [grads[k] for k in order], mo, vo, step, lr=1e-3, weight_decay=0.01)
    m = _model(cfg, train=True, context=band)
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
    band = (None, 0)
    cfg, text, audio, key_pad, emotion = _case("tiny_ragged")
    ref_logits, _, _ = _oracle("tiny_ragged", band)
    m = _model(cfg, precision="bf16", context=band)
    with torch.inference_mode():
        logits = m(*_cuda(text, audio, key_pad)).cpu()
    err = (logits - ref_logits).abs()[~key_pad].max().item()
    print(f"bf16 causal: eval logits err {err:.3e}")
    assert err < TOL_LOGITS_BF16, err
    m.train()
    loss = m.train_step(*_cuda(text, audio, key_pad, emotion), use_graph=False)
    assert torch.isfinite(loss)
    for k, p in m.named_parameters():
        assert p.grad is None or torch.isfinite(p.grad).all(), k


# ---- blind to the future ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_logits_up_to_n_do_not_depend_on_what_follows(precision):
    name, n = "tiny_odd_heads", 9
    cfg, text, audio, key_pad, _ = _case(name)
    m = _model(cfg, precision=precision, context=(None, 0))
    t, a, kp = _cuda(text, audio, key_pad)
    with torch.inference_mode():
        first = m(t, a, kp).clone()
        g = torch.Generator().manual_seed(5)
        t2, a2 = t.clone(), a.clone()
        t2[:, n + 1:] = (torch.randn(t2[:, n + 1:].shape, generator=g) * 3.0).cuda()
        a2[:, n + 1:] = (torch.randn(a2[:, n + 1:].shape, generator=g) * 3.0).cuda()
        second = m(t2, a2, kp).clone()
        assert len(m.engine().plans) == 1                           # (same batch shape, same plan)
        assert torch.equal(first[:, :n + 1], second[:, :n + 1])
        later = ~kp[:, n + 1:]
        assert not torch.equal(first[:, n + 1:][later], second[:, n + 1:][later])
        # the same dialogues cut after utterance n: another bucket (16 slots instead of 48), the same numbers within two fp32 bounds
        if precision == "fp32":
            cut = m(t[:, :n + 1].contiguous(), a[:, :n + 1].contiguous(), kp[:, :n + 1].contiguous())
            assert len(m.engine().plans) == 2
            valid = ~kp[:, :n + 1]
            err = (cut - first[:, :n + 1])[valid].abs().max().item()
            print(f"truncated dialogues: {err:.3e}")
            assert err < 2e-4, err
    # a model without the band does depend on the future (the test can fail)
    m0 = _model(cfg, precision=precision)
    with torch.inference_mode():
        assert not torch.equal(m0(t, a, kp)[:, :n + 1][~kp[:, :n + 1]], m0(t2, a2, kp)[:, :n + 1][~kp[:, :n + 1]])


# ---- the default model is untouched --------------------------------------------------------------------------------------------------
def _logits_and_grads(m, batch):
    m.eval()
    with torch.inference_mode():
        logits = m(*batch[:3]).clone()
    m.train()
    m.train_step(*batch, use_graph=False)
    return logits, [p.grad.clone() for p in m.parameters()]


def test_default_model_is_bit_for_bit_what_it_was_and_bands_keep_their_plans():
    cfg, text, audio, key_pad, emotion = _case("tiny_ragged")
    batch = _cuda(text, audio, key_pad, emotion)
    want_logits, want_grads = _logits_and_grads(_model(cfg), batch)
    ref_logits = _oracle("tiny_ragged", (2, 0))[0]
    assert (want_logits.cpu() - ref_logits).abs()[~key_pad].max().item() > 1e-3      # (the band changes the numbers: the test can fail)
    got_logits, got_grads = _logits_and_grads(_model(cfg, context=None), batch)
    assert torch.equal(got_logits, want_logits) and all(torch.equal(a, b) for a, b in zip(got_grads, want_grads))

    m = _model(cfg, context=(2, 0))
    banded_logits, _ = _logits_and_grads(m, batch)
    assert (banded_logits.cpu() - ref_logits).abs()[~key_pad].max().item() < 1e-4
    eng = m.engine()
    banded = dict(eng.plans)
    assert len(banded) == 2 and all(k[-2] == ("context", 2, 0) for k in banded)
    m.set_context(None, None)
    assert m.context == (None, None)
    got_logits, got_grads = _logits_and_grads(m, batch)
    assert torch.equal(got_logits, want_logits) and all(torch.equal(a, b) for a, b in zip(got_grads, want_grads))
    assert len(eng.plans) == 4 and all(eng.plans[k] is pl for k, pl in banded.items())          # new plans beside the old ones
    for k, pl in eng.plans.items():
        assert pl.band == ((2, 0) if k in banded else (None, None)), k
        assert (len(k) == 8) == (k in banded)                       # (a default key is the 6 fields + the instance it always was)
    m.set_context(2, 0)                                             # and back: the band's own plans, still holding its band
    again, _ = _logits_and_grads(m, batch)
    assert torch.equal(again, banded_logits) and len(eng.plans) == 4


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


def test_drop_in_loop_trains_validates_and_tests_under_runtime_context(tmp_path, monkeypatch):
    monkeypatch.chdir(ROOT)
    import dataset as ds
    import train as tr
    import test as te
    from utils import AttrDict, get_config
    cfg = AttrDict(dict(get_config()))
    cfg.model = AttrDict(synth._cfg(40, 48, 64, 4, 4, 4, 1, 1, 1, dropout=0.1))
    cfg.runtime = AttrDict(dict(cfg.runtime, context=AttrDict(past=4, future=0)))
    cfg.solver = AttrDict(dict(cfg.solver, epochs=1, lr=2e-3, early_stopping=AttrDict(enabled=False, patience=2, restore_best_weights=False),
                               scheduler=AttrDict(enabled=False, scheduler_fn="ExponentialLR", gamma=0.9)))
    cfg.checkpoint = AttrDict(save_path=str(tmp_path / "ck" / "m2fnet.pth"), load_path=str(tmp_path / "ck" / "m2fnet.pth"),
                              save_checkpoint=False, load_checkpoint=False)
    assert tr.context_settings(cfg) == (4, 0)
    d_train, d_val = _dataset(24, 48, 40, 1), _dataset(8, 48, 40, 2)
    dl_train = torch.utils.data.DataLoader(d_train, collate_fn=ds.collate_fn, batch_size=8, shuffle=True)
    dl_val = torch.utils.data.DataLoader(d_val, collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = tr.build_model(cfg, device)                             # (what train.py's main builds)
    assert model.context == (4, 0)
    crit = tr.M2FCrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    opt = tr.FusedAdam(model, lr=cfg.solver.lr, weight_decay=cfg.solver.weight_decay)
    out = tr.training_loop(model, dl_train, dl_val, crit, opt, None, 0, cfg, device)
    assert len(out["loss_values"]) == 1 and np.isfinite(out["loss_values"][0]) and np.isfinite(out["val_loss_values"][0])
    loss_v, acc, f1 = tr.validate(model, dl_val, crit, device)
    assert np.isfinite(loss_v) and 0.0 <= acc <= 1.0 and 0.0 <= f1 <= 1.0
    plans = model.engine().plans
    assert plans and all(pl.band == (4, 0) for pl in plans.values())          # train and validation plans alike
    tested = te.build_model(cfg, device)                            # (what test.py's main builds)
    assert tested.context == (4, 0)
    tested.load_state_dict(model.state_dict())
    acc_t, f1_t = te.test(tested, dl_val, device)
    assert abs(acc_t - acc) < 1e-9 and abs(f1_t - f1) < 1e-9
    assert all(pl.band == (4, 0) for pl in tested.engine().plans.values())
