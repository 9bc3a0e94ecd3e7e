"""M2FNet.attention_maps / last_attention and FusionAttentionModule(need_weights=True): the attention maps of every site against the
recorder of tests/attention_maps_ref.py (the oracle's own probabilities) and, at the first fusion layer, against the head-averaged
weights the real reference wrote into the fixtures (fam0_attn_avg) - padded, bucketed, packed and long-dialogue plans, after forward,
eval_step and train_step - and the logits of a model that was asked for its maps against one that never was, bit for bit.

Bounds: 1e-4 in fp32 mode (the eval-logits bound of tests/test_model_gpu.py; probabilities are O(1), so it is absolute), 3e-2 in bf16
mode.  Every comparison prints its measured maximum (DESIGN.md section 3 records them)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_maps_ref as A  # noqa: E402
import band_ref as R  # noqa: E402
import long_cases  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import layout  # noqa: E402
from mer_amd.metrics import DeviceScores  # noqa: E402
from mer_amd.model import FusionAttentionModule, M2FNet  # noqa: E402
from oracle import m2fnet_oracle as O  # noqa: E402

TOL = {"fp32": 1e-4, "bf16": 3e-2}
FIXTURES = ["tiny_ragged", "tiny_shared_norm", "tiny_odd_heads"]
FAM0 = "fusion_layers.0.multihead_attention"


def _case(name):
    if name in long_cases.CASES:
        return long_cases.inputs(name)
    cfg, B, L, lengths, kind = synth.CASES[name]
    return (cfg,) + synth.make_inputs(cfg, B, L, lengths, kind)


@functools.lru_cache(maxsize=None)
def _recorded(name, band=(None, None)):
    """(oracle logits, {site: P [B, H, L, L]}, the oracle's intermediates) - computed once per (case, band), never changed"""
    cfg, text, audio, key_pad, _ = _case(name)
    inter = {}
    with A.recording(band) as rec:
        logits = O.forward(synth.make_state_dict(cfg), cfg, text, audio, key_pad, inter=inter)
    assert list(rec) == [n for n, _, _ in layout.attention_sites(cfg)]
    return logits, rec, inter


def _model(cfg, precision="fp32", train=False, **kw):
    m = M2FNet(cfg, precision=precision, **kw)
    m.load_state_dict(synth.make_state_dict(cfg))
    m = m.to("cuda")
    return m.train() if train else m.eval()


def _cuda(*ts):
    return [t.cuda() for t in ts]


def _err(got, ref, sel=None):
    d = (got.detach().cpu().double() - ref.double()).abs()
    return (d if sel is None else d[sel.expand_as(d)]).max().item()


def _check_against_recorder(maps, rec, key_pad, tol, label, rows=None):
    """per-head maps of every site against the recorder, on the query rows `rows` ([B, L] bool; default: every row); pad keys exactly 0"""
    worst = 0.0
    B, L = key_pad.shape
    for name, p in rec.items():
        got = maps[name]
        assert got.shape == p.shape, (name, got.shape, p.shape)
        assert torch.isfinite(got).all(), name
        sel = None if rows is None else rows[:, None, :, None]
        worst = max(worst, _err(got, p, sel))
        assert torch.all(got.cpu()[key_pad[:, None, None, :].expand_as(got)] == 0), (name, "a padded key must have weight exactly 0")
    print(f"{label}: max |map - recorder| over {len(rec)} sites = {worst:.3e} (bound {tol:.0e})")
    assert worst < tol, (label, worst)
    return worst


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", FIXTURES)
def test_maps_match_the_reference_fixture_and_the_recorder(golden_dir, name, precision):
    fx = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    cfg, text, audio, key_pad, _ = _case(name)
    _, rec, _ = _recorded(name)
    t, a, kp = _cuda(text, audio, key_pad)
    m = _model(cfg, precision)
    logits, per_head = m.attention_maps(t, a, kp, average_heads=False)
    assert list(per_head) == [n for n, _, _ in layout.attention_sites(cfg)]
    _check_against_recorder(per_head, rec, key_pad, TOL[precision], f"{name} {precision}")
    avg = m.last_attention()
    err = _err(avg[FAM0], torch.from_numpy(fx["fam0_attn_avg"]))
    print(f"{name} {precision}: max |fusion_layers.0 averaged - reference fam0_attn_avg| = {err:.3e}")
    assert err < TOL[precision], err
    for n in per_head:                                  # the averaged form IS the rule applied to the per-head form
        assert torch.equal(avg[n], A.head_average(per_head[n])), n
    # nothing on the step path changed: a model that was never asked gives the same logits
    with torch.no_grad():
        assert torch.equal(_model(cfg, precision)(t, a, kp), logits)
        assert torch.equal(m(t, a, kp), logits)


@pytest.mark.parametrize("name", ["tiny_ragged", "tiny_odd_heads"])
def test_same_maps_from_every_entry_and_layout(name):
    cfg, text, audio, key_pad, emotion = _case(name)
    _, rec, _ = _recorded(name)
    t, a, kp, em = _cuda(text, audio, key_pad, emotion)
    valid = ~key_pad
    m = _model(cfg)                                     # bucketed padded plan (the default)
    with torch.no_grad():
        m(t, a, kp)
    base = m.last_attention(average_heads=False)
    _check_against_recorder(base, rec, key_pad, TOL["fp32"], f"{name} forward, bucketed")
    # eval_step: the same plan, the same launches
    m.eval_step(t, a, kp, em, DeviceScores(cfg["CLASSIFIER"]["output_size"], "cuda"))
    again = m.last_attention(average_heads=False)
    for n in base:
        assert torch.equal(again[n], base[n]), ("eval_step", n)
    # train_step with dropout 0: a train plan of the same shape
    mt = _model(cfg, train=True)
    mt.train_step(t, a, kp, em, use_graph=False)
    tr = mt.last_attention(average_heads=False)
    for n in base:                                      # (fp32 mode: the same attention kernel on the same layout and the same inputs)
        assert torch.equal(tr[n], base[n]), ("train_step", n)
    mt.train_step(t, a, kp, em, use_graph=True)         # ... and through the captured step
    mt.train_step(t, a, kp, em, use_graph=True)
    for n, v in mt.last_attention(average_heads=False).items():
        assert torch.equal(v, tr[n]), ("train_step graph", n)
    # the exact shape instead of a bucket
    mx = _model(cfg, shape_buckets=False)
    _, exact = mx.attention_maps(t, a, kp, average_heads=False)
    _check_against_recorder(exact, rec, key_pad, TOL["fp32"], f"{name} exact shape")
    # packed plan: valid rows within the bound of the oracle (and of the padded plan), pad rows and columns exactly zero
    mp = _model(cfg, packed=True)
    _, packed = mp.attention_maps(t, a, kp, average_heads=False)
    assert any(pl.packed for pl in mp.engine().plans.values())
    _check_against_recorder(packed, rec, key_pad, TOL["fp32"], f"{name} packed", rows=valid)
    for n, v in packed.items():
        v = v.cpu()
        assert _err(v, base[n].cpu(), valid[:, None, :, None]) < TOL["fp32"], n
        assert torch.all(v[key_pad[:, None, :, None].expand_as(v)] == 0), (n, "rows of pad slots are zero in packed plans")
    pavg = mp.last_attention()
    for n in packed:
        assert torch.equal(pavg[n], A.head_average(packed[n])), n


def test_long_dialogues_under_a_window():
    band = (3, 0)
    cfg, text, audio, key_pad, _ = _case("long_tiny")
    _, rec, _ = _recorded("long_tiny", band)
    B, L = key_pad.shape
    m = _model(cfg, context=band)
    _, maps = m.attention_maps(*_cuda(text, audio, key_pad), average_heads=False)
    valid = ~key_pad
    _check_against_recorder(maps, rec, key_pad, TOL["fp32"], "long_tiny (3, 0)", rows=valid)
    hide = A.hidden(key_pad, L, band) | key_pad[:, None, :, None]
    for n, v in maps.items():
        v = v.cpu()
        assert torch.all(v[hide.expand_as(v)] == 0), (n, "hidden pairs and pad rows are exactly zero")
        rows = v.sum(-1)[valid[:, None].expand(B, v.shape[1], L)]
        assert (rows - 1).abs().max().item() < 1e-5, n


def test_site_selection_and_refusals():
    cfg, text, audio, key_pad, _ = _case("tiny_shared_norm")
    m = _model(cfg)
    with pytest.raises(RuntimeError, match="no forward has run"):
        m.last_attention()
    t, a, kp = _cuda(text, audio, key_pad)
    _, all_maps = m.attention_maps(t, a, kp)
    want = ["text_encoders.2.layers.1.self_attn", FAM0]
    some = m.last_attention(sites=want)
    assert list(some) == want
    for n in want:
        assert torch.equal(some[n], all_maps[n])
        assert some[n].shape == (key_pad.shape[0], key_pad.shape[1], key_pad.shape[1])
    with pytest.raises(ValueError, match="unknown attention site"):
        m.last_attention(sites=["fusion_layers.7.multihead_attention"])
    plan = next(iter(m.engine().plans.values()))
    plan.close()
    with pytest.raises(RuntimeError, match="destroyed"):
        m.last_attention()


@pytest.mark.parametrize("name", FIXTURES)
def test_fusion_module_need_weights_matches_the_reference(golden_dir, name):
    fx = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    cfg, text, audio, key_pad, _ = _case(name)
    _, _, inter = _recorded(name)
    sd = synth.make_state_dict(cfg)
    pre = "fusion_layers.0."
    f = FusionAttentionModule(cfg["FAM"]["embedding_size"], cfg["FAM"]["n_head"], 0.0)
    f.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)})
    f = f.cuda().eval()
    args = _cuda(inter["text_proj"], inter["audio_proj"], key_pad)
    with torch.no_grad():
        y, w = f(*args, need_weights=True)
        y_only = f(*args)
    assert torch.equal(y, y_only)                       # the default is untouched
    err = _err(w, torch.from_numpy(fx["fam0_attn_avg"]))
    print(f"{name}: FusionAttentionModule weights vs reference fam0_attn_avg: {err:.3e}")
    assert err < TOL["fp32"], err
    assert _err(y, torch.from_numpy(fx["fam0_out"]), (~key_pad)[..., None]) < TOL["fp32"]


@pytest.mark.parametrize("device_metrics", [False, True])
def test_test_pass_writes_the_maps_of_every_dialogue(tmp_path, device_metrics):
    """src/test.py with runtime.attention_maps: one array per dialogue of the pass and site, cut to the dialogue's utterances"""
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    sys.path.insert(0, os.path.join(root, "src"))
    import test as te
    cfg, text, audio, key_pad, emotion = _case("tiny_ragged")
    _, rec, _ = _recorded("tiny_ragged")
    B = key_pad.shape[0]
    loader = [dict(text=text[:3], audio=audio[:3], emotion=emotion[:3], padding_mask=key_pad[:3]),
              dict(text=text[3:], audio=audio[3:], emotion=emotion[3:], padding_mask=key_pad[3:])]
    m = _model(cfg)
    m.device_metrics = device_metrics
    path = str(tmp_path / "maps.npz")
    m.attention_maps_out = (path, [FAM0, "text_encoders.0.layers.1.self_attn"])
    scores = te.test(m, loader, torch.device("cuda:0"))
    plain = _model(cfg)
    plain.device_metrics = device_metrics
    assert te.test(plain, loader, torch.device("cuda:0")) == scores          # the pass scores what it scored
    got = np.load(path)
    assert sorted(got.files) == sorted(f"{b}/{n}" for b in range(B) for n in m.attention_maps_out[1])
    lengths = (~key_pad).sum(1).tolist()
    for b, n in enumerate(lengths):
        for name in m.attention_maps_out[1]:
            a = got[f"{b}/{name}"]
            assert a.shape == (n, n) and a.dtype == np.float32
            want = A.head_average(rec[name])[b, :n, :n]
            assert np.abs(a - want.numpy()).max() < TOL["fp32"], (b, name)
