"""The drop-in loop with runtime.ema (src/train.py, src/test.py) on a synthetic MELD-shaped dataset: validation and early stopping
score the averaged weights, the checkpoints carry the average beside the LIVE weights, resume restores it, test.py scores it and
says so - and with the block disabled the loop and its checkpoint are what they were."""
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import synth  # noqa: E402


def _dataset(n_dia, d_t, d_a, seed):
    import dataset as ds
    g = np.random.default_rng(seed)
    rows = [(f"utt {d}-{u}", list(ds.EMOTIONS)[int(g.integers(0, 7))], d, u) for d in range(n_dia) for u in range(int(g.integers(1, 10)))]
    table = pd.DataFrame(rows, columns=["Utterance", "Emotion", "Dialogue_ID", "Utterance_ID"])
    text = torch.from_numpy(g.standard_normal((len(rows), d_t)).astype(np.float32))
    audio = torch.from_numpy(g.standard_normal((len(rows), d_a)).astype(np.float32))
    lab = table["Emotion"].map(ds.EMOTIONS).to_numpy()
    text[np.arange(len(rows)), lab] += 3.0                  # the label is learnable from the text rows
    return ds.Dataset("train", text_embeddings=text, audio_embeddings=audio, table=table)


def _config(tmp_path, **runtime):
    from utils import AttrDict, get_config
    cfg = AttrDict(dict(get_config()))
    cfg.model = AttrDict(synth._cfg(40, 48, 64, 4, 4, 4, 1, 1, 1, dropout=0.0))      # dropout off: two runs are compared
    cfg.runtime = AttrDict(dict(cfg.runtime, **runtime))
    cfg.solver = AttrDict(dict(cfg.solver, epochs=2, lr=2e-3, weight_decay=0.01,
                               early_stopping=AttrDict(enabled=True, patience=5, restore_best_weights=True),
                               scheduler=AttrDict(enabled=False, scheduler_fn="ExponentialLR", gamma=0.9)))
    cfg.checkpoint = AttrDict(save_path=str(tmp_path / "ck" / "m2fnet.pth"), load_path=str(tmp_path / "ck" / "m2fnet.pth"),
                              save_checkpoint=True, load_checkpoint=True)
    cfg.test = AttrDict(data_loader=AttrDict(batch_size=8, shuffle=False, num_workers=0))
    return cfg


def _loaders():
    import dataset as ds
    d_train, d_val = _dataset(40, 48, 40, 1), _dataset(12, 48, 40, 2)
    return (torch.utils.data.DataLoader(d_train, collate_fn=ds.collate_fn, batch_size=8, shuffle=True),
            torch.utils.data.DataLoader(d_val, collate_fn=ds.collate_fn, batch_size=8, shuffle=False), d_val)


@pytest.mark.parametrize("device_metrics", [False, True])
def test_loop_validates_checkpoints_resumes_and_tests_with_the_average(tmp_path, monkeypatch, capsys, device_metrics):
    monkeypatch.chdir(ROOT)
    import train as tr
    import test as te
    cfg = _config(tmp_path, ema={"enabled": True, "decay": 0.9, "warmup": True, "evaluate": True}, device_metrics=device_metrics)
    dl_train, dl_val, d_val = _loaders()
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = tr.M2FNet(cfg.model).to(device)
    model.device_metrics = device_metrics
    crit = tr.M2FCrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    opt = tr.build_optimizer(cfg, model)
    assert (opt.ema_decay, opt.ema_warmup) == (0.9, True)
    out = tr.training_loop(model, dl_train, dl_val, crit, opt, None, 0, cfg, device)
    assert len(out["val_loss_values"]) == 2 and opt.n_averaged == 2 * len(dl_train)
    printed = capsys.readouterr().out

    # the reported numbers are those of the averaged weights
    live = {n: p.detach().clone() for n, p in model.named_parameters()}
    with opt.averaged_parameters():
        by_hand = tr.validate(model, dl_val, crit, device)
    on_live = tr.validate(model, dl_val, crit, device)
    print(f"validation loss: reported {out['val_loss_values'][-1]!r}, by hand under averaged_parameters() {by_hand[0]!r}, live weights {on_live[0]!r}")
    assert out["val_loss_values"][-1] == by_hand[0]
    assert on_live[0] != by_hand[0]
    assert f"Val=[{by_hand[0]:.3E}]" in printed
    for n, p in model.named_parameters():
        assert torch.equal(p, live[n]), n                                    # the context gave the live weights back

    # checkpoints: the three entries with the LIVE weights, and the average beside them (best-weights file too)
    ck = torch.load(cfg.checkpoint.save_path)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "ema_state_dict"}
    for n, p in model.named_parameters():
        assert torch.equal(ck["model_state_dict"][n], p), n
    esd = opt.ema_state_dict()
    assert (ck["ema_state_dict"]["decay"], ck["ema_state_dict"]["warmup"], ck["ema_state_dict"]["n_averaged"]) == (0.9, True, opt.n_averaged)
    assert list(ck["ema_state_dict"]["parameters"]) == list(ck["model_state_dict"])
    for k, v in esd["parameters"].items():
        assert torch.equal(ck["ema_state_dict"]["parameters"][k], v), k
    best = torch.load(os.path.join(os.path.dirname(cfg.checkpoint.save_path), "best_weights.pth"))
    assert "ema_state_dict" in best

    # resume restores the average (and everything else, exactly)
    model2 = tr.M2FNet(cfg.model).to(device)
    opt2 = tr.build_optimizer(cfg, model2)
    assert tr.resume_if_requested(cfg, model2, opt2, device) == 2
    assert opt2.n_averaged == opt.n_averaged and torch.equal(opt2.ema_parameters(), opt.ema_parameters())
    for (n, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(p, q), n
    # ... a checkpoint without the entry resumes with a fresh average and says so
    old = str(tmp_path / "ck" / "old.pth")
    torch.save({k: ck[k] for k in tr.CHECKPOINT_KEYS}, old)
    cfg_old = _config(tmp_path, ema={"enabled": True, "decay": 0.9})
    cfg_old.checkpoint.load_path = old
    model3 = tr.M2FNet(cfg.model).to(device)
    opt3 = tr.build_optimizer(cfg_old, model3)
    capsys.readouterr()
    assert tr.resume_if_requested(cfg_old, model3, opt3, device) == 2
    assert "starts afresh" in capsys.readouterr().out and opt3.n_averaged == 0

    # test.py scores the averaged weights and says which
    model.eval()
    with opt.averaged_parameters():
        want = te.test(model, dl_val, device)
    monkeypatch.setattr(te, "get_config", lambda: cfg)
    monkeypatch.setattr(te, "Dataset", lambda mode: d_val)
    te.main()
    said = capsys.readouterr().out
    assert "Scoring the averaged weights" in said and "decay 0.9" in said
    got = [float(x) for x in re.search(r"Accuracy=\[([0-9.]+)%\] Weighted_F1=\[([0-9.]+)%\]", said).groups()]
    assert got == [float(f"{want[0] * 100:.3f}"), float(f"{want[1] * 100:.3f}")]
    # ... and the live ones when evaluate is off
    cfg.runtime = type(cfg.runtime)(dict(cfg.runtime, ema={"enabled": True, "decay": 0.9, "evaluate": False}))
    te.main()
    assert "Scoring the live weights" in capsys.readouterr().out


def test_disabled_block_leaves_the_loop_and_its_checkpoint_as_they_were(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(ROOT)
    import train as tr
    import test as te
    runs = []
    for ema in ({"enabled": False, "decay": 0.5, "warmup": False, "evaluate": True}, None):
        rt = {} if ema is None else {"ema": ema}
        cfg = _config(tmp_path, **rt)
        if ema is None:
            cfg.runtime.pop("ema", None)
        dl_train, dl_val, d_val = _loaders()
        device = torch.device("cuda:0")
        torch.manual_seed(0)
        model = tr.M2FNet(cfg.model).to(device)
        crit = tr.M2FCrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
        opt = tr.build_optimizer(cfg, model)
        assert opt.ema_decay is None
        out = tr.training_loop(model, dl_train, dl_val, crit, opt, None, 0, cfg, device)
        ck = torch.load(cfg.checkpoint.save_path)
        assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict"}
        assert opt.n_averaged == 0 and opt._ema is None
        runs.append((out, {n: p.detach().clone() for n, p in model.named_parameters()}))
    assert runs[0][0] == runs[1][0]
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n
    capsys.readouterr()
    monkeypatch.setattr(te, "get_config", lambda: cfg)
    monkeypatch.setattr(te, "Dataset", lambda mode: d_val)
    te.main()
    assert "Scoring the live weights" in capsys.readouterr().out
