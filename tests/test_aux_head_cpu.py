"""Host side of the auxiliary label head: the float64 reference (tests/golden/aux_head_ref.py) against nn.Linear + F.cross_entropy, the
head module (init, views, state_dict), the argument checks (criterion.resolve), Dataset(sentiment=True) / collate_fn, the drop-in
parser (src/train.py aux_head_settings), the loop with the key off and on (a stand-in model: the calls, the log lines and the checkpoint
entry), the shipped runtime.* keys and the header / ctypes agreement.  No GPU."""
import os
import sys
import types

import pandas as pd
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import aux_head_ref as ref  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import runtime  # noqa: E402
from mer_amd.aux_head import AuxiliaryHead, check_pair  # noqa: E402
from mer_amd.criterion import PLAIN, resolve  # noqa: E402


@pytest.mark.parametrize("N,D,A,eps", [(1, 20, 2, 0.0), (15, 100, 3, 0.1), (65, 20, 3, 0.1), (130, 64, 16, 0.0)])
def test_reference_is_linear_plus_cross_entropy(N, D, A, eps):
    """No class weights, rows dead only by a -1 in either label: lam * aux / den is lam * CrossEntropyLoss(ignore_index=-1,
    label_smoothing)(Linear(h), s) per labelled utterance, value and gradients, to 1e-12."""
    C, lam = 7, 0.7
    h, y, s, params, _ = ref.random_case(N, D, A, C, seed=3 * N)
    s = torch.where(s >= A, torch.full_like(s, -1), s)
    lin = torch.nn.Linear(D, A).double()
    with torch.no_grad():
        lin.weight.copy_(params[: A * D].view(A, D))
        lin.bias.copy_(params[A * D:])
    hd = h.double().requires_grad_(True)
    loss = ref.torch_loss(hd, y, s, lin, C, lam, eps)
    loss.backward()
    r = ref.aux_head(h, y, s, lin.weight.detach(), lin.bias.detach(), C, None, lam, eps)
    den = r["den"]
    scale = lambda x: max(x.abs().max().item(), 1e-300)          # noqa: E731
    errs = (abs(loss.item() - (lam * r["aux"] / den).item()), (hd.grad - r["dfeat"] / den).abs().max().item() / scale(hd.grad),
            (lin.weight.grad - r["dW"] / den).abs().max().item() / scale(lin.weight.grad),
            (lin.bias.grad - r["db"] / den).abs().max().item() / scale(lin.bias.grad), (lin(h.double()) - r["logits"]).abs().max().item())
    print(f"N {N} D {D} A {A} eps {eps}: {int(r['live'].sum())} live rows; loss, dfeat, dW, db, logits errors {errs}")
    assert all(e <= 1e-12 for e in errs)
    # its own autograd agrees with its closed form; dead rows are exact zeros, whatever they hold
    W = lin.weight.detach().clone().requires_grad_(True)
    r2 = ref.aux_head(h, y, s, W, lin.bias.detach(), C, None, lam, eps)
    (lam * r2["aux"]).backward()
    assert (W.grad - r["dW"]).abs().max().item() <= 1e-12 * scale(r["dW"])
    bad = h.clone()
    bad[~r["live"]] = float("nan")
    rb = ref.aux_head(bad, y, s, lin.weight.detach(), lin.bias.detach(), C, None, lam, eps)
    assert torch.equal(rb["dW"], r["dW"]) and torch.equal(rb["rows"], r["rows"]) and not rb["dfeat"][~r["live"]].any()


def test_reference_weights_only_by_the_emotion_class_and_ignores_either_label():
    h, y, s, params, w = ref.random_case(40, 16, 3, 7, seed=1)
    W, b = params[:48].view(3, 16), params[48:]
    r = ref.aux_head(h, y, s, W, b, 7, w)
    live = (y >= 0) & (s >= 0) & (s < 3)
    assert torch.equal(r["live"], live) and not r["rows"][~live].any() and not r["g"][~live].any()
    assert torch.allclose(r["rows"][live], w.double()[y[live]] * r["a"][live], rtol=1e-15, atol=0)
    assert abs(r["den"].item() - w.double()[y[y >= 0]].sum().item()) <= 1e-12
    none = ref.aux_head(h, y, torch.full_like(s, -1), W, b, 7, w)
    assert not none["rows"].any() and not none["dfeat"].any() and not none["dW"].any() and not none["db"].any()


def test_head_module_is_a_linear_layer_over_one_block():
    torch.manual_seed(5)
    head = AuxiliaryHead(20, 3)
    torch.manual_seed(5)
    lin = torch.nn.Linear(20, 3)
    assert torch.equal(head.weight, lin.weight) and torch.equal(head.bias, lin.bias)          # nn.Linear's init under the caller's seed
    assert [n for n, _ in head.named_parameters()] == ["params"] and head.params.shape == (63,) and head.params.dtype == torch.float32
    assert head.weight.data_ptr() == head.params.data_ptr() and head.bias.data_ptr() == head.params.data_ptr() + 4 * 60
    sd = head.state_dict()
    assert list(sd) == ["weight", "bias"] and sd["weight"].shape == (3, 20) and sd["bias"].shape == (3,)
    other = AuxiliaryHead(20, 3)
    assert not torch.equal(other.params, head.params)
    other.load_state_dict(sd)
    assert torch.equal(other.params, head.params)
    lin.load_state_dict(sd)                                                                     # ... and an nn.Linear reads it
    with pytest.raises(RuntimeError, match="size mismatch for weight"):
        AuxiliaryHead(24, 3).load_state_dict(sd)
    with pytest.raises(RuntimeError, match="Missing key"):
        other.load_state_dict({"weight": sd["weight"]})
    assert head.trainable and not head.params.requires_grad_(False).requires_grad and not head.trainable
    p, g = head.step_buffers("cpu")
    assert g is None and p.data_ptr() == head.params.data_ptr()
    head.params.requires_grad_(True)
    p, g = head.step_buffers("cpu")
    assert g.shape == (63,) and head.step_buffers("cpu")[1] is g
    head.publish_grad()
    assert head.params.grad is g
    for bad in (1, 17, 3.0, True):
        with pytest.raises(ValueError, match="num_classes must be an integer in \\[2, 16\\]"):
            AuxiliaryHead(20, bad)
    for bad in (0, 1025, 8.0):
        with pytest.raises(ValueError, match="in_features must be an integer in \\[1, 1024\\]"):
            AuxiliaryHead(bad, 3)


def check_step_args(who, aux, in_features, mask_shape=None, label_smoothing=0.0, device="cpu", **kw):
    """`aux=` through criterion.resolve -> the checked (head, aux_labels, weight, label_smoothing), or PLAIN for None"""
    spec = resolve(who, num_classes=7, cls_hidden=in_features, mask_shape=mask_shape, device=device, label_smoothing=0.1, class_weights=None,
                   aux=aux, aux_label_smoothing=label_smoothing, **kw)
    return spec if spec is PLAIN else spec.aux


def test_check_step_args():
    from mer_amd.crf import LinearChainCRF
    head, s = AuxiliaryHead(64, 3), torch.zeros(4, 6, dtype=torch.int64)
    assert check_step_args("step", None, 64) is PLAIN
    assert check_step_args("step", (head, s, 1), 64, (4, 6), 0.1) == (head, s, 1.0, 0.1)
    assert check_pair(0, 0) == (0.0, 0.0)
    # (valid values beside it: the arguments that PRIORITY looks at before aux are checked before it)
    beside = {"teacher_logits": torch.zeros(4, 6, 7), "distill": (0.5, 2.0), "crf": LinearChainCRF(7), "rdrop": 1.0, "supcon": (0.1, 0.1)}
    for name, why in (("teacher_logits", "no distillation form"), ("distill", "no distillation form"), ("crf", "no auxiliary form"),
                      ("rdrop", "fourth float"), ("supcon", "hidden activation's gradient")):
        with pytest.raises(ValueError, match=f"step: aux and {name} do not combine .*{why}"):
            check_step_args("step", (head, s, 0.5), 64, (4, 6), **{name: beside[name]})
    for bad, msg in (((head, s), "must be a triple"), ((torch.nn.Linear(64, 3), s, 0.5), "needs an AuxiliaryHead first"),
                     ((AuxiliaryHead(48, 3), s, 0.5), "in_features 48, the model's classifier hidden width is 64"),
                     ((head, s[:, :5], 0.5), "labels must be int64 \\[4, 6\\]"), ((head, s.int(), 0.5), "labels must be int64"),
                     ((head, [0, 1], 0.5), "labels must be int64"), ((head, s, -0.5), "weight must be >= 0"),
                     ((head, s, float("nan")), "weight must be a finite number"), ((head, s, True), "weight must be a finite number")):
        with pytest.raises(ValueError, match="step: aux.*" + msg):
            check_step_args("step", bad, 64, (4, 6))
    for eps in (1.0, -0.1, float("inf"), "0.1"):
        with pytest.raises(ValueError, match="step: aux.*smoothing"):
            check_step_args("step", (head, s, 0.5), 64, (4, 6), eps)
    with pytest.raises(ValueError, match="a trainable aux= head does not combine with gradient accumulation"):
        check_step_args("step", (head, s, 0.5), 64, (4, 6), accumulating=True)
    with pytest.raises(ValueError, match="a trainable aux= head does not combine with DataParallelStep"):
        check_step_args("step", (head, s, 0.5), 64, (4, 6), data_parallel=True)
    with pytest.raises(ValueError, match="step: aux= labels are on cpu, the step runs on cuda:0"):
        check_step_args("step", (head, s, 0.5), 64, (4, 6), device="cuda:0")
    assert check_step_args("step", (head, s, 0.5), 64, (4, 6), device="cpu")[1] is s
    head.params.requires_grad_(False)                                     # a frozen head works with both
    assert check_step_args("step", (head, s, 0.5), 64, (4, 6), accumulating=True, data_parallel=True)[2] == 0.5


def test_header_and_bindings_agree():
    text = open(os.path.join(ROOT, "include", "m2fnet_hip.h")).read()
    assert "M2F_BUF_AUX = 26" in text and "M2F_BUF_AUX_LABELS = 27" in text and "M2F_BUF_AUX_LOGITS = 28" in text and "M2F_BUF_END = 29" in text
    assert (runtime.BUF_AUX, runtime.BUF_AUX_LABELS, runtime.BUF_AUX_LOGITS) == (26, 27, 28)
    for name in ("m2f_plan_aux_head", "m2f_aux_head", "m2f_aux_head_scratch_floats", "m2f_aux_head_forward", "m2f_aux_head_backward",
                 "m2f_aux_head_join"):
        assert name + "(" in text and name in runtime.SIGNATURES, name
    assert len(runtime.SIGNATURES["m2f_plan_aux_head"][1]) == 4 and len(runtime.SIGNATURES["m2f_aux_head"][1]) == 18


def _table(tmp_path):
    import dataset as ds
    rows = [("a", "joy", "positive", 0, 0), ("b", "anger", "negative", 0, 1), ("c", "neutral", "neutral", 0, 2),
            ("d", "sadness", "mixed", 1, 0), ("e", "fear", "negative", 1, 1), ("f", "disgust", "positive", 2, 0)]
    path = tmp_path / "train_sent_emo.csv"
    pd.DataFrame(rows, columns=["Utterance", "Emotion", "Sentiment", "Dialogue_ID", "Utterance_ID"]).to_csv(path, index=False)
    g = torch.Generator().manual_seed(0)
    return ds, pd.read_csv(path), torch.randn(6, 8, generator=g), torch.randn(6, 4, generator=g)


def test_dataset_yields_the_sentiment_and_collate_pads_it(tmp_path):
    ds, table, text, audio = _table(tmp_path)
    assert ds.SENTIMENTS == {"neutral": 0, "positive": 1, "negative": 2}
    data = ds.Dataset("train", text_embeddings=text, audio_embeddings=audio, table=table.copy(), sentiment=True)
    assert [data[i]["sentiment"].tolist() for i in range(3)] == [[1, 2, 0], [-1, 2], [1]]          # an unknown string: -1
    assert data[0]["sentiment"].dtype == torch.int64
    batch = ds.collate_fn([data[i] for i in range(3)])
    assert batch["sentiment"].tolist() == [[1, 2, 0], [-1, 2, -1], [1, -1, -1]] and batch["sentiment"].dtype == torch.int64
    assert batch["emotion"].tolist() == [[1, 3, 0], [2, 5, -1], [6, -1, -1]]
    plain = ds.Dataset("train", text_embeddings=text, audio_embeddings=audio, table=table.copy())
    assert "sentiment" not in plain[0] and "sentiment" not in ds.collate_fn([plain[0], plain[1]])
    with pytest.raises(ValueError, match="runtime.aux_head needs the Sentiment column"):
        ds.Dataset("train", text_embeddings=text, audio_embeddings=audio, table=table.drop(columns=["Sentiment"]), sentiment=True)


def test_drop_in_parser_and_shipped_keys(monkeypatch):
    monkeypatch.chdir(ROOT)
    import train as tr
    from utils import get_config
    cfg = get_config()
    shipped = {"enabled": False, "labels": "sentiment", "weight": 0.5, "label_smoothing": 0.0, "lr": 1.0e-3, "warmup_steps": 0}
    assert dict(cfg.runtime.aux_head) == shipped
    assert tr.aux_head_settings(cfg) is None and tr.aux_head_settings({"runtime": {}}) is None
    on = dict(shipped, enabled=True, weight=0.25, warmup_steps=4)
    assert tr.aux_head_settings({"runtime": {"aux_head": on}}) == {k: v for k, v in on.items() if k != "enabled"}
    assert tr.aux_head_settings({"runtime": {"aux_head": {"enabled": True}}}) == {k: v for k, v in shipped.items() if k != "enabled"}
    for bad, msg in (({"enabled": 1}, "enabled must be true or false"), ({"enabled": True, "weight": -1.0}, "weight"),
                     ({"enabled": False, "label_smoothing": 1.0}, "smoothing"), ({"enabled": True, "lr": 0.0}, "lr must be a finite number > 0"),
                     ({"enabled": True, "warmup_steps": -1}, "warmup_steps"), ({"enabled": True, "warmup_steps": 1.5}, "warmup_steps"),
                     ({"enabled": True, "labels": "speaker"}, "labels must be one of"), ({"enabled": True, "alpha": 1.0}, "unknown key"),
                     ("yes", "must be a mapping")):
        with pytest.raises(ValueError, match="runtime.aux_head.*" + msg):
            tr.aux_head_settings({"runtime": {"aux_head": bad}})
    base = {"enabled": True}
    with pytest.raises(ValueError, match="runtime.aux_head.enabled needs runtime.device_batcher: False"):
        tr.aux_head_settings({"runtime": {"aux_head": base, "device_batcher": True}})
    assert tr.aux_head_settings({"runtime": {"aux_head": {"enabled": False}, "device_batcher": True}}) is None
    with pytest.raises(ValueError, match="runtime.aux_head.enabled needs runtime.fused_step: True"):
        tr.aux_head_settings({"runtime": {"aux_head": base, "fused_step": False}})
    with pytest.raises(ValueError, match="runtime.aux_head.enabled needs solver.loss_fn: CE or Focal"):
        tr.aux_head_settings({"runtime": {"aux_head": base}, "solver": {"loss_fn": "CRF"}})
    assert tr.aux_head_settings({"runtime": {"aux_head": base}, "solver": {"loss_fn": "Focal"}}) is not None
    with pytest.raises(ValueError, match="runtime.aux_head.enabled does not combine with runtime.rdrop.enabled"):
        tr.aux_head_settings({"runtime": {"aux_head": base, "rdrop": {"enabled": True}}})
    with pytest.raises(ValueError, match="runtime.aux_head.enabled does not combine with runtime.supcon.enabled"):
        tr.aux_head_settings({"runtime": {"aux_head": base, "supcon": {"enabled": True}}})
    with pytest.raises(ValueError, match="runtime.aux_head.enabled does not combine with runtime.grad_accumulation > 1"):
        tr.aux_head_settings({"runtime": {"aux_head": base, "grad_accumulation": 2}})
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="runtime.aux_head.enabled runs in one process"):
        tr.aux_head_settings({"runtime": {"aux_head": base}})
    monkeypatch.delenv("WORLD_SIZE")
    # the schedule: weight * (step + 1) / n until n
    m = types.SimpleNamespace()
    batch = {"sentiment": torch.tensor([[0, 1, -1]])}
    assert tr._aux_kw(m, batch, "cpu", 0) == {}
    tr.attach_aux_head(m, None, 64, "cpu")
    assert m.aux_head is None and tr._aux_kw(m, batch, "cpu", 0) == {}
    tr.attach_aux_head(m, {"labels": "sentiment", "weight": 0.4, "label_smoothing": 0.1, "lr": 2e-3, "warmup_steps": 4}, 64, "cpu")
    assert isinstance(m.aux_head, AuxiliaryHead) and (m.aux_head.in_features, m.aux_head.num_classes) == (64, 3)
    assert m.aux_head.optimizer.param_groups[0]["lr"] == 2e-3
    kws = [tr._aux_kw(m, batch, "cpu", s) for s in (0, 1, 3, 9)]
    assert [k["aux"][2] for k in kws] == [0.1, 0.2, 0.4, 0.4] and all(k["aux_label_smoothing"] == 0.1 and k["aux"][0] is m.aux_head for k in kws)
    assert torch.equal(kws[0]["aux"][1], batch["sentiment"])
    with pytest.raises(ValueError, match="the batch carries no 'sentiment'"):
        tr._aux_kw(m, {}, "cpu", 0)


class _StandIn(torch.nn.Module):
    """What train() needs of a model, on the CPU: train_step records its keyword arguments, returns a loss that depends on them and
    leaves a gradient on its one parameter - and, given aux=, on the head's block as the fused step does (the module's own buffer)."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(3))
        self.calls = []
        self._terms = (torch.tensor(0.0), torch.tensor(0.0))

    def train_step(self, text, audio, mask, emotion, use_graph=True, aux=None, aux_label_smoothing=0.0, **kw):
        self.calls.append(dict(kw, aux=aux, aux_label_smoothing=aux_label_smoothing))
        ce = (self.w * text.mean()).sum() ** 2 + 1.0
        self.w.grad = torch.full_like(self.w, 0.1)
        if aux is None:
            return ce.detach().reshape(1)[0]
        head, labels, weight = aux
        share = (labels >= 0).float().mean() + head.params.detach().abs().mean()
        p, g = head.step_buffers("cpu")
        g.fill_(0.5)
        head.publish_grad()
        self._terms = (ce.detach(), share)
        return (ce + weight * share).detach()

    def aux_terms(self):
        return self._terms


def test_loop_logs_both_shares_and_is_unchanged_with_the_key_off(tmp_path, monkeypatch):
    monkeypatch.chdir(ROOT)
    import train as tr
    from utils import AttrDict
    ds, table, text, audio = _table(tmp_path)
    logs = []
    monkeypatch.setattr(tr, "wandb", types.SimpleNamespace(log=lambda d: logs.append(dict(d))))
    crit = tr.M2FCrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    settings = {"labels": "sentiment", "weight": 0.5, "label_smoothing": 0.1, "lr": 1e-2, "warmup_steps": 0}

    def run(aux, attach=True, sentiment=True):
        torch.manual_seed(0)
        data = ds.Dataset("train", text_embeddings=text, audio_embeddings=audio, table=table.copy(), **({"sentiment": True} if sentiment else {}))
        dl = torch.utils.data.DataLoader(data, collate_fn=ds.collate_fn, batch_size=2, shuffle=False)
        m = _StandIn()
        if attach:
            tr.attach_aux_head(m, aux, 8, "cpu")
        m.initial_block = m.aux_head.params.detach().clone() if getattr(m, "aux_head", None) is not None else None
        opt = torch.optim.SGD(m.parameters(), lr=0.1)
        del logs[:]
        mean = tr.train(m, dl, crit, opt, 0, True, "cpu")
        return m, opt, mean, [dict(d) for d in logs]

    m_on, opt_on, mean_on, on = run(settings)
    assert len(on) == 2 and all(c["aux"][0] is m_on.aux_head and c["aux"][2] == 0.5 and c["aux_label_smoothing"] == 0.1 for c in m_on.calls)
    assert m_on.calls[0]["aux"][1].tolist() == [[1, 2, 0], [-1, 2, -1]] and m_on.calls[1]["aux"][1].tolist() == [[1]]
    for d in on:
        full = d["Train/CE"] + 0.5 * d["Train/Aux"]
        print(f"Train/Running_loss {d['Train/Running_loss']!r} = CE {d['Train/CE']!r} + 0.5 * Aux {d['Train/Aux']!r} = {full!r}")
        assert d["Train/Aux"] > 0.0 and abs(full - d["Train/Running_loss"]) <= 2e-6 * abs(d["Train/Running_loss"])
    assert not torch.equal(m_on.aux_head.params.detach(), m_on.initial_block)              # the head's own Adam stepped its block
    # the key off (the shipped default), absent, and a model main() never touched: the loop as it was, byte for byte
    m_off, _, mean_off, off = run(None)
    m_none, _, mean_none, none = run(None, attach=False, sentiment=False)
    assert m_off.aux_head is None and not hasattr(m_none, "aux_head")
    assert mean_off == mean_none and repr(off) == repr(none) and all("Train/CE" not in d and "Train/Aux" not in d for d in off)
    assert all(c["aux"] is None and c["aux_label_smoothing"] == 0.0 for c in m_off.calls + m_none.calls)
    rest = lambda m: [{k: v for k, v in c.items() if k not in ("aux", "aux_label_smoothing")} for c in m.calls]          # noqa: E731
    assert rest(m_off) == rest(m_none)
    assert mean_on != mean_off
    # checkpoints carry the head, a resume restores it
    path = str(tmp_path / "ckpt.pt")
    tr.write_checkpoint(path, 3, m_on, opt_on)
    state = torch.load(path)
    assert list(state[tr.AUX_KEY]) == ["weight", "bias"] and torch.equal(state[tr.AUX_KEY]["weight"], m_on.aux_head.weight)
    tr.write_checkpoint(str(tmp_path / "plain.pt"), 3, m_off, torch.optim.SGD(m_off.parameters(), lr=0.1))
    assert tr.AUX_KEY not in torch.load(str(tmp_path / "plain.pt"))
    m_new = _StandIn()
    tr.attach_aux_head(m_new, settings, 8, "cpu")
    assert not torch.equal(m_new.aux_head.params, m_on.aux_head.params)
    cfg = AttrDict({"checkpoint": AttrDict({"load_path": path, "load_checkpoint": True}), "runtime": AttrDict({})})
    assert tr.resume_if_requested(cfg, m_new, torch.optim.SGD(m_new.parameters(), lr=0.1), "cpu") == 4
    assert torch.equal(m_new.aux_head.params, m_on.aux_head.params)


def test_validation_reports_the_heads_accuracy(tmp_path, monkeypatch):
    monkeypatch.chdir(ROOT)
    import train as tr
    ds, table, text, audio = _table(tmp_path)
    data = ds.Dataset("val", text_embeddings=text, audio_embeddings=audio, table=table.copy(), sentiment=True)
    batch = ds.collate_fn([data[0], data[1]])
    m = types.SimpleNamespace()
    tr.attach_aux_head(m, {"labels": "sentiment", "weight": 0.5, "label_smoothing": 0.0, "lr": 1e-3, "warmup_steps": 0}, 8, "cpu")
    feats = torch.zeros(2, 3, 8)
    m.last_features = lambda: feats
    want = torch.tensor([[1, 2, 0], [2, 2, 0]])                             # what the stand-in head below predicts
    m.aux_head.forward = lambda f: torch.nn.functional.one_hot(want, 3).float()
    acc = tr.AuxAccuracy(m)
    acc.update(m, batch, "cpu")
    assert (acc.hits, acc.count) == (4, 4) and acc.result() == 1.0          # labels [[1, 2, 0], [-1, 2, -1]]: the -1 slots do not count
    m.aux_head.forward = lambda f: torch.nn.functional.one_hot(torch.zeros(2, 3, dtype=torch.int64), 3).float()
    acc.update(m, batch, "cpu")
    assert (acc.hits, acc.count) == (5, 8)
    off = tr.AuxAccuracy(types.SimpleNamespace())
    off.update(m, batch, "cpu")
    assert off.result() is None
