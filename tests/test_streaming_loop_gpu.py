"""The drop-in loop's runtime.streaming: src/test.py scores every batch through DialogueStream.run and gets the predictions of the batched
pass; a context that looks ahead is refused on the host."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import synth  # noqa: E402
from test_train_loop_gpu import _dataset  # noqa: E402  (the synthetic MELD-shaped tables of the loop tests)


def _config(tmp_path, context, streaming):
    from utils import AttrDict, get_config
    cfg = AttrDict(dict(get_config()))
    cfg.model = AttrDict(synth._cfg(40, 48, 64, 4, 4, 4, 1, 1, 1, dropout=0.1))
    cfg.runtime = AttrDict(dict(cfg.runtime, context=None if context is None else AttrDict(past=context[0], future=context[1]),
                                streaming=streaming))
    cfg.checkpoint = AttrDict(save_path=str(tmp_path / "m2fnet.pth"), load_path=str(tmp_path / "m2fnet.pth"), save_checkpoint=False,
                              load_checkpoint=False)
    return cfg


@pytest.mark.parametrize("past", [None, 3])
def test_streamed_test_pass_returns_the_batched_predictions(tmp_path, monkeypatch, past):
    monkeypatch.chdir(ROOT)
    import dataset as ds
    import test as te
    cfg = _config(tmp_path, (past, 0), True)
    assert te.streaming_settings(cfg) is True
    loader = torch.utils.data.DataLoader(_dataset(20, 48, 40, 3), collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = te.build_model(cfg, device)
    assert model.context == (past, 0)
    acc_b, f1_b = te.test(model, loader, device)                       # the batched pass (forward)
    batched, streamed = [], []
    with torch.inference_mode():
        for b in loader:
            batched.append(model(b["text"].to(device), b["audio"].to(device), b["padding_mask"].to(device)).argmax(2).cpu())
    model.streaming = True                                             # what main() sets from runtime.streaming
    acc_s, f1_s = te.test(model, loader, device)
    st = model._test_stream
    assert st.capacity == (64 if past is None else past + 1) and st.max_streams == 8
    with torch.inference_mode():
        for b in loader:
            streamed.append(st.run(b["text"].to(device), b["audio"].to(device), b["padding_mask"].to(device)).argmax(2).cpu())
    for b, p, q in zip(loader, batched, streamed):
        valid = ~b["padding_mask"]
        assert torch.equal(p[valid], q[valid])
    print(f"past={past}: batched {acc_b:.6f} / {f1_b:.6f}, streamed {acc_s:.6f} / {f1_s:.6f}")
    assert abs(acc_s - acc_b) <= 1e-6 and abs(f1_s - f1_b) <= 1e-6
    assert np.isfinite(acc_s) and 0.0 <= acc_s <= 1.0


@pytest.mark.parametrize("context", [None, (None, None), (2, 1), (None, 4)])
def test_a_context_that_looks_ahead_is_refused(tmp_path, monkeypatch, context):
    monkeypatch.chdir(ROOT)
    import test as te
    with pytest.raises(ValueError, match="runtime.streaming needs a causal runtime.context"):
        te.streaming_settings(_config(tmp_path, context, True))
    assert te.streaming_settings(_config(tmp_path, context, False)) is False
