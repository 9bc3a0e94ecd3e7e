"""The drop-in loop's runtime.stream_chunk: src/test.py opens its stream with max_chunk and feeds every batch through the chunk plan;
the logits and the scores are those of the column-fed pass."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

from test_streaming_loop_gpu import _config  # noqa: E402
from test_streaming_model_gpu import TOL_LOGITS  # noqa: E402
from test_train_loop_gpu import _dataset  # noqa: E402  (the synthetic MELD-shaped tables of the loop tests)


def _chunk_config(tmp_path, past, chunk):
    from utils import AttrDict
    cfg = _config(tmp_path, (past, 0), True)
    cfg.runtime = AttrDict(dict(cfg.runtime, stream_chunk=chunk))
    return cfg


@pytest.mark.parametrize("past,chunk", [(None, 4), (3, 4), (3, 16)])
def test_chunk_fed_test_pass_returns_the_column_fed_scores(tmp_path, monkeypatch, past, chunk):
    monkeypatch.chdir(ROOT)
    import dataset as ds
    import test as te
    cfg = _chunk_config(tmp_path, past, chunk)
    assert te.streaming_settings(cfg) is True and te.stream_chunk_settings(cfg) == chunk
    loader = torch.utils.data.DataLoader(_dataset(20, 48, 40, 3), collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = te.build_model(cfg, device)
    model.streaming = True                                             # what main() sets from runtime.streaming ...
    model.stream_chunk = 1
    acc_c, f1_c = te.test(model, loader, device)                       # column by column
    assert model._test_stream.max_chunk == 1 and model._test_stream.chunk_plan is None
    with torch.inference_mode():
        columns = [model._test_stream.run(b["text"].to(device), b["audio"].to(device), b["padding_mask"].to(device)).cpu() for b in loader]
    model.stream_chunk = te.stream_chunk_settings(cfg)                 # ... and from runtime.stream_chunk
    acc_p, f1_p = te.test(model, loader, device)
    st = model._test_stream
    assert st.max_chunk == chunk and st.chunk_plan is not None and st.max_streams == 8
    with torch.inference_mode():
        for b, want in zip(loader, columns):
            got = st.run(b["text"].to(device), b["audio"].to(device), b["padding_mask"].to(device)).cpu()
            valid = ~b["padding_mask"]
            err = (got - want).abs()[valid].max().item()
            assert err < TOL_LOGITS, err
            assert torch.all(got[~valid] == 0)
            assert torch.equal(got.argmax(2)[valid], want.argmax(2)[valid])
    print(f"past={past} chunk={chunk}: column-fed {acc_c:.6f} / {f1_c:.6f}, chunk-fed {acc_p:.6f} / {f1_p:.6f}")
    assert abs(acc_p - acc_c) <= 1e-6 and abs(f1_p - f1_c) <= 1e-6


@pytest.mark.parametrize("chunk", [0, 65, 2.5, True, "4"])
def test_a_chunk_length_outside_1_to_64_is_refused(tmp_path, monkeypatch, chunk):
    monkeypatch.chdir(ROOT)
    import test as te
    with pytest.raises(ValueError, match="runtime.stream_chunk"):
        te.stream_chunk_settings(_chunk_config(tmp_path, None, chunk))
    assert te.stream_chunk_settings(_config(tmp_path, (None, 0), True)) == 1
