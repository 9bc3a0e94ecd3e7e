"""bench.py's measurement contract: `--steps` is the number of timed steps of `ms_per_step`, and `--dump-outputs DIR` writes what
the timed path computed in its last step (loss, logits, a fixed seeded sample of parameters / gradients / Adam moments) as float
.npy files under 64 MB, the same from run to run of the same arguments.  What is measured after the timed steps needs `--full`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr, r.stderr[-2000:]


def test_bench_refuses_after_step_figures_without_full(tmp_path):
    for extra in (["--dump-launches", str(tmp_path / "launches.txt")], ["--repeats", "3"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2"] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "need --full" in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "launches.txt").exists()


def _run(out_dir, steps, **kw):
    import bench
    dev = torch.device("cuda", 0)
    return bench.run_workload(bench.WORKLOADS["c1"], "bf16", 0, 1, dev, steps, 1, True, False, 4, "bf16", dump_outputs=str(out_dir), **kw)


@pytest.mark.gpu
def test_dump_outputs_of_the_timed_step(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    res = _run(a, 3)
    assert res["steps"] == 3 and res["ms_per_step"] > 0
    names = {"loss", "logits", "param_index", "params", "grads", "exp_avg", "exp_avg_sq"}
    assert {f[:-4] for f in os.listdir(a)} == names and set(res["outputs_dumped"]["arrays"]) == names
    arr = {n: np.load(a / (n + ".npy")) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in arr.values())
    assert sum(os.path.getsize(a / (n + ".npy")) for n in names) <= 64 * 2 ** 20
    assert arr["logits"].shape == (4, 16, 7) and np.isfinite(arr["logits"]).all()
    assert arr["loss"].shape == (1,) and arr["loss"][0] == np.float32(res["loss"])
    n = res["outputs_dumped"]["params_total"]
    idx = arr["param_index"]
    assert len(idx) == min(n, 1 << 20) and (np.diff(idx) > 0).all() and idx[-1] < n
    assert all(arr[k].shape == idx.shape for k in ("params", "grads", "exp_avg", "exp_avg_sq"))
    assert np.abs(arr["exp_avg"]).max() > 0 and np.abs(arr["grads"]).max() > 0
    # same arguments -> same inputs, same sample: a second run computes the same step
    _run(b, 3)
    for k in names:
        assert np.allclose(np.load(b / (k + ".npy")), arr[k], rtol=1e-5, atol=1e-6), k
    assert (np.load(b / "param_index.npy") == idx).all()


@pytest.mark.gpu
def test_plain_run_leaves_the_after_step_figures_to_full(tmp_path):
    """A plain run reports the timed steps only; `full` adds the legs measured after them, and the timed steps compute the same."""
    extras = {"repeats", "fwd_bwd_only", "fp32_gradients", "comm", "roofline"}
    plain = _run(tmp_path / "plain", 3)
    assert not extras & set(plain)
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0 and plain["value"] > 0
    table = tmp_path / "launches.txt"
    full = _run(tmp_path / "full", 3, full=True, repeats=2, dump=str(table))
    assert set(full) - set(plain) == extras - {"comm"}                  # (comm: N > 1 only)
    assert full["repeats"]["n"] == 2 and full["repeats"]["ms_per_step"][0] == full["ms_per_step"]
    assert full["fwd_bwd_only"]["ms_per_step"] > 0 and full["fp32_gradients"]["ms_per_step"] > 0
    assert full["roofline"]["launches_per_step"] > 0 and full["roofline"]["achieved"] > 0
    assert len(table.read_text().splitlines()) >= full["roofline"]["launches_per_step"]
    assert full["loss"] == pytest.approx(plain["loss"], rel=1e-5)
    for k in ("params", "exp_avg", "exp_avg_sq", "logits"):
        assert np.allclose(np.load(tmp_path / "full" / (k + ".npy")), np.load(tmp_path / "plain" / (k + ".npy")), rtol=1e-5, atol=1e-6), k
