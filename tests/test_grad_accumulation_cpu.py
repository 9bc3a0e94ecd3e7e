"""Host side of gradient accumulation over micro-batches: the C entry point, the config key, src/train.py's grouping of DataLoader
batches and its refusals (raised before any GPU use)."""
import os
import re
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

from mer_amd import runtime  # noqa: E402


def test_header_declares_and_library_exports_accumulate_grads():
    header = open(runtime.HEADER_PATH).read()
    assert re.search(r"int\s+m2f_plan_accumulate_grads\s*\(\s*m2f_plan\s*\*\s*plan\s*,\s*int\s+on\s*\)", header)
    assert "m2f_plan_accumulate_grads" in runtime.SIGNATURES
    assert runtime.lib().m2f_plan_accumulate_grads is not None
    # a NULL plan fails through m2f_last_error (no GPU call)
    assert runtime.lib().m2f_plan_accumulate_grads(None, 1) != 0
    assert "NULL plan" in runtime.lib().m2f_last_error().decode()


def test_config_has_grad_accumulation_one():
    from utils import get_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        cfg = get_config()
    finally:
        os.chdir(cwd)
    assert cfg.runtime.grad_accumulation == 1


def test_group_batches():
    import train as tr
    assert list(tr.group_batches(range(5), 1)) == [[0], [1], [2], [3], [4]]
    assert list(tr.group_batches(range(6), 3)) == [[0, 1, 2], [3, 4, 5]]
    assert list(tr.group_batches(range(7), 3)) == [[0, 1, 2], [3, 4, 5], [6]]
    assert list(tr.group_batches([], 2)) == []


def _cfg(**rt):
    return {"runtime": dict(rt)}


def test_grad_accumulation_refusals_before_gpu_use():
    import train as tr
    assert tr.grad_accumulation_steps(_cfg()) == 1
    assert tr.grad_accumulation_steps(_cfg(grad_accumulation=4)) == 4
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="integer >= 1"):
            tr.grad_accumulation_steps(_cfg(grad_accumulation=bad))
    with pytest.raises(ValueError, match="fused_step"):
        tr.grad_accumulation_steps(_cfg(grad_accumulation=2, fused_step=False))
    with pytest.raises(ValueError, match="fused_optimizer"):
        tr.grad_accumulation_steps(_cfg(grad_accumulation=2, fused_optimizer=True))
    with pytest.raises(ValueError, match="grad_bf16"):
        tr.grad_accumulation_steps(_cfg(grad_accumulation=2, grad_bf16=True))
    assert tr.grad_accumulation_steps(_cfg(grad_accumulation=2, grad_bf16=True), world=2) == 2
    with pytest.raises(ValueError, match="grad_overlap"):
        tr.grad_accumulation_steps(_cfg(grad_accumulation=2, grad_overlap=True), world=2)
    # k = 1 refuses nothing; one rank ignores grad_overlap
    assert tr.grad_accumulation_steps(_cfg(grad_accumulation=1, fused_step=False, fused_optimizer=True)) == 1
    assert tr.grad_accumulation_steps(_cfg(grad_accumulation=2, grad_overlap=True), world=1) == 2
