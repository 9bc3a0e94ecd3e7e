"""Data-parallel micro-batches (mer_amd.dp.DataParallelStep(..., sync=False)): two REAL rank processes (tests/dp_accum_worker.py)
each run groups of two micro-batches - sync=False, then sync=True - and the result must match ONE process accumulating all four
micro-batches (M2FNet.set_grad_accumulation, train_step(normalise=False), FusedAdam with grad_scale = the group's den).

The rank processes are started while this module is imported - during collection, before this process (or any test) has touched
the GPU: a process that has initialised the GPU must not start programs on this pool - and waited for right there, so that they
never share the device with this process's own GPU tests.  They are not started without a GPU, when the GPU is already
initialised (the test then fails and says so), or when the run deselects GPU tests (-m "not gpu")."""
import os
import socket
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _gpu_tests_deselected() -> bool:
    argv = sys.argv
    for i, a in enumerate(argv):
        expr = argv[i + 1] if a == "-m" and i + 1 < len(argv) else (a[2:] if a.startswith("-m") and len(a) > 2 else None)
        if expr is not None and "not gpu" in expr:
            return True
    return False


def _start_ranks():
    """-> (rc, out_dir, log text) of the 2-rank run, or a string saying why it did not run."""
    if torch.cuda.device_count() < 1:
        return "no GPU on this box"
    if _gpu_tests_deselected():
        return "GPU tests deselected"
    if torch.cuda.is_initialized():
        return "this process had initialised the GPU before the rank processes could be started"
    out = tempfile.mkdtemp(prefix="m2f_dpacc_")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    with open(os.path.join(out, "worker.log"), "w") as log:
        p = subprocess.Popen([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                              "--master-addr", "127.0.0.1", "--master-port", str(port),
                              os.path.join(ROOT, "tests", "dp_accum_worker.py"), out], env=env, stdout=log, stderr=subprocess.STDOUT)
        try:
            rc = p.wait(timeout=600)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()
            rc = -9
    return rc, out, open(os.path.join(out, "worker.log")).read()[-4000:]


RUN = _start_ranks()


@pytest.fixture(scope="module")
def ranks():
    if isinstance(RUN, str):
        if RUN == "no GPU on this box":
            pytest.skip(RUN)
        pytest.fail(f"the 2-rank worker processes were not started: {RUN}")
    rc, out, log = RUN
    errs = "".join(open(os.path.join(out, f)).read() for f in sorted(os.listdir(out)) if f.startswith("acc_error_rank"))
    assert rc == 0, f"2-rank worker exited with {rc}\n{errs}\n--- log tail ---\n{log}"
    return [torch.load(os.path.join(out, f"acc_rank{r}.pt"), weights_only=False) for r in range(2)]


def _single_process(name, r0, r1):
    """One process, one model: every group accumulates rank 0's and rank 1's shards of both micro-batches, then one step."""
    import synth
    import dp_accum_worker as W
    from mer_amd.model import M2FNet
    from mer_amd.optim import FusedAdam
    precision = "bf16" if name == "bf16" else "fp32"
    cfg, _ = W.global_micro_batches("empty" if name == "empty" else "full")
    torch.manual_seed(0)
    m = M2FNet(cfg, precision=precision).to("cuda").train()
    m.load_state_dict({k: v.cuda() for k, v in synth.make_state_dict(cfg).items()})
    m.set_grad_accumulation(True)
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.01)
    start = m.flat_parameters().detach().cpu().clone()
    losses, params = [], []
    for _ in range(2):
        opt.zero_grad()
        for j in range(2):
            for sh in (r0[name]["shards"][j], r1[name]["shards"][j]):
                if sh[2].shape[0]:
                    m.train_step(*[t.cuda() for t in sh], normalise=False, use_graph=False)
        terms = m.loss_terms()
        losses.append(float(terms[2] / terms[1]))
        opt.grad_scale = terms[1:2]
        opt.step()
        torch.cuda.synchronize()
        params.append(m.flat_parameters().detach().cpu().clone())
    return start, losses, params


@pytest.mark.parametrize("name", ["fp32", "empty", "bf16"])
def test_two_rank_micro_batches_equal_one_process_accumulating_all(ranks, name):
    r0, r1 = ranks
    assert r0["world"] == r1["world"] == 2
    a, b = r0[name], r1[name]
    assert a["losses"] == b["losses"]
    for pa, pb in zip(a["params"], b["params"]):
        assert torch.equal(pa, pb)                          # the replicas stay identical
    if name == "empty":
        assert b["shards"][1][2].shape[0] == 0               # rank 1 ran an empty second micro-batch
    assert not a["g16"] and not b["g16"]                     # micro-batches keep fp32 gradients (the bf16 exchange casts per bucket)
    start, losses, params = _single_process(name, r0, r1)
    # fp32 exchange: summation order of the ranks' partial sums only; bf16 exchange: each rank's accumulated gradients are rounded
    # once to bf16 before the sum
    tol_loss, tol_rel = (1e-5, 1e-4) if name != "bf16" else (2e-3, 3e-2)
    assert max(abs(x - y) for x, y in zip(a["losses"], losses)) < tol_loss, (a["losses"], losses)
    for pa, ref in zip(a["params"], params):
        rel = float((pa - ref).double().norm() / (ref - start).double().norm())
        assert rel < tol_rel, rel
